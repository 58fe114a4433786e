// Implicit-GEMM convolution kernels for gfx950 (MI355X): forward / data-gradient (one kernel,
// driven by a tap table), its LDS-DMA and grouped variants, the halo-tile 3x3 kernels, the split-K
// finishing pass, the folded-BatchNorm GLU epilogue of the inference generator, and the dispatch
// behind the sba_conv_igemm* entry points.  NHWC activations,
// [Cout][tap][Cin] packed weights, MFMA 32x32 tiles with f32 accumulation
// (v_mfma_f32_32x32x16_bf16 for bf16 storage, v_mfma_f32_32x32x2_f32 for f32).
// The weight gradients (sba_conv_wgrad) are in wgrad.hip, weight packing and 2x2 pooling in pack.hip;
// conv_common.h holds what this file and wgrad.hip share (the LDS-DMA primitives, geom_ok).
//
// Replaces cuDNN under nn.Conv2d forward/backward in the reference
// (model.py:32-35 conv3x3, :552 downBlock conv4x4 s2, :41 fused nearest x2).
#include <math.h>
#include <stdlib.h>

#include "common.h"
#include "conv_common.h"
#include <type_traits>

namespace {

// ---------------------------------------------------------------------------
// MFMA over one 64-byte K slab held in LDS as rows of ROWB bytes
// ---------------------------------------------------------------------------
// optional epilogue operands: per-channel bias, and a ReLU mask source (same layout as y): outputs are
// zeroed where mask <= 0 -- the backward of the ReLU that produced the tensor whose gradient this is
// yh: store the (bf16-typed) output as IEEE binary16 bits (SBA_BF16_YH: the pre-BatchNorm tensor)
// glu_c > 0: the folded-BatchNorm GLU epilogue of the inference generator (tile_epilogue_glu): glu_c output channels
struct EpiX { const float* bias; const void* mask; int yh; int glu_c; };

// keep the bf16 halves of v whose counterpart in m is > 0
__device__ __forceinline__ uint32_t relu_mask_bf16x2(uint32_t v, uint32_t m) {
    const uint32_t lo = ((m & 0x7fffu) != 0u && (m & 0x8000u) == 0u) ? 0x0000ffffu : 0u;
    const uint32_t hi = ((m & 0x7fff0000u) != 0u && (m & 0x80000000u) == 0u) ? 0xffff0000u : 0u;
    return v & (lo | hi);
}

// two packed bf16 values + two packed bf16 values, rounded back to bf16
__device__ __forceinline__ uint32_t add_bf16x2(uint32_t p, uint32_t q) {
    const float lo = __uint_as_float(p << 16) + __uint_as_float(q << 16);
    const float hi = __uint_as_float(p & 0xffff0000u) + __uint_as_float(q & 0xffff0000u);
    return (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
}

template <typename T> struct Mma;

template <> struct Mma<bf16_t> {
    // slab = 32 bf16 = two 16-deep MFMA steps; lane l holds row (l&31), k = 8*(l>>5)+j
    template <int TM, int TN, int ROWB>
    static __device__ __forceinline__ void slab(const unsigned char* a_rows, const unsigned char* b_rows,
                                                int lane, f32x16_t (&acc)[TM][TN]) {
        const int r = lane & 31, h = lane >> 5;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8_t a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                a[i] = *reinterpret_cast<const bf16x8_t*>(a_rows + (i * 32 + r) * ROWB + kk * 32 + h * 16);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                b[j] = *reinterpret_cast<const bf16x8_t*>(b_rows + (j * 32 + r) * ROWB + kk * 32 + h * 16);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
};

template <> struct Mma<float> {
    // slab = 16 floats = eight 2-deep MFMA steps; lane l holds row (l&31), k = (l>>5)
    template <int TM, int TN, int ROWB>
    static __device__ __forceinline__ void slab(const unsigned char* a_rows, const unsigned char* b_rows,
                                                int lane, f32x16_t (&acc)[TM][TN]) {
        const int r = lane & 31, h = lane >> 5;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            float a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                a[i] = *reinterpret_cast<const float*>(a_rows + (i * 32 + r) * ROWB + (2 * kk + h) * 4);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                b[j] = *reinterpret_cast<const float*>(b_rows + (j * 32 + r) * ROWB + (2 * kk + h) * 4);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
};

// ---------------------------------------------------------------------------
// shared tile epilogue: per-channel BatchNorm statistics, bias / ReLU, residual addend, NHWC store
// (bf16 tiles are transposed through LDS into 16-byte row stores).  `lead` marks the threads that
// own accumulators; rowoff[row] = output pixel index of tile row `row` (or -1).
// ---------------------------------------------------------------------------
template <typename T, int BM, int BN, int TM, int TN, int NTT, int STAGE_BYTES>
__device__ __forceinline__ void tile_epilogue(f32x16_t (&acc)[TM][TN], const bool lead, unsigned char* lds_all,
                                              const int* rowoff, float* s_stat, const int wm0, const int wn0,
                                              const int lane, const int n_base, const int ycs,
                                              const sba_conv_geom& g, T* __restrict__ y,
                                              const T* __restrict__ addend, float* __restrict__ stats,
                                              const EpiX ex, const int slot_id = -1) {
    const float* __restrict__ bias = ex.bias;
    const T* __restrict__ rmask = reinterpret_cast<const T*>(ex.mask);
    // epilogue: C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
    const int col_l = lane & 31, rsel = 4 * (lane >> 5);
    constexpr bool kStageOut = sizeof(T) == 2;       // bf16: transpose through LDS -> 16-byte row stores
    constexpr int OROW = BN * 2 + 16;                // staged output row: BN bf16 + 16 B pad
    static_assert(!kStageOut || BM * OROW <= STAGE_BYTES, "output tile fits in the staging buffers");
    if (lead) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int co = n_base + wn0 + j * 32 + col_l;
        float csum = 0.f, csq = 0.f;
        const float bco = bias ? bias[co < g.Cout ? co : 0] : 0.f;      // one load per column, not per element
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + rsel;
                float v = acc[i][j][r];
                csum += v;
                csq += v * v;
                if (bias) v += bco;
                if (g.relu) v = fmaxf(v, 0.f);
                if (kStageOut) {
                    // (the main loop's last barrier has passed: the staging buffers are free)
                    *reinterpret_cast<bf16_t*>(lds_all + row * OROW + (wn0 + j * 32 + col_l) * 2) =
                        ex.yh ? f2h_bits(v) : f2bf(v);
                } else {
                    const int pix = rowoff[row];
                    if (pix >= 0 && co < g.Cout) {
                        const int64_t o = (int64_t)pix * ycs + g.y_coff + co;
                        if (addend) v += to_f<T>(addend[o]);
                        if (rmask && !(to_f<T>(rmask[o]) > 0.f)) v = 0.f;
                        y[o] = from_f<T>(v);
                    }
                }
            }
        }
        if (stats) {
            csum += __shfl_xor(csum, 32, 64);
            csq += __shfl_xor(csq, 32, 64);
            if (lane < 32) {
                atomicAdd(&s_stat[wn0 + j * 32 + col_l], csum);
                atomicAdd(&s_stat[BN + wn0 + j * 32 + col_l], csq);
            }
        }
    }
    }
    if (kStageOut || stats) __syncthreads();
    if (kStageOut) {
        constexpr int CPRO = BN / 8;                 // 16-byte chunks per output row
        for (int idx = threadIdx.x; idx < BM * CPRO; idx += NTT) {
            const int row = idx / CPRO, cc = idx - row * CPRO;
            const int pix = rowoff[row];
            const int co = n_base + cc * 8;
            if (pix < 0 || co >= g.Cout) continue;
            uint4 v = *reinterpret_cast<const uint4*>(lds_all + row * OROW + cc * 16);
            const int64_t o = (int64_t)pix * ycs + g.y_coff + co;
            if (co + 8 <= g.Cout) {
                if (addend) {
                    const uint4 a = *reinterpret_cast<const uint4*>(addend + o);
                    v.x = add_bf16x2(v.x, a.x);
                    v.y = add_bf16x2(v.y, a.y);
                    v.z = add_bf16x2(v.z, a.z);
                    v.w = add_bf16x2(v.w, a.w);
                }
                if (rmask) {
                    const uint4 m = *reinterpret_cast<const uint4*>(rmask + o);
                    v.x = relu_mask_bf16x2(v.x, m.x);
                    v.y = relu_mask_bf16x2(v.y, m.y);
                    v.z = relu_mask_bf16x2(v.z, m.z);
                    v.w = relu_mask_bf16x2(v.w, m.w);
                }
                *reinterpret_cast<uint4*>(y + o) = v;
            } else {                                  // ragged Cout tail: scalar
                // (fully unrolled with static indices: a dynamically indexed private array would be
                // promoted to LDS and make every wave read the AQL dispatch packet for its flat id)
                const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (co + k < g.Cout) {
                        float f = bf2f((bf16_t)((k & 1) ? (vw[k >> 1] >> 16) : (vw[k >> 1] & 0xffffu)));
                        if (addend) f += to_f<T>(addend[o + k]);
                        if (rmask && !(to_f<T>(rmask[o + k]) > 0.f)) f = 0.f;
                        y[o + k] = from_f<T>(f);
                    }
                }
            }
        }
    }
    if (stats) {
        // one of SBA_BN_STAT_SLOTS replicas per workgroup: 1/SLOTS of the same-address atomic traffic
        const int sid = slot_id >= 0 ? slot_id : (int)(blockIdx.x + blockIdx.z);
        float* slot = stats + (int64_t)(sid & (SBA_BN_STAT_SLOTS - 1)) * 2 * g.Cout;
        for (int c = threadIdx.x; c < BN; c += NTT) {
            const int co = n_base + c;
            if (co < g.Cout) {
                atomicAdd(&slot[co], s_stat[c]);
                atomicAdd(&slot[g.Cout + co], s_stat[BN + c]);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// GLU epilogue of the inference path (sba_conv_igemm_glu): the weight rows were packed by sba_fold_bn_pack with the
// eval-mode BatchNorm scale folded in and the output channels interleaved in granules of 32 -- packed rows
// 64 b .. 64 b + 31 are value channels 32 b .. 32 b + 31, rows 64 b + 32 .. 64 b + 63 their gates.  The C/D layout of
// the 32 x 32 MFMA puts column (lane & 31) of an accumulator tile in one lane, so a wave that owns an EVEN number of
// 32-column tiles (WN % 64 == 0) holds value channel c in acc[i][j] and its gate in acc[i][j + 1] of the SAME lane:
//     out[pixel][c] = (acc_v + b'_v) * sigmoid(acc_g + b'_g)
// needs no cross-lane or LDS exchange.  The C = ex.glu_c output channels are stored NHWC: f32 directly, one dword per
// lane (the 32 lanes of a half-wave hold 32 consecutive channels of one pixel = one coalesced 128-byte row segment;
// 16-byte stores per lane would need the transpose through LDS this path avoids), bf16 through the staging tile the plain epilogue uses as well (half its width), as 16-byte
// row stores.  g.Cout is the PACKED row count (a multiple of 64; rows of channels >= C are zero).
// ---------------------------------------------------------------------------
template <typename T, int BM, int BN, int TM, int TN, int NTT, int STAGE_BYTES>
__device__ __forceinline__ void tile_epilogue_glu(f32x16_t (&acc)[TM][TN], unsigned char* lds_all, const int* rowoff,
                                                  const int wm0, const int wn0, const int lane, const int n_base,
                                                  const sba_conv_geom& g, T* __restrict__ y, const EpiX ex) {
    static_assert(TN % 2 == 0 && BN % 64 == 0, "a wave owns whole (value, gate) granule pairs");
    const float* __restrict__ bias = ex.bias;
    const int C = ex.glu_c;
    const int ycs = g.y_cstride ? g.y_cstride : C;
    const int col_l = lane & 31, rsel = 4 * (lane >> 5);
    constexpr bool kStageOut = sizeof(T) == 2;
    constexpr int BNO = BN / 2;                      // output channels of the tile
    constexpr int OROW = BNO * 2 + 16;
    static_assert(!kStageOut || BM * OROW <= STAGE_BYTES, "output tile fits in the staging buffers");
#pragma unroll
    for (int j = 0; j < TN; j += 2) {
        const int rv = n_base + wn0 + j * 32 + col_l;               // packed row of the value channel; gate: rv + 32
        // (in range: g.Cout is a multiple of 64 and every launch grid covers exactly g.Cout packed rows)
        const float bv = bias[rv], bg = bias[rv + 32];
        const int lc = (wn0 >> 1) + (j >> 1) * 32 + col_l;          // output column inside the tile
        const int oc = (n_base >> 1) + lc;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + rsel;
                const float v = (acc[i][j][r] + bv) * sigmoidf_(acc[i][j + 1][r] + bg);
                if (kStageOut) {
                    *reinterpret_cast<bf16_t*>(lds_all + row * OROW + lc * 2) = f2bf(v);
                } else {
                    const int pix = rowoff[row];
                    if (pix >= 0 && oc < C) y[(int64_t)pix * ycs + g.y_coff + oc] = from_f<T>(v);
                }
            }
        }
    }
    if (kStageOut) {
        __syncthreads();
        constexpr int CPRO = BNO / 8;                // 16-byte chunks per output row
        for (int idx = threadIdx.x; idx < BM * CPRO; idx += NTT) {
            const int row = idx / CPRO, cc = idx - row * CPRO;
            const int pix = rowoff[row];
            const int oc = (n_base >> 1) + cc * 8;
            if (pix < 0 || oc >= C) continue;        // (C % 8 == 0 is checked on the host: whole chunks only)
            const uint4 v = *reinterpret_cast<const uint4*>(lds_all + row * OROW + cc * 16);
            *reinterpret_cast<uint4*>(y + (int64_t)pix * ycs + g.y_coff + oc) = v;
        }
    }
}

// Split-K partial sums: every split adds its partial tile into the zero-filled f32 workspace with device-scope
// atomics; splitk_finish_kernel then runs the epilogue and leaves the workspace zero.  (The last arriving split finishing
// its tile inside the GEMM kernel -- one ticket per tile in the workspace tail -- passed the GPU suite but measured no
// gain on the step, 14.96 vs 14.78 ms with 75 finishing launches fewer: the last arrival's 16 KB device-scope reload +
// epilogue sits at the tail of every tile, where the finishing launch spreads the same work over the whole chip; removed.)
template <int TM, int TN>
__device__ __forceinline__ void splitk_accumulate(float* __restrict__ ws, const f32x16_t (&acc)[TM][TN], const int m0,
                                                  const int n0, const int lane, const int M, const int Cout) {
    const int col_s = lane & 31, rsel_s = 4 * (lane >> 5);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int co = n0 + j * 32 + col_s;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + rsel_s;
                if (m < M && co < Cout) atomicAdd(&ws[(int64_t)m * Cout + co], acc[i][j][r]);
            }
    }
}

// ---------------------------------------------------------------------------
// What the three GEMM bodies below (igemm_kernel, igemm_dma_body, igemm_dma2_body) share in front of and behind their K
// loops.  What they still spell out themselves changed a kernel's register counts when it came from a helper: the
// packing of the tap words in all three, and in igemm_kernel the dead-row test of a_row_origin and gemm_tail.
// ---------------------------------------------------------------------------
// tap offsets are packed 4 bits each (offset + 8), 16 to a word, so that the per-step lookup is scalar shifts instead
// of a dynamically indexed kernarg array: the offsets of tap `tap` out of the packed words
__device__ __forceinline__ void tap_offsets(const uint64_t (&tyb)[2], const uint64_t (&txb)[2], const int tap, int& ty,
                                            int& tx) {
    const int tsel = tap < SBA_MAX_TAPS ? tap : 0;
    const uint64_t tyw = tsel < 16 ? tyb[0] : tyb[1], txw = tsel < 16 ? txb[0] : txb[1];
    ty = (int)((tyw >> (4 * (tsel & 15))) & 15) - 8;
    tx = (int)((txw >> (4 * (tsel & 15))) & 15) - 8;
}

// GEMM row m = output pixel (oy, ox) of the OHs x OWs sub-grid (sub = OHs * OWs pixels) of image n
__device__ __forceinline__ void row_pixel(const sba_conv_geom& g, const int sub, const int m, int& n, int& oy, int& ox) {
    n = m / sub;
    const int rem = m - n * sub;
    oy = rem / g.OWs;
    ox = rem - oy * g.OWs;
}

// the A row a thread stages (fixed over the K loop): tap (ty, tx) reads input pixel (iy0 + ty, ix0 + tx) of the image
// that starts at pixel nb; a row that is not `live` (beyond M or the tile) is out of bounds for every tap -> zero rows
__device__ __forceinline__ void a_row_origin(const sba_conv_geom& g, const int sub, const int m, const bool live,
                                             int& iy0, int& ix0, int& nb) {
    if (live) {
        int n, oy, ox;
        row_pixel(g, sub, m, n, oy, ox);
        iy0 = oy * g.sy;
        ix0 = ox * g.sx;
        nb = n * g.IH * g.IW;
    } else {
        iy0 = -100000;
        ix0 = 0;
        nb = 0;
    }
}

template <int TM, int TN>
__device__ __forceinline__ void zero_acc(f32x16_t (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// LDS-DMA bodies, workgroup L -> tile (mt, nt); false = a padding slot of the grid.  Ids L and L + 8 share an XCD.
// M-major: the N tiles of an M tile (they share its input rows) take consecutive slots of one XCD, each XCD's L2 fetches
// the weights once (x read ~once, w up to 8 times); N-major (weight-heavy GEMM-like layers: a few M tiles against
// megabytes of weights): the M tiles of an N tile on one XCD -- its weight slice is fetched by that XCD only
__device__ __forceinline__ bool xcd_tile(const int L, const int gx, const int gy, const int nmajor, int& mt, int& nt) {
    const int xcd = L & 7, q = L >> 3;
    if (nmajor) {
        nt = xcd + 8 * (q / gx);
        mt = q - (q / gx) * gx;
        return nt < gy;
    }
    mt = xcd + 8 * (q / gy);
    nt = q - (q / gy) * gy;
    return mt < gx;
}

// Behind the K loop of the LDS-DMA bodies (it ended with a barrier: the ring is free).  ws != NULL: a split-K partial, the
// epilogue is splitk_finish_kernel's.  Otherwise the epilogue's row table and statistics accumulators, then the epilogue.
template <typename T, int BM, int BN, int TM, int TN, int NT, int LDS_BYTES>
__device__ __forceinline__ void gemm_tail(f32x16_t (&acc)[TM][TN], float* __restrict__ ws, unsigned char* lds, int* rowoff,
                                          float* s_stat, const int m_base, const int n_base, const int wm0, const int wn0,
                                          const int lane, const int M, const int ycs, const sba_conv_geom& g,
                                          T* __restrict__ y, const T* __restrict__ addend, float* __restrict__ stats,
                                          const EpiX ex, const int slot_id) {
    if (ws) {
        splitk_accumulate<TM, TN>(ws, acc, m_base + wm0, n_base + wn0, lane, M, g.Cout);
        return;
    }
    const int sub = g.OHs * g.OWs;
    for (int r = threadIdx.x; r < BM; r += NT) {
        const int m = m_base + r;
        int off = -1;
        if (m < M) {
            int n, oy, ox;
            row_pixel(g, sub, m, n, oy, ox);
            off = (n * g.OH + oy * g.osy + g.ooy) * g.OW + ox * g.osx + g.oox;
        }
        rowoff[r] = off;
    }
    for (int c = threadIdx.x; c < 2 * BN; c += NT) s_stat[c] = 0.f;
    __syncthreads();
    tile_epilogue<T, BM, BN, TM, TN, NT, LDS_BYTES>(acc, true, lds, rowoff, s_stat, wm0, wn0, lane, n_base, ycs, g, y, addend,
                                                    stats, ex, slot_id);
}

// ---------------------------------------------------------------------------
// forward / data-gradient implicit GEMM
//   rows  = output pixels of the (OHs x OWs) sub-grid, M = N*OHs*OWs
//   cols  = output channels
//   K     = ntaps * Cin, walked in 64-byte slabs (one tap, 32 bf16 / 16 f32 channels)
// 256 threads = 4 waves laid out (BM/WM) x (BN/WN); each wave owns WM x WN.
// LDS: double-buffered A[BM] and B[BN] rows of 80 B (64 data + 16 pad: the
// pad makes the 16-lane ds_read_b128 groups hit 16 distinct 4-bank slots).
// ---------------------------------------------------------------------------
template <typename T, int BM, int BN, int WM, int WN, int KS, int GLU = 0>
__global__ __launch_bounds__((BM / WM) * (BN / WN) * 64, (sizeof(T) == 2 && BM * BN == 128 * 128 && KS == 1) ? 3 : 1) void igemm_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                    T* __restrict__ y, const T* __restrict__ addend,
                                                    float* __restrict__ stats, const sba_conv_geom g,
                                                    const int M, float* __restrict__ ws,
                                                    const int slabs_per_split, const EpiX ex) {
    constexpr int ROWB = 80;
    constexpr int KS_CH = 64 / (int)sizeof(T);   // channels per slab
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int WAVES_N = BN / WN;
    constexpr int NT = (BM / WM) * (BN / WN) * 64;   // one wave per WM x WN sub-tile
    constexpr int RP = NT / 4;                       // tile rows staged per pass (4 threads x 16 B per row)
    constexpr int AI = (BM + RP - 1) / RP, BI = (BN + RP - 1) / RP;    // 16-byte loads per thread per slab
    static_assert(BM % WM == 0 && BN % WN == 0 && WM % 32 == 0 && WN % 32 == 0, "tile");
    constexpr int TILE_BYTES = (BM + BN) * ROWB;
    constexpr int STAGING_BYTES = 2 * KS * TILE_BYTES;      // double-buffered LDS, global loads one stage ahead

    // KS slabs are staged per barrier (KS > 1 for the small tiles, whose MFMA work per slab is short)
    // The epilogue's row table and statistics accumulators live INSIDE the (by then free) staging buffers,
    // behind the staged bf16 output tile: the 64x64 tile then needs 36 KB instead of 40.75 KB of LDS and a CU
    // holds four workgroups instead of three.
    constexpr int EPI_OFF = sizeof(T) == 2 ? BM * (BN * 2 + 16) : 0;
    constexpr int EPI_END = EPI_OFF + BM * 4 + BN * 8;
    constexpr int LDS_BYTES = STAGING_BYTES > EPI_END ? STAGING_BYTES : EPI_END;
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    int* rowoff = reinterpret_cast<int*>(lds + EPI_OFF);
    float* s_stat = reinterpret_cast<float*>(lds + EPI_OFF + BM * 4);

    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int wm0 = (wid / WAVES_N) * WM, wn0 = (wid % WAVES_N) * WN;
    const int m_base = blockIdx.x * BM, n_base = blockIdx.y * BN;
    const int IHL = g.ups ? 2 * g.IH : g.IH, IWL = g.ups ? 2 * g.IW : g.IW;
    const int sub = g.OHs * g.OWs;

    // per-thread description of the A rows it stages (fixed over the K loop)
    const int chunk = tid & 3;
    int a_iy0[AI], a_ix0[AI], a_nb[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int m = m_base + (tid >> 2) + RP * i;
        if (m < M && (tid >> 2) + RP * i < BM) {
            int n, oy, ox;
            row_pixel(g, sub, m, n, oy, ox);
            a_iy0[i] = oy * g.sy;
            a_ix0[i] = ox * g.sx;
            a_nb[i] = n * g.IH * g.IW;
        } else {
            a_iy0[i] = -100000;   // always out of bounds -> zero rows
            a_ix0[i] = 0;
            a_nb[i] = 0;
        }
    }
    const int cpt = g.Cin / KS_CH;            // slabs per tap
    const int nsteps = g.ntaps * cpt;
    uint64_t tyb[2] = {0, 0}, txb[2] = {0, 0};     // packed tap offsets: see tap_offsets
#pragma unroll
    for (int t = 0; t < SBA_MAX_TAPS; ++t) {
        tyb[t >> 4] |= (uint64_t)((g.ty[t] + 8) & 15) << (4 * (t & 15));
        txb[t >> 4] |= (uint64_t)((g.tx[t] + 8) & 15) << (4 * (t & 15));
    }
    const int xcs = g.x_cstride ? g.x_cstride : g.Cin;       // input pixel stride (channels)
    const int ycs = g.y_cstride ? g.y_cstride : g.Cout;      // output pixel stride (channels)

    // split-K: this block walks slabs [s_begin, s_end)
    const int s_begin = blockIdx.z * slabs_per_split;
    const int s_end = min(s_begin + slabs_per_split, nsteps);

    // Address generation is hoisted out of the per-slab path: slabs are consumed in order, so the
    // (tap, channel-slab) position is tracked incrementally (no division), the per-row gather
    // offsets are recomputed only when the tap changes, and everything is 32-bit byte offsets
    // (tensors are < 4 GiB, checked on the host).
    // Loads are BRANCH-FREE buffer loads: an out-of-image tap, a row beyond M or a slab beyond this
    // split's range gets the offset 0xFFFFFFFF, which the buffer bounds check turns into zeros.
    int g_tap = s_begin / cpt, g_c = s_begin - g_tap * cpt, g_step = s_begin;
    int cur_tap = -1;
    constexpr uint32_t OOB = 0xFFFFFFFFu;
    uint32_t a_off[AI];           // byte offset of (n, iy, ix, channel 0) for the current tap, or OOB
#pragma unroll
    for (int i = 0; i < AI; ++i) a_off[i] = OOB;
    uint32_t w_off[BI];           // byte offset of (co, slab, chunk); K is contiguous per co
    const uint32_t krow_bytes = (uint32_t)g.ntaps * (uint32_t)g.Cin * (uint32_t)sizeof(T);
#pragma unroll
    for (int i = 0; i < BI; ++i) {
        const int r = (tid >> 2) + RP * i;
        const int co = n_base + r;
        const bool ok = (co < g.Cout) && (r < BN);
        w_off[i] = ok ? (uint32_t)co * krow_bytes + (uint32_t)s_begin * 64u + (uint32_t)chunk * 16u : OOB;
    }
    const uint32_t x_bytes = (uint32_t)((int64_t)g.N * g.IH * g.IW * xcs * (int64_t)sizeof(T));
    const uint32_t w_bytes = (uint32_t)g.Cout * krow_bytes;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, w_bytes, 0x00020000);
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

    uint4 rra[KS][AI], rrb[KS][BI];
    auto gload = [&](uint4 (&ra)[KS][AI], uint4 (&rb)[KS][BI]) {
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const bool live = g_step < s_end;
            if (g_tap != cur_tap) {                     // (uniform) new tap: refresh the gather offsets
                cur_tap = g_tap;
                int ty, tx;
                tap_offsets(tyb, txb, g_tap, ty, tx);
#pragma unroll
                for (int i = 0; i < AI; ++i) {
                    int iy = a_iy0[i] + ty, ix = a_ix0[i] + tx;
                    const bool ok = (iy >= 0) & (iy < IHL) & (ix >= 0) & (ix < IWL);
                    if (g.ups) { iy >>= 1; ix >>= 1; }
                    const uint32_t o = (uint32_t)(a_nb[i] + iy * g.IW + ix) * (uint32_t)(xcs * (int)sizeof(T)) +
                                       (uint32_t)(g.x_coff * (int)sizeof(T)) + (uint32_t)chunk * 16u;
                    a_off[i] = ok ? o : OOB;
                }
            }
            const uint32_t cbytes = (uint32_t)g_c * 64u;
#pragma unroll
            for (int i = 0; i < AI; ++i) {
                const uint32_t o = (live && a_off[i] != OOB) ? a_off[i] + cbytes : OOB;
                const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(xr, o, 0, 0);
                ra[k][i] = make_uint4(v[0], v[1], v[2], v[3]);
            }
#pragma unroll
            for (int i = 0; i < BI; ++i) {
                const uint32_t o = (live && w_off[i] != OOB) ? w_off[i] : OOB;
                const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(wr, o, 0, 0);
                rb[k][i] = make_uint4(v[0], v[1], v[2], v[3]);
                if (w_off[i] != OOB) w_off[i] += 64u;
            }
            ++g_step;
            if (++g_c == cpt) { g_c = 0; ++g_tap; }
        }
    };
    auto lstore = [&](int buf, const uint4 (&ra)[KS][AI], const uint4 (&rb)[KS][BI]) {
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            unsigned char* base = lds + (buf * KS + k) * TILE_BYTES;
#pragma unroll
            for (int i = 0; i < AI; ++i)
                if ((tid >> 2) + RP * i < BM)
                    *reinterpret_cast<uint4*>(base + ((tid >> 2) + RP * i) * ROWB + chunk * 16) = ra[k][i];
#pragma unroll
            for (int i = 0; i < BI; ++i)
                if ((tid >> 2) + RP * i < BN)
                    *reinterpret_cast<uint4*>(base + (BM + (tid >> 2) + RP * i) * ROWB + chunk * 16) = rb[k][i];
        }
    };

    f32x16_t acc[TM][TN];
    zero_acc(acc);

    const int nstages = (s_end - s_begin + KS - 1) / KS;
    gload(rra, rrb);
    lstore(0, rra, rrb);
    __syncthreads();
    for (int s = 0; s < nstages; ++s) {
        const int buf = s & 1;
        if (s + 1 < nstages) gload(rra, rrb);
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const unsigned char* base = lds + (buf * KS + k) * TILE_BYTES;
            Mma<T>::template slab<TM, TN, ROWB>(base + wm0 * ROWB, base + (BM + wn0) * ROWB, lane, acc);
        }
        if (s + 1 < nstages) lstore(buf ^ 1, rra, rrb);
        __syncthreads();
    }

    // (as gemm_tail, with the GLU epilogue; the main loop ended with a barrier: the staging buffers are free)
    if (ws) {           // split-K: splitk_finish_kernel runs the epilogue
        splitk_accumulate<TM, TN>(ws, acc, m_base + wm0, n_base + wn0, lane, M, g.Cout);
        return;
    }
    for (int r = threadIdx.x; r < BM; r += NT) {
        const int m = m_base + r;
        int off = -1;
        if (m < M) {
            int n, oy, ox;
            row_pixel(g, sub, m, n, oy, ox);
            off = (n * g.OH + oy * g.osy + g.ooy) * g.OW + ox * g.osx + g.oox;
        }
        rowoff[r] = off;
    }
    for (int c = threadIdx.x; c < 2 * BN; c += NT) s_stat[c] = 0.f;
    __syncthreads();
    if constexpr (GLU) {
        tile_epilogue_glu<T, BM, BN, TM, TN, NT, LDS_BYTES>(acc, lds, rowoff, wm0, wn0, lane, n_base, g, y, ex);
    } else {
        tile_epilogue<T, BM, BN, TM, TN, NT, LDS_BYTES>(acc, true, lds, rowoff, s_stat, wm0, wn0, lane, n_base, ycs, g,
                                                        y, addend, stats, ex);
    }
}

// ---------------------------------------------------------------------------
// The same implicit GEMM with the operands staged by LDS-DMA (bf16): `buffer_load_dwordx4 ... lds` moves
// 16 bytes per lane from a per-lane global offset straight into LDS (wave-uniform base + lane * 16), so a
// K stage costs no staging VGPRs and no ds_write pass, and a ring of D stages keeps D-1 of them in flight:
// the generic kernel above exposes one full global-load latency per stage on the launch-latency-bound
// layers (273-workgroup grids of the Inception trunk: ~1440 cycles per 64-deep stage for 128 cycles of MFMA).
//   * LDS image of one 32-channel slab: rows of 64 B, unpadded (the DMA destination is lane-linear: 4 lanes
//     per row, 16 rows per wave-instruction); the 16-byte chunk c of row r lives at chunk c ^ ((r >> 2) & 3),
//     applied on the SOURCE side (each lane loads the chunk its slot holds) and on the fragment reads: every
//     16-lane phase of a ds_read_b128 then covers all 64 banks.
//   * out-of-image taps, rows beyond M and slabs beyond the split's range are out-of-range buffer offsets:
//     the DMA writes zeros (tools/ldsdma_probe.hip).
//   * the DMA is issued from inline asm (lds_dma16 of conv_common.h; hipcc would otherwise drain ALL of it -- vmcnt(0) -- in front of
//     every LDS read); completion is counted by hand: before stage s is read every wave waits until only the
//     (D-2) younger stages it issued are outstanding, then the workgroup barrier makes all waves' parts visible
//     and proves that nobody still reads the buffer the next issue overwrites.
//   * workgroups are numbered so that the N tiles of one M tile run on one XCD, back to back (shared A rows
//     are served by that XCD's L2).
// ---------------------------------------------------------------------------

#ifdef SBA_DMA_TRACE     // tools/trace_dma.py: per-stage s_memtime stamps of wave 0 of the first workgroups
static unsigned long long* g_dma_trace = nullptr;
extern "C" void sba_set_dma_trace(unsigned long long* p) { g_dma_trace = p; }
#define DMA_TRACE_PARAM , unsigned long long* __restrict__ trace
#define DMA_TRACE_ARG , g_dma_trace
#define DMA_TRACE_ARG_FWD , trace
#define DMA_STAMP(slot) do { if (trace && L < 32 && tid == 0 && s < 30) { asm volatile("" ::: "memory"); \
    trace[(L * 32 + s) * 8 + (slot)] = __builtin_amdgcn_s_memtime(); asm volatile("" ::: "memory"); } } while (0)
#else
#define DMA_TRACE_PARAM
#define DMA_TRACE_ARG
#define DMA_TRACE_ARG_FWD
#define DMA_STAMP(slot) do { } while (0)
#endif

template <int BM, int BN, int WM, int WN, int KS, int D>
__device__ __forceinline__ void igemm_dma_body(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w, bf16_t* __restrict__ y,
    const bf16_t* __restrict__ addend, float* __restrict__ stats, const sba_conv_geom& g, const int M,
    float* __restrict__ ws, const int slabs_per_split, const EpiX ex, const int gx,
    const int gy, const int L, const int bz, const int nmajor DMA_TRACE_PARAM) {
    typedef bf16_t T;
    constexpr int TM = WM / 32, TN = WN / 32, WAVES_N = BN / WN;
    constexpr int NW = (BM / WM) * (BN / WN), NT = NW * 64;
    // every wave issues the same number of DMA loads per slab (the vmcnt bookkeeping is per wave): the weight
    // rows are padded to BNL, a multiple of 16 * NW; the padding rows load zeros (out of range) and are never read
    static_assert(BM % (16 * NW) == 0, "A rows divide evenly over the waves");
    constexpr int BNL = ((BN + 16 * NW - 1) / (16 * NW)) * (16 * NW);
    constexpr int AI = BM / (16 * NW), BI = BNL / (16 * NW);
    constexpr int SLAB_BYTES = (BM + BNL) * 64, STAGE_BYTES = KS * SLAB_BYTES, RING_BYTES = D * STAGE_BYTES;
    constexpr int LPS = KS * (AI + BI);                       // DMA loads per thread per stage
    static_assert(D >= 3 && (D - 2) * LPS <= 63, "vmcnt field");
    static_assert(RING_BYTES <= 160 * 1024, "LDS");           // (DMA destinations beyond 64 KiB work: tools/ldsdma_probe.hip)
    constexpr int EPI_OFF = BM * (BN * 2 + 16);
    constexpr int EPI_END = EPI_OFF + BM * 4 + BN * 8;
    constexpr int LDS_BYTES = RING_BYTES > EPI_END ? RING_BYTES : EPI_END;
    __shared__ __attribute__((aligned(1024))) unsigned char lds_all[LDS_BYTES];
    int* rowoff = reinterpret_cast<int*>(lds_all + EPI_OFF);
    float* s_stat = reinterpret_cast<float*>(lds_all + EPI_OFF + BM * 4);

    int mt, nt;
    if (!xcd_tile(L, gx, gy, nmajor, mt, nt)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wid / WAVES_N) * WM, wn0 = (wid % WAVES_N) * WN;
    const int m_base = mt * BM, n_base = nt * BN;
    const int IHL = g.ups ? 2 * g.IH : g.IH, IWL = g.ups ? 2 * g.IW : g.IW;
    const int sub = g.OHs * g.OWs;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds_all;

    // rows this thread's lane slot belongs to: instruction i of wave `wid` covers tile rows 16 * (wid + NW * i) ..+16
    const int rsub = lane >> 2;
    const uint32_t chunk = (uint32_t)((lane & 3) ^ ((lane >> 4) & 3));       // logical 16-byte chunk of the slot
    int a_iy0[AI], a_ix0[AI], a_nb[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int m = m_base + 16 * (wid + NW * i) + rsub;
        a_row_origin(g, sub, m, m < M, a_iy0[i], a_ix0[i], a_nb[i]);
    }
    const int cpt = g.Cin / 32;
    const int nsteps = g.ntaps * cpt;
    uint64_t tyb[2] = {0, 0}, txb[2] = {0, 0};     // packed tap offsets: see tap_offsets
#pragma unroll
    for (int t = 0; t < SBA_MAX_TAPS; ++t) {
        tyb[t >> 4] |= (uint64_t)((g.ty[t] + 8) & 15) << (4 * (t & 15));
        txb[t >> 4] |= (uint64_t)((g.tx[t] + 8) & 15) << (4 * (t & 15));
    }
    const int xcs = g.x_cstride ? g.x_cstride : g.Cin;
    const int ycs = g.y_cstride ? g.y_cstride : g.Cout;
    const int s_begin = bz * slabs_per_split;
    const int s_end = min(s_begin + slabs_per_split, nsteps);

    int g_tap = s_begin / cpt, g_c = s_begin - g_tap * cpt, g_step = s_begin;
    int cur_tap = -1;
    constexpr uint32_t OOB = 0xFFFFFFFFu;
    uint32_t a_off[AI];           // per-lane byte offset of (pixel of the current tap, channel 0, this lane's chunk)
#pragma unroll
    for (int i = 0; i < AI; ++i) a_off[i] = OOB;
    uint32_t w_off[BI];           // per-lane byte offset of (co, K = 0, this lane's chunk): constant over the K loop
    const uint32_t krow_bytes = (uint32_t)g.ntaps * (uint32_t)g.Cin * 2u;
#pragma unroll
    for (int i = 0; i < BI; ++i) {
        const int r = 16 * (wid + NW * i) + rsub, co = n_base + r;
        w_off[i] = (r < BN && co < g.Cout) ? (uint32_t)co * krow_bytes + chunk * 16u : OOB;
    }
    const uint32_t x_bytes = (uint32_t)((int64_t)g.N * g.IH * g.IW * xcs * 2);
    const uint32_t w_bytes = (uint32_t)g.Cout * krow_bytes;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, w_bytes, 0x00020000);
    const uint32_t lds_wave = lds_base + (uint32_t)(wid * 1024);
    uint32_t v_oob = OOB;
    asm volatile("" : "+v"(v_oob));         // a VGPR that holds the out-of-range offset (dead stages)

    // issue the DMA of one stage (KS consecutive slabs) into the ring buffer at LDS offset `dst`
    auto issue = [&](const uint32_t dst0) {
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const uint32_t dst = dst0 + (uint32_t)(k * SLAB_BYTES);
            if (g_step < s_end) {
                if (g_tap != cur_tap) {             // (uniform) new tap: per-lane pixel offsets
                    cur_tap = g_tap;
                    int ty, tx;
                    tap_offsets(tyb, txb, g_tap, ty, tx);
#pragma unroll
                    for (int i = 0; i < AI; ++i) {
                        int iy = a_iy0[i] + ty, ix = a_ix0[i] + tx;
                        const bool ok = (iy >= 0) & (iy < IHL) & (ix >= 0) & (ix < IWL);
                        if (g.ups) { iy >>= 1; ix >>= 1; }
                        const uint32_t o = (uint32_t)(a_nb[i] + iy * g.IW + ix) * (uint32_t)(xcs * 2) +
                                           (uint32_t)(g.x_coff * 2) + chunk * 16u;
                        a_off[i] = ok ? o : OOB;
                    }
                }
                const uint32_t sa = (uint32_t)g_c * 64u, sw = (uint32_t)g_step * 64u;
#pragma unroll
                for (int i = 0; i < AI; ++i) lds_dma16(xr, a_off[i], sa, dst + (uint32_t)(NW * i * 1024));
#pragma unroll
                for (int i = 0; i < BI; ++i) lds_dma16(wr, w_off[i], sw, dst + (uint32_t)(BM * 64 + NW * i * 1024));
                ++g_step;
                if (++g_c == cpt) { g_c = 0; ++g_tap; }
            } else {                                 // past this split's K range: zeros (keeps the vmcnt count uniform)
#pragma unroll
                for (int i = 0; i < AI; ++i) lds_dma16(xr, v_oob, 0u, dst + (uint32_t)(NW * i * 1024));
#pragma unroll
                for (int i = 0; i < BI; ++i) lds_dma16(wr, v_oob, 0u, dst + (uint32_t)(BM * 64 + NW * i * 1024));
            }
        }
    };

    f32x16_t acc[TM][TN];
    zero_acc(acc);

    // fragment addressing: lane l reads row (l & 31), logical chunk 2 * kk + (l >> 5), swizzled by its row
    const int fr = lane & 31, fh = lane >> 5, fsw = (fr >> 2) & 3;
    const int foff0 = fr * 64 + ((fh ^ fsw) << 4), foff1 = fr * 64 + (((2 + fh) ^ fsw) << 4);

    const int nstages = (s_end - s_begin + KS - 1) / KS;
    uint32_t idst = lds_wave;               // LDS destination (this wave's 1 KB slot) of the next stage to issue
    const uint32_t idst_end = lds_wave + (uint32_t)RING_BYTES;
#pragma unroll
    for (int p = 0; p < D - 1; ++p) { issue(idst); idst += STAGE_BYTES; }
    if (idst == idst_end) idst = lds_wave;
    const unsigned char* cptr = lds_all;
    for (int s = 0; s < nstages; ++s) {
        DMA_STAMP(0);
        wait_vmcnt<(D - 2) * LPS>();        // this wave's part of stage s has landed ...
        DMA_STAMP(1);
        wg_barrier();                       // ... and everybody else's; nobody reads buffer (s - 1) % D any more
        DMA_STAMP(2);
        issue(idst);                        // stage s + D - 1 (zeros past the end) into that buffer
        idst += STAGE_BYTES;
        if (idst == idst_end) idst = lds_wave;
        DMA_STAMP(3);
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const unsigned char* base = cptr + k * SLAB_BYTES;
            const unsigned char* ar = base + wm0 * 64;
            const unsigned char* br = base + (BM + wn0) * 64;
            bf16x8_t a0[TM], a1[TM], b0[TN], b1[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                a0[i] = *reinterpret_cast<const bf16x8_t*>(ar + i * 2048 + foff0);
                a1[i] = *reinterpret_cast<const bf16x8_t*>(ar + i * 2048 + foff1);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                b0[j] = *reinterpret_cast<const bf16x8_t*>(br + j * 2048 + foff0);
                b1[j] = *reinterpret_cast<const bf16x8_t*>(br + j * 2048 + foff1);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[i], b0[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[i], b1[j], acc[i][j], 0, 0, 0);
        }
        cptr += STAGE_BYTES;
        if (cptr == lds_all + RING_BYTES) cptr = lds_all;
#ifdef SBA_DMA_TRACE
        { float keep = 0.f;             // make the stamp wait for the MFMA results of this stage
#pragma unroll
          for (int i = 0; i < TM; ++i) for (int j = 0; j < TN; ++j) keep += acc[i][j][0];
          asm volatile("" :: "v"(keep)); }
        DMA_STAMP(4);
#endif
    }
    wait_vmcnt<0>();        // the dead stages issued past the end still write (zeros) into the ring
    wg_barrier();

    gemm_tail<T, BM, BN, TM, TN, NT, LDS_BYTES>(acc, ws, lds_all, rowoff, s_stat, m_base, n_base, wm0, wn0, lane, M, ycs, g,
                                                y, addend, stats, ex, mt + bz);
}

template <int BM, int BN, int WM, int WN, int KS, int D>
__global__ __launch_bounds__((BM / WM) * (BN / WN) * 64) void igemm_dma_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w, bf16_t* __restrict__ y,
    const bf16_t* __restrict__ addend, float* __restrict__ stats, const sba_conv_geom g, const int M,
    float* __restrict__ ws, const int slabs_per_split, const EpiX ex, const int gx,
    const int gy, const int nmajor DMA_TRACE_PARAM) {
    igemm_dma_body<BM, BN, WM, WN, KS, D>(x, w, y, addend, stats, g, M, ws, slabs_per_split, ex, gx, gy,
                                          (int)blockIdx.x, (int)blockIdx.z, nmajor DMA_TRACE_ARG_FWD);
}

// ---------------------------------------------------------------------------
// Second-generation LDS-DMA implicit GEMM (bf16, Cin % 64 == 0).  Per-stage s_memtime stamps of the kernel above
// (tools/trace_dma.py, profiles/r02_dma_stage_trace.txt) showed where a 64-deep stage of a 64x64 tile spends its
// ~1200 cycles: ~0 waiting for data, 80 in the barrier, ~430 ISSUING four DMA loads per wave (~100 cycles per
// buffer_load ... lds: each instruction touches 16 half cache lines) and ~450 in ds_read -> MFMA with nothing
// overlapping either.  Hence:
//   * slabs of 64 channels: LDS rows of 128 B = whole cache lines, 8 rows per DMA instruction (half the lines
//     per instruction); chunk c of row r lives at chunk c ^ ((r >> 1) & 7) -- every 16-lane phase of a
//     ds_read_b128 covers all 64 banks;
//   * the fragments of stage t+1 are read into a second register set right after the barrier, and the MFMAs of
//     stage t run interleaved with the DMA issue of stage t+D: LDS latency, matrix pipe and the load-issue
//     stall of one wave overlap each other;
//   * the buffer of stage t is free as soon as its fragments sit in registers (all waves' reads are drained
//     before the barrier), so the ring keeps D full stages in flight with D buffers.
// Everything else (zero-filled out-of-range taps / rows / dead stages, XCD-aware tile numbering, split-K into
// the f32 workspace, shared epilogue) is as in the kernel above.
// ---------------------------------------------------------------------------
// (the body is shared by the one-conv kernel and the grouped kernel below: L = the workgroup's index among this
// conv's tiles, bz = its K split)
template <int BM, int BN, int WM, int WN, int D>
__device__ __forceinline__ void igemm_dma2_body(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w, bf16_t* __restrict__ y,
    const bf16_t* __restrict__ addend, float* __restrict__ stats, const sba_conv_geom& g, const int M,
    float* __restrict__ ws, const int slabs_per_split, const EpiX ex, const int gx,
    const int gy, const int L, const int bz, const int nmajor DMA_TRACE_PARAM) {
    typedef bf16_t T;
    constexpr int TM = WM / 32, TN = WN / 32, WAVES_N = BN / WN;
    constexpr int NW = (BM / WM) * (BN / WN), NT = NW * 64;
    static_assert(BM % (8 * NW) == 0, "A rows divide evenly over the waves");
    constexpr int BNL = ((BN + 8 * NW - 1) / (8 * NW)) * (8 * NW);     // weight rows padded: same DMA count per wave
    constexpr int AI = BM / (8 * NW), BI = BNL / (8 * NW);
    constexpr int STAGE_BYTES = (BM + BNL) * 128, RING_BYTES = D * STAGE_BYTES;
    constexpr int LPS = AI + BI;                               // DMA loads per thread per stage
    constexpr int NM = 4 * TM * TN;                            // MFMAs per wave per stage
    static_assert(D >= 2 && (D - 1) * LPS <= 63, "vmcnt field");
    static_assert(RING_BYTES <= 160 * 1024, "LDS");
    constexpr int EPI_OFF = BM * (BN * 2 + 16);
    constexpr int EPI_END = EPI_OFF + BM * 4 + BN * 8;
    constexpr int LDS_BYTES = RING_BYTES > EPI_END ? RING_BYTES : EPI_END;
    __shared__ __attribute__((aligned(1024))) unsigned char lds_all[LDS_BYTES];
    int* rowoff = reinterpret_cast<int*>(lds_all + EPI_OFF);
    float* s_stat = reinterpret_cast<float*>(lds_all + EPI_OFF + BM * 4);

    int mt, nt;
    if (!xcd_tile(L, gx, gy, nmajor, mt, nt)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wid / WAVES_N) * WM, wn0 = (wid % WAVES_N) * WN;
    const int m_base = mt * BM, n_base = nt * BN;
    const int IHL = g.ups ? 2 * g.IH : g.IH, IWL = g.ups ? 2 * g.IW : g.IW;
    const int sub = g.OHs * g.OWs;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds_all;

    // DMA instruction i of wave `wid` covers tile rows 8 * (wid + NW * i) .. +8, 8 lanes (128 B) per row
    const int rsub = lane >> 3;
    int a_iy0[AI], a_ix0[AI], a_nb[AI];
    uint32_t a_chunk[AI], w_off[BI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int r = 8 * (wid + NW * i) + rsub, m = m_base + r;
        a_chunk[i] = (uint32_t)(((lane & 7) ^ ((r >> 1) & 7)) * 16);
        a_row_origin(g, sub, m, m < M, a_iy0[i], a_ix0[i], a_nb[i]);
    }
    const int cpt = g.Cin / 64;               // slabs per tap
    const int nsteps = g.ntaps * cpt;
    uint64_t tyb[2] = {0, 0}, txb[2] = {0, 0};     // packed tap offsets: see tap_offsets
#pragma unroll
    for (int t = 0; t < SBA_MAX_TAPS; ++t) {
        tyb[t >> 4] |= (uint64_t)((g.ty[t] + 8) & 15) << (4 * (t & 15));
        txb[t >> 4] |= (uint64_t)((g.tx[t] + 8) & 15) << (4 * (t & 15));
    }
    const int xcs = g.x_cstride ? g.x_cstride : g.Cin;
    const int ycs = g.y_cstride ? g.y_cstride : g.Cout;
    const int s_begin = bz * slabs_per_split;
    const int s_end = min(s_begin + slabs_per_split, nsteps);
    int g_tap = s_begin / cpt, g_c = s_begin - g_tap * cpt, g_step = s_begin;
    int cur_tap = -1;
    constexpr uint32_t OOB = 0xFFFFFFFFu;
    uint32_t a_off[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) a_off[i] = OOB;
    const uint32_t krow_bytes = (uint32_t)g.ntaps * (uint32_t)g.Cin * 2u;
#pragma unroll
    for (int i = 0; i < BI; ++i) {
        const int r = 8 * (wid + NW * i) + rsub, co = n_base + r;
        w_off[i] = (r < BN && co < g.Cout) ? (uint32_t)co * krow_bytes + (uint32_t)(((lane & 7) ^ ((r >> 1) & 7)) * 16)
                                           : OOB;
    }
    const uint32_t x_bytes = (uint32_t)((int64_t)g.N * g.IH * g.IW * xcs * 2);
    const uint32_t w_bytes = (uint32_t)g.Cout * krow_bytes;
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, w_bytes, 0x00020000);
    const uint32_t lds_wave = lds_base + (uint32_t)(wid * 1024);

    // per-stage bookkeeping, split from the loads so that the loads can be spread between the MFMAs
    bool st_live = false;
    uint32_t st_sa = 0, st_sw = 0;
    auto stage_begin = [&]() {
        st_live = g_step < s_end;
        if (st_live) {
            if (g_tap != cur_tap) {             // (uniform) new tap: per-lane pixel offsets
                cur_tap = g_tap;
                int ty, tx;
                tap_offsets(tyb, txb, g_tap, ty, tx);
#pragma unroll
                for (int i = 0; i < AI; ++i) {
                    int iy = a_iy0[i] + ty, ix = a_ix0[i] + tx;
                    const bool ok = (iy >= 0) & (iy < IHL) & (ix >= 0) & (ix < IWL);
                    if (g.ups) { iy >>= 1; ix >>= 1; }
                    const uint32_t o = (uint32_t)(a_nb[i] + iy * g.IW + ix) * (uint32_t)(xcs * 2) +
                                       (uint32_t)(g.x_coff * 2) + a_chunk[i];
                    a_off[i] = ok ? o : OOB;
                }
            }
            st_sa = (uint32_t)g_c * 128u;
            st_sw = (uint32_t)g_step * 128u;
            ++g_step;
            if (++g_c == cpt) { g_c = 0; ++g_tap; }
        } else {
            st_sa = st_sw = 0u;
        }
    };
    auto stage_load = [&](const int qd, const uint32_t dst0) {       // qd = 0 .. LPS-1 (compile-time after unrolling)
        if (qd < AI) {
            const uint32_t o = st_live ? a_off[qd < AI ? qd : 0] : OOB;
            lds_dma16(xr, o, st_sa, dst0 + (uint32_t)(NW * qd * 1024));
        } else {
            const int i = qd - AI;
            const uint32_t o = st_live ? w_off[(i >= 0 && i < BI) ? i : 0] : OOB;
            lds_dma16(wr, o, st_sw, dst0 + (uint32_t)(BM * 128 + NW * i * 1024));
        }
    };

    f32x16_t acc[TM][TN];
    zero_acc(acc);

    // fragment addressing: lane l reads row (l & 31), logical chunk 2 * kk + (l >> 5), swizzled by its row
    const int fr = lane & 31, fh = lane >> 5, fsw = (fr >> 1) & 7;
    int foff[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) foff[kk] = fr * 128 + (((2 * kk + fh) ^ fsw) << 4);

    struct Frags { bf16x8_t a[4][TM], b[4][TN]; };
    auto read_frags = [&](Frags& F, const unsigned char* base) {
        const unsigned char* ar = base + wm0 * 128;
        const unsigned char* br = base + (BM + wn0) * 128;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
            for (int i = 0; i < TM; ++i) F.a[kk][i] = *reinterpret_cast<const bf16x8_t*>(ar + i * 4096 + foff[kk]);
#pragma unroll
            for (int j = 0; j < TN; ++j) F.b[kk][j] = *reinterpret_cast<const bf16x8_t*>(br + j * 4096 + foff[kk]);
        }
    };

    const int nstages = s_end - s_begin;
    uint32_t idst = lds_wave;
    const uint32_t idst_end = lds_wave + (uint32_t)RING_BYTES;
#pragma unroll
    for (int p = 0; p < D; ++p) {
        stage_begin();
#pragma unroll
        for (int qd = 0; qd < LPS; ++qd) stage_load(qd, idst);
        idst += STAGE_BYTES;
    }
    idst = lds_wave;
    const unsigned char* rptr = lds_all;            // buffer of the stage whose fragments are read next
    Frags F0, F1;
    wait_vmcnt<(D - 1) * LPS>();
    wg_barrier();
    read_frags(F0, rptr);
    rptr += STAGE_BYTES;
    if (rptr == lds_all + RING_BYTES) rptr = lds_all;

    // one stage: fragments of stage t in Fc (their reads are in flight), stage t+1 -> Fn, DMA of stage t+D
    int s = 0;              // (stage counter of the trace build)
    auto stage = [&](Frags& Fc, Frags& Fn) {
        DMA_STAMP(0);
        wait_vmcnt<(D - 2) * LPS>();                // this wave's part of stage t+1 has landed
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // ... and its reads of stage t are in registers
        DMA_STAMP(1);
        wg_barrier();                               // everybody's: buffer t is free, buffer t+1 is complete
        DMA_STAMP(2);
        read_frags(Fn, rptr);
        rptr += STAGE_BYTES;
        if (rptr == lds_all + RING_BYTES) rptr = lds_all;
        stage_begin();
        DMA_STAMP(3);
        int qd = 0;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Fc.a[kk][i], Fc.b[kk][j], acc[i][j], 0, 0, 0);
                    const int m = (kk * TM + i) * TN + j;
                    // spread the LPS loads evenly between the NM MFMAs
                    if (((m + 1) * LPS) / NM > (m * LPS) / NM) {
#pragma unroll
                        for (int u = (m * LPS) / NM; u < ((m + 1) * LPS) / NM; ++u) stage_load(u, idst);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
        (void)qd;
        idst += STAGE_BYTES;
        if (idst == idst_end) idst = lds_wave;
#ifdef SBA_DMA_TRACE
        { float keep = 0.f;
#pragma unroll
          for (int i = 0; i < TM; ++i) for (int j = 0; j < TN; ++j) keep += acc[i][j][0];
          asm volatile("" :: "v"(keep)); }
        DMA_STAMP(4);
#endif
        ++s;
    };
    (void)s;
    for (int t = 0; t < nstages; t += 2) {
        stage(F0, F1);
        if (t + 1 < nstages) stage(F1, F0);
    }
    wait_vmcnt<0>();        // the dead stages issued past the end still write (zeros) into the ring
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wg_barrier();

    gemm_tail<T, BM, BN, TM, TN, NT, LDS_BYTES>(acc, ws, lds_all, rowoff, s_stat, m_base, n_base, wm0, wn0, lane, M, ycs, g,
                                                y, addend, stats, ex, mt + bz);
}

template <int BM, int BN, int WM, int WN, int D>
__global__ __launch_bounds__((BM / WM) * (BN / WN) * 64) void igemm_dma2_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ w, bf16_t* __restrict__ y,
    const bf16_t* __restrict__ addend, float* __restrict__ stats, const sba_conv_geom g, const int M,
    float* __restrict__ ws, const int slabs_per_split, const EpiX ex, const int gx,
    const int gy, const int nmajor DMA_TRACE_PARAM) {
    igemm_dma2_body<BM, BN, WM, WN, D>(x, w, y, addend, stats, g, M, ws, slabs_per_split, ex, gx, gy,
                                       (int)blockIdx.x, (int)blockIdx.z, nmajor DMA_TRACE_ARG_FWD);
}

// ---------------------------------------------------------------------------
// GROUPED launch: up to SBA_GROUP_MAX independent convolutions (the branches of one Inception block at one depth
// level: model.py:226-262 runs them one after the other) as ONE grid.  Each of them alone is 120..273 workgroups of
// a 64 x 64 tile on 256 CUs -- one wave per SIMD, nothing to overlap the LDS / DMA-issue latency of a stage with, a
// nearly empty second round, ~4.4 us of launch floor -- and hipGraph replay runs the branches' streams back to back.
// Grouped, their tiles share the chip: two workgroups per CU co-resident, one launch floor, one tail.  The item
// descriptors travel BY VALUE in the kernarg segment (pointers change every eager step; no device-side table to
// refresh, nothing for a captured graph to copy).
// ---------------------------------------------------------------------------
struct GroupItem {
    const bf16_t* x; const bf16_t* w; bf16_t* y; const bf16_t* addend; const float* bias; const void* mask;
    sba_conv_geom g;
    int M, gx, gy, tile_begin, nmajor, pad;
    float* ws;              // split-K partial sums of this item ([M][Cout] f32, zero-filled), or NULL
};
struct GroupArgs { int n; int sps; GroupItem it[SBA_GROUP_MAX]; };      // sps: 64-channel slabs per K split (0 = no split)

template <int BM, int BN, int WM, int WN, int D>
__global__ __launch_bounds__((BM / WM) * (BN / WN) * 64) void igemm_dma2_group_kernel(const GroupArgs A DMA_TRACE_PARAM) {
    int i = 0;
#pragma unroll
    for (int k = 1; k < SBA_GROUP_MAX; ++k)
        if (k < A.n && (int)blockIdx.x >= A.it[k].tile_begin) i = k;
    const GroupItem& it = A.it[i];
    const sba_conv_geom g = it.g;
    // A.sps != 0: grid.z K splits, partial sums added into the item's f32 workspace, finished by splitk_finish_group_kernel
    igemm_dma2_body<BM, BN, WM, WN, D>(it.x, it.w, it.y, it.addend, nullptr, g, it.M, A.sps ? it.ws : nullptr,
                                       A.sps ? A.sps : g.ntaps * (g.Cin / 64), EpiX{it.bias, it.mask, 0}, it.gx, it.gy,
                                       (int)blockIdx.x - it.tile_begin, (int)blockIdx.z, it.nmajor DMA_TRACE_ARG_FWD);
}

// the same for members whose Cin is a multiple of 32 only (32-channel slabs, first-generation body)
template <int BM, int BN, int WM, int WN, int KS, int D>
__global__ __launch_bounds__((BM / WM) * (BN / WN) * 64) void igemm_dma_group_kernel(const GroupArgs A DMA_TRACE_PARAM) {
    int i = 0;
#pragma unroll
    for (int k = 1; k < SBA_GROUP_MAX; ++k)
        if (k < A.n && (int)blockIdx.x >= A.it[k].tile_begin) i = k;
    const GroupItem& it = A.it[i];
    const sba_conv_geom g = it.g;
    igemm_dma_body<BM, BN, WM, WN, KS, D>(it.x, it.w, it.y, it.addend, nullptr, g, it.M, nullptr,
                                          g.ntaps * (g.Cin / 32), EpiX{it.bias, it.mask, 0}, it.gx, it.gy,
                                          (int)blockIdx.x - it.tile_begin, 0, it.nmajor DMA_TRACE_ARG_FWD);
}

// ---------------------------------------------------------------------------
// 3x3 stride-1 convolution (optionally behind a nearest x2 upsample) from a HALO TILE:
// a workgroup owns an 8 x 32 block of output pixels of one image and stages the (8+2) x (32+2)
// input pixels it touches (6 x 18 source pixels when upsampling) in LDS ONCE; the nine taps are then
// nine shifted views of that tile.  Compared with the generic implicit GEMM above this removes 8/9 of
// the A-operand global->LDS traffic, all per-slab address generation and half of the barriers (one per
// tap, for the double-buffered weight rows), so the main loop is just ds_read_b128 + MFMA.
// Pixel / weight rows are (2*CIN + 16) bytes apart: the 16-lane phases of a ds_read_b128 then hit 16
// distinct 4-bank groups (x2 upsampling: lane pairs share a pixel -> broadcast).
// Waves: wave w owns tile rows 2w, 2w+1 (two 32-pixel M tiles) x all BN output channels.
// ---------------------------------------------------------------------------
template <int CIN, int BN, int UPS, int GLU = 0>
__global__ __launch_bounds__(256) void conv3x3_halo_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                           bf16_t* __restrict__ y, const bf16_t* __restrict__ addend,
                                                           float* __restrict__ stats, const sba_conv_geom g,
                                                           const EpiX ex) {
    typedef bf16_t T;
    constexpr int TH = 8, TW = 32, BM = TH * TW;
    constexpr int PIXB = CIN * 2 + 16;
    constexpr int HR = UPS ? TH / 2 + 2 : TH + 2, HC = UPS ? TW / 2 + 2 : TW + 2;
    constexpr int A_BYTES = HR * HC * PIXB, B_BYTES = BN * PIXB;
    constexpr int OUT_BYTES = BM * (BN * 2 + 16);         // the epilogue's bf16 staging tile reuses the buffers
    constexpr int STAGE = A_BYTES + 2 * B_BYTES > OUT_BYTES ? A_BYTES + 2 * B_BYTES : OUT_BYTES;
    constexpr int TM = 2, TN = BN / 32;
    constexpr int CPP = CIN / 8;                          // 16-byte chunks per pixel / weight row
    constexpr int BI = (BN * CPP + 255) / 256;            // weight chunks per thread per tap
    __shared__ __attribute__((aligned(16))) unsigned char lds[STAGE + BM * 4 + BN * 8];
    unsigned char* const lA = lds;
    unsigned char* const lB = lds + A_BYTES;
    int* rowoff = reinterpret_cast<int*>(lds + STAGE);
    float* s_stat = reinterpret_cast<float*>(lds + STAGE + BM * 4);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int tiles_x = g.OW / TW, tiles_y = g.OH / TH;
    const int tx_ = blockIdx.x % tiles_x, ty_ = (blockIdx.x / tiles_x) % tiles_y, n = blockIdx.x / (tiles_x * tiles_y);
    const int oy0 = ty_ * TH, ox0 = tx_ * TW;
    const int n_base = blockIdx.y * BN;
    const int xcs = g.x_cstride ? g.x_cstride : g.Cin;
    const int ycs = g.y_cstride ? g.y_cstride : g.Cout;
    {
        const int r = tid;                                // BM == 256 threads
        rowoff[r] = (n * g.OH + oy0 + (r >> 5)) * g.OW + ox0 + (r & 31);
    }
    for (int c = tid; c < 2 * BN; c += 256) s_stat[c] = 0.f;

    constexpr uint32_t OOB = 0xFFFFFFFFu;
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
    const uint32_t x_bytes = (uint32_t)((int64_t)g.N * g.IH * g.IW * xcs * 2);
    const uint32_t w_bytes = (uint32_t)((int64_t)g.Cout * 9 * g.Cin * 2);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, w_bytes, 0x00020000);
    // Cin = nchunks x CIN: the halo tile is staged and walked once per CIN-channel chunk (same LDS footprint and
    // occupancy as Cin = CIN); the weight taps stream through the two B buffers across the chunk boundary
    const int nchunks = g.Cin / CIN, ntaps_all = 9 * nchunks;

    // ---- halo tile: source rows sy0 .. sy0+HR-1, columns sx0 .. sx0+HC-1 (zeros outside the image)
    const int sy0 = UPS ? (oy0 >> 1) - 1 : oy0 - 1, sx0 = UPS ? (ox0 >> 1) - 1 : ox0 - 1;
    // (loads are issued in batches of HB before the first LDS write: a load -> wait -> ds_write loop pays the
    // global latency once per iteration, 4 (upsampling) to 11 times per workgroup)
    constexpr int NCH = HR * HC * CPP, NI = (NCH + 255) / 256, HB = 6;
    auto stage_halo = [&](const int chunk) {
        const uint32_t cbytes = (uint32_t)(g.x_coff * 2 + chunk * CIN * 2);
#pragma unroll
        for (int i0 = 0; i0 < NI; i0 += HB) {
            u32x4_t hv[HB];
#pragma unroll
            for (int u = 0; u < HB; ++u) {
                const int idx = tid + 256 * (i0 + u);
                const int p = idx / CPP, ch = idx - p * CPP;
                const int hr = p / HC, hc = p - hr * HC;
                const int iy = sy0 + hr, ix = sx0 + hc;
                const bool ok = i0 + u < NI && idx < NCH && iy >= 0 && iy < g.IH && ix >= 0 && ix < g.IW;
                const uint32_t o = ok ? (uint32_t)((n * g.IH + iy) * g.IW + ix) * (uint32_t)(xcs * 2) + cbytes +
                                            (uint32_t)ch * 16u
                                      : OOB;
                hv[u] = __builtin_amdgcn_raw_buffer_load_b128(xr, o, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < HB; ++u) {
                const int idx = tid + 256 * (i0 + u);
                const int p = idx / CPP, ch = idx - p * CPP;
                if (i0 + u < NI && idx < NCH)
                    *reinterpret_cast<uint4*>(lA + p * PIXB + ch * 16) = make_uint4(hv[u][0], hv[u][1], hv[u][2], hv[u][3]);
            }
        }
    };
    // ---- weights of one (chunk, tap): BN rows of CIN channels; t = chunk * 9 + tap
    uint4 rb[BI];
    auto bload = [&](const int t) {
        const int chunk = t / 9, tap = t - chunk * 9;
#pragma unroll
        for (int i = 0; i < BI; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx / CPP, ch = idx - row * CPP;
            const int co = n_base + row;
            const uint32_t o = (row < BN && co < g.Cout)
                                   ? (((uint32_t)co * 9u + (uint32_t)tap) * (uint32_t)g.Cin + (uint32_t)(chunk * CIN)) * 2u +
                                         (uint32_t)ch * 16u
                                   : OOB;
            const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(wr, o, 0, 0);
            rb[i] = make_uint4(v[0], v[1], v[2], v[3]);
        }
    };
    auto bstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < BI; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx / CPP, ch = idx - row * CPP;
            if (row < BN) *reinterpret_cast<uint4*>(lB + buf * B_BYTES + row * PIXB + ch * 16) = rb[i];
        }
    };
    bload(0);
    bstore(0);

    f32x16_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int rl = lane & 31, hf = lane >> 5;
#pragma unroll 1
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        stage_halo(chunk);          // (chunk > 0: the barrier that ended the previous chunk's last tap freed lA)
        __syncthreads();
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int t = chunk * 9 + tap;
            if (t + 1 < ntaps_all) bload(t + 1);
            const int ky = tap / 3, kx = tap - ky * 3;
            const unsigned char* ap[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                int hr, hc;
                if (UPS) {
                    hr = ((2 * wid + i + ky - 1) >> 1) + 1;
                    hc = ((rl + kx - 1) >> 1) + 1;
                } else {
                    hr = 2 * wid + i + ky;
                    hc = rl + kx;
                }
                ap[i] = lA + (hr * HC + hc) * PIXB + hf * 16;
            }
            const unsigned char* bp = lB + (t & 1) * B_BYTES + rl * PIXB + hf * 16;
#pragma unroll
            for (int k16 = 0; k16 < CIN / 16; ++k16) {
                bf16x8_t a[TM], b[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(ap[i] + k16 * 32);
#pragma unroll
                for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const bf16x8_t*>(bp + j * 32 * PIXB + k16 * 32);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
            }
            if (t + 1 < ntaps_all) bstore((t + 1) & 1);
            __syncthreads();
        }
    }
    if constexpr (GLU) {
        tile_epilogue_glu<T, BM, BN, TM, TN, 256, STAGE>(acc, lds, rowoff, wid * 64, 0, lane, n_base, g, y, ex);
    } else {
        tile_epilogue<T, BM, BN, TM, TN, 256, STAGE>(acc, true, lds, rowoff, s_stat, wid * 64, 0, lane, n_base, ycs, g, y,
                                                     addend, stats, ex);
    }
}

// ---------------------------------------------------------------------------
// Halo-tile 3x3 convolution, third form: WEIGHT FRAGMENTS IN REGISTERS.  PMC of the kernel above on the ResBlock conv
// (64 -> 64 at 128 x 128, B = 20; profiles/r04_pmc_halo_res128.txt): waves parked at a barrier / s_waitcnt 53 % of their
// cycles, matrix cores busy 12 %, LDS array active 11 % -- it is bound by the nine per-tap barriers of the
// double-buffered weight rows and by two workgroups per CU (69 KB of LDS each), not by LDS bandwidth or the MFMAs.
// Here the weights never enter LDS: they are packed FRAGMENT-MAJOR (sba_pack_frag_multi: the 64 lanes' 16-byte B
// fragments of one (tap, 32-channel column tile, 16-deep k-step) are 1 KB contiguous), every wave loads the eight
// fragments of the NEXT tap with eight coalesced 1 KB instructions while it multiplies the current one (they are L1 / L2
// hits: 72 KB per layer shared by the whole grid), and the main loop has no barrier at all: the halo tile is read-only
// after the staging barrier.  LDS = the halo tile alone (49 KB; 37 KB behind the nearest x2 upsample): three workgroups
// per CU, and half the LDS reads per MFMA (A fragments only).
// ---------------------------------------------------------------------------
template <int CIN, int UPS, int GLU = 0>
__global__ __launch_bounds__(256, 3) void conv3x3_halo3_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wf,
                                                               bf16_t* __restrict__ y, const bf16_t* __restrict__ addend,
                                                               float* __restrict__ stats, const sba_conv_geom g,
                                                               const EpiX ex) {
    typedef bf16_t T;
    constexpr int TH = 8, TW = 32, BM = TH * TW, BN = 64;
    constexpr int PIXB = CIN * 2 + 16;
    constexpr int HR = UPS ? TH / 2 + 2 : TH + 2, HC = UPS ? TW / 2 + 2 : TW + 2;
    constexpr int A_BYTES = HR * HC * PIXB;
    constexpr int OUT_BYTES = BM * (BN * 2 + 16);         // the epilogue's bf16 staging tile reuses the halo buffer
    constexpr int STAGE = A_BYTES > OUT_BYTES ? A_BYTES : OUT_BYTES;
    constexpr int TM = 2, TN = 2;
    constexpr int CPP = CIN / 8;                          // 16-byte chunks per pixel
    __shared__ __attribute__((aligned(16))) unsigned char lds[STAGE + BM * 4 + BN * 8];
    unsigned char* const lA = lds;
    int* rowoff = reinterpret_cast<int*>(lds + STAGE);
    float* s_stat = reinterpret_cast<float*>(lds + STAGE + BM * 4);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_x = g.OW / TW, tiles_y = g.OH / TH;
    const int tx_ = blockIdx.x % tiles_x, ty_ = (blockIdx.x / tiles_x) % tiles_y, n = blockIdx.x / (tiles_x * tiles_y);
    const int oy0 = ty_ * TH, ox0 = tx_ * TW;
    const int n_base = blockIdx.y * BN;
    const int xcs = g.x_cstride ? g.x_cstride : g.Cin;
    const int ycs = g.y_cstride ? g.y_cstride : g.Cout;
    rowoff[tid] = (n * g.OH + oy0 + (tid >> 5)) * g.OW + ox0 + (tid & 31);      // BM == 256 threads
    for (int c = tid; c < 2 * BN; c += 256) s_stat[c] = 0.f;

    constexpr uint32_t OOB = 0xFFFFFFFFu;
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
    const uint32_t x_bytes = (uint32_t)((int64_t)g.N * g.IH * g.IW * xcs * 2);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, x_bytes, 0x00020000);
    const int nchunks = g.Cin / CIN, ntaps_all = 9 * nchunks;
    const int sy0 = UPS ? (oy0 >> 1) - 1 : oy0 - 1, sx0 = UPS ? (ox0 >> 1) - 1 : ox0 - 1;
    constexpr int NCH = HR * HC * CPP, NI = (NCH + 255) / 256, HB = 4;
    auto stage_halo = [&](const int chunk) {
        const uint32_t cbytes = (uint32_t)(g.x_coff * 2 + chunk * CIN * 2);
#pragma unroll
        for (int i0 = 0; i0 < NI; i0 += HB) {
            u32x4_t hv[HB];
#pragma unroll
            for (int u = 0; u < HB; ++u) {
                const int idx = tid + 256 * (i0 + u);
                const int p = idx / CPP, ch = idx - p * CPP;
                const int hr = p / HC, hc = p - hr * HC;
                const int iy = sy0 + hr, ix = sx0 + hc;
                const bool ok = i0 + u < NI && idx < NCH && iy >= 0 && iy < g.IH && ix >= 0 && ix < g.IW;
                const uint32_t o = ok ? (uint32_t)((n * g.IH + iy) * g.IW + ix) * (uint32_t)(xcs * 2) + cbytes +
                                            (uint32_t)ch * 16u
                                      : OOB;
                hv[u] = __builtin_amdgcn_raw_buffer_load_b128(xr, o, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < HB; ++u) {
                const int idx = tid + 256 * (i0 + u);
                const int p = idx / CPP, ch = idx - p * CPP;
                if (i0 + u < NI && idx < NCH)
                    *reinterpret_cast<uint4*>(lA + p * PIXB + ch * 16) = make_uint4(hv[u][0], hv[u][1], hv[u][2], hv[u][3]);
            }
        }
    };
    // weight fragments of (chunk, tap): [n-block][chunk][tap][j][k16][lane][8]
    // weight fragments: [64-row block][tap][j][K / 16 k-steps][lane][8]; (chunk, tap) t -> k-steps chunk * CIN/16 ..
    struct BFrag { bf16x8_t v[TN][CIN / 16]; };
    const int KSW = g.Cin / 16;                 // k-steps of one (tap, j) row
    const bf16_t* const wbase = wf + ((int64_t)blockIdx.y * 9 * 2) * KSW * 512 + lane * 8;
    auto wptr = [&](const int t) {              // t = chunk * 9 + tap
        const int chunk = t / 9, tap = t - chunk * 9;
        return wbase + ((int64_t)(tap * 2) * KSW + chunk * (CIN / 16)) * 512;
    };
    auto bload = [&](BFrag& b, const int t) {
        const bf16_t* p = wptr(t);
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int k = 0; k < CIN / 16; ++k)
                b.v[j][k] = *reinterpret_cast<const bf16x8_t*>(p + ((int64_t)j * KSW + k) * 512);
    };

    f32x16_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int rl = lane & 31, hf = lane >> 5;
    // ONE set of weight fragments (32 registers): fragment (j, k16) of the NEXT tap is loaded into its registers right
    // behind the last MFMA that reads the current tap's -- a 16-MFMA (~0.2 us) head start on an L1 / L2 hit, the other
    // waves of the SIMD cover the rest (two sets, 64 registers, spilled at three waves per SIMD)
    BFrag b;
    bload(b, 0);
#pragma unroll 1
    for (int t = 0; t < ntaps_all; ++t) {
        const int chunk = t / 9, tap = t - chunk * 9;
        if (tap == 0) {                         // (wave-uniform) a new 64-channel chunk of Cin: (re)stage the halo tile
            if (chunk) __syncthreads();         // everybody has finished reading the previous chunk's tile
            stage_halo(chunk);
            __syncthreads();
        }
        const int ky = tap / 3, kx = tap - ky * 3;
        const unsigned char* ap[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            int hr, hc;
            if (UPS) {
                hr = ((2 * wid + i + ky - 1) >> 1) + 1;
                hc = ((rl + kx - 1) >> 1) + 1;
            } else {
                hr = 2 * wid + i + ky;
                hc = rl + kx;
            }
            ap[i] = lA + (hr * HC + hc) * PIXB + hf * 16;
        }
        const bool more = t + 1 < ntaps_all;
        const bf16_t* pn = wptr(more ? t + 1 : t);
#pragma unroll
        for (int k16 = 0; k16 < CIN / 16; ++k16) {
            bf16x8_t a[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(ap[i] + k16 * 32);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b.v[j][k16], acc[i][j], 0, 0, 0);
            if (more) {
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    b.v[j][k16] = *reinterpret_cast<const bf16x8_t*>(pn + ((int64_t)j * KSW + k16) * 512);
            }
        }
    }
    __syncthreads();                            // the epilogue stages through the halo buffer
    if constexpr (GLU) {
        tile_epilogue_glu<T, BM, BN, TM, TN, 256, STAGE>(acc, lds, rowoff, wid * 64, 0, lane, n_base, g, y, ex);
    } else {
        tile_epilogue<T, BM, BN, TM, TN, 256, STAGE>(acc, true, lds, rowoff, s_stat, wid * 64, 0, lane, n_base, ycs, g, y,
                                                     addend, stats, ex);
    }
}

// ---------------------------------------------------------------------------
// The register-weight halo-tile kernel for ANY stride-1 3 x 3 window (round 4): ragged maps (tiles of 8 x 32 output
// pixels cut at the border), taps anywhere in a 3 x 3 window of offsets ('same', 'valid', their data gradients, flipped
// orders), Cin in chunks of CIN = 32 or 64 channels, 32 * TN output channels per workgroup.  Written for the first 3 x 3
// layers of the Inception trunk (model.py:170-199: 32 -> 32 and 32 -> 64 at 147 x 147, 80 -> 192 at 71 x 71) and their data
// gradients: the implicit-GEMM kernels gather every tap separately through L2 -> LDS (9x the input bytes) and run them
// at ~85 TFLOP/s -- 94 us for a layer whose tensors take 11 us to stream -- six launches on the image encoder's chain,
// the critical one of the step.
// ---------------------------------------------------------------------------
template <int CIN, int TN>
__global__ __launch_bounds__(256, 3) void conv3x3_halo3g_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wf,
                                                                bf16_t* __restrict__ y, const bf16_t* __restrict__ addend,
                                                                const sba_conv_geom g, const EpiX ex) {
    typedef bf16_t T;
    constexpr int TH = 8, TW = 32, BM = TH * TW, BN = 32 * TN;
    constexpr int PIXB = CIN * 2 + 16;
    constexpr int HR = TH + 2, HC = TW + 2;
    constexpr int A_BYTES = HR * HC * PIXB;
    constexpr int OUT_BYTES = BM * (BN * 2 + 16);
    constexpr int STAGE = A_BYTES > OUT_BYTES ? A_BYTES : OUT_BYTES;
    constexpr int TM = 2;
    constexpr int CPP = CIN / 8;
    __shared__ __attribute__((aligned(16))) unsigned char lds[STAGE + BM * 4 + BN * 8];
    unsigned char* const lA = lds;
    int* rowoff = reinterpret_cast<int*>(lds + STAGE);
    float* s_stat = reinterpret_cast<float*>(lds + STAGE + BM * 4);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_x = (g.OW + TW - 1) / TW, tiles_y = (g.OH + TH - 1) / TH;
    const int tx_ = blockIdx.x % tiles_x, ty_ = (blockIdx.x / tiles_x) % tiles_y, n = blockIdx.x / (tiles_x * tiles_y);
    const int oy0 = ty_ * TH, ox0 = tx_ * TW;
    const int n_base = blockIdx.y * BN;
    const int xcs = g.x_cstride ? g.x_cstride : g.Cin;
    const int ycs = g.y_cstride ? g.y_cstride : g.Cout;
    {
        const int oy = oy0 + (tid >> 5), ox = ox0 + (tid & 31);
        rowoff[tid] = (oy < g.OH && ox < g.OW) ? (n * g.OH + oy) * g.OW + ox : -1;
    }
    for (int c = tid; c < 2 * BN; c += 256) s_stat[c] = 0.f;
    // the 3 x 3 window of tap offsets
    int ymin = g.ty[0], xmin = g.tx[0];
#pragma unroll
    for (int t = 1; t < 9; ++t) { ymin = min(ymin, (int)g.ty[t]); xmin = min(xmin, (int)g.tx[t]); }
    uint32_t kyx = 0;                               // 4 bits per tap: ky * 4 + kx (taps 0..7; tap 8 apart)
#pragma unroll
    for (int t = 0; t < 8; ++t) kyx |= (uint32_t)((g.ty[t] - ymin) * 4 + (g.tx[t] - xmin)) << (4 * t);
    const uint32_t kyx8 = (uint32_t)((g.ty[8] - ymin) * 4 + (g.tx[8] - xmin));

    constexpr uint32_t OOB = 0xFFFFFFFFu;
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
    const uint32_t x_bytes = (uint32_t)((int64_t)g.N * g.IH * g.IW * xcs * 2);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, x_bytes, 0x00020000);
    const int nchunks = g.Cin / CIN, ntaps_all = 9 * nchunks;
    const int sy0 = oy0 + ymin, sx0 = ox0 + xmin;
    constexpr int NCH = HR * HC * CPP, NI = (NCH + 255) / 256, HB = 4;
    auto stage_halo = [&](const int chunk) {
        const uint32_t cbytes = (uint32_t)(g.x_coff * 2 + chunk * CIN * 2);
#pragma unroll
        for (int i0 = 0; i0 < NI; i0 += HB) {
            u32x4_t hv[HB];
#pragma unroll
            for (int u = 0; u < HB; ++u) {
                const int idx = tid + 256 * (i0 + u);
                const int p = idx / CPP, ch = idx - p * CPP;
                const int hr = p / HC, hc = p - hr * HC;
                const int iy = sy0 + hr, ix = sx0 + hc;
                const bool ok = i0 + u < NI && idx < NCH && iy >= 0 && iy < g.IH && ix >= 0 && ix < g.IW;
                const uint32_t o = ok ? (uint32_t)((n * g.IH + iy) * g.IW + ix) * (uint32_t)(xcs * 2) + cbytes +
                                            (uint32_t)ch * 16u
                                      : OOB;
                hv[u] = __builtin_amdgcn_raw_buffer_load_b128(xr, o, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < HB; ++u) {
                const int idx = tid + 256 * (i0 + u);
                const int p = idx / CPP, ch = idx - p * CPP;
                if (i0 + u < NI && idx < NCH)
                    *reinterpret_cast<uint4*>(lA + p * PIXB + ch * 16) = make_uint4(hv[u][0], hv[u][1], hv[u][2], hv[u][3]);
            }
        }
    };
    // weight fragments: [64-row block][tap][j][K / 16][lane][8]; this workgroup's rows n_base .. n_base + BN
    struct BFrag { bf16x8_t v[TN][CIN / 16]; };
    const int KSW = g.Cin / 16;
    const int j0 = (n_base >> 5) & 1;               // BN = 32: the odd 32-row tiles are j = 1 of their 64-row block
    const bf16_t* const wbase = wf + ((int64_t)(n_base >> 6) * 9 * 2) * KSW * 512 + lane * 8;
    auto wptr = [&](const int t) {                  // t = chunk * 9 + tap
        const int chunk = t / 9, tap = t - chunk * 9;
        return wbase + ((int64_t)(tap * 2 + j0) * KSW + chunk * (CIN / 16)) * 512;
    };
    f32x16_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int rl = lane & 31, hf = lane >> 5;
    BFrag b;
    {
        const bf16_t* p = wptr(0);
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int k = 0; k < CIN / 16; ++k) b.v[j][k] = *reinterpret_cast<const bf16x8_t*>(p + ((int64_t)j * KSW + k) * 512);
    }
#pragma unroll 1
    for (int t = 0; t < ntaps_all; ++t) {
        const int chunk = t / 9, tap = t - chunk * 9;
        if (tap == 0) {
            if (chunk) __syncthreads();
            stage_halo(chunk);
            __syncthreads();
        }
        const uint32_t code = tap < 8 ? (kyx >> (4 * tap)) & 15u : kyx8;
        const int ky = (int)(code >> 2), kx = (int)(code & 3u);
        const unsigned char* ap[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) ap[i] = lA + ((2 * wid + i + ky) * HC + rl + kx) * PIXB + hf * 16;
        const bool more = t + 1 < ntaps_all;
        const bf16_t* pn = wptr(more ? t + 1 : t);
#pragma unroll
        for (int k16 = 0; k16 < CIN / 16; ++k16) {
            bf16x8_t a[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(ap[i] + k16 * 32);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b.v[j][k16], acc[i][j], 0, 0, 0);
            if (more) {
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    b.v[j][k16] = *reinterpret_cast<const bf16x8_t*>(pn + ((int64_t)j * KSW + k16) * 512);
            }
        }
    }
    __syncthreads();
    tile_epilogue<T, BM, BN, TM, TN, 256, STAGE>(acc, true, lds, rowoff, s_stat, wid * 64, 0, lane, n_base, ycs, g, y,
                                                 addend, nullptr, ex);
}

// split-K finish: y[pix(m)][co] = ws[m][co] (+ addend), per-channel stats; thread = 4 channels x 8 rows
template <typename T>
__device__ __forceinline__ void splitk_finish_body(float* __restrict__ ws, T* __restrict__ y,
                                                   const T* __restrict__ addend,
                                                   float* __restrict__ stats, const sba_conv_geom& g,
                                                   const int M, const EpiX ex) {
    const int ycs = g.y_cstride ? g.y_cstride : g.Cout;
    const int cq = g.Cout / 4;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cq) return;
    const int c = t * 4;
    const int m0 = blockIdx.y * 8, m1 = min(m0 + 8, M);
    if (m0 >= M) return;
    const int sub = g.OHs * g.OWs;
    float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
    float4 rows[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {                       // all loads in flight before any use
        const int m = m0 + r;
        float4* wp = reinterpret_cast<float4*>(ws + (int64_t)(m < m1 ? m : m0) * g.Cout + c);
        rows[r] = *wp;
        if (m < m1) *wp = make_float4(0.f, 0.f, 0.f, 0.f);      // leave the workspace zero-filled for its next user
    }
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (ex.bias) {
#pragma unroll
        for (int k = 0; k < 4; ++k) bv[k] = ex.bias[c + k];
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int m = m0 + r;
        if (m >= m1) break;
        float v[4] = {rows[r].x, rows[r].y, rows[r].z, rows[r].w};
        const int n = m / sub, rem = m - n * sub;
        const int oy = rem / g.OWs, ox = rem - oy * g.OWs;
        const int64_t o = ((int64_t)(n * g.OH + oy * g.osy + g.ooy) * g.OW + ox * g.osx + g.oox) * ycs + g.y_coff + c;
        // 4 consecutive channels: one 8-byte (bf16) / 16-byte (f32) access for y, addend and the ReLU mask
        typedef typename std::conditional<sizeof(T) == 2, uint2, uint4>::type V4;
        T av[4], mv[4], ov[4];
        if (addend) *reinterpret_cast<V4*>(av) = *reinterpret_cast<const V4*>(addend + o);
        if (ex.mask) *reinterpret_cast<V4*>(mv) = *reinterpret_cast<const V4*>(reinterpret_cast<const T*>(ex.mask) + o);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s0[k] += v[k];
            s1[k] += v[k] * v[k];
            v[k] += bv[k];
            if (g.relu) v[k] = fmaxf(v[k], 0.f);
            if (addend) v[k] += to_f<T>(av[k]);
            if (ex.mask && !(to_f<T>(mv[k]) > 0.f)) v[k] = 0.f;
            if (sizeof(T) == 2 && ex.yh) *reinterpret_cast<bf16_t*>(&ov[k]) = f2h_bits(v[k]);
            else ov[k] = from_f<T>(v[k]);
        }
        *reinterpret_cast<V4*>(y + o) = *reinterpret_cast<const V4*>(ov);
    }
    if (stats) {
        float* slot = stats + (int64_t)(blockIdx.y & (SBA_BN_STAT_SLOTS - 1)) * 2 * g.Cout;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            atomicAdd(&slot[c + k], s0[k]);
            atomicAdd(&slot[g.Cout + c + k], s1[k]);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void splitk_finish_kernel(float* __restrict__ ws, T* __restrict__ y,
                                                            const T* __restrict__ addend,
                                                            float* __restrict__ stats, const sba_conv_geom g,
                                                            const int M, const EpiX ex) {
    splitk_finish_body<T>(ws, y, addend, stats, g, M, ex);
}

// the finishing pass of a grouped split-K launch: blockIdx.z = item
__global__ __launch_bounds__(256) void splitk_finish_group_kernel(const GroupArgs A) {
    const GroupItem& it = A.it[blockIdx.z];
    const sba_conv_geom g = it.g;
    splitk_finish_body<bf16_t>(it.ws, it.y, it.addend, nullptr, g, it.M, EpiX{it.bias, it.mask, 0});
}

// ---- tile configurations and their selection --------------------------------------------
struct IgemmCfg { int bm, bn, ks, occ; float eff; bool split; };
// A: big square tile, B: wide-M tile for Cout = 64, C: mid tile, D: small tile (+split-K),
// E: skinny GEMM tile for the 4x4 / 8x8 maps with thousands of channels (+split-K)
// (In-workgroup K groups and three stages of loads in flight were measured on the latency-bound small layers and removed:
// neither beat D -- 1 KB of LDS fragments per MFMA and one wave per SIMD bound them, not the K loop.  A 256x128 tile
// with 128x64 per-wave tiles (less LDS traffic per MFMA, but 4 waves and one workgroup per CU) lost to E everywhere.)
static const IgemmCfg kCfg[5] = {
    {128, 128, 1, 3, 1.00f, false}, {256, 64, 1, 3, 1.00f, false}, {128, 64, 2, 2, 0.80f, false},
    {64, 64, 2, 4, 0.50f, true},    {320, 128, 2, 1, 0.90f, true}};
constexpr int IGEMM_SPLIT_MAX_M = 2048;     // split-K only pays on the GEMM-like maps: M up to this

// ---- the tile table ------------------------------------------------------------------------------------------
// THE table of tile ids (sba_conv_geom.tile, 1..SBA_IGEMM_TILES; row 0 is unused): every dispatch below, the grouped
// launches and sba_conv_igemm_tile_shape read it, nothing else lists the ids.  BM x BN workgroup tile, one wave per
// WM x WN sub-tile.
//   d2        ring depth of the gen-2 form (igemm_dma2_kernel: 64-channel slabs, Cin % 64 == 0 only); 0 = none
//   ks1, d1   slabs per stage and ring depth of the gen-1 form (igemm_dma_kernel: 32-channel slabs), same tile shape;
//             d1 = 0: no gen-1 form (ids >= 13 go back to the rules when Cin % 64 != 0)
//   d2 = d1 = 0 (id 11): the register-staged igemm_kernel with ks1 slabs per stage, whatever Cin is
//   group     0 = no grouped form.  Otherwise sba_conv_igemm_group* takes the id: the gen-2 form of this row when every
//             member has Cin % 64 == 0, else the gen-1 form of row `group` (7 falls back to 5: no 128-wide gen-1 group)
// Even ids 2..10 are the odd id before them with a deeper ring (64..72 KB -> 120..144 KB of LDS: ~100 KB of loads in
// flight per CU; an L2-hit load takes ~1 us under load, so a workgroup alone on its CU moves bytes_in_flight / 1 us,
// measured 36-42 GB/s with 48 KB in flight).  13..15 put the WHOLE batch of a 4x4 map (M = 16 B = 320) in one M tile:
// every weight byte is staged once per M tile, so those weight-streaming layers (4..38 MB of weights against 320..640
// rows) move 1/3..1/5 of the L2->LDS bytes of the 64- / 96-row tiles; 15 is 14 with a 2-stage ring (60 KB: two
// workgroups per CU).  16..18: 256x128 with 128x64 or 64x64 wave tiles.
struct IgemmTile { int bm, bn, wm, wn, d2, ks1, d1, group; };
constexpr IgemmTile kTiles[SBA_IGEMM_TILES + 1] = {
    {},
    {64, 64, 32, 32, 4, 2, 4, 1},       //  1
    {64, 64, 32, 32, 8, 2, 8, 0},       //  2
    {96, 64, 32, 64, 3, 2, 3, 3},       //  3
    {96, 64, 32, 64, 6, 2, 6, 0},       //  4
    {128, 64, 32, 64, 3, 1, 4, 5},      //  5
    {128, 64, 32, 64, 6, 2, 6, 0},      //  6
    {128, 128, 64, 64, 3, 1, 4, 5},     //  7
    {128, 128, 64, 64, 4, 1, 8, 0},     //  8
    {256, 64, 64, 64, 3, 1, 3, 0},      //  9
    {256, 64, 64, 64, 4, 1, 6, 0},      // 10
    {320, 128, 64, 64, 0, 2, 0, 0},     // 11  register-staged (configuration E)
    {96, 128, 32, 128, 5, 1, 8, 0},     // 12
    {320, 64, 64, 64, 3, 0, 0, 0},      // 13  5 waves
    {160, 64, 32, 64, 4, 0, 0, 0},      // 14  5 waves
    {160, 64, 32, 64, 2, 0, 0, 0},      // 15
    {256, 128, 128, 64, 3, 0, 0, 0},    // 16
    {256, 128, 64, 64, 3, 0, 0, 0},     // 17
    {256, 128, 128, 64, 2, 0, 0, 0},    // 18
};

// runtime tile id -> compile-time row: f(std::integral_constant<int, id>) for id in 1..SBA_IGEMM_TILES, else SBA_E_ARG
template <int I = 1, typename F>
static int with_tile(int id, F&& f) {
    if constexpr (I <= SBA_IGEMM_TILES) return id == I ? f(std::integral_constant<int, I>{}) : with_tile<I + 1>(id, f);
    else return SBA_E_ARG;
}

// N-major tile numbering (see igemm_dma2_body) when the weights outweigh the input tensor
static int nmajor_for(const sba_conv_geom& g) {
    const int64_t wb = (int64_t)g.Cout * g.ntaps * g.Cin, xb = (int64_t)g.N * g.IH * g.IW * g.Cin;
    return wb > xb ? 1 : 0;
}

// What launch_body needs to know of a GEMM body: its kernel and tile, SLAB = channels per K slab, KS = slabs per stage
// (a K split is a whole number of stages), XCD = the grid is the XCD-aware one-dimensional tile numbering.
template <typename T, int BM_, int BN_, int WM, int WN, int KS_> struct RegBody {
    static constexpr int BM = BM_, BN = BN_, NT = (BM / WM) * (BN / WN) * 64, SLAB = 64 / (int)sizeof(T), KS = KS_;
    static constexpr bool XCD = false;
    static constexpr auto kernel = igemm_kernel<T, BM, BN, WM, WN, KS>;
};
template <int BM_, int BN_, int WM, int WN, int KS_, int D> struct DmaBody {
    static constexpr int BM = BM_, BN = BN_, NT = (BM / WM) * (BN / WN) * 64, SLAB = 32, KS = KS_;
    static constexpr bool XCD = true;
    static constexpr auto kernel = igemm_dma_kernel<BM, BN, WM, WN, KS, D>;
};
template <int BM_, int BN_, int WM, int WN, int D> struct Dma2Body {
    static constexpr int BM = BM_, BN = BN_, NT = (BM / WM) * (BN / WN) * 64, SLAB = 64, KS = 1;
    static constexpr bool XCD = true;
    static constexpr auto kernel = igemm_dma2_kernel<BM, BN, WM, WN, D>;
};

// the one launcher of the three bodies: the GEMM grid, and the finishing pass behind a split-K launch
template <typename B, typename T>
static int launch_body(const T* xp, const T* wp, T* yp, const T* ap, float* stats, const sba_conv_geom& g, int M,
                       int split, float* ws, hipStream_t st, const EpiX ex) {
    const int nslabs = g.ntaps * (g.Cin / B::SLAB);
    int sps = nslabs;
    if (split > 1) {
        sps = cdiv(cdiv(nslabs, split), B::KS) * B::KS;
        split = cdiv(nslabs, sps);
    }
    float* part = split > 1 ? ws : nullptr;
    const int gx = cdiv(M, B::BM), gy = cdiv(g.Cout, B::BN);
    if constexpr (B::XCD) {
        const int nmajor = nmajor_for(g);
        dim3 grid(nmajor ? 8 * cdiv(gy, 8) * gx : 8 * cdiv(gx, 8) * gy, 1, split);
        SBA_LAUNCH(B::kernel, grid, dim3(B::NT), 0, st, xp, wp, yp, ap, stats, g, M, part, sps, ex, gx, gy,
                   nmajor DMA_TRACE_ARG);
    } else {
        SBA_LAUNCH(B::kernel, dim3(gx, gy, split), dim3(B::NT), 0, st, xp, wp, yp, ap, stats, g, M, part, sps, ex);
    }
    if (split > 1) {
        dim3 fgrid(cdiv(g.Cout / 4, 256), cdiv(M, 8));
        SBA_LAUNCH((splitk_finish_kernel<T>), fgrid, dim3(256), 0, st, ws, yp, ap, stats, g, M, ex);
    }
    return SBA_CHECK_LAUNCH();
}

// ---- halo-tile 3x3 path: which geometries qualify, and its launch
static bool halo_ok(const sba_conv_geom& g) {
    if (g.ntaps != 9 || g.sy != 1 || g.sx != 1 || g.osy != 1 || g.osx != 1 || g.ooy || g.oox) return false;
    // Cin = 128 (data gradient of the ResBlocks' 64 -> 128 conv): the kernel walks the tile once per 64-channel chunk
    if (g.OHs != g.OH || g.OWs != g.OW || (g.Cin != 64 && g.Cin != 128) || g.Cout % 64) return false;
    if (g.OH % 8 || g.OW % 32) return false;
    if (g.ups ? (g.IH * 2 != g.OH || g.IW * 2 != g.OW) : (g.IH != g.OH || g.IW != g.OW)) return false;
    for (int t = 0; t < 9; ++t)
        if (g.ty[t] != t / 3 - 1 || g.tx[t] != t % 3 - 1) return false;
    const int64_t tiles = (int64_t)g.N * (g.OH / 8) * (g.OW / 32);
    return tiles >= 128 && tiles <= 0x7fffffff;
}

// the general register-weight halo kernel (fragment-major weights only): any stride-1 3 x 3 window, ragged maps
static bool halo3g_ok(const sba_conv_geom& g) {
    if (g.w_layout != 1 || g.ups) return false;
    if (g.ntaps != 9 || g.sy != 1 || g.sx != 1 || g.osy != 1 || g.osx != 1 || g.ooy || g.oox) return false;
    if (g.OHs != g.OH || g.OWs != g.OW || g.Cin % 32 || g.Cout % 32) return false;
    int ymin = g.ty[0], ymax = g.ty[0], xmin = g.tx[0], xmax = g.tx[0];
    unsigned seen = 0;
    for (int t = 0; t < 9; ++t) {
        ymin = g.ty[t] < ymin ? g.ty[t] : ymin; ymax = g.ty[t] > ymax ? g.ty[t] : ymax;
        xmin = g.tx[t] < xmin ? g.tx[t] : xmin; xmax = g.tx[t] > xmax ? g.tx[t] : xmax;
    }
    if (ymax - ymin != 2 || xmax - xmin != 2) return false;
    for (int t = 0; t < 9; ++t) seen |= 1u << ((g.ty[t] - ymin) * 3 + (g.tx[t] - xmin));
    if (seen != 0x1ffu) return false;               // the nine taps are the nine cells of the window
    const int64_t tiles = (int64_t)g.N * cdiv(g.OH, 8) * cdiv(g.OW, 32);
    return tiles >= 128 && tiles <= 0x7fffffff;
}

static void launch_halo3g(const sba_conv_geom& g, const bf16_t* x, const bf16_t* w, bf16_t* y, const bf16_t* addend,
                          const EpiX ex, hipStream_t st) {
    const int tiles = g.N * cdiv(g.OH, 8) * cdiv(g.OW, 32);
    const bool tn2 = g.Cout % 64 == 0;
    dim3 grid(tiles, g.Cout / (tn2 ? 64 : 32));
    if (g.Cin % 64 == 0) {
        if (tn2) SBA_LAUNCH((conv3x3_halo3g_kernel<64, 2>), grid, dim3(256), 0, st, x, w, y, addend, g, ex);
        else SBA_LAUNCH((conv3x3_halo3g_kernel<64, 1>), grid, dim3(256), 0, st, x, w, y, addend, g, ex);
    } else {
        if (tn2) SBA_LAUNCH((conv3x3_halo3g_kernel<32, 2>), grid, dim3(256), 0, st, x, w, y, addend, g, ex);
        else SBA_LAUNCH((conv3x3_halo3g_kernel<32, 1>), grid, dim3(256), 0, st, x, w, y, addend, g, ex);
    }
}

static void launch_halo(const sba_conv_geom& g, const bf16_t* x, const bf16_t* w, bf16_t* y, const bf16_t* addend,
                        float* stats, const EpiX ex, hipStream_t st) {
    const int tiles = g.N * (g.OH / 8) * (g.OW / 32);
    // (A persistent variant -- one workgroup per CU, weights resident in LDS, the next tile's halo by LDS-DMA -- measured
    // SLOWER than these per-tile kernels at three workgroups per CU: G3 upBlock 151 vs 113 us, ResBlock 86 vs 80 us; with
    // one wave per SIMD the epilogue of a tile overlaps nothing.  Removed.)
    // BN = 64 for every Cout: the 128-wide variant needs 86 KB of LDS (one workgroup per CU) and
    // measured slower; re-staging the halo tile for the second channel block is cheap
    dim3 grid(tiles, g.Cout / 64);
    if (g.w_layout == 1) {      // fragment-major weights: the register-resident form (geom_ok has checked the layout's needs)
        if (g.ups) SBA_LAUNCH((conv3x3_halo3_kernel<64, 1>), grid, dim3(256), 0, st, x, w, y, addend, stats, g, ex);
        else SBA_LAUNCH((conv3x3_halo3_kernel<64, 0>), grid, dim3(256), 0, st, x, w, y, addend, stats, g, ex);
        return;
    }
    if (g.ups) SBA_LAUNCH((conv3x3_halo_kernel<64, 64, 1>), grid, dim3(256), 0, st, x, w, y, addend, stats, g, ex);
    else SBA_LAUNCH((conv3x3_halo_kernel<64, 64, 0>), grid, dim3(256), 0, st, x, w, y, addend, stats, g, ex);
}

template <typename T>
int launch_igemm(const void* x, const void* w, void* y, const void* addend, float* stats,
                 const sba_conv_geom& g, void* workspace, int64_t ws_bytes, hipStream_t st,
                 const EpiX ex = EpiX{nullptr, nullptr, 0}, int* plan = nullptr) {
    // plan != NULL: do not launch -- report the kernel this geometry goes to: plan[0] = family (0 halo-tile 3x3, 1 LDS-DMA
    // gen 2 (64-channel slabs), 2 LDS-DMA gen 1, 3 register-staged), plan[1] = tile id / configuration, plan[2] = K splits
    const int M = g.N * g.OHs * g.OWs;
    const T* xp = (const T*)x; const T* wp = (const T*)w; T* yp = (T*)y; const T* ap = (const T*)addend;
    // fragment-major weights: the halo-tile kernels only (family 0: the strict form; family 4: the general form)
    if (g.w_layout != 0 && !(g.w_layout == 1 && sizeof(T) == 2 && (halo_ok(g) || halo3g_ok(g)))) return SBA_E_ARG;
    if (sizeof(T) == 2 && g.w_layout == 1 && !halo_ok(g)) {
        if (plan) { plan[0] = 4; plan[1] = g.Cin % 64 == 0 ? 64 : 32; plan[2] = 1; return SBA_OK; }
        if (stats) return SBA_E_ARG;
        launch_halo3g(g, (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, (const bf16_t*)addend, ex, st);
        return SBA_CHECK_LAUNCH();
    }
    if (sizeof(T) == 2 && halo_ok(g)) {
        if (plan) { plan[0] = 0; plan[1] = g.ups ? 1 : 0; plan[2] = 1; return SBA_OK; }
        launch_halo(g, (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, (const bf16_t*)addend, stats, ex, st);
        return SBA_CHECK_LAUNCH();
    }
    const int nslabs = g.ntaps * (g.Cin / (64 / (int)sizeof(T)));
    const bool can_split = workspace && g.Cout % 4 == 0 && (int64_t)M * g.Cout * 4 <= ws_bytes && nslabs >= 16;
    // Rule table calibrated with tools/bench_conv.py on the B=20 layer shapes (profiles/r01_conv_tiles.txt):
    //  - GEMM-like maps (M <= 2048): small tile D with split-K;
    //  - Cout multiple of 128: A when it yields >= 320 workgroups, E (320x128, 10 waves) when it yields
    //    thousands, otherwise the mid tile C;
    //  - narrow Cout (64): B when >= 256 workgroups, otherwise C.
    int best, best_split = 1;
    const int wgA = (g.Cout % 128 == 0) ? cdiv(M, 128) * (g.Cout / 128) : 0;
    if (M <= 2048) {
        best = (g.Cout >= 1024 && (nslabs >= 512 || (M >= 1280 && nslabs >= 256))) ? 4 : 3;
    } else if ((g.Cout == 128 && M >= 40000) || (g.Cout == 256 && M >= 40000 && nslabs >= 48)) {
        best = 4;
    } else if (wgA >= 320) {
        best = 0;
    } else if (g.Cout <= 64 && cdiv(M, 256) >= 256) {
        best = 1;
    } else if (cdiv(M, 128) * cdiv(g.Cout, 64) >= 256) {
        best = 2;
    } else {
        best = 3;       // too few mid tiles to fill the chip: small tiles (+ split-K when K is long)
    }
    {
        const IgemmCfg& k = kCfg[best];
        const int tiles = cdiv(M, k.bm) * cdiv(g.Cout, k.bn);
        const int slots = 256 * k.occ;
        if (k.split && can_split && tiles < slots && M <= IGEMM_SPLIT_MAX_M) {
            int split = slots / tiles;          // floor: one more split than fits leaves a nearly empty second round
            if (split > nslabs / 8) split = nslabs / 8;
            if (split > 32) split = 32;
            if (split > 1) best_split = split;
        }
    }
    const bool det = sba_det_on();      // deterministic mode: no split-K (its partial sums meet in f32 atomics)
    if (det) best_split = 1;
    float* ws = (float*)workspace;
    if constexpr (sizeof(T) == 2) {
        // bf16: the LDS-DMA staged kernels, and the register-staged 320x128 tile (configuration E) as tile 11
        const bf16_t* xb = (const bf16_t*)x; const bf16_t* wb = (const bf16_t*)w; bf16_t* yb = (bf16_t*)y;
        const bf16_t* ab = (const bf16_t*)addend;
        // g.tile: a row of kTiles; the rules name rows 7 / 9 / 5 / 1 / 11 for configurations A / B / C / D / E
        static const int rule_tile[4] = {7, 9, 5, 1};
        int tile = g.tile;
        int split = best_split;
        if (tile <= 0 || tile > SBA_IGEMM_TILES) {
            tile = best <= 3 ? rule_tile[best] : 11;
        } else if (g.ksplit >= 1) {
            split = g.ksplit;
            if (split > 1 && !(workspace && g.Cout % 4 == 0 && (int64_t)M * g.Cout * 4 <= ws_bytes)) split = 1;
            if (split > nslabs / 2) split = nslabs / 2 > 0 ? nslabs / 2 : 1;
        }
        if (det) split = 1;
        if (tile >= 13 && g.Cin % 64 != 0) {       // gen-2 only: back to the rules
            tile = best <= 3 ? rule_tile[best] : 11;
            split = det ? 1 : best_split;
        }
        if (g.Cin % 64 == 0 && tile != 11) {
            // 128-byte rows, fragment double buffering, DMA issue between the MFMAs (igemm_dma2_kernel)
            const int ns64 = nslabs / 2;
            int sp = split;
            if (sp > ns64 / 2) sp = ns64 / 2 > 0 ? ns64 / 2 : 1;
            if (plan) { plan[0] = 1; plan[1] = tile; plan[2] = sp; return SBA_OK; }
            return with_tile(tile, [&](auto id) {
                constexpr IgemmTile t = kTiles[decltype(id)::value];
                if constexpr (t.d2 > 0)
                    return launch_body<Dma2Body<t.bm, t.bn, t.wm, t.wn, t.d2>>(xb, wb, yb, ab, stats, g, M, sp, ws, st, ex);
                else return SBA_E_ARG;
            });
        }
        if (tile != 11) {       // (ids >= 13 never get here: they went back to the rules above)
            if (plan) { plan[0] = 2; plan[1] = tile; plan[2] = split; return SBA_OK; }
            return with_tile(tile, [&](auto id) {
                constexpr IgemmTile t = kTiles[decltype(id)::value];
                if constexpr (t.d1 > 0)
                    return launch_body<DmaBody<t.bm, t.bn, t.wm, t.wn, t.ks1, t.d1>>(xb, wb, yb, ab, stats, g, M, split, ws, st, ex);
                else return SBA_E_ARG;
            });
        }
        // tile 11: the register-staged 320x128 tile (configuration E)
        if (plan) { plan[0] = 3; plan[1] = 4; plan[2] = split; return SBA_OK; }
        constexpr IgemmTile e = kTiles[11];
        return launch_body<RegBody<T, e.bm, e.bn, e.wm, e.wn, e.ks1>>(xp, wp, yp, ap, stats, g, M, split, ws, st, ex);
    } else {
        if (plan) { plan[0] = 3; plan[1] = best; plan[2] = best_split; return SBA_OK; }
        switch (best) {
            case 0: return launch_body<RegBody<T, 128, 128, 64, 64, 1>>(xp, wp, yp, ap, stats, g, M, best_split, ws, st, ex);
            case 1: return launch_body<RegBody<T, 256, 64, 64, 64, 1>>(xp, wp, yp, ap, stats, g, M, best_split, ws, st, ex);
            case 2: return launch_body<RegBody<T, 128, 64, 32, 64, 2>>(xp, wp, yp, ap, stats, g, M, best_split, ws, st, ex);
            case 3: return launch_body<RegBody<T, 64, 64, 32, 32, 2>>(xp, wp, yp, ap, stats, g, M, best_split, ws, st, ex);
            default: return launch_body<RegBody<T, 320, 128, 64, 64, 2>>(xp, wp, yp, ap, stats, g, M, best_split, ws, st, ex);
        }
    }
}

// the launch writes every pixel and channel of a dense [N*OH*OW][Cout] tensor
bool dense_output(const sba_conv_geom& g) {
    return g.OHs == g.OH && g.OWs == g.OW && g.osy == 1 && g.osx == 1 && g.ooy == 0 && g.oox == 0 &&
           (g.y_cstride == 0 || g.y_cstride == g.Cout) && g.y_coff == 0;
}

// ---- inference: conv + folded BatchNorm(eval) + GLU in one launch ----------------------------------------------
// Kernel choice for sba_conv_igemm_glu.  plan[0] = family: 0 the halo-tile kernels (plan[1] = 0 / 1: plain / behind the
// nearest x2 upsample; +2 with fragment-major weights = conv3x3_halo3_kernel), 3 the register-staged igemm_kernel
// (plan[1] = configuration: 0 128x128, 1 256x64, 2 128x64, 5 the two-wave 64x64 tile).  Every configuration gives a
// wave 64 packed columns (one value granule + its gate granule).
// NO split-K in this path (plan[2] = 1 always): the partial sums of a split meet in the f32 workspace and the GLU would
// have to move into the finishing pass, i.e. a second launch over the 2C-channel tensor -- the traffic this path exists
// to remove.  The shape that decided it: the first upBlock (512 -> 2 x 256 at 8 x 8, B = 20: M = 1280, 144 K slabs) is
// 160 workgroups of the 64x64 tile and ~1 % of the generator's forward time; the generator's large layers never split.
template <typename T>
int launch_igemm_glu(const void* x, const void* w, void* y, const sba_conv_geom& g, hipStream_t st, const EpiX ex,
                     int* plan = nullptr) {
    const int M = g.N * g.OHs * g.OWs;
    const T* xp = (const T*)x; const T* wp = (const T*)w; T* yp = (T*)y;
    if (g.w_layout != 0 && !(g.w_layout == 1 && sizeof(T) == 2 && halo_ok(g))) return SBA_E_ARG;
    if constexpr (sizeof(T) == 2) {
        if (halo_ok(g)) {
            if (plan) { plan[0] = 0; plan[1] = (g.ups ? 1 : 0) + (g.w_layout == 1 ? 2 : 0); plan[2] = 1; return SBA_OK; }
            dim3 grid(g.N * (g.OH / 8) * (g.OW / 32), g.Cout / 64);
            const bf16_t* np = nullptr;
            if (g.w_layout == 1) {
                if (g.ups) SBA_LAUNCH((conv3x3_halo3_kernel<64, 1, 1>), grid, dim3(256), 0, st, xp, wp, yp, np, (float*)nullptr, g, ex);
                else SBA_LAUNCH((conv3x3_halo3_kernel<64, 0, 1>), grid, dim3(256), 0, st, xp, wp, yp, np, (float*)nullptr, g, ex);
            } else {
                if (g.ups) SBA_LAUNCH((conv3x3_halo_kernel<64, 64, 1, 1>), grid, dim3(256), 0, st, xp, wp, yp, np, (float*)nullptr, g, ex);
                else SBA_LAUNCH((conv3x3_halo_kernel<64, 64, 0, 1>), grid, dim3(256), 0, st, xp, wp, yp, np, (float*)nullptr, g, ex);
            }
            return SBA_CHECK_LAUNCH();
        }
    }
    const int nslabs = g.ntaps * (g.Cin / (64 / (int)sizeof(T)));
    int cfg;
    if (g.Cout % 128 == 0 && cdiv(M, 128) * (g.Cout / 128) >= 320) cfg = 0;
    else if (cdiv(M, 256) * (g.Cout / 64) >= 256) cfg = 1;
    else if (cdiv(M, 128) * (g.Cout / 64) >= 256) cfg = 2;
    else cfg = 5;
    if (plan) { plan[0] = 3; plan[1] = cfg; plan[2] = 1; return SBA_OK; }
    const T* np = nullptr;
    float* nf = nullptr;
    switch (cfg) {
        case 0:
            SBA_LAUNCH((igemm_kernel<T, 128, 128, 64, 64, 1, 1>), dim3(cdiv(M, 128), g.Cout / 128), dim3(256), 0, st, xp, wp,
                       yp, np, nf, g, M, nf, nslabs, ex);
            break;
        case 1:
            SBA_LAUNCH((igemm_kernel<T, 256, 64, 64, 64, 1, 1>), dim3(cdiv(M, 256), g.Cout / 64), dim3(256), 0, st, xp, wp,
                       yp, np, nf, g, M, nf, nslabs, ex);
            break;
        case 2:
            SBA_LAUNCH((igemm_kernel<T, 128, 64, 32, 64, 2, 1>), dim3(cdiv(M, 128), g.Cout / 64), dim3(256), 0, st, xp, wp,
                       yp, np, nf, g, M, nf, nslabs, ex);
            break;
        default:
            SBA_LAUNCH((igemm_kernel<T, 64, 64, 32, 64, 2, 1>), dim3(cdiv(M, 64), g.Cout / 64), dim3(128), 0, st, xp, wp,
                       yp, np, nf, g, M, nf, nslabs, ex);
            break;
    }
    return SBA_CHECK_LAUNCH();
}

// argument check shared by sba_conv_igemm_glu and its plan query; *out = the geometry the kernels get
bool glu_geom(int dtype, const sba_conv_geom* g, int C, sba_conv_geom* out) {
    if (!g || C <= 0 || g->Cout != 64 * ((C + 31) / 32)) return false;     // packed rows: 64 per 32 output channels
    if (g->y_cstride != 0 || g->y_coff != 0 || g->relu) return false;       // dense C-channel output
    if (dtype == SBA_BF16 && C % 8) return false;                           // 16-byte row stores
    if (!geom_ok(g, dtype)) return false;
    if (g->OHs != g->OH || g->OWs != g->OW) return false;
    *out = *g;
    out->y_cstride = C;
    return true;
}

}  // namespace

extern "C" int sba_conv_igemm_glu(int dtype, const void* x, const void* w, const float* bias, void* y, int C,
                                  const sba_conv_geom* g, void* stream) {
    sba_conv_geom gg;
    if (!x || !w || !bias || !y || !glu_geom(dtype, g, C, &gg)) return SBA_E_ARG;
    SBA_DISPATCH(dtype, return launch_igemm_glu<T>(x, w, y, gg, (hipStream_t)stream, EpiX{bias, nullptr, 0, C}));
    return SBA_E_ARG;
}

extern "C" int sba_conv_igemm_glu_plan(int dtype, const sba_conv_geom* g, int C, int* plan) {
    sba_conv_geom gg;
    if (!plan || !glu_geom(dtype, g, C, &gg)) return SBA_E_ARG;
    SBA_DISPATCH(dtype, return launch_igemm_glu<T>(nullptr, nullptr, nullptr, gg, nullptr, EpiX{nullptr, nullptr, 0, C}, plan));
    return SBA_E_ARG;
}

extern "C" int sba_conv_igemm(int dtype, const void* x, const void* w, void* y, const void* addend,
                              float* stats, const sba_conv_geom* g, void* workspace, int64_t workspace_bytes,
                              void* stream) {
    if (dtype == SBA_BF16_YH) {
        // bf16 operands, y stored as binary16 (the pre-BatchNorm tensor: include/sbagan_hip.h)
        if (!x || !w || !y || !geom_ok(g, SBA_BF16) || addend || g->relu || g->Cout % 8) return SBA_E_ARG;
        if (((uintptr_t)workspace & 15) != 0) return SBA_E_ARG;
        const EpiX ex{nullptr, nullptr, 1};
        if (sba_det_on() && stats) {
            if (!dense_output(*g)) return SBA_E_ARG;
            const int rc = launch_igemm<bf16_t>(x, w, y, nullptr, nullptr, *g, workspace, workspace_bytes, (hipStream_t)stream, ex);
            if (rc != SBA_OK) return rc;
            return sba_bn_stats(dtype, y, stats, (int64_t)g->N * g->OH * g->OW, 1, g->Cout, stream);
        }
        return launch_igemm<bf16_t>(x, w, y, nullptr, stats, *g, workspace, workspace_bytes, (hipStream_t)stream, ex);
    }
    if (!x || !w || !y || !geom_ok(g, dtype)) return SBA_E_ARG;
    if (((uintptr_t)workspace & 15) != 0) return SBA_E_ARG;
    if (sba_det_on() && stats) {
        // deterministic mode: the epilogue's statistics meet in f32 atomics (LDS and global); take them from the
        // stored tensor with the ordered bn_stats pass instead (needs a dense output: it is one BatchNorm batch)
        if (!dense_output(*g) || addend) return SBA_E_ARG;
        int rc = SBA_E_ARG;
        SBA_DISPATCH(dtype, rc = launch_igemm<T>(x, w, y, addend, nullptr, *g, workspace, workspace_bytes,
                                                 (hipStream_t)stream));
        if (rc != SBA_OK) return rc;
        return sba_bn_stats(dtype, y, stats, (int64_t)g->N * g->OH * g->OW, 1, g->Cout, stream);
    }
    SBA_DISPATCH(dtype, return launch_igemm<T>(x, w, y, addend, stats, *g, workspace, workspace_bytes,
                                               (hipStream_t)stream));
    return SBA_E_ARG;
}

extern "C" int sba_conv_igemm_bias(int dtype, const void* x, const void* w, void* y, const void* addend,
                                   float* stats, const float* bias, const void* relu_mask,
                                   const sba_conv_geom* g, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!x || !w || !y || !geom_ok(g, dtype)) return SBA_E_ARG;
    if (((uintptr_t)workspace & 15) != 0) return SBA_E_ARG;
    if (sba_det_on() && stats) return SBA_E_ARG;        // (no caller asks for statistics behind a bias / ReLU epilogue)
    SBA_DISPATCH(dtype, return launch_igemm<T>(x, w, y, addend, stats, *g, workspace, workspace_bytes,
                                               (hipStream_t)stream, EpiX{bias, relu_mask, 0}));
    return SBA_E_ARG;
}

extern "C" int sba_conv_igemm_plan(int dtype, const sba_conv_geom* g, int64_t workspace_bytes, int* plan) {
    if (!plan || (dtype != SBA_F32 && dtype != SBA_BF16) || !geom_ok(g, dtype)) return SBA_E_ARG;
    static char dummy_ws[16];
    void* ws = workspace_bytes > 0 ? (void*)dummy_ws : nullptr;       // (only its presence and size enter the decision)
    if (dtype == SBA_F32) return launch_igemm<float>(nullptr, nullptr, nullptr, nullptr, nullptr, *g, ws, workspace_bytes,
                                                     nullptr, EpiX{nullptr, nullptr, 0}, plan);
    return launch_igemm<bf16_t>(nullptr, nullptr, nullptr, nullptr, nullptr, *g, ws, workspace_bytes, nullptr,
                                EpiX{nullptr, nullptr, 0}, plan);
}

template <int BM, int BN, int WM, int WN, int D, int KS = 0>
static int launch_group(const sba_conv_group_item* items, int n, hipStream_t st, int split = 1, float* ws = nullptr) {
    GroupArgs A;
    A.n = n;
    A.sps = 0;
    int tiles = 0, max_m = 0, max_co = 0, ns64 = 0;
    for (int i = 0; i < n; ++i) {
        const sba_conv_geom& g = *items[i].g;
        GroupItem& it = A.it[i];
        it.x = (const bf16_t*)items[i].x; it.w = (const bf16_t*)items[i].w; it.y = (bf16_t*)items[i].y;
        it.addend = (const bf16_t*)items[i].addend; it.bias = items[i].bias; it.mask = items[i].relu_mask;
        it.g = g;
        it.M = g.N * g.OHs * g.OWs;
        it.gx = cdiv(it.M, BM);
        it.gy = cdiv(g.Cout, BN);
        it.nmajor = nmajor_for(g);
        it.pad = 0;
        it.ws = nullptr;
        it.tile_begin = tiles;
        tiles += it.nmajor ? 8 * cdiv(it.gy, 8) * it.gx : 8 * cdiv(it.gx, 8) * it.gy;
        if (it.M > max_m) max_m = it.M;
        if (g.Cout > max_co) max_co = g.Cout;
        const int k = g.ntaps * (g.Cin / 64);
        if (k > ns64) ns64 = k;
    }
    if (split > 1 && KS == 0 && ws) {
        // every item is cut into the same number of K splits (slabs per split from the longest K); item i adds its
        // partial sums into its own [M][Cout] f32 slice of the zero-filled workspace
        A.sps = cdiv(ns64, split);
        split = cdiv(ns64, A.sps);
        float* p = ws;
        for (int i = 0; i < n; ++i) { A.it[i].ws = p; p += (int64_t)A.it[i].M * A.it[i].g.Cout; }
        if (split <= 1) { A.sps = 0; split = 1; }
    } else {
        split = 1;
    }
    for (int i = n; i < SBA_GROUP_MAX; ++i) A.it[i] = A.it[0];
    constexpr int NT = (BM / WM) * (BN / WN) * 64;
    if (KS == 0) SBA_LAUNCH((igemm_dma2_group_kernel<BM, BN, WM, WN, D>), dim3(tiles, 1, split), dim3(NT), 0, st, A DMA_TRACE_ARG);
    else SBA_LAUNCH((igemm_dma_group_kernel<BM, BN, WM, WN, (KS ? KS : 1), D>), dim3(tiles), dim3(NT), 0, st, A DMA_TRACE_ARG);
    if (A.sps) {
        dim3 fgrid(cdiv(max_co / 4, 256), cdiv(max_m, 8), n);
        SBA_LAUNCH(splitk_finish_group_kernel, fgrid, dim3(256), 0, st, A);
    }
    return SBA_CHECK_LAUNCH();
}

static int group_dispatch(int dtype, int n, const sba_conv_group_item* items, int tile, int ksplit, void* workspace,
                          int64_t ws_bytes, hipStream_t st) {
    if (dtype != SBA_BF16 || !items || n < 1 || n > SBA_GROUP_MAX) return SBA_E_ARG;
    bool all64 = true;
    int64_t need = 0;
    for (int i = 0; i < n; ++i) {
        const sba_conv_group_item& it = items[i];
        if (!it.x || !it.w || !it.y || !geom_ok(it.g, dtype)) return SBA_E_ARG;     // (geom_ok: Cin % 32 == 0)
        all64 = all64 && it.g->Cin % 64 == 0;
        need += (int64_t)it.g->N * it.g->OHs * it.g->OWs * it.g->Cout * 4;
        if (ksplit > 1 && it.g->Cout % 4) ksplit = 1;
    }
    if (ksplit > 1 && (!workspace || need > ws_bytes || ((uintptr_t)workspace & 15) || !all64 || sba_det_on())) ksplit = 1;
    if (ksplit < 1) ksplit = 1;
    float* ws = (float*)workspace;
    return with_tile(tile ? tile : 1, [&](auto id) {
        constexpr IgemmTile t = kTiles[decltype(id)::value], m = kTiles[t.group];
        if constexpr (t.group == 0) return SBA_E_ARG;
        // 64-channel slabs, second-generation body; some member with Cin % 64 == 32: 32-channel slabs for the whole group
        else return all64 ? launch_group<t.bm, t.bn, t.wm, t.wn, t.d2>(items, n, st, ksplit, ws)
                          : launch_group<m.bm, m.bn, m.wm, m.wn, m.d1, m.ks1>(items, n, st);
    });
}

extern "C" int sba_conv_igemm_tile_shape(int tile, int* bm, int* bn) {
    if (tile < 1 || tile > SBA_IGEMM_TILES || !bm || !bn) return SBA_E_ARG;
    *bm = kTiles[tile].bm;
    *bn = kTiles[tile].bn;
    return SBA_OK;
}

extern "C" int sba_conv_igemm_group(int dtype, int n, const sba_conv_group_item* items, int tile, void* stream) {
    return group_dispatch(dtype, n, items, tile, 1, nullptr, 0, (hipStream_t)stream);
}

extern "C" int sba_conv_igemm_group_splitk(int dtype, int n, const sba_conv_group_item* items, int tile, int ksplit,
                                           void* workspace, int64_t workspace_bytes, void* stream) {
    return group_dispatch(dtype, n, items, tile, ksplit, workspace, workspace_bytes, (hipStream_t)stream);
}
