// Weight gradients of the implicit-GEMM convolutions for gfx950 (MI355X): sba_conv_wgrad and its kernels.
// dw[co][tap][ci] (f32) from NHWC x and dy; the forward / data-gradient path is in igemm.hip.
#include "common.h"
#include "conv_common.h"

namespace {

// Division of a pixel index (< 2^21) by a launch-constant: one 64-bit multiply instead of the
// ~30-instruction integer division sequence (the weight-gradient kernels decode (n, oy, ox) for
// every staged pixel, which made address generation their bottleneck).
struct FastDiv {
    uint64_t magic;     // ceil(2^42 / d), 0 = use the plain division
    uint32_t d;
};
static inline FastDiv make_fastdiv(uint32_t d, int64_t max_n) {
    FastDiv f;
    f.d = d;
    f.magic = (max_n < (1 << 21) && d > 0) ? (((uint64_t)1 << 42) + d - 1) / d : 0;
    return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
    return f.magic ? (uint32_t)(((uint64_t)n * f.magic) >> 42) : n / f.d;
}

// ---------------------------------------------------------------------------
// Head and tail shared by the kernels below.  (The tap lookup, the buffer-resource setup and the ring driver of the two
// LDS-DMA kernels, and the epilogue of wgrad_row_dma_kernel stay written out in their kernels: as helpers they changed
// the kernels' VGPR / SGPR counts -- profiles/wgrad_plan_refactor.txt.)
// ---------------------------------------------------------------------------
__device__ __forceinline__ void zero_acc(f32x16_t (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}
template <int N> __device__ __forceinline__ void zero_acc(f32x16_t (&acc)[N][2][2]) {
#pragma unroll
    for (int s = 0; s < N; ++s) zero_acc(acc[s]);
}

// output pixel m -> (n, oy, ox) on a map of `sub` = rows x `ow` pixels per image
__device__ __forceinline__ void pixel_decode(const int m, const int sub, const int ow, const FastDiv& dsub, const FastDiv& dow,
                                             int& n, int& oy, int& ox) {
    n = (int)fdiv(m, dsub);
    const int rem = m - n * sub;
    oy = (int)fdiv(rem, dow);
    ox = rem - oy * ow;
}

// the input pixel tap (ty, tx) of output pixel (n, oy, ox) reads: false = padding; IHL x IWL = the map the taps walk on
// (the upsampled one behind a nearest x2 upsample)
__device__ __forceinline__ bool x_gather(const sba_conv_geom& g, const int IHL, const int IWL, const int n, const int oy, const int ox,
                                         const int ty, const int tx, int64_t& pix) {
    int iy = oy * g.sy + ty, ix = ox * g.sx + tx;
    const bool ok = (iy >= 0) & (iy < IHL) & (ix >= 0) & (ix < IWL);
    if (g.ups) { iy >>= 1; ix >>= 1; }
    pix = (int64_t)(n * g.IH + iy) * g.IW + ix;
    return ok;
}
__device__ __forceinline__ int64_t dy_pixel(const sba_conv_geom& g, const int n, const int oy, const int ox) {
    return (int64_t)(n * g.OH + oy * g.osy + g.ooy) * g.OW + ox * g.osx + g.oox;
}

// one element of dw: mode 0 = +=, 1 = f32 atomic (pixel splits), 2 = store (first write of a cleared gradient, or a
// deterministic-mode partial tensor)
__device__ __forceinline__ void dw_emit(float* p, const float v, const int mode) {
    if (mode == 1) atomicAdd(p, v);
    else if (mode == 2) *p = v;
    else *p += v;
}
// a wave's 64(co) x 64(ci) accumulator tile of tap `tap` -> dwz[co][tap][ci]
// (OWNER = false: wgrad_rows_kernel, whose waves never own dw -- atomics or store only)
template <bool OWNER>
__device__ __forceinline__ void store_tile(const f32x16_t (&acc)[2][2], float* dwz, const sba_conv_geom& g, const int co0,
                                           const int ci0, const int tap, const int mode, const int lane) {
    const int col_l = lane & 31, rsel = 4 * (lane >> 5);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + i * 32 + (r & 3) + 8 * (r >> 2) + rsel;
                const int ci = ci0 + j * 32 + col_l;
                if (co < g.Cout && ci < g.Cin) {
                    float* p = dwz + ((int64_t)co * g.ntaps + tap) * g.Cin + ci;
                    if (OWNER) dw_emit(p, acc[i][j][r], mode);
                    else if (mode == 2) *p = acc[i][j][r];
                    else atomicAdd(p, acc[i][j][r]);
                }
            }
}

// ---------------------------------------------------------------------------
// weight gradient: dw[co][tap][ci] += sum_pixels dy[pixel][co] * x[gather(pixel,tap)][ci]
// Workgroup = one 64(co) x 64(ci) tile of one tap; its 4 waves each walk their
// own 16-pixel slices of the workgroup's pixel range, then reduce through LDS.
// Both operands are pixel-major in memory; the MFMA wants 8 consecutive
// pixels per lane, so bf16 fragments are read with ds_read_b64_tr_b16 (4
// pixels x 16 channels transposed per 16-lane group); f32 fragments are single
// elements and need no transpose.
// ---------------------------------------------------------------------------
template <typename T> struct WgFrag;

template <> struct WgFrag<bf16_t> {
    static constexpr int ROWS = 64 * 2 + 64;   // bytes per pixel row: 128 data + 64 pad (bank spread)
    // fragment of channels [c32, c32+32) over pixels [0,16) of a slice
    static __device__ __forceinline__ bf16x8_t load(const unsigned char* slice, int c32, int lane) {
        const int g16 = lane >> 4, i16 = lane & 15;
        const int cbase = c32 + 16 * (g16 & 1), kbase = 8 * (g16 >> 1);
        const int q = i16 >> 2, p = i16 & 3;
        const unsigned char* a0 = slice + (kbase + q) * ROWS + (cbase + 4 * p) * 2;
        typedef __attribute__((address_space(3))) s16x4_t* lptr;
        s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)(a0));
        s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)(a0 + 4 * ROWS));
        bf16x8_t r;
        r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
        r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
        return r;
    }
    static __device__ __forceinline__ void mma(const unsigned char* sa, const unsigned char* sb, int lane,
                                               f32x16_t (&acc)[2][2]) {
        bf16x8_t a[2], b[2];
        a[0] = load(sa, 0, lane); a[1] = load(sa, 32, lane);
        b[0] = load(sb, 0, lane); b[1] = load(sb, 32, lane);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
};

template <> struct WgFrag<float> {
    static constexpr int ROWS = 64 * 4 + 64;
    static __device__ __forceinline__ void mma(const unsigned char* sa, const unsigned char* sb, int lane,
                                               f32x16_t (&acc)[2][2]) {
        const int r = lane & 31, h = lane >> 5;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = *reinterpret_cast<const float*>(sa + (2 * kk + h) * ROWS + (i * 32 + r) * 4);
                b[i] = *reinterpret_cast<const float*>(sb + (2 * kk + h) * ROWS + (i * 32 + r) * 4);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
};

template <typename T>
__global__ __launch_bounds__(256) void wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                    float* __restrict__ dw, const sba_conv_geom g,
                                                    const int M, const int chunks_per_split,
                                                    const int mode, const FastDiv dsub, const FastDiv dow,
                                                    const int64_t zstride) {
    constexpr int ROWS = WgFrag<T>::ROWS;
    constexpr int CH = 16 / (int)sizeof(T);          // elements per 16-byte chunk
    constexpr int CPR = 64 / CH;                     // chunks per 64-channel pixel row
    constexpr int LPT = 16 * CPR / 64;               // 16-byte loads per lane per slice
    constexpr int SLICE = 16 * ROWS;
    static_assert(4 * 2 * SLICE >= 64 * 64 * 4, "reduction buffer fits in the staging area");
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * 2 * SLICE];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int co0 = blockIdx.x * 64;
    const int ci_tiles = (g.Cin + 63) / 64;
    const int tap = blockIdx.y / ci_tiles, ci0 = (blockIdx.y - tap * ci_tiles) * 64;
    int ty = 0, tx = 0;
#pragma unroll
    for (int t = 0; t < SBA_MAX_TAPS; ++t)
        if (t == tap) { ty = g.ty[t]; tx = g.tx[t]; }
    const int IHL = g.ups ? 2 * g.IH : g.IH, IWL = g.ups ? 2 * g.IW : g.IW;
    const int sub = g.OHs * g.OWs;

    unsigned char* sa = lds + wid * 2 * SLICE;
    unsigned char* sb = sa + SLICE;

    f32x16_t acc[2][2];
    zero_acc(acc);

    const int chunk_lo = blockIdx.z * chunks_per_split;
    const int total_chunks = (M + 63) / 64;
    const int chunk_hi = min(chunk_lo + chunks_per_split, total_chunks);

    uint4 va[LPT], vb[LPT];
    auto gload = [&](int ck) {
        const int m0 = ck * 64 + wid * 16;          // this wave's 16 pixels
#pragma unroll
        for (int u = 0; u < LPT; ++u) {
            const int idx = lane + 64 * u;
            const int pix = idx / CPR, cc = idx - pix * CPR;
            const int m = m0 + pix;
            va[u] = make_uint4(0, 0, 0, 0);
            vb[u] = make_uint4(0, 0, 0, 0);
            if (m < M) {
                int n, oy, ox;
                pixel_decode(m, sub, g.OWs, dsub, dow, n, oy, ox);
                const int co = co0 + cc * CH;
                if (co < g.Cout) va[u] = *reinterpret_cast<const uint4*>(dy + dy_pixel(g, n, oy, ox) * g.Cout + co);
                int64_t pi;
                const bool ok = x_gather(g, IHL, IWL, n, oy, ox, ty, tx, pi);
                const int ci = ci0 + cc * CH;
                if (ok && ci < g.Cin) vb[u] = *reinterpret_cast<const uint4*>(x + pi * g.Cin + ci);
            }
        }
    };
    if (chunk_lo < chunk_hi) gload(chunk_lo);
    for (int ck = chunk_lo; ck < chunk_hi; ++ck) {
        __syncthreads();    // previous slice fully consumed by this wave's MFMA reads
#pragma unroll
        for (int u = 0; u < LPT; ++u) {
            const int idx = lane + 64 * u;
            const int pix = idx / CPR, cc = idx - pix * CPR;
            *reinterpret_cast<uint4*>(sa + pix * ROWS + cc * 16) = va[u];
            *reinterpret_cast<uint4*>(sb + pix * ROWS + cc * 16) = vb[u];
        }
        __syncthreads();
        if (ck + 1 < chunk_hi) gload(ck + 1);     // next chunk's loads fly under this chunk's MFMAs
        WgFrag<T>::mma(sa, sb, lane, acc);
    }

    // cross-wave reduction through LDS, wave by wave (a fixed order: no LDS atomics), then one add per element
    __syncthreads();
    float* red = reinterpret_cast<float*>(lds);
    const int col_l = lane & 31, rsel = 4 * (lane >> 5);
#pragma unroll 1
    for (int wv = 0; wv < 4; ++wv) {
        if (wid == wv) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = i * 32 + (r & 3) + 8 * (r >> 2) + rsel;   // co
                        float* q = &red[row * 64 + j * 32 + col_l];
                        *q = wv == 0 ? acc[i][j][r] : *q + acc[i][j][r];
                    }
        }
        __syncthreads();
    }
    float* dwz = dw + (int64_t)blockIdx.z * zstride;    // deterministic mode: this pixel split's own partial tensor
    for (int i = tid; i < 64 * 64; i += 256) {
        const int co = co0 + (i >> 6), ci = ci0 + (i & 63);
        if (co < g.Cout && ci < g.Cin) {
            dw_emit(dwz + ((int64_t)co * g.ntaps + tap) * g.Cin + ci, red[i], mode);
        }
    }
}

// ---------------------------------------------------------------------------
// weight gradient, small-pixel-count regime (GEMM-like layers at 4x4 / 8x8 maps with
// thousands of channels): every wave owns its own 64(co) x 64(ci) tile of one tap and walks
// ALL pixels of the block's range, so there is no cross-wave reduction; the four waves of a
// workgroup share the dy slice (same co tile) and differ in (tap, ci tile).  (Two co tiles per wave against the
// same x slice, 0.375 instead of 0.625 KB of operands per MFMA: measured 20-35 % SLOWER at 4 waves per SIMD, removed.)
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256, 2) void wgrad_small_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                          float* __restrict__ dw, const sba_conv_geom g,
                                                          const int M, const int chunks_per_split,
                                                          const int mode, const FastDiv dsub,
                                                          const FastDiv dow, const int64_t zstride) {
    constexpr int ROWS = WgFrag<T>::ROWS;
    constexpr int CH = 16 / (int)sizeof(T);
    constexpr int CPR = 64 / CH;
    constexpr int LPT = 16 * CPR / 64;               // 16-byte loads per lane for a wave-private slice
    constexpr int APT = (16 * CPR + 255) / 256;      // 16-byte loads per thread for the shared dy slice
    constexpr int SLICE = 16 * ROWS;
    __shared__ __attribute__((aligned(16))) unsigned char lds[5 * SLICE];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int co0 = blockIdx.x * 64;
    const int ci_tiles = (g.Cin + 63) / 64;
    const int item = blockIdx.y * 4 + wid;
    const bool active = item < g.ntaps * ci_tiles;
    const int tap = active ? item / ci_tiles : 0;
    const int ci0 = active ? (item - tap * ci_tiles) * 64 : 0;
    int ty = 0, tx = 0;
#pragma unroll
    for (int t = 0; t < SBA_MAX_TAPS; ++t)
        if (t == tap) { ty = g.ty[t]; tx = g.tx[t]; }
    const int IHL = g.ups ? 2 * g.IH : g.IH, IWL = g.ups ? 2 * g.IW : g.IW;
    const int sub = g.OHs * g.OWs;

    unsigned char* sa = lds;
    unsigned char* sb = lds + (1 + wid) * SLICE;

    f32x16_t acc[2][2];
    zero_acc(acc);

    const int total_chunks = (M + 15) / 16;
    const int chunk_lo = blockIdx.z * chunks_per_split;
    const int chunk_hi = min(chunk_lo + chunks_per_split, total_chunks);

    uint4 va[APT], vb[LPT];
    auto gload = [&](int ck) {
        const int m0 = ck * 16;
#pragma unroll
        for (int u = 0; u < APT; ++u) {
            const int idx = tid + 256 * u;
            va[u] = make_uint4(0, 0, 0, 0);
            if (idx < 16 * CPR) {
                const int pix = idx / CPR, cc = idx - pix * CPR;
                const int m = m0 + pix, co = co0 + cc * CH;
                if (m < M && co < g.Cout) {
                    int n, oy, ox;
                    pixel_decode(m, sub, g.OWs, dsub, dow, n, oy, ox);
                    va[u] = *reinterpret_cast<const uint4*>(dy + dy_pixel(g, n, oy, ox) * g.Cout + co);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < LPT; ++u) {
            const int idx = lane + 64 * u;
            const int pix = idx / CPR, cc = idx - pix * CPR;
            const int m = m0 + pix;
            vb[u] = make_uint4(0, 0, 0, 0);
            if (active && m < M) {
                int n, oy, ox;
                pixel_decode(m, sub, g.OWs, dsub, dow, n, oy, ox);
                int64_t pi;
                const bool ok = x_gather(g, IHL, IWL, n, oy, ox, ty, tx, pi);
                const int ci = ci0 + cc * CH;
                if (ok && ci < g.Cin) vb[u] = *reinterpret_cast<const uint4*>(x + pi * g.Cin + ci);
            }
        }
    };
    if (chunk_lo < chunk_hi) gload(chunk_lo);
    for (int ck = chunk_lo; ck < chunk_hi; ++ck) {
        __syncthreads();          // everyone is done reading the previous slices
#pragma unroll
        for (int u = 0; u < APT; ++u) {
            const int idx = tid + 256 * u;
            if (idx < 16 * CPR) {
                const int pix = idx / CPR, cc = idx - pix * CPR;
                *reinterpret_cast<uint4*>(sa + pix * ROWS + cc * 16) = va[u];
            }
        }
#pragma unroll
        for (int u = 0; u < LPT; ++u) {
            const int idx = lane + 64 * u;
            const int pix = idx / CPR, cc = idx - pix * CPR;
            *reinterpret_cast<uint4*>(sb + pix * ROWS + cc * 16) = vb[u];
        }
        __syncthreads();
        if (ck + 1 < chunk_hi) gload(ck + 1);
        WgFrag<T>::mma(sa, sb, lane, acc);
    }

    if (!active) return;
    store_tile<true>(acc, dw + (int64_t)blockIdx.z * zstride, g, co0, ci0, tap, mode, lane);
}

// ---------------------------------------------------------------------------
// The same decomposition (one 64 x 64 tile of one tap per wave, the workgroup's waves share the dy slices) fed by
// LDS-DMA through a D-deep ring instead of register staging.  The register-staged kernel above prefetches ONE
// 16-pixel chunk (four MFMAs, ~0.1 us) ahead of an L2 round trip of ~1 us, so every chunk costs a full memory
// latency: 320 pixels = 20 chunks ~ 30 us per workgroup whatever the MFMA work is.  Here a stage is 32 pixels
// (two MFMA k-steps): per wave four 1 KB DMA instructions for its own x slice (the im2col gather is the per-lane
// address) and CT for its share of the dy slices; D - 1 stages are in flight, completion is counted with
// s_waitcnt vmcnt + one workgroup barrier per stage, exactly like igemm_dma_kernel of igemm.hip.  Rows are 128 bytes (64
// channels, no padding: the DMA writes lane l at M0 + 16 l); the 16-byte chunk position is XORed with bit 1 of the
// row so that the four rows x 32 bytes a 16-lane group reads with ds_read_b64_tr_b16 fall in different banks.
// ---------------------------------------------------------------------------
struct WgFragDma {
    // fragment of channels [c32, c32+32) over pixels [16 k16, 16 k16 + 16) of a 32-row slice
    static __device__ __forceinline__ bf16x8_t load(const unsigned char* slice, int k16, int c32, int lane) {
        const int g16 = lane >> 4, i16 = lane & 15;
        const int cbase = c32 + 16 * (g16 & 1), row = 16 * k16 + 8 * (g16 >> 1) + (i16 >> 2), p = i16 & 3;
        const int cpos = (cbase >> 3) ^ (((row >> 1) & 1) << 2);
        const unsigned char* a0 = slice + row * 128 + cpos * 16 + p * 8;
        typedef __attribute__((address_space(3))) s16x4_t* lptr;
        s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)(a0));
        s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)(a0 + 4 * 128));
        bf16x8_t r;
        r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
        r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
        return r;
    }
};

template <int CT, int D>
__global__ __launch_bounds__(256, 2) void wgrad_small_dma_kernel(const bf16_t* __restrict__ x,
                                                              const bf16_t* __restrict__ dy,
                                                              float* __restrict__ dw, const sba_conv_geom g,
                                                              const int M, const int chunks_per_split,
                                                              const int mode, const FastDiv dsub,
                                                              const FastDiv dow, const int64_t zstride) {
    constexpr int SL = 32 * 128;                 // one slice: 32 pixels x 64 channels
    constexpr int STAGE = (CT + 4) * SL;         // [dy slices (shared)] [x slice of wave 0..3]
    constexpr int LPS = 4 + CT;                  // DMA instructions per wave per stage
    extern __shared__ __attribute__((aligned(1024))) unsigned char wg_lds[];

    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int co0 = blockIdx.x * (64 * CT);
    const int ci_tiles = (g.Cin + 63) / 64;
    const int item = blockIdx.y * 4 + wid;
    const bool active = item < g.ntaps * ci_tiles;
    const int tap = active ? item / ci_tiles : 0;
    const int ci0 = active ? (item - tap * ci_tiles) * 64 : 0;
    int ty = 0, tx = 0;
#pragma unroll
    for (int t = 0; t < SBA_MAX_TAPS; ++t)
        if (t == tap) { ty = g.ty[t]; tx = g.tx[t]; }
    const int IHL = g.ups ? 2 * g.IH : g.IH, IWL = g.ups ? 2 * g.IW : g.IW;
    const int sub = g.OHs * g.OWs;

    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)wg_lds;
    const uint32_t x_bytes = (uint32_t)((int64_t)g.N * g.IH * g.IW * g.Cin * 2);
    const uint32_t dy_bytes = (uint32_t)((int64_t)g.N * g.OH * g.OW * g.Cout * 2);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc((void*)dy, 0, dy_bytes, 0x00020000);
    constexpr uint32_t OOB = 0xFFFFFFFFu;

    // lane l of a DMA instruction fills 16-byte position (l & 7) of row (l >> 3) of its 8-row block; that position
    // holds channel chunk (l & 7) ^ 4 * bit1(row)
    const int rsub = lane >> 3, cg = (lane & 7) ^ (((lane >> 4) & 1) << 2);
    const bool x_ok = active && ci0 + cg * 8 < g.Cin;
    const uint32_t x_coff = (uint32_t)(ci0 + cg * 8) * 2u;
    const int dslice = CT == 1 ? 0 : (wid >> 1);
    const bool d_ok = co0 + dslice * 64 + cg * 8 < g.Cout;
    const uint32_t d_coff = (uint32_t)(co0 + dslice * 64 + cg * 8) * 2u;
    const uint32_t x_pix = (uint32_t)g.Cin * 2u, d_pix = (uint32_t)g.Cout * 2u;

    const int total_chunks = (M + 31) / 32;
    const int chunk_lo = blockIdx.z * chunks_per_split;
    const int chunk_hi = min(chunk_lo + chunks_per_split, total_chunks);
    int g_ck = chunk_lo;

    auto issue = [&](const uint32_t dst) {
        const bool live = g_ck < chunk_hi;
        const int m0 = g_ck * 32;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + 8 * i + rsub;
            uint32_t off = OOB;
            if (live && x_ok && m < M) {
                const int n = (int)fdiv(m, dsub), rem = m - n * sub;
                const int oy = (int)fdiv(rem, dow), ox = rem - oy * g.OWs;
                int iy = oy * g.sy + ty, ix = ox * g.sx + tx;
                const bool ok = (iy >= 0) & (iy < IHL) & (ix >= 0) & (ix < IWL);
                if (g.ups) { iy >>= 1; ix >>= 1; }
                if (ok) off = (uint32_t)((n * g.IH + iy) * g.IW + ix) * x_pix + x_coff;
            }
            lds_dma16(xr, off, 0u, dst + (uint32_t)((CT + wid) * SL + i * 1024));
        }
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            const int i = CT == 1 ? wid : 2 * (wid & 1) + j;
            const int m = m0 + 8 * i + rsub;
            uint32_t off = OOB;
            if (live && d_ok && m < M) {
                const int n = (int)fdiv(m, dsub), rem = m - n * sub;
                const int oy = (int)fdiv(rem, dow), ox = rem - oy * g.OWs;
                off = (uint32_t)((n * g.OH + oy * g.osy + g.ooy) * g.OW + ox * g.osx + g.oox) * d_pix + d_coff;
            }
            lds_dma16(dr, off, 0u, dst + (uint32_t)(dslice * SL + i * 1024));
        }
        ++g_ck;
    };

    f32x16_t acc[CT][2][2];
    zero_acc(acc);

    int islot = 0;
#pragma unroll
    for (int p = 0; p < D - 1; ++p) { issue(lds_base + (uint32_t)(islot * STAGE)); ++islot; }
    if (islot == D) islot = 0;
    int cslot = 0;
    for (int ck = chunk_lo; ck < chunk_hi; ++ck) {
        wait_vmcnt<(D - 2) * LPS>();         // this wave's part of stage ck has landed ...
        wg_barrier();                        // ... and everybody else's; nobody reads slot (ck - 1) % D any more
        issue(lds_base + (uint32_t)(islot * STAGE));
        if (++islot == D) islot = 0;
        const unsigned char* st = wg_lds + cslot * STAGE;
        const unsigned char* sb = st + (CT + wid) * SL;
#pragma unroll
        for (int k16 = 0; k16 < 2; ++k16) {
            bf16x8_t b[2];
            b[0] = WgFragDma::load(sb, k16, 0, lane);
            b[1] = WgFragDma::load(sb, k16, 32, lane);
#pragma unroll
            for (int s = 0; s < CT; ++s) {
                bf16x8_t a[2];
                a[0] = WgFragDma::load(st + s * SL, k16, 0, lane);
                a[1] = WgFragDma::load(st + s * SL, k16, 32, lane);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[s][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[s][i][j], 0, 0, 0);
            }
        }
        if (++cslot == D) cslot = 0;
    }
    wait_vmcnt<0>();            // the dead stages issued past the end still write (zeros) into the ring
    wg_barrier();

    if (!active) return;
#pragma unroll
    for (int s = 0; s < CT; ++s)
        store_tile<true>(acc[s], dw + (int64_t)blockIdx.z * zstride, g, co0 + s * 64, ci0, tap, mode, lane);
}

// ---------------------------------------------------------------------------
// Kernel-row decomposition: the workgroup's waves = the KW taps of ONE kernel row kh and one 64-channel input tile.
// wgrad_small_dma_kernel gathers a 32-pixel x slice per wave (tap): 32 KW pixel rows per stage.  The kw taps of a kernel
// row read the SAME input row(s) at column offsets 0..KW-1 of a stride-SX walk, so here the stage holds that input row
// segment once -- R output rows x Wc output columns = 32 pixels (Wc = min(OW, 32)) need R x (SX (Wc - 1) + KW) input
// pixels -- and wave kw reads pixel (r, j) of it at LDS row r XW + SX j + kw.
//   <4, 2>: the 4x4 / stride-2 down blocks (encode_image_by_16times and the extra down blocks, model.py:540-575): <= 72
//           input pixels instead of 128: 4 KB (dy) + 9 KB per stage instead of 20 KB, four DMA instructions per wave
//           instead of five, 1.6x fewer bytes L2 -> LDS per MFMA (the roofline of this family);
//   <3, 1>: 3x3 stride-1 convs (the generator's 64 x 64 maps): <= 40 input pixels instead of 96, three waves.
// DMA blocks (8 rows x 128 B) of a stage: 0..3 = the dy slice, 4.. = the x rows, dealt round-robin to the waves.
// Stride 2: channel chunk c of LDS row L sits at 16-byte position c ^ 2 ((L >> 1) & 3) -- the four stride-2 rows a 16-lane
// group reads with ds_read_b64_tr_b16 fall into four different 32-byte bank groups; stride 1: c ^ 4 bit1(L) as above.
// ---------------------------------------------------------------------------
template <int SX>
struct WgFragRow {
    // fragment of channels [c32, c32+32) over output pixels [16 k16, 16 k16 + 16) of the chunk, tap column kw
    static __device__ __forceinline__ int swz(int L) { return SX == 2 ? (((L >> 1) & 3) << 1) : (((L >> 1) & 1) << 2); }
    // Stride 2: a wave's rows all have the parity of kw, and a 128-byte row covers half the banks -- every read would use 32 of
    // the 64 banks (PMC: SQ_LDS_BANK_CONFLICT = a third of the LDS cycles).  Segment row L therefore lives in LDS row
    // L ^ bit1(L) (an involution; swz() does not see bit 0): rows L and L + 2 fall into different halves.
    static __device__ __forceinline__ int slot(int L) { return SX == 2 ? (L ^ ((L >> 1) & 1)) : L; }
    static __device__ __forceinline__ bf16x8_t load(const unsigned char* xs, int k16, int c32, int lane, int kw, int wclog,
                                                    int xw, int ups, int tx0) {
        const int g16 = lane >> 4, i16 = lane & 15;
        const int cbase = c32 + 16 * (g16 & 1), p = 16 * k16 + 8 * (g16 >> 1) + (i16 >> 2), q = i16 & 3;
        const int r = p >> wclog, j = p & ((1 << wclog) - 1);
        // (behind a nearest x2 upsample the segment holds LOW-resolution pixels: column (ox0 + j + kw + tx0) >> 1, ox0 even)
        const int col = ups ? ((j + kw + tx0) >> 1) - (tx0 >> 1) : SX * j + kw;
        // pixel p + 4: four columns on in the same output row (Wc >= 8), or the next output row (Wc = 4)
        const int L0 = r * xw + col, L1 = L0 + (wclog == 2 ? xw : (ups ? 2 : 4 * SX));
        const int c0 = (cbase >> 3) ^ swz(L0), c1 = (cbase >> 3) ^ swz(L1);
        typedef __attribute__((address_space(3))) s16x4_t* lptr;
        s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)(xs + slot(L0) * 128 + c0 * 16 + q * 8));
        s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lptr)(xs + slot(L1) * 128 + c1 * 16 + q * 8));
        bf16x8_t v;
        v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
        v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
        return v;
    }
};

// One kernel row per workgroup, one wave per tap column.  (All kernel rows per workgroup -- nine waves for a 3x3 conv,
// the dy slice shared by the nine taps -- measured SLOWER almost everywhere: ResBlock 128 x 128 58.9 -> 71.4 us, 64 x 64
// 29.5 -> 42.3, upsample4 54.5 -> 68.9; only the 256 px upBlock gained, 183.6 -> 156.8; removed.)
template <int KW, int XB> struct WgRowCfg {         // XB: 8-row DMA blocks of one x segment
    static constexpr int LPS = (4 + XB + KW - 1) / KW;           // DMA instructions per wave per stage
    static constexpr int STAGE = LPS * KW * 1024;
};

template <int KW, int SX, int XB, int D>
__global__ __launch_bounds__(64 * KW, 2) void wgrad_row_dma_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                                float* __restrict__ dw, const sba_conv_geom g, const int M,
                                                                const int chunks_per_split, const int use_atomic,
                                                                const FastDiv dsub, const FastDiv dow, const int64_t zstride,
                                                                const int wclog) {
    constexpr int LPS = WgRowCfg<KW, XB>::LPS, STAGE = WgRowCfg<KW, XB>::STAGE;
    extern __shared__ __attribute__((aligned(1024))) unsigned char wg_lds[];

    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kw = wv;                                      // this wave's tap column
    const int co0 = blockIdx.x * 64;
    const int ci_tiles = g.Cin / 64;
    const int kh = blockIdx.y / ci_tiles;                   // the workgroup's kernel row
    const int ci0 = (blockIdx.y - kh * ci_tiles) * 64;
    const int tap = kh * KW + kw;
    // taps are row-structured (checked by the host): row kh starts at (ty0, tx0) = (g.ty[kh KW], g.tx[kh KW])
    int ty0 = 0, tx0 = 0;
#pragma unroll
    for (int t = 0; t < SBA_MAX_TAPS; ++t) {
        if (t == kh * KW) { ty0 = g.ty[t]; tx0 = g.tx[t]; }
    }
    const int ups = g.ups;            // (KW = 3, SX = 1 only) x is the LOW-resolution input of a nearest x2 upsample
    const int Wc = 1 << wclog, R = 32 >> wclog, XW = ups ? (Wc >> 1) + 2 : SX * (Wc - 1) + KW, XR = R * XW;
    const int sub = g.OH * g.OW;

    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)wg_lds;
    const uint32_t x_bytes = (uint32_t)((int64_t)g.N * g.IH * g.IW * g.Cin * 2);
    const uint32_t dy_bytes = (uint32_t)((int64_t)g.N * g.OH * g.OW * g.Cout * 2);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t dr = __builtin_amdgcn_make_buffer_rsrc((void*)dy, 0, dy_bytes, 0x00020000);
    constexpr uint32_t OOB = 0xFFFFFFFFu;

    // lane l of a DMA instruction fills 16-byte position (l & 7) of row (l >> 3) of its 8-row block
    const int rsub = lane >> 3;
    const int cgx = (lane & 7) ^ WgFragRow<SX>::swz(rsub);              // x rows (8-row blocks: swz(L) = swz(L & 7))
    const int cgd = (lane & 7) ^ (((lane >> 4) & 1) << 2);              // dy rows: as in wgrad_small_dma_kernel
    const uint32_t x_coff = (uint32_t)(ci0 + cgx * 8) * 2u, d_coff = (uint32_t)(co0 + cgd * 8) * 2u;
    const uint32_t x_pix = (uint32_t)g.Cin * 2u, d_pix = (uint32_t)g.Cout * 2u;
    // this wave's blocks b = kw + KW i.  b < 4: rows 8 b .. of the dy slice (role 0: rr = pixel of the chunk);
    // 4 <= b < 4 + XB: rows of the x segment (role 1: rr / rc = input row / column relative to the chunk's first pixel);
    // else a dummy that zero-fills its block (role 2)
    // (a 4 x 4 map has 16 pixels: a chunk then spans rows_img = OH rows of each of 32 / 16 = 2 images)
    const int rows_img = g.OH < R ? g.OH : R;
    int role[LPS], rr[LPS], rc[LPS], rn[LPS];
#pragma unroll
    for (int i = 0; i < LPS; ++i) {
        const int b = wv + KW * i;
        role[i] = 2; rr[i] = 0; rc[i] = 0; rn[i] = 0;
        if (b < 4) { role[i] = 0; rr[i] = 8 * b + rsub; }
        else if (b < 4 + XB) {
            const int L = WgFragRow<SX>::slot(8 * (b - 4) + rsub);      // the segment row this LDS row holds
            if (L < XR) {
                const int r = L / XW;
                role[i] = 1;
                rn[i] = r / rows_img;
                rr[i] = (r - rn[i] * rows_img) * g.sy + ty0;           // (ups: an offset in UPSAMPLED rows)
                rc[i] = ups ? L - r * XW : L - r * XW + tx0;            // (ups: the segment's low-resolution column index)
            }
        }
    }

    const int chunk_lo = blockIdx.z * chunks_per_split;
    const int chunk_hi = min(chunk_lo + chunks_per_split, M >> 5);
    int g_ck = chunk_lo;

    auto issue = [&](const uint32_t dst) {
        const bool live = g_ck < chunk_hi;
        const int m0 = g_ck * 32;
        const int n = (int)fdiv(m0, dsub), rem = m0 - n * sub;
        const int oy0 = (int)fdiv(rem, dow), ox0 = rem - oy0 * g.OW;
        const int iy0 = oy0 * g.sy, ix0 = ox0 * g.sx;
#pragma unroll
        for (int i = 0; i < LPS; ++i) {
            uint32_t off = OOB;
            if (role[i] == 0) {
                if (live) off = (uint32_t)(m0 + rr[i]) * d_pix + d_coff;
                lds_dma16(dr, off, 0u, dst + (uint32_t)((wv + KW * i) * 1024));
            } else {
                int iy = iy0 + rr[i], ix = ix0 + rc[i];
                if (ups) {              // upsampled row v -> low-resolution row v >> 1 (v = -1 and v = 2 IH are the padding)
                    iy >>= 1;
                    ix = ((ox0 + tx0) >> 1) + rc[i];
                }
                const bool ok = live & (role[i] == 1) & (iy >= 0) & (iy < g.IH) & (ix >= 0) & (ix < g.IW);
                if (ok) off = (uint32_t)(((n + rn[i]) * g.IH + iy) * g.IW + ix) * x_pix + x_coff;
                lds_dma16(xr, off, 0u, dst + (uint32_t)((wv + KW * i) * 1024));
            }
        }
        ++g_ck;
    };

    f32x16_t acc[2][2];
    zero_acc(acc);

    int islot = 0;
#pragma unroll
    for (int p = 0; p < D - 1; ++p) { issue(lds_base + (uint32_t)(islot * STAGE)); ++islot; }
    if (islot == D) islot = 0;
    int cslot = 0;
    for (int ck = chunk_lo; ck < chunk_hi; ++ck) {
        wait_vmcnt<(D - 2) * LPS>();         // this wave's part of stage ck has landed ...
        wg_barrier();                        // ... and everybody else's; nobody reads slot (ck - 1) % D any more
        issue(lds_base + (uint32_t)(islot * STAGE));
        if (++islot == D) islot = 0;
        const unsigned char* st = wg_lds + cslot * STAGE;
        const unsigned char* xs = st + 4 * 1024;
#pragma unroll
        for (int k16 = 0; k16 < 2; ++k16) {
            bf16x8_t a[2], b[2];
            b[0] = WgFragRow<SX>::load(xs, k16, 0, lane, kw, wclog, XW, ups, tx0);
            b[1] = WgFragRow<SX>::load(xs, k16, 32, lane, kw, wclog, XW, ups, tx0);
            a[0] = WgFragDma::load(st, k16, 0, lane);
            a[1] = WgFragDma::load(st, k16, 32, lane);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (++cslot == D) cslot = 0;
    }
    wait_vmcnt<0>();            // the dead stages issued past the end still write (zeros) into the ring
    wg_barrier();

    const int col_l = lane & 31, rsel = 4 * (lane >> 5);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + i * 32 + (r & 3) + 8 * (r >> 2) + rsel;
                const int ci = ci0 + j * 32 + col_l;
                float* p = dw + (int64_t)blockIdx.z * zstride + ((int64_t)co * g.ntaps + tap) * g.Cin + ci;
                if (use_atomic == 1) atomicAdd(p, acc[i][j][r]);
                else if (use_atomic == 2) *p = acc[i][j][r];       // first write of a cleared gradient
                else *p += acc[i][j][r];
            }
}

// ---------------------------------------------------------------------------
// weight gradient, large-map 3x3 stride-1 convs (optionally over a nearest-x2 upsampled input)
// with OW % 64 == 0: the generator's 64..256 px layers, where ~all wgrad FLOPs are.
// A workgroup owns one 64(co) x 64(ci) tile for ALL nine taps: per 64-pixel segment of an output
// row it stages the dy tile once and, per kernel row kh, ONE input row with a 1-pixel halo
// (66 x 64 channels); the three kw taps are the same LDS rows read at a +kw row offset, so each
// input pixel is fetched once per kh instead of once per tap.  Wave kh (3 waves) accumulates its
// three taps (192 accumulator registers) over the workgroup's whole pixel range, then adds them
// to dw with f32 atomics.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(192) void wgrad_rows_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                         float* __restrict__ dw, const sba_conv_geom g,
                                                         const int total_segs, const int segs_per_wg,
                                                         const int mode, const int64_t zstride) {
    constexpr int ROWS = WgFrag<T>::ROWS;
    constexpr int CH = 16 / (int)sizeof(T);
    constexpr int CPR = 64 / CH;                       // 16-byte chunks per 64-channel pixel row
    constexpr int XR = 66;                             // 64 pixels + halo
    constexpr int XROWS_ALLOC = 80;                    // rows reserved per x tile (>= 64 + 2 + 15 read slack)
    __shared__ __attribute__((aligned(16))) unsigned char lds[(64 + 3 * XROWS_ALLOC) * ROWS];

    const int tid = threadIdx.x, lane = tid & 63, kh = tid >> 6;
    const int co0 = blockIdx.x * 64, ci0 = blockIdx.y * 64;
    const int IHL = g.ups ? 2 * g.IH : g.IH, IWL = g.ups ? 2 * g.IW : g.IW;
    const int segs_per_row = g.OW / 64;
    unsigned char* sa = lds;
    unsigned char* sx = lds + (64 + kh * XROWS_ALLOC) * ROWS;

    // rows 66..79 of the x tile are only ever read by discarded k positions? no: every read row
    // index is < 16*3 + 2 + 16 = 66, so the slack rows are never touched; zero them once anyway
    for (int i = lane; i < (XROWS_ALLOC - XR) * ROWS / 16; i += 64)
        *reinterpret_cast<uint4*>(sx + XR * ROWS + i * 16) = make_uint4(0, 0, 0, 0);

    f32x16_t acc[3][2][2];
    zero_acc(acc);

    const int seg_lo = blockIdx.z * segs_per_wg;
    const int seg_hi = min(seg_lo + segs_per_wg, total_segs);
    constexpr int A_PT = (64 * CPR + 191) / 192;
    constexpr int X_PT = (XR * CPR + 63) / 64;
    uint4 va[A_PT], vx[X_PT];
    auto gload = [&](int seg) {
        const int n = seg / (g.OH * segs_per_row);
        const int rem = seg - n * g.OH * segs_per_row;
        const int oy = rem / segs_per_row, ox0 = (rem - oy * segs_per_row) * 64;
#pragma unroll
        for (int u = 0; u < A_PT; ++u) {
            const int idx = tid + 192 * u;
            va[u] = make_uint4(0, 0, 0, 0);
            if (idx < 64 * CPR) {
                const int pix = idx / CPR, cc = idx - pix * CPR;
                const int co = co0 + cc * CH;
                if (co < g.Cout) {
                    const int64_t po = ((int64_t)(n * g.OH + oy) * g.OW + ox0 + pix);
                    va[u] = *reinterpret_cast<const uint4*>(dy + po * g.Cout + co);
                }
            }
        }
        int iy = oy + kh - 1;
        const bool row_ok = (iy >= 0) & (iy < IHL);
        if (g.ups) iy >>= 1;
#pragma unroll
        for (int u = 0; u < X_PT; ++u) {
            const int idx = lane + 64 * u;
            vx[u] = make_uint4(0, 0, 0, 0);
            if (idx < XR * CPR) {
                const int j = idx / CPR, cc = idx - j * CPR;
                int ix = ox0 - 1 + j;
                const bool ok = row_ok & (ix >= 0) & (ix < IWL);
                if (g.ups) ix >>= 1;
                const int ci = ci0 + cc * CH;
                if (ok && ci < g.Cin) {
                    const int64_t pi = (int64_t)(n * g.IH + iy) * g.IW + ix;
                    vx[u] = *reinterpret_cast<const uint4*>(x + pi * g.Cin + ci);
                }
            }
        }
    };
    if (seg_lo < seg_hi) gload(seg_lo);
    for (int seg = seg_lo; seg < seg_hi; ++seg) {
        __syncthreads();        // previous segment's tiles fully consumed
#pragma unroll
        for (int u = 0; u < A_PT; ++u) {
            const int idx = tid + 192 * u;
            if (idx < 64 * CPR) {
                const int pix = idx / CPR, cc = idx - pix * CPR;
                *reinterpret_cast<uint4*>(sa + pix * ROWS + cc * 16) = va[u];
            }
        }
#pragma unroll
        for (int u = 0; u < X_PT; ++u) {
            const int idx = lane + 64 * u;
            if (idx < XR * CPR) {
                const int j = idx / CPR, cc = idx - j * CPR;
                *reinterpret_cast<uint4*>(sx + j * ROWS + cc * 16) = vx[u];
            }
        }
        __syncthreads();
        if (seg + 1 < seg_hi) gload(seg + 1);     // prefetch the next segment under the 48 MFMAs below
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
                WgFrag<T>::mma(sa + 16 * ks * ROWS, sx + (16 * ks + kw) * ROWS, lane, acc[kw]);
        }
    }

    // (mode 1, f32 atomics: the three waves of a workgroup never own dw; mode 2: deterministic mode, the split's own partial tensor)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw)
        store_tile<false>(acc[kw], dw + (int64_t)blockIdx.z * zstride, g, co0, ci0, kh * 3 + kw, mode, lane);
}

// ---------------------------------------------------------------------------
// Host side: wgrad_plan decides (pure: no global state, no device), wgrad_launch does what the plan says.
// ---------------------------------------------------------------------------
enum WgradFamily { WG_ROW_DMA = 0, WG_SMALL_DMA = 1, WG_SMALL = 2, WG_ROWS = 3, WG_GENERIC = 4 };

struct WgradPlan {
    int family;
    int v[4];           // template arguments: row-DMA <KW, SX, XB, D>, small-DMA <CT, D>; the other families: the dtype
    dim3 grid;          // z = pixel splits
    int block, lds;     // threads, dynamic LDS bytes
    int per_split;      // chunks (wgrad_rows_kernel: 64-pixel segments) per pixel split
    int mode;           // epilogue: 0 = +=, 1 = f32 atomics, 2 = store
    int npart;          // deterministic mode: partial tensors folded in order by sba_det_fold (0 = none)
    int wclog;          // row-DMA: log2 of the output columns of a 32-pixel chunk
};

// Pixel splits of a grid of `wgs` workgroups over `chunks` chunks of pixels: fill `target_wgs`, keep >= `min_chunks`
// behind every split (each split costs a full f32-atomic copy of dW), then even the splits out.
static int pixel_splits(int target_wgs, int wgs, int chunks, int min_chunks, int* per_split) {
    int sp = cdiv(target_wgs, wgs);
    if (sp > chunks / min_chunks) sp = chunks / min_chunks > 0 ? chunks / min_chunks : 1;
    *per_split = cdiv(chunks, sp);
    return cdiv(chunks, *per_split);
}

static bool wgrad_plan(int dtype, const sba_conv_geom* g, int ksplit, bool det_on, WgradPlan* p) {
    if (!geom_ok(g, dtype)) return false;
    if (g->Cin % 8 != 0 || g->Cout % 8 != 0) return false;
    if (g->x_cstride || g->x_coff || g->y_cstride || g->y_coff || g->ntaps > 16) return false;
    const int M = g->N * g->OHs * g->OWs;
    if (ksplit < 1) ksplit = 1;
    const int fw = g->first_write ? 2 : 0;       // epilogue mode of an unsplit launch of the exclusive-owner kernels
    const int co_tiles = cdiv(g->Cout, 64), items = cdiv(g->Cin, 64) * g->ntaps;
    // the LDS-DMA kernels address x and dy with 32-bit byte offsets (x: geom_ok has checked it, x_cstride == 0 here)
    const bool dma_ok = dtype == SBA_BF16 && (int64_t)g->N * g->OH * g->OW * g->Cout * 2 < (1ll << 32);
    // Deterministic mode: pixel splits do not meet in f32 atomics -- split z STORES its partial gradient into its own
    // tensor of the scratch ring (mode 2, offset z * zstride) and sba_det_fold adds the splits up in order.
    auto fill = [&](int family, int v0, int v1, int v2, int v3, dim3 grid, int block, int lds, int per_split, int unsplit_mode) {
        *p = WgradPlan{family, {v0, v1, v2, v3}, grid, block, lds, per_split, 0, 0, 0};
        const int nz = (int)grid.z;
        p->npart = det_on && (nz > 1 || family == WG_ROWS) ? nz : 0;       // (wgrad_rows_kernel: its three waves never own dw)
        p->mode = p->npart ? 2 : (nz > 1 ? 1 : unsplit_mode);
        return grid.y <= 65535 && grid.z <= 65535;
    };
    // Kernel-row decomposition (wgrad_row_dma_kernel): the kw taps of a kernel row share one staged input row segment.
    // 4x4 / stride-2 down blocks, and 3x3 / stride-1 convs on maps of 8 x 8 .. -- also in the all-taps halo-row kernel's
    // range and behind the nearest x2 upsample (G upsample1..4 73 / 92 / 102 / 80 -> 41 / 56 / 55 / 53 us, upBlock -> 128 px
    // 123 -> 100, -> 256 px 192 -> 187) -- tools/bench_wgrad.py, B = 20: ResBlock 64 x 64 44.0 -> 28.4 us, 64->128 @64 61.6 -> 38.3; at 128 x 128
    // against wgrad_rows_kernel: 64->64 95.8 -> 54.9 us, 64->128 122.8 -> 92.8 (profiles/r04_wgrad_s2_rows.txt).
    // The 4 x 4 maps (two images per chunk) included -- B = 40: D256's 3x3 2048->1024 78.6 -> 55.8 us, D128's 1024->512
    // 38.1 -> 27.3, 512->1024 4x4/s2 35.8 -> 27.9.
    {
        const int kwn = g->ntaps == 16 ? 4 : (g->ntaps == 9 ? 3 : 0), sxy = g->sx;
        bool ok = dma_ok && kwn && g->sy == sxy && (!g->ups || kwn == 3) && g->osy == 1 && g->osx == 1 && g->ooy == 0 &&
                  g->oox == 0 && g->OHs == g->OH && g->OWs == g->OW && g->Cin % 64 == 0 && g->Cout % 64 == 0 &&
                  g->OW >= 4 && (g->OW & (g->OW - 1)) == 0 && !(g->OW == 4 && (g->ups || g->OH != 4)) && M % 32 == 0 &&
                  ((g->OH * g->OW) % 32 == 0 || g->OW == 4);
        ok = ok && ((kwn == 4 && sxy == 2) || (kwn == 3 && sxy == 1));
        for (int t = 0; t < g->ntaps && ok; ++t)
            ok = g->ty[t] == g->ty[(t / kwn) * kwn] && g->tx[t] == g->tx[(t / kwn) * kwn] + (t % kwn);
        if (ok) {
            const int wc = g->OW < 32 ? g->OW : 32;
            int wclog = 0;
            while ((1 << wclog) < wc) ++wclog;
            const int wgs = co_tiles * kwn * (g->Cin / 64);
            // pixel splits: each one adds a full f32-atomic copy of dW (~1.3 TB/s chip-wide): fill the chip about twice,
            // keep >= 12 chunks behind a copy
            // (tools/bench_wgrad.py, B = 40: 128->256 @64 71 us at 512 workgroups, 78 at 384, 94 at 256; the 64->128 layers,
            // 8 workgroups per split: @128 89 / 86 / 94, @64 42 / 37 / 36)
            constexpr int ROW_WGS = 512;
            int cps32;
            const int sp = pixel_splits(wgs <= 8 ? (ROW_WGS * 3) / 4 : ROW_WGS, wgs, M / 32, 12, &cps32);
            // x segment of a stage: <= 72 rows (4x4 / stride 2, OW >= 8) or 80 rows (two 4 x 4 maps): XB = 10; 3x3 on a
            // 4 x 4 map: 8 rows x 6 = 48 rows: XB = 6; 3x3 otherwise <= 40 rows: XB = 5
            // (ring depth: 3 and 4 measure the same, 6 is 30-60 % slower -- occupancy: profiles/r04_wgrad_s2_rows.txt)
            const int xb = kwn == 4 ? 10 : (g->OW == 4 ? 6 : 5);
            const int stage = kwn == 4 ? WgRowCfg<4, 10>::STAGE : (g->OW == 4 ? WgRowCfg<3, 6>::STAGE : WgRowCfg<3, 5>::STAGE);
            if (fill(WG_ROW_DMA, kwn, sxy, xb, 4, dim3(co_tiles, kwn * (g->Cin / 64), sp), 64 * kwn, 4 * stage, cps32, fw)) {
                p->wclog = wclog;
                return true;
            }
        }
    }
    constexpr int SMALL_M = 12000;      // small-pixel-count decomposition: output pixels up to this
    if (M <= SMALL_M && co_tiles * items >= 256) {
        // GEMM-like layer: one tile per wave, all pixels (ksplit re-derived for this decomposition)
        const int wgs = co_tiles * cdiv(items, 4);
        // pixel splits: each one adds a full f32-atomic copy of every 64x64 tile (the atomics run at ~1.3 TB/s),
        // so split only up to ~3 workgroups per CU and keep >= 24 chunks (384 pixels) of MFMA work behind a copy
        // (measured on the discriminator shapes: joint conv 68 -> 44 us, s64_2 68 -> 46, c4 166 -> 133)
        constexpr int SMALL_WGS = 768, SMALL_MINC = 24;
        const int target = wgs >= SMALL_WGS / 2 ? wgs : SMALL_WGS;         // (half the target is there already: no split)
        int cps;
        const int split = pixel_splits(target, wgs, cdiv(M, 16), SMALL_MINC, &cps);
        const dim3 grid(co_tiles, cdiv(items, 4), split);
        if (grid.y > 65535 || grid.z > 65535) return false;
        // LDS-DMA ring of depth 4 (tools/bench_wgrad.py, B = 20): 15-25 % faster than the register-staged kernel up to ~512
        // workgroups (joint conv 29 -> 25 us, D s32 61 -> 50, s32_1 49 -> 37); beyond that the launches are bound by
        // the L2 traffic of the operand slices either way and the 80 KB ring costs occupancy (s64 145 -> 175 us)
        constexpr int DMA_WGS = 512;
        // beyond DMA_WGS: the DMA kernel with TWO co tiles per wave (0.375 KB of operands per MFMA) -- pays once the
        // epilogue is a plain store (first write: D256 s64 119 -> 95 us, s64_1 89 -> 79, G upsample1 84 -> 72); with the
        // read-modify-write epilogue it is no faster than the register-staged kernel (148 vs 146 us).
        if (fw == 2 && wgs > DMA_WGS && g->Cout % 128 == 0 && dma_ok) {
            fill(WG_SMALL_DMA, 2, 3, 0, 0, dim3(co_tiles / 2, cdiv(items, 4), 1), 256, 3 * 6 * 32 * 128, cdiv(M, 32), fw);
            return true;
        }
        if (wgs <= DMA_WGS && dma_ok) {
            // stages of 32 pixels; the same split rule restated in 32-pixel chunks
            int cps32;
            const int sp = pixel_splits(target, wgs, cdiv(M, 32), SMALL_MINC / 2, &cps32);
            return fill(WG_SMALL_DMA, 1, 4, 0, 0, dim3(co_tiles, cdiv(items, 4), sp), 256, 4 * 5 * 32 * 128, cps32, fw);
        }
        return fill(WG_SMALL, dtype, 0, 0, 0, grid, 256, 0, cps, fw);
    }
    // generator-style 3x3 stride-1 conv on a wide map: all nine taps per workgroup from halo tiles.  From 128x128 maps
    // up (B = 20: M >= 327 k) it beats the LDS-DMA decomposition below (upBlock -> 256 px 189 vs 349 us); at 64x64
    // (M = 82 k) the DMA kernel wins (ResBlock 51 -> 40 us, 64->128: 69 -> 60), tools/bench_wgrad.py.
    constexpr int ROWS_M = 131072;
    bool rows_ok = g->ntaps == 9 && g->sy == 1 && g->sx == 1 && g->osy == 1 && g->osx == 1 && g->ooy == 0 &&
                   g->oox == 0 && g->OHs == g->OH && g->OWs == g->OW && g->OW % 64 == 0 && M >= ROWS_M;
    for (int t = 0; t < 9 && rows_ok; ++t) rows_ok = g->ty[t] == t / 3 - 1 && g->tx[t] == t % 3 - 1;
    if (rows_ok) {
        const int ci_t = cdiv(g->Cin, 64);
        // every pixel split adds a full copy of the tile's 9 x 64 x 64 outputs to the f32 atomics
        // (~1.3 TB/s chip-wide), so use few, fat workgroups: ~1 per CU and >= 16 segments each
        int spw;
        const int nz = pixel_splits(256, co_tiles * ci_t, g->N * g->OH * (g->OW / 64), 16, &spw);
        // (deterministic mode: also for nz == 1 -- every workgroup's three waves store, nothing adds)
        return fill(WG_ROWS, dtype, 0, 0, 0, dim3(co_tiles, ci_t, nz), 192, 0, spw, 1);
    }
    // Big-M layers that are not 3x3 / OW % 64 == 0 (the discriminators' 4x4/s2 down blocks at 32..128 px): the
    // register-staged kernel below shares nothing between its waves (1 KB of operands per MFMA from L2 = the
    // 300 TFLOP/s on-chip-bandwidth roofline of a 64x64 tile); the small-pixel-count decomposition shares the dy
    // slices between the four (tap, ci tile) items of a workgroup (0.625 KB per MFMA) and walks its pixel split
    // through the LDS-DMA ring.  Measured (tools/bench_wgrad.py, B = 20): D256 down 64->128 @128 px 200 -> 110 us,
    // 128->256 @64 193 -> 107, D128 down @64 99 -> 48, D64 down @32 43 -> 24; two co tiles per wave are no better.
    if (dma_ok) {
        constexpr int GEN_WGS = 512;
        int cps32;
        const int sp = pixel_splits(GEN_WGS, co_tiles * cdiv(items, 4), cdiv(M, 32), 12, &cps32);
        if (fill(WG_SMALL_DMA, 1, 4, 0, 0, dim3(co_tiles, cdiv(items, 4), sp), 256, 4 * 5 * 32 * 128, cps32, fw)) return true;
    }
    const int total_chunks = cdiv(M, 64);
    if (ksplit > total_chunks) ksplit = total_chunks;
    const int cps = cdiv(total_chunks, ksplit);
    return fill(WG_GENERIC, dtype, 0, 0, 0, dim3(co_tiles, items, cdiv(total_chunks, cps)), 256, 0, cps, 0);
}

// One launch of a dynamic-LDS kernel; its LDS limit is raised once per kernel symbol.
template <auto Kernel, typename... Args>
static void launch_dyn_lds(const WgradPlan& p, hipStream_t st, Args... args) {
    static bool once = false;
    if (!once) { (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds); once = true; }
    SBA_LAUNCH(Kernel, p.grid, dim3(p.block), p.lds, st, args...);
}

static int wgrad_launch(const WgradPlan& p, int dtype, const void* x, const void* dy, float* dw, const sba_conv_geom* g,
                        hipStream_t st) {
    const int M = g->N * g->OHs * g->OWs;
    const FastDiv dsub = make_fastdiv((uint32_t)(g->OHs * g->OWs), (int64_t)M + 64);
    const FastDiv dow = make_fastdiv((uint32_t)g->OWs, (int64_t)M + 64);
    const int64_t dwn = (int64_t)g->Cout * g->ntaps * g->Cin;
    float* part = nullptr;
    if (p.npart) { part = sba_det_alloc((int64_t)p.npart * dwn); if (!part) return SBA_E_ARG; }
    float* dwa = part ? part : dw;
    const int64_t zs = part ? dwn : 0;
    const bf16_t* xh = (const bf16_t*)x;
    const bf16_t* dyh = (const bf16_t*)dy;
    switch (p.family) {
    case WG_ROW_DMA:
        if (p.v[0] == 4) launch_dyn_lds<wgrad_row_dma_kernel<4, 2, 10, 4>>(p, st, xh, dyh, dwa, *g, M, p.per_split, p.mode, dsub, dow, zs, p.wclog);
        else if (p.v[2] == 6) launch_dyn_lds<wgrad_row_dma_kernel<3, 1, 6, 4>>(p, st, xh, dyh, dwa, *g, M, p.per_split, p.mode, dsub, dow, zs, p.wclog);
        else launch_dyn_lds<wgrad_row_dma_kernel<3, 1, 5, 4>>(p, st, xh, dyh, dwa, *g, M, p.per_split, p.mode, dsub, dow, zs, p.wclog);
        break;
    case WG_SMALL_DMA:
        if (p.v[0] == 2) launch_dyn_lds<wgrad_small_dma_kernel<2, 3>>(p, st, xh, dyh, dwa, *g, M, p.per_split, p.mode, dsub, dow, zs);
        else launch_dyn_lds<wgrad_small_dma_kernel<1, 4>>(p, st, xh, dyh, dwa, *g, M, p.per_split, p.mode, dsub, dow, zs);
        break;
    case WG_SMALL:
        SBA_DISPATCH(dtype, SBA_LAUNCH((wgrad_small_kernel<T>), p.grid, dim3(p.block), 0, st, (const T*)x, (const T*)dy, dwa, *g, M,
                                       p.per_split, p.mode, dsub, dow, zs));
        break;
    case WG_ROWS:
        SBA_DISPATCH(dtype, SBA_LAUNCH((wgrad_rows_kernel<T>), p.grid, dim3(p.block), 0, st, (const T*)x, (const T*)dy, dwa, *g,
                                       g->N * g->OH * (g->OW / 64), p.per_split, p.mode, zs));
        break;
    default:
        SBA_DISPATCH(dtype, SBA_LAUNCH((wgrad_kernel<T>), p.grid, dim3(p.block), 0, st, (const T*)x, (const T*)dy, dwa, *g, M,
                                       p.per_split, p.mode, dsub, dow, zs));
    }
    if (part) sba_det_fold(part, 1, p.npart, dwn, dw, 0, g->first_write ? 1 : 0, st);
    return SBA_CHECK_LAUNCH();
}

}  // namespace

extern "C" int sba_conv_wgrad_plan(int dtype, const sba_conv_geom* g, int ksplit, int det, int* plan) {
    WgradPlan p;
    if (!plan || !wgrad_plan(dtype, g, ksplit, det != 0, &p)) return SBA_E_ARG;
    const int out[SBA_WGRAD_PLAN_INTS] = {p.family, p.v[0], p.v[1], p.v[2], p.v[3], (int)p.grid.x, (int)p.grid.y, (int)p.grid.z,
                                          p.block, p.lds, p.per_split, p.mode, p.npart, p.wclog};
    for (int i = 0; i < SBA_WGRAD_PLAN_INTS; ++i) plan[i] = out[i];
    return SBA_OK;
}

extern "C" int sba_conv_wgrad(int dtype, const void* x, const void* dy, float* dw, const sba_conv_geom* g,
                              int ksplit, void* stream) {
    WgradPlan p;
    if (!x || !dy || !dw || !wgrad_plan(dtype, g, ksplit, sba_det_on(), &p)) return SBA_E_ARG;
    return wgrad_launch(p, dtype, x, dy, dw, g, (hipStream_t)stream);
}
