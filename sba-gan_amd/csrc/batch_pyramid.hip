// Training batches from the device-resident image cache (sba_batch_pyramid in sbagan_hip.h; sbagan/device_data.py).
//
// One launch per batch: gather B cached uint8 images by index, crop a T x T window, mirror it, and write every scale of
// the pyramid as normalised planar f32 -- the bytes PIL's crop / FLIP_LEFT_RIGHT / 8-bit BILINEAR resize produce, the
// floats ToTensor + Normalize make of them (a 256-entry table built on the host by those very torch operations).
// Workgroup = one 32 x 32 tile of the level-0 crop of one image, in OUTPUT (mirrored) coordinates; its 16 x 16 and 8 x 8
// coarse tiles need the crop 2 pixels around it.  No atomics, no workspace: plain loads and stores.
#include "common.h"

namespace {

constexpr int BP_THREADS = 256;
constexpr int BP_TILE = 32;             // level-0 tile side; a multiple of 4, so the coarse tiles align
constexpr int BP_HALO = 2;              // factor 4 reaches 2 pixels beyond the 4 it covers, factor 2 one
constexpr int BP_ROWS = BP_TILE + 2 * BP_HALO;      // 36 rows of raw bytes per channel
constexpr int BP_PAD = 4;               // the tile's first column sits at byte 4 of a row: level 0 reads aligned words
constexpr int BP_STRIDE = BP_TILE + 2 * BP_PAD;     // 40 bytes per row
constexpr int BP_TAPS = 8;              // widest window of a table row {xmin, n, k0..k7}
constexpr int BP_ROW_INTS = 2 + BP_TAPS;  // a host table row
constexpr int BP_LDS_ROW = 4 + BP_TAPS;   // the same row in LDS
constexpr int BP_BITS = 22;             // PIL's 8-bit coefficient precision: 32 - 8 - 2

__device__ __forceinline__ uint8_t bp_clip8(int acc) {
    const int v = acc >> BP_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One pass of PIL's 8-bit resampling for one output: byte = clip((2^21 + sum_j src[first + j] k_j) >> 22).  `row` is the
// output's table row in LDS, {xmin, n, -, -, k0..k7} (the coefficients 16-byte aligned); src is indexed from `base` (the
// crop coordinate of src[0]) with element stride `step`.  Branch-free: a tap at or beyond n, or outside [0, limit) of src
// -- a well-formed table has none -- reads src[0] with coefficient 0.  Factor 2 never has more than 4 taps.
template <int TAPS>
__device__ __forceinline__ uint8_t bp_resample(const uint8_t* src, int step, int base, int limit, const int32_t* row) {
    const int first = row[0] - base, n = row[1];
    int k[BP_TAPS];
    *reinterpret_cast<int4*>(&k[0]) = *reinterpret_cast<const int4*>(row + 4);
    if (TAPS > 4) *reinterpret_cast<int4*>(&k[4]) = *reinterpret_cast<const int4*>(row + 8);
    int acc = 1 << (BP_BITS - 1);
#pragma unroll
    for (int j = 0; j < TAPS; ++j) {
        const int p = first + j;
        const bool ok = j < n && p >= 0 && p < limit;
        acc += (int)src[ok ? p * step : 0] * (ok ? k[j] : 0);
    }
    return bp_clip8(acc);
}

// rows [o0, o0 + rows) of a host table [T_l][10] into LDS rows of BP_LDS_ROW ints; a row at or beyond T_l gets n = 0
__device__ __forceinline__ void bp_stage_table(int32_t* dst, const int32_t* __restrict__ tab, int o0, int rows, int Tl) {
    for (int e = threadIdx.x; e < rows * BP_ROW_INTS; e += BP_THREADS) {
        const int r = e / BP_ROW_INTS, k = e % BP_ROW_INTS;
        dst[r * BP_LDS_ROW + (k < 2 ? k : k + 2)] = o0 + r < Tl ? tab[(size_t)(o0 + r) * BP_ROW_INTS + k] : 0;
    }
}

struct BpOut {
    float* p[3];        // out_l [B][3][T >> l][T >> l]
};

// grid = (tiles, tiles, B).  LDS: raw bytes 3 x 36 x 40, the horizontal intermediates 3 x 36 x 16 and 3 x 36 x 8, the
// byte -> float table and the tile's table rows (columns and rows, both levels): 10.2 KB.  Everything a pass needs is in
// LDS before the first barrier, so the passes behind it wait on no global load.
__global__ __launch_bounds__(BP_THREADS) void batch_pyramid_kernel(
    const uint8_t* __restrict__ cache, const int64_t* __restrict__ offset, const int32_t* __restrict__ hw, int N,
    const int32_t* __restrict__ params, int T, int levels, const int32_t* __restrict__ tab1,
    const int32_t* __restrict__ tab2, const float* __restrict__ lut, BpOut out, int vec) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[3][BP_ROWS][BP_STRIDE];
    __shared__ uint8_t h1[3][BP_ROWS][BP_TILE / 2];
    __shared__ uint8_t h2[3][BP_ROWS][BP_TILE / 4];
    __shared__ float flut[256];
    __shared__ __attribute__((aligned(16))) int32_t tb1[2][BP_TILE / 2][BP_LDS_ROW];      // [columns | rows]
    __shared__ __attribute__((aligned(16))) int32_t tb2[2][BP_TILE / 4][BP_LDS_ROW];

    const int t = threadIdx.x, b = blockIdx.z;
    const int tx0 = blockIdx.x * BP_TILE, ty0 = blockIdx.y * BP_TILE;
    // the whole workgroup takes the same way out: a row that does not name a window inside a cached image writes nothing
    const int idx = params[b * 4], x1 = params[b * 4 + 1], y1 = params[b * 4 + 2], flip = params[b * 4 + 3];
    if (idx < 0 || idx >= N) return;
    const int H = hw[idx * 2], W = hw[idx * 2 + 1];
    if (x1 < 0 || y1 < 0 || T > W || T > H || x1 > W - T || y1 > H - T) return;
    const uint8_t* img = cache + offset[idx];

    flut[t] = lut[t];
    const int T1 = T >> 1, T2 = T >> 2;
    if (levels >= 2) {
        bp_stage_table(&tb1[0][0][0], tab1, tx0 / 2, BP_TILE / 2, T1);
        bp_stage_table(&tb1[1][0][0], tab1, ty0 / 2, BP_TILE / 2, T1);
    }
    if (levels > 2) {
        bp_stage_table(&tb2[0][0][0], tab2, tx0 / 4, BP_TILE / 4, T2);
        bp_stage_table(&tb2[1][0][0], tab2, ty0 / 4, BP_TILE / 4, T2);
    }
    // raw[c][r][q] = crop byte at row ty0 - 2 + r, column tx0 - 4 + q of the mirrored crop; 0 outside the crop or the halo
    for (int e = t; e < BP_ROWS * BP_STRIDE; e += BP_THREADS) {
        const int r = e / BP_STRIDE, q = e % BP_STRIDE;
        const int cy = ty0 - BP_HALO + r, cx = tx0 - BP_PAD + q;
        uint8_t v0 = 0, v1 = 0, v2 = 0;
        if (q >= BP_PAD - BP_HALO && q < BP_PAD + BP_TILE + BP_HALO && cy >= 0 && cy < T && cx >= 0 && cx < T) {
            const int sx = x1 + (flip ? T - 1 - cx : cx);
            const uint8_t* px = img + ((size_t)(y1 + cy) * W + sx) * 3;
            v0 = px[0]; v1 = px[1]; v2 = px[2];
        }
        raw[0][r][q] = v0; raw[1][r][q] = v1; raw[2][r][q] = v2;
    }
    __syncthreads();

    // level 0: out0 = lut[byte]
    if (vec) {              // T % 4 == 0 and out0 16-byte aligned: one float4 per thread and channel
        const int r = t >> 3, x4 = (t & 7) * 4;
        const int y = ty0 + r, x = tx0 + x4;
        if (y < T && x < T) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(&raw[c][r + BP_HALO][BP_PAD + x4]);
                float4 v;
                v.x = flut[w & 255]; v.y = flut[(w >> 8) & 255]; v.z = flut[(w >> 16) & 255]; v.w = flut[w >> 24];
                *reinterpret_cast<float4*>(out.p[0] + (((size_t)b * 3 + c) * T + y) * T + x) = v;
            }
        }
    } else {
        for (int e = t; e < 3 * BP_TILE * BP_TILE; e += BP_THREADS) {
            const int c = e / (BP_TILE * BP_TILE), r = (e / BP_TILE) % BP_TILE, q = e % BP_TILE;
            const int y = ty0 + r, x = tx0 + q;
            if (y < T && x < T)
                out.p[0][(((size_t)b * 3 + c) * T + y) * T + x] = flut[raw[c][r + BP_HALO][BP_PAD + q]];
        }
    }
    if (levels < 2) return;

    // horizontal passes over every raw row of the crop, rounded to bytes
    for (int e = t; e < 3 * BP_ROWS * (BP_TILE / 2); e += BP_THREADS) {
        const int c = e / (BP_ROWS * (BP_TILE / 2)), r = (e / (BP_TILE / 2)) % BP_ROWS, q = e % (BP_TILE / 2);
        h1[c][r][q] = bp_resample<4>(&raw[c][r][0], 1, tx0 - BP_PAD, BP_STRIDE, tb1[0][q]);
    }
    if (levels > 2) {
        for (int e = t; e < 3 * BP_ROWS * (BP_TILE / 4); e += BP_THREADS) {
            const int c = e / (BP_ROWS * (BP_TILE / 4)), r = (e / (BP_TILE / 4)) % BP_ROWS, q = e % (BP_TILE / 4);
            h2[c][r][q] = bp_resample<8>(&raw[c][r][0], 1, tx0 - BP_PAD, BP_STRIDE, tb2[0][q]);
        }
    }
    __syncthreads();

    // vertical passes; rows outside the crop are never taps of a table built for T, and hold 0
    for (int e = t; e < 3 * (BP_TILE / 2) * (BP_TILE / 2); e += BP_THREADS) {
        const int c = e / ((BP_TILE / 2) * (BP_TILE / 2)), r = (e / (BP_TILE / 2)) % (BP_TILE / 2), q = e % (BP_TILE / 2);
        const int oy = ty0 / 2 + r, ox = tx0 / 2 + q;
        if (oy < T1 && ox < T1) {
            const uint8_t v = bp_resample<4>(&h1[c][0][q], BP_TILE / 2, ty0 - BP_HALO, BP_ROWS, tb1[1][r]);
            out.p[1][(((size_t)b * 3 + c) * T1 + oy) * T1 + ox] = flut[v];
        }
    }
    if (levels > 2 && t < 3 * (BP_TILE / 4) * (BP_TILE / 4)) {
        const int c = t / ((BP_TILE / 4) * (BP_TILE / 4)), r = (t / (BP_TILE / 4)) % (BP_TILE / 4), q = t % (BP_TILE / 4);
        const int oy = ty0 / 4 + r, ox = tx0 / 4 + q;
        if (oy < T2 && ox < T2) {
            const uint8_t v = bp_resample<8>(&h2[c][0][q], BP_TILE / 4, ty0 - BP_HALO, BP_ROWS, tb2[1][r]);
            out.p[2][(((size_t)b * 3 + c) * T2 + oy) * T2 + ox] = flut[v];
        }
    }
}

}  // namespace

extern "C" int sba_batch_pyramid(const uint8_t* cache, const int64_t* offset, const int32_t* hw, int N,
                                 const int32_t* params, int B, int T, int levels, const int32_t* tab1,
                                 const int32_t* tab2, const float* lut, float* out0, float* out1, float* out2,
                                 void* stream) {
    if (!cache || !offset || !hw || !params || !lut || !out0) return SBA_E_ARG;
    if (levels < 1 || levels > 3 || T < 4 || T > 1024 || T % (1 << (levels - 1))) return SBA_E_ARG;
    if (B < 1 || B > 65535 || N < 1) return SBA_E_ARG;
    if (levels >= 2 && (!tab1 || !out1)) return SBA_E_ARG;
    if (levels >= 3 && (!tab2 || !out2)) return SBA_E_ARG;
    BpOut out;
    out.p[0] = out0;
    out.p[1] = levels >= 2 ? out1 : nullptr;
    out.p[2] = levels >= 3 ? out2 : nullptr;
    const int vec = T % 4 == 0 && ((uintptr_t)out0 & 15) == 0;
    const int tiles = cdiv(T, BP_TILE);
    SBA_LAUNCH(batch_pyramid_kernel, dim3(tiles, tiles, B), dim3(BP_THREADS), 0, (hipStream_t)stream, cache, offset, hw,
               N, params, T, levels, tab1, tab2, lut, out, vec);
    return SBA_CHECK_LAUNCH();
}
