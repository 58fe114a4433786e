// Shared by the evaluation units fid.hip, prdc.hip, knn.hip, retrieval.hip and kid.hip: the 64 x 64 float64 tile on the f64
// matrix instruction (v_mfma_f64_16x16x4_f64) that 256 threads compute as four waves of 2 x 2 MFMA tiles.  All use the lane
// map and the MFMA step; prdc.hip and knn.hip (through d2_tile.h), retrieval.hip and kid.hip also the feature-major pair
// tile (dot products of 64 A rows with 64 B rows, the f32 rows widened in registers, features in ascending order) and the
// host side of its column splits.
// Internal linkage, as common.h.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4_t;    // accumulator of one 16x16x4 f64 MFMA

constexpr int F64T_TILE = 64;                   // tile edge: A rows per workgroup and B rows per tile
constexpr int F64T_THREADS = 256;               // four waves, each a 32 x 32 quadrant as 2 x 2 MFMA tiles
constexpr int F64T_KC = 32;                     // features staged per chunk
constexpr int F64T_LD = F64T_KC + 2;            // LDS row stride in floats: the 4-byte operand reads of a 32-lane group (16
                                                // rows x 2 features) fall on bank (2 row + feature) mod 32, all distinct;
                                                // a staged row is 8-byte aligned, so it is stored as two float2
constexpr int F64T_VEC = 2 * F64T_TILE * F64T_KC / 4 / F64T_THREADS;   // float4 loads per thread and chunk (4)
constexpr int F64T_MAX_SPLITS = 32;
constexpr int F64T_FILL = 512;                  // workgroups the library's own split choice aims at (2 per CU)

static_assert(F64T_VEC == 4, "slots 0, 1 stage A rows and slots 2, 3 stage B rows");

// MFMA operands (f32 16x16x4 lane map, one f64 per lane): A[i = lc][k = lk], B[k = lk][j = lc].  C/D of the f64
// instruction: col = lc, row = lk + 4 * reg.
struct F64Lanes {
    int wi, wj;                                 // quadrant of this wave inside the tile
    int lc, lk;                                 // lane & 15, lane >> 4
};
__device__ __forceinline__ F64Lanes f64t_lanes() {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    return F64Lanes{(wave >> 1) * 32, (wave & 1) * 32, lane & 15, lane >> 4};
}
// acc[x][y] += a_x b_y^T over the 4 values of k the lanes hold
__device__ __forceinline__ void f64t_mfma(double a0, double a1, double b0, double b1, f64x4_t (&acc)[2][2]) {
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
}
// f(i, j, value) for this thread's 16 elements of the tile, in (x, y, reg) order
template <class F>
__device__ __forceinline__ void f64t_each(const F64Lanes& l, const f64x4_t (&acc)[2][2], F&& f) {
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int r = 0; r < 4; ++r) f(l.wi + 16 * x + l.lk + 4 * r, l.wj + 16 * y + l.lc, acc[x][y][r]);
}

// ---- the feature-major pair tile.  LDS: float sh[2][F64T_STAGE], staged rows 0 .. 63 of A and 64 .. 127 of B.
constexpr int F64T_STAGE = 2 * F64T_TILE * F64T_LD;

// Slot s of a thread: staged row (threadIdx.x >> 3) + 32 s, features 4 (threadIdx.x & 7) .. + 3 of the chunk.  The address
// of that row's first feature of the slot, or null for a row that reads as zeros: a position past the end of the m
// positions or a row number outside [0, n).  idx: row number per position, null = the position itself.  No address is
// formed from an invalid row.
__device__ __forceinline__ const float* f64t_row(const float* __restrict__ x, int n, int64_t ld,
                                                 const int32_t* __restrict__ idx, int m, int pos) {
    if (pos >= m) return nullptr;
    const int row = idx ? idx[pos] : pos;
    if (row < 0 || row >= n) return nullptr;
    return x + (int64_t)row * ld + ((threadIdx.x & 7) << 2);
}
// (the load goes through a pointer typed as global memory: a row pointer kept across the tile loop is otherwise read
// with flat loads, which also count as LDS traffic in the waits)
__device__ __forceinline__ void f64t_fetch(float4 (&v)[F64T_VEC], const float* (&row)[F64T_VEC], int d0) {
    typedef __attribute__((ext_vector_type(4))) float f32x4_t;
#pragma unroll
    for (int s = 0; s < F64T_VEC; ++s) {
        v[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row[s]) {
            const f32x4_t g = *(const __attribute__((address_space(1))) f32x4_t*)(row[s] + d0);
            v[s] = make_float4(g.x, g.y, g.z, g.w);
        }
    }
}
// registers -> LDS; hook(s, v[s]) sees every slot in order (prdc.hip adds its squared norms there)
struct F64NoHook {
    __device__ __forceinline__ void operator()(int, const float4&) const {}
};
template <class Hook>
__device__ __forceinline__ void f64t_stage(float* __restrict__ buf, const float4 (&v)[F64T_VEC], Hook&& hook) {
#pragma unroll
    for (int s = 0; s < F64T_VEC; ++s) {
        const int e = threadIdx.x + F64T_THREADS * s;
        float* __restrict__ p = buf + (e >> 3) * F64T_LD + ((e & 7) << 2);
        *reinterpret_cast<float2*>(p) = make_float2(v[s].x, v[s].y);
        *reinterpret_cast<float2*>(p + 2) = make_float2(v[s].z, v[s].w);
        hook(s, v[s]);
    }
}
// acc += the dot products of the tile over the chunk of features staged in buf.  The chunk loop around it (fetch the next
// chunk, this, stage the next chunk, one barrier) stays written out in d2t_tile (d2_tile.h) and kid_kernel: as a function here,
// the compiler stopped hoisting the stage and epilogue addresses out of the tile loop, and kid_kernel measured 0.3 - 0.6 %
// slower (profiles/eval_tile_refactor.txt).
__device__ __forceinline__ void f64t_chunk(const float* __restrict__ buf, const F64Lanes& l, f64x4_t (&acc)[2][2]) {
    for (int s = 0; s < F64T_KC / 4; ++s) {
        const int d = 4 * s + l.lk;
        const double a0 = (double)buf[(l.wi + l.lc) * F64T_LD + d], a1 = (double)buf[(l.wi + 16 + l.lc) * F64T_LD + d];
        const double b0 = (double)buf[(F64T_TILE + l.wj + l.lc) * F64T_LD + d];
        const double b1 = (double)buf[(F64T_TILE + l.wj + 16 + l.lc) * F64T_LD + d];
        f64t_mfma(a0, a1, b0, b1, acc);
    }
}
// the B tiles [t0, t1) of column split blockIdx.y of gridDim.y: [y T / S, (y + 1) T / S)
__device__ __forceinline__ void f64t_split_range(int nb, int& t0, int& t1) {
    const int tiles = (nb + F64T_TILE - 1) / F64T_TILE, S = gridDim.y;
    t0 = (int)((int64_t)blockIdx.y * tiles / S);
    t1 = (int)((int64_t)(blockIdx.y + 1) * tiles / S);
}

// ---- host side
inline bool f64t_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// f32 feature rows the kernels can read: n >= 1 rows of D % 64 == 0 features, 16-byte aligned, row stride ld >= D and a
// multiple of 4
inline bool f64t_rows_ok(const float* x, int n, int D, int ld) {
    return x && n >= 1 && D >= F64T_TILE && D % F64T_TILE == 0 && ld >= D && ld % 4 == 0 && f64t_aligned(x, 16);
}

// the column splits of a launch of `blocks` workgroups a split over `tiles` B tiles: the caller's, or enough to put
// F64T_FILL workgroups on the chip; never more than B tiles
inline int f64t_splits(int64_t blocks, int tiles, int requested) {
    int s = requested > 0 ? requested : cdiv(F64T_FILL, blocks);
    s = s < F64T_MAX_SPLITS ? s : F64T_MAX_SPLITS;
    return s < tiles ? s : tiles;
}

}  // namespace
