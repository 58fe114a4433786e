// Kernel Inception Distance (sba_kid_kernel_sums in sbagan_hip.h): for every subset s, the sum over pairs of subset
// positions (i, j) of the polynomial kernel k(x, y) = (x . y / D + 1)^3 between gathered f32 feature rows,
//     sums[s] = sum_{i < ma, j < mb, (i != j)} k(a[idx_a[s][i]], b[idx_b[s][j]]).
// The dot product runs on the f64 matrix instruction (v_mfma_f64_16x16x4_f64) over the feature axis in ascending order,
// on the 64 x 64 tile of prdc.hip (same instruction, lane map and LDS stride; no norms); the f32 inputs are widened in
// registers, so every product is exact.  The m x m kernel matrix is never written.  No atomics, no memset, no allocation:
// every workgroup writes one f64 partial to a caller-provided workspace and a second small launch adds the partials of a
// subset in (block, split) order.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4_t;    // accumulator of one 16x16x4 f64 MFMA

constexpr int KID_TILE = 64;                    // A positions per workgroup and B positions per tile
constexpr int KID_THREADS = 256;                // four waves, each a 32 x 32 quadrant as 2 x 2 MFMA tiles
constexpr int KID_KC = 32;                      // features staged per chunk
constexpr int KID_LD = KID_KC + 2;              // LDS row stride in floats (bank-conflict free: see prdc.hip)
constexpr int KID_VEC = 2 * KID_TILE * KID_KC / 4 / KID_THREADS;       // float4 loads per thread and chunk (4)
constexpr int KID_MAX_SPLITS = 32;
constexpr int KID_MAX_SUBSETS = 1024;
constexpr int KID_FILL = 512;                   // workgroups the library's own split choice aims at (2 per CU)

static_assert(KID_VEC == 4, "slots 0, 1 stage A rows and slots 2, 3 stage B rows");

// Slot v of a thread: staged row (threadIdx.x >> 3) + 32 v (0 .. 63 of A, 64 .. 127 of B), features 4 (threadIdx.x & 7)
// .. + 3 of the chunk.  The address of that row's first feature of the slot, or null for a row that reads as zeros: a
// position past the end of the subset or an index outside [0, n).  No address is formed from such an index.
__device__ __forceinline__ const float* kid_row(const float* __restrict__ x, int n, int64_t ld,
                                                const int32_t* __restrict__ idx, int m, int pos) {
    if (pos >= m) return nullptr;
    const int row = idx ? idx[pos] : pos;
    if (row < 0 || row >= n) return nullptr;
    return x + (int64_t)row * ld + ((threadIdx.x & 7) << 2);
}
__device__ __forceinline__ void kid_fetch(float4 (&v)[KID_VEC], const float* (&row)[KID_VEC], int d0) {
#pragma unroll
    for (int s = 0; s < KID_VEC; ++s)
        v[s] = row[s] ? *reinterpret_cast<const float4*>(row[s] + d0) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void kid_stage(float* __restrict__ buf, const float4 (&v)[KID_VEC]) {
#pragma unroll
    for (int s = 0; s < KID_VEC; ++s) {
        const int e = threadIdx.x + KID_THREADS * s;
        float* __restrict__ p = buf + (e >> 3) * KID_LD + ((e & 7) << 2);
        *reinterpret_cast<float2*>(p) = make_float2(v[s].x, v[s].y);
        *reinterpret_cast<float2*>(p + 2) = make_float2(v[s].z, v[s].w);
    }
}

// blockIdx.x: block of 64 A positions; blockIdx.y: column split, B tiles [y T / S, (y + 1) T / S); blockIdx.z: subset.
// part[(z * gridDim.x + x) * gridDim.y + y] = this workgroup's sum.
// MFMA operands and C/D layout as in prdc_kernel: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15];
// C/D: col = lane & 15, row = (lane >> 4) + 4 * reg.
__global__ __launch_bounds__(KID_THREADS) void kid_kernel(const float* __restrict__ a, int na, int64_t lda,
                                                          const int32_t* __restrict__ idx_a, int ma,
                                                          const float* __restrict__ b, int nb, int64_t ldb,
                                                          const int32_t* __restrict__ idx_b, int mb, int D,
                                                          int exclude_diag, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sh[2][2 * KID_TILE * KID_LD];
    __shared__ int sh_ok[2 * KID_TILE];                 // per staged row: it counts (in its subset and in its row set)
    __shared__ double sh_red[KID_THREADS];

    const int i0 = blockIdx.x * KID_TILE, sub = blockIdx.z;
    const int tiles = (mb + KID_TILE - 1) / KID_TILE, S = gridDim.y;
    const int t0 = (int)((int64_t)blockIdx.y * tiles / S), t1 = (int)((int64_t)(blockIdx.y + 1) * tiles / S);
    const int32_t* __restrict__ ia = idx_a ? idx_a + (int64_t)sub * ma : nullptr;
    const int32_t* __restrict__ ib = idx_b ? idx_b + (int64_t)sub * mb : nullptr;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;      // quadrant of this wave inside the tile
    const int lc = lane & 15, lk = lane >> 4;
    const int sr = threadIdx.x >> 3;                            // staged row of slot 0; slot v: + 32 v

    const float* row[KID_VEC];
    row[0] = kid_row(a, na, lda, ia, ma, i0 + sr);
    row[1] = kid_row(a, na, lda, ia, ma, i0 + sr + 32);
    const double width = (double)D;
    double total = 0.0;

    const int chunks = D / KID_KC;
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * KID_TILE;
        row[2] = kid_row(b, nb, ldb, ib, mb, j0 + sr);
        row[3] = kid_row(b, nb, ldb, ib, mb, j0 + sr + 32);
        f64x4_t acc[2][2];
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) acc[x][y] = f64x4_t{0.0, 0.0, 0.0, 0.0};

        float4 v[KID_VEC];
        kid_fetch(v, row, 0);
        __syncthreads();                // the previous tile's epilogue has read sh_ok
        kid_stage(sh[0], v);
        if ((threadIdx.x & 7) == 0) {
#pragma unroll
            for (int s = 0; s < KID_VEC; ++s) sh_ok[sr + 32 * s] = row[s] != nullptr;
        }
        __syncthreads();
        for (int c = 0; c < chunks; ++c) {
            const float* __restrict__ buf = sh[c & 1];
            const bool more = c + 1 < chunks;
            if (more) kid_fetch(v, row, (c + 1) * KID_KC);
            for (int s = 0; s < KID_KC / 4; ++s) {
                const int d = 4 * s + lk;
                const double a0 = (double)buf[(wi + lc) * KID_LD + d], a1 = (double)buf[(wi + 16 + lc) * KID_LD + d];
                const double b0 = (double)buf[(KID_TILE + wj + lc) * KID_LD + d];
                const double b1 = (double)buf[(KID_TILE + wj + 16 + lc) * KID_LD + d];
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
            if (more) kid_stage(sh[(c + 1) & 1], v);          // last read in iteration c - 1, which every wave has left
            __syncthreads();
        }

        // the polynomial of this thread's 16 elements, added in (x, y, reg) order; pairs are told apart by POSITION
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = wi + 16 * x + lk + 4 * r, j = wj + 16 * y + lc;
                    const bool on = sh_ok[i] && sh_ok[KID_TILE + j] && !(exclude_diag && i0 + i == j0 + j);
                    const double tt = acc[x][y][r] / width + 1.0;
                    const double kk = (tt * tt) * tt;
                    total += on ? kk : 0.0;
                }
    }

    // the 256 thread sums, halved in one fixed order
    sh_red[threadIdx.x] = total;
    __syncthreads();
#pragma unroll
    for (int h = KID_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh_red[threadIdx.x] += sh_red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[((int64_t)sub * gridDim.x + blockIdx.x) * S + blockIdx.y] = sh_red[0];
}

// sums[s] = the P partials of subset s, added in (block, split) order
__global__ __launch_bounds__(256) void kid_finish_kernel(const double* __restrict__ part, int subsets, int P,
                                                         double* __restrict__ sums) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= subsets) return;
    const double* __restrict__ p = part + (int64_t)s * P;
    double t = p[0];
    for (int q = 1; q < P; ++q) t += p[q];
    sums[s] = t;
}

inline bool kid_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// the column splits of a launch: the caller's, or enough to put KID_FILL workgroups on the chip; never more than B tiles
inline int kid_splits(int ma, int mb, int subsets, int splits) {
    const int64_t groups = (int64_t)cdiv(ma, KID_TILE) * subsets;
    const int tiles = cdiv(mb, KID_TILE);
    int s = splits > 0 ? splits : cdiv(KID_FILL, groups);
    s = s < KID_MAX_SPLITS ? s : KID_MAX_SPLITS;
    return s < tiles ? s : tiles;
}

inline bool kid_shape_ok(int ma, int mb, int subsets, int splits) {
    return ma >= 1 && mb >= 1 && subsets >= 1 && subsets <= KID_MAX_SUBSETS && splits >= 0 && splits <= KID_MAX_SPLITS;
}

inline bool kid_rows_ok(const float* x, int n, int D, int ld) {
    return x && n >= 1 && D >= KID_TILE && D % KID_TILE == 0 && ld >= D && ld % 4 == 0 && kid_aligned(x, 16);
}

}  // namespace

extern "C" int64_t sba_kid_workspace_bytes(int ma, int mb, int subsets, int splits) {
    if (!kid_shape_ok(ma, mb, subsets, splits)) return -1;
    const int64_t P = (int64_t)cdiv(ma, KID_TILE) * kid_splits(ma, mb, subsets, splits);
    return P == 1 ? 0 : P * subsets * (int64_t)sizeof(double);
}

extern "C" int sba_kid_kernel_sums(const float* a, int na, int lda, const int32_t* idx_a, int ma, const float* b, int nb,
                                   int ldb, const int32_t* idx_b, int mb, int D, int subsets, int exclude_diag,
                                   int splits, double* sums, void* ws, int64_t ws_bytes, void* stream) {
    if (!kid_rows_ok(a, na, D, lda) || !kid_rows_ok(b, nb, D, ldb) || !kid_shape_ok(ma, mb, subsets, splits))
        return SBA_E_ARG;
    if (!kid_aligned(idx_a, 4) || !kid_aligned(idx_b, 4) || !sums || !kid_aligned(sums, 8)) return SBA_E_ARG;
    if (exclude_diag && ma != mb) return SBA_E_ARG;
    const int blocks = cdiv(ma, KID_TILE), S = kid_splits(ma, mb, subsets, splits), P = blocks * S;
    if (P > 1 && (!ws || !kid_aligned(ws, 8) || ws_bytes < sba_kid_workspace_bytes(ma, mb, subsets, splits)))
        return SBA_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    SBA_LAUNCH(kid_kernel, dim3(blocks, S, subsets), dim3(KID_THREADS), 0, st, a, na, (int64_t)lda, idx_a, ma, b, nb,
               (int64_t)ldb, idx_b, mb, D, exclude_diag ? 1 : 0, P == 1 ? sums : (double*)ws);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    if (P == 1) return SBA_OK;
    SBA_LAUNCH(kid_finish_kernel, dim3(cdiv(subsets, 256)), dim3(256), 0, st, (const double*)ws, subsets, P, sums);
    return SBA_CHECK_LAUNCH();
}
