// Kernel Inception Distance (sba_kid_kernel_sums in sbagan_hip.h): for every subset s, the sum over pairs of subset
// positions (i, j) of the polynomial kernel k(x, y) = (x . y / D + 1)^3 between gathered f32 feature rows,
//     sums[s] = sum_{i < ma, j < mb, (i != j)} k(a[idx_a[s][i]], b[idx_b[s][j]]).
// The dot product runs on the f64 matrix instruction (v_mfma_f64_16x16x4_f64) over the feature axis in ascending order,
// on the 64 x 64 pair tile of f64_tile.h (the one prdc.hip uses; no norms); the f32 inputs are widened in registers, so
// every product is exact.  The m x m kernel matrix is never written.  No atomics, no memset, no allocation: every
// workgroup writes one f64 partial to a caller-provided workspace and a second small launch adds the partials of a
// subset in (block, split) order.
#include "f64_tile.h"

namespace {

constexpr int KID_MAX_SUBSETS = 1024;

// blockIdx.x: block of 64 A positions; blockIdx.y: column split (f64t_split_range); blockIdx.z: subset.
// part[(z * gridDim.x + x) * gridDim.y + y] = this workgroup's sum.
__global__ __launch_bounds__(F64T_THREADS) void kid_kernel(const float* __restrict__ a, int na, int64_t lda,
                                                           const int32_t* __restrict__ idx_a, int ma,
                                                           const float* __restrict__ b, int nb, int64_t ldb,
                                                           const int32_t* __restrict__ idx_b, int mb, int D,
                                                           int exclude_diag, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sh[2][F64T_STAGE];
    __shared__ int sh_ok[2 * F64T_TILE];                // per staged row: it counts (in its subset and in its row set)
    __shared__ double sh_red[F64T_THREADS];

    const int i0 = blockIdx.x * F64T_TILE, sub = blockIdx.z;
    int t0, t1;
    f64t_split_range(mb, t0, t1);
    const int32_t* __restrict__ ia = idx_a ? idx_a + (int64_t)sub * ma : nullptr;
    const int32_t* __restrict__ ib = idx_b ? idx_b + (int64_t)sub * mb : nullptr;

    const F64Lanes l = f64t_lanes();
    const int sr = threadIdx.x >> 3;                            // staged row of slot 0; slot v: + 32 v

    const float* row[F64T_VEC];
    row[0] = f64t_row(a, na, lda, ia, ma, i0 + sr);
    row[1] = f64t_row(a, na, lda, ia, ma, i0 + sr + 32);
    const double width = (double)D;
    double total = 0.0;

    const int chunks = D / F64T_KC;
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * F64T_TILE;
        row[2] = f64t_row(b, nb, ldb, ib, mb, j0 + sr);
        row[3] = f64t_row(b, nb, ldb, ib, mb, j0 + sr + 32);
        f64x4_t acc[2][2];
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) acc[x][y] = f64x4_t{0.0, 0.0, 0.0, 0.0};
        float4 v[F64T_VEC];
        f64t_fetch(v, row, 0);
        __syncthreads();                // the previous tile's epilogue has read sh_ok
        f64t_stage(sh[0], v, F64NoHook());
        if ((threadIdx.x & 7) == 0) {
#pragma unroll
            for (int s = 0; s < F64T_VEC; ++s) sh_ok[sr + 32 * s] = row[s] != nullptr;
        }
        __syncthreads();
        for (int c = 0; c < chunks; ++c) {
            const bool more = c + 1 < chunks;
            if (more) f64t_fetch(v, row, (c + 1) * F64T_KC);
            f64t_chunk(sh[c & 1], l, acc);
            if (more) f64t_stage(sh[(c + 1) & 1], v, F64NoHook());    // last read in iteration c - 1, which every
                                                                      // wave has left
            __syncthreads();
        }

        // the polynomial of this thread's 16 elements, added in (x, y, reg) order; pairs are told apart by POSITION
        // (not through f64t_each: with the walk the compiler branches around the flag tests instead of selecting)
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = l.wi + 16 * x + l.lk + 4 * r, j = l.wj + 16 * y + l.lc;
                    const bool on = sh_ok[i] && sh_ok[F64T_TILE + j] && !(exclude_diag && i0 + i == j0 + j);
                    const double tt = acc[x][y][r] / width + 1.0;
                    const double kk = (tt * tt) * tt;
                    total += on ? kk : 0.0;
                }
    }

    // the 256 thread sums, halved in one fixed order
    sh_red[threadIdx.x] = total;
    __syncthreads();
#pragma unroll
    for (int h = F64T_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh_red[threadIdx.x] += sh_red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[((int64_t)sub * gridDim.x + blockIdx.x) * gridDim.y + blockIdx.y] = sh_red[0];
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

inline int kid_splits(int ma, int mb, int subsets, int splits) {
    return f64t_splits((int64_t)cdiv(ma, F64T_TILE) * subsets, cdiv(mb, F64T_TILE), splits);
}

inline bool kid_shape_ok(int ma, int mb, int subsets, int splits) {
    return ma >= 1 && mb >= 1 && subsets >= 1 && subsets <= KID_MAX_SUBSETS && splits >= 0 && splits <= F64T_MAX_SPLITS;
}

}  // namespace

extern "C" int64_t sba_kid_workspace_bytes(int ma, int mb, int subsets, int splits) {
    if (!kid_shape_ok(ma, mb, subsets, splits)) return -1;
    const int64_t P = (int64_t)cdiv(ma, F64T_TILE) * kid_splits(ma, mb, subsets, splits);
    return P == 1 ? 0 : P * subsets * (int64_t)sizeof(double);
}

extern "C" int sba_kid_kernel_sums(const float* a, int na, int lda, const int32_t* idx_a, int ma, const float* b, int nb,
                                   int ldb, const int32_t* idx_b, int mb, int D, int subsets, int exclude_diag,
                                   int splits, double* sums, void* ws, int64_t ws_bytes, void* stream) {
    if (!f64t_rows_ok(a, na, D, lda) || !f64t_rows_ok(b, nb, D, ldb) || !kid_shape_ok(ma, mb, subsets, splits))
        return SBA_E_ARG;
    if (!f64t_aligned(idx_a, 4) || !f64t_aligned(idx_b, 4) || !sums || !f64t_aligned(sums, 8)) return SBA_E_ARG;
    if (exclude_diag && ma != mb) return SBA_E_ARG;
    const int blocks = cdiv(ma, F64T_TILE), S = kid_splits(ma, mb, subsets, splits), P = blocks * S;
    if (P > 1 && (!ws || !f64t_aligned(ws, 8) || ws_bytes < sba_kid_workspace_bytes(ma, mb, subsets, splits)))
        return SBA_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    SBA_LAUNCH(kid_kernel, dim3(blocks, S, subsets), dim3(F64T_THREADS), 0, st, a, na, (int64_t)lda, idx_a, ma, b, nb,
               (int64_t)ldb, idx_b, mb, D, exclude_diag ? 1 : 0, P == 1 ? sums : (double*)ws);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    if (P == 1) return SBA_OK;
    SBA_LAUNCH(kid_finish_kernel, dim3(cdiv(subsets, 256)), dim3(256), 0, st, (const double*)ws, subsets, P, sums);
    return SBA_CHECK_LAUNCH();
}
