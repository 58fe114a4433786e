// k-nearest-neighbour manifold metrics (sba_prdc_knn_radius / sba_prdc_ball_counts in sbagan_hip.h): all-pairs squared
// distances between two sets of f32 feature rows with a row-wise selection fused behind them; the na x nb matrix is never
// written.  d2(i, j) = max((na[i] + nb[j]) - 2 g(i, j), 0), g the dot product on the f64 matrix instruction
// (v_mfma_f64_16x16x4_f64) over the feature axis in ascending order, na / nb the squared norms in f64 in one fixed order
// that depends on the feature index alone.  The f32 inputs are widened in registers: every product is exact in f64.  So
// d2(i, j) has the same bits whichever tile or column split computed it, and d2(i, j) == d2(j, i) bitwise for A = B.
// No atomics, no memset, no allocation: partial results of column splits go to a caller-provided workspace and a second
// small launch merges them in split order.
#include "d2_tile.h"

namespace {

constexpr int PRDC_TLD = D2T_LD;
constexpr int PRDC_K = 8;                       // the longest neighbour list

// ascending list of the PRDC_K smallest values seen
__device__ __forceinline__ void prdc_insert(double (&l)[PRDC_K], double v) {
    if (v < l[PRDC_K - 1]) {
        l[PRDC_K - 1] = v;
#pragma unroll
        for (int m = PRDC_K - 1; m > 0; --m) {
            const double lo = fmin(l[m - 1], l[m]), hi = fmax(l[m - 1], l[m]);
            l[m - 1] = lo;
            l[m] = hi;
        }
    }
}

// MODE 0, k-NN radius (b == a): out_d[(split * na + i) * 8 ..] = the 8 smallest d2(i, j), j != i, of this split's
// columns, ascending, +inf where there are fewer; with `direct` (one split) radius2[i] = entry k - 1 instead.
// MODE 1, ball counts: out_i[(split * na + i) * 2 ..] = #{j : d2 <= rb[j]}, #{j : d2 <= ra[i]} over this split's columns;
// with `direct` they go to in_b[i] / in_own[i].  A null radius vector makes its count 0 (and `direct` skips the write).
// blockIdx.x: block of 64 A rows; blockIdx.y: column split (f64t_split_range).
template <int MODE>
__global__ __launch_bounds__(F64T_THREADS) void prdc_kernel(const float* __restrict__ a, int na, int64_t lda,
                                                            const float* __restrict__ b, int nb, int64_t ldb, int D,
                                                            const double* __restrict__ ra, const double* __restrict__ rb,
                                                            int k, int direct, double* __restrict__ out_d,
                                                            int32_t* __restrict__ out_i0, int32_t* __restrict__ out_i1) {
    __shared__ D2TShared sh;
    double* sh_d2 = d2t_tile_of(sh);                    // the finished tile, afterwards the lists / counts of a row

    const int i0 = blockIdx.x * F64T_TILE;
    int t0, t1;
    f64t_split_range(nb, t0, t1);

    const F64Lanes l = f64t_lanes();
    const int er = threadIdx.x & 63, eq = threadIdx.x >> 6;     // epilogue: row of the tile, 16-column quarter
    const int gi = i0 + er;
    const int sr = threadIdx.x >> 3;                            // staged row of slot 0; slot v: + 32 v

    const float* row[F64T_VEC];
    row[0] = f64t_row(a, na, lda, nullptr, na, i0 + sr);
    row[1] = f64t_row(a, na, lda, nullptr, na, i0 + sr + 32);

    double best[PRDC_K];
#pragma unroll
    for (int m = 0; m < PRDC_K; ++m) best[m] = INFINITY;
    int cnt_b = 0, cnt_own = 0;
    const double r_own = (MODE == 1 && ra && gi < na) ? ra[gi] : 0.0;

    const int chunks = D / F64T_KC;
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * F64T_TILE;
        row[2] = f64t_row(b, nb, ldb, nullptr, nb, j0 + sr);
        row[3] = f64t_row(b, nb, ldb, nullptr, nb, j0 + sr + 32);
        d2t_tile<false>(sh, row, l, chunks);

        // row-wise epilogue: thread (er, eq) takes columns 16 eq .. 16 eq + 15 of row er
        if (gi < na) {
#pragma unroll 4
            for (int q = 0; q < 16; ++q) {
                const int j = 16 * eq + q, gj = j0 + j;
                if (gj >= nb) break;
                const double d2 = sh_d2[er * PRDC_TLD + j];
                if (MODE == 0) {
                    if (gj != gi) prdc_insert(best, d2);        // self is excluded by index: a twin counts, at 0
                } else {
                    if (rb) cnt_b += d2 <= rb[gj];
                    cnt_own += d2 <= r_own;
                }
            }
        }
    }

    // the four quarters of a row, merged in quarter order
    __syncthreads();
    if (MODE == 0) {
#pragma unroll
        for (int m = 0; m < PRDC_K; ++m) sh_d2[(er * 4 + eq) * PRDC_K + m] = best[m];
    } else {
        reinterpret_cast<int*>(sh_d2)[(er * 4 + eq) * 2] = cnt_b;
        reinterpret_cast<int*>(sh_d2)[(er * 4 + eq) * 2 + 1] = cnt_own;
    }
    __syncthreads();
    if (threadIdx.x < F64T_TILE && gi < na) {
        if (MODE == 0) {
            for (int m = PRDC_K; m < 4 * PRDC_K; ++m) prdc_insert(best, sh_d2[er * 4 * PRDC_K + m]);
            if (direct) {
                double r2 = best[0];
#pragma unroll
                for (int m = 1; m < PRDC_K; ++m) r2 = m < k ? best[m] : r2;
                out_d[gi] = r2;
            } else {
                double* __restrict__ o = out_d + ((int64_t)blockIdx.y * na + gi) * PRDC_K;
#pragma unroll
                for (int m = 0; m < PRDC_K; ++m) o[m] = best[m];
            }
        } else {
            const int* __restrict__ p = reinterpret_cast<const int*>(sh_d2) + er * 8;
            const int cb = p[0] + p[2] + p[4] + p[6], co = p[1] + p[3] + p[5] + p[7];
            if (direct) {
                if (out_i0) out_i0[gi] = cb;
                if (out_i1) out_i1[gi] = co;
            } else {
                out_i0[((int64_t)blockIdx.y * na + gi) * 2] = cb;
                out_i0[((int64_t)blockIdx.y * na + gi) * 2 + 1] = co;
            }
        }
    }
}

// the split lists of a row, merged in split order: radius2[i] = the k-th smallest
__global__ __launch_bounds__(256) void prdc_merge_knn_kernel(const double* __restrict__ ws, int n, int S, int k,
                                                             double* __restrict__ radius2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double best[PRDC_K];
#pragma unroll
    for (int m = 0; m < PRDC_K; ++m) best[m] = ws[(int64_t)i * PRDC_K + m];
    for (int s = 1; s < S; ++s)
#pragma unroll
        for (int m = 0; m < PRDC_K; ++m) prdc_insert(best, ws[((int64_t)s * n + i) * PRDC_K + m]);
    double r2 = best[0];
#pragma unroll
    for (int m = 1; m < PRDC_K; ++m) r2 = m < k ? best[m] : r2;
    radius2[i] = r2;
}

__global__ __launch_bounds__(256) void prdc_merge_counts_kernel(const int32_t* __restrict__ ws, int n, int S,
                                                                int32_t* __restrict__ in_b, int32_t* __restrict__ in_own) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int cb = 0, co = 0;
    for (int s = 0; s < S; ++s) {
        cb += ws[((int64_t)s * n + i) * 2];
        co += ws[((int64_t)s * n + i) * 2 + 1];
    }
    if (in_b) in_b[i] = cb;
    if (in_own) in_own[i] = co;
}

inline int prdc_splits(int na, int nb, int splits) {
    return f64t_splits(cdiv(na, F64T_TILE), cdiv(nb, F64T_TILE), splits);
}

}  // namespace

extern "C" int64_t sba_prdc_workspace_bytes(int na, int nb, int splits) {
    if (na < 1 || nb < 1 || splits < 0 || splits > F64T_MAX_SPLITS) return -1;
    const int s = prdc_splits(na, nb, splits);
    return s == 1 ? 0 : (int64_t)s * na * PRDC_K * (int64_t)sizeof(double);
}

extern "C" int sba_prdc_knn_radius(const float* x, int n, int D, int ld, int k, int splits, double* radius2, void* ws,
                                   int64_t ws_bytes, void* stream) {
    if (!radius2 || !f64t_aligned(radius2, 8) || !f64t_rows_ok(x, n, D, ld)) return SBA_E_ARG;
    if (k < 1 || k > PRDC_K || n < k + 1 || splits < 0 || splits > F64T_MAX_SPLITS) return SBA_E_ARG;
    const int S = prdc_splits(n, n, splits);
    if (S > 1 && (!ws || !f64t_aligned(ws, 8) || ws_bytes < sba_prdc_workspace_bytes(n, n, splits))) return SBA_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    SBA_LAUNCH(prdc_kernel<0>, dim3(cdiv(n, F64T_TILE), S), dim3(F64T_THREADS), 0, st, x, n, (int64_t)ld, x, n, (int64_t)ld,
               D, (const double*)nullptr, (const double*)nullptr, k, S == 1 ? 1 : 0, S == 1 ? radius2 : (double*)ws,
               (int32_t*)nullptr, (int32_t*)nullptr);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    if (S == 1) return SBA_OK;
    SBA_LAUNCH(prdc_merge_knn_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, (const double*)ws, n, S, k, radius2);
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_prdc_ball_counts(const float* a, int na, int lda, const float* b, int nb, int ldb, int D,
                                    const double* radius_a, const double* radius_b, int splits, int32_t* in_b,
                                    int32_t* in_own, void* ws, int64_t ws_bytes, void* stream) {
    if (!f64t_rows_ok(a, na, D, lda) || !f64t_rows_ok(b, nb, D, ldb)) return SBA_E_ARG;
    // a count goes with its radius vector: without the vector it is not written, with it it needs somewhere to go
    if ((radius_a && !in_own) || (radius_b && !in_b) || (!radius_a && !radius_b)) return SBA_E_ARG;
    if (!radius_a) in_own = nullptr;
    if (!radius_b) in_b = nullptr;
    if (!f64t_aligned(radius_a, 8) || !f64t_aligned(radius_b, 8) || !f64t_aligned(in_b, 4) || !f64t_aligned(in_own, 4))
        return SBA_E_ARG;
    if (splits < 0 || splits > F64T_MAX_SPLITS) return SBA_E_ARG;
    const int S = prdc_splits(na, nb, splits);
    if (S > 1 && (!ws || !f64t_aligned(ws, 8) || ws_bytes < sba_prdc_workspace_bytes(na, nb, splits))) return SBA_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    SBA_LAUNCH(prdc_kernel<1>, dim3(cdiv(na, F64T_TILE), S), dim3(F64T_THREADS), 0, st, a, na, (int64_t)lda, b, nb,
               (int64_t)ldb, D, radius_a, radius_b, 0, S == 1 ? 1 : 0, (double*)nullptr, S == 1 ? in_b : (int32_t*)ws,
               S == 1 ? in_own : (int32_t*)nullptr);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    if (S == 1) return SBA_OK;
    SBA_LAUNCH(prdc_merge_counts_kernel, dim3(cdiv(na, 256)), dim3(256), 0, st, (const int32_t*)ws, na, S, in_b, in_own);
    return SBA_CHECK_LAUNCH();
}
