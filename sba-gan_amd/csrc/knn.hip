// Nearest rows of another set (sba_knn_topk in sbagan_hip.h): for every row i of A the k rows j of B with the smallest key
// (d2(i, j), j), ascending, d2 the float64 squared distance of d2_tile.h -- the value prdc.hip computes, bit for bit; the
// na x nb matrix is never written.  The key is a total order on the listable pairs (a NaN compares below nothing, so it
// is never listed; an unused place is (+inf, -1), below which no pair with j >= 0 and d2 = +inf falls), so the k smallest
// are the same set in the same order however they were gathered: per thread over a quarter of each tile, per row over the
// four quarters, per launch over the column splits.  No atomics, no memset, no allocation: the lists of column splits go
// to a caller-provided workspace and a second small launch merges them.
#include "d2_tile.h"

namespace {

constexpr int KNN_K = 8;                        // the longest neighbour list

struct KnnList {                                // ascending under knn_less; unused places (+inf, -1)
    double d[KNN_K];
    int32_t j[KNN_K];
};

__device__ __forceinline__ bool knn_less(double d, int32_t j, double e, int32_t i) { return d < e || (d == e && j < i); }

__device__ __forceinline__ void knn_clear(KnnList& l) {
#pragma unroll
    for (int m = 0; m < KNN_K; ++m) {
        l.d[m] = INFINITY;
        l.j[m] = -1;
    }
}

__device__ __forceinline__ void knn_insert(KnnList& l, double d, int32_t j) {
    if (knn_less(d, j, l.d[KNN_K - 1], l.j[KNN_K - 1])) {
        l.d[KNN_K - 1] = d;
        l.j[KNN_K - 1] = j;
#pragma unroll
        for (int m = KNN_K - 1; m > 0; --m) {
            const bool up = knn_less(l.d[m], l.j[m], l.d[m - 1], l.j[m - 1]);
            const double dlo = up ? l.d[m] : l.d[m - 1], dhi = up ? l.d[m - 1] : l.d[m];
            const int32_t jlo = up ? l.j[m] : l.j[m - 1], jhi = up ? l.j[m - 1] : l.j[m];
            l.d[m - 1] = dlo;
            l.d[m] = dhi;
            l.j[m - 1] = jlo;
            l.j[m] = jhi;
        }
    }
}

// out_d / out_j [(split * na + i) * k ..]: the k smallest (d2(i, j), j) over this split's columns.  With one split that
// is the result itself, with several the workspace.  blockIdx.x: block of 64 A rows; blockIdx.y: column split
// (f64t_split_range).  Three waves per SIMD, which the 44 032 bytes of LDS a workgroup takes admit as well: with that bound
// the compiler keeps the accumulators and the lists in 166 VGPRs, no AGPRs and no scratch (without it 166 + 32 and two
// waves).
__global__ __launch_bounds__(F64T_THREADS, 3) void knn_kernel(const float* __restrict__ a, int na, int64_t lda,
                                                           const float* __restrict__ b, int nb, int64_t ldb, int D, int k,
                                                           double* __restrict__ out_d, int32_t* __restrict__ out_j) {
    __shared__ D2TShared sh;
    static_assert(F64T_TILE * 4 * KNN_K * (sizeof(double) + sizeof(int32_t)) <= sizeof(D2TShared::stage),
                  "the quarter lists of the 64 rows live in the staging buffers");
    double* sh_d2 = d2t_tile_of(sh);                    // the finished tile, afterwards the quarter lists of the rows
    int32_t* sh_j = reinterpret_cast<int32_t*>(sh_d2 + F64T_TILE * 4 * KNN_K);

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

    KnnList best;
    knn_clear(best);

    const int chunks = D / F64T_KC;
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * F64T_TILE;
        row[2] = f64t_row(b, nb, ldb, nullptr, nb, j0 + sr);
        row[3] = f64t_row(b, nb, ldb, nullptr, nb, j0 + sr + 32);
        d2t_tile<true>(sh, row, l, chunks);

        // row-wise epilogue: thread (er, eq) takes columns 16 eq .. 16 eq + 15 of row er
        if (gi < na) {
#pragma unroll 4
            for (int q = 0; q < 16; ++q) {
                const int j = 16 * eq + q, gj = j0 + j;
                if (gj >= nb) break;
                knn_insert(best, sh_d2[er * D2T_LD + j], gj);
            }
        }
    }

    // the four quarters of a row, merged under the same key
    __syncthreads();
#pragma unroll
    for (int m = 0; m < KNN_K; ++m) {
        sh_d2[(er * 4 + eq) * KNN_K + m] = best.d[m];
        sh_j[(er * 4 + eq) * KNN_K + m] = best.j[m];
    }
    __syncthreads();
    if (threadIdx.x < F64T_TILE && gi < na) {
        for (int m = KNN_K; m < 4 * KNN_K; ++m) knn_insert(best, sh_d2[er * 4 * KNN_K + m], sh_j[er * 4 * KNN_K + m]);
        const int64_t o = ((int64_t)blockIdx.y * na + gi) * k;
#pragma unroll
        for (int m = 0; m < KNN_K; ++m)
            if (m < k) {
                out_d[o + m] = best.d[m];
                out_j[o + m] = best.j[m];
            }
    }
}

// the split lists of a row [S][n][k], merged under the same key
__global__ __launch_bounds__(256) void knn_merge_kernel(const double* __restrict__ ws_d, const int32_t* __restrict__ ws_j,
                                                        int n, int S, int k, double* __restrict__ d2,
                                                        int32_t* __restrict__ idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    KnnList best;
    knn_clear(best);
    for (int s = 0; s < S; ++s) {
        const int64_t o = ((int64_t)s * n + i) * k;
        for (int m = 0; m < k; ++m) knn_insert(best, ws_d[o + m], ws_j[o + m]);
    }
#pragma unroll
    for (int m = 0; m < KNN_K; ++m)
        if (m < k) {
            d2[(int64_t)i * k + m] = best.d[m];
            idx[(int64_t)i * k + m] = best.j[m];
        }
}

inline int knn_splits(int na, int nb, int splits) {
    return f64t_splits(cdiv(na, F64T_TILE), cdiv(nb, F64T_TILE), splits);
}

}  // namespace

extern "C" int64_t sba_knn_workspace_bytes(int na, int nb, int k, int splits) {
    if (na < 1 || nb < 1 || k < 1 || k > KNN_K || splits < 0 || splits > F64T_MAX_SPLITS) return -1;
    const int s = knn_splits(na, nb, splits);
    return s == 1 ? 0 : (int64_t)s * na * k * (int64_t)(sizeof(double) + sizeof(int32_t));
}

extern "C" int sba_knn_topk(const float* a, int na, int lda, const float* b, int nb, int ldb, int D, int k, int splits,
                            double* d2, int32_t* idx, void* ws, int64_t ws_bytes, void* stream) {
    if (!d2 || !idx || !f64t_aligned(d2, 8) || !f64t_aligned(idx, 4)) return SBA_E_ARG;
    if (!f64t_rows_ok(a, na, D, lda) || !f64t_rows_ok(b, nb, D, ldb)) return SBA_E_ARG;
    if (k < 1 || k > KNN_K || splits < 0 || splits > F64T_MAX_SPLITS) return SBA_E_ARG;
    const int S = knn_splits(na, nb, splits);
    if (S > 1 && (!ws || !f64t_aligned(ws, 8) || ws_bytes < sba_knn_workspace_bytes(na, nb, k, splits))) return SBA_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    double* ws_d = (double*)ws;                         // [S][na][k] distances, then as many row numbers
    int32_t* ws_j = S > 1 ? (int32_t*)(ws_d + (int64_t)S * na * k) : nullptr;
    SBA_LAUNCH(knn_kernel, dim3(cdiv(na, F64T_TILE), S), dim3(F64T_THREADS), 0, st, a, na, (int64_t)lda, b, nb, (int64_t)ldb,
               D, k, S == 1 ? d2 : ws_d, S == 1 ? idx : ws_j);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    if (S == 1) return SBA_OK;
    SBA_LAUNCH(knn_merge_kernel, dim3(cdiv(na, 256)), dim3(256), 0, st, (const double*)ws_d, (const int32_t*)ws_j, na, S, k,
               d2, idx);
    return SBA_CHECK_LAUNCH();
}
