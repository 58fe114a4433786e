// Cross-modal retrieval ranks (sba_retrieval_own_best / sba_retrieval_counts in sbagan_hip.h): all-pairs cosine scores
// between two sets of f32 code rows with a row-wise selection fused behind them; the na x nb matrix is never written.
//     s(i, j) = g(i, j) / max(sqrt(na[i] * nb[j]), eps)
// g the dot product on the f64 matrix instruction (v_mfma_f64_16x16x4_f64) over the feature axis in ascending order, na /
// nb the squared norms in f64 in one fixed order that depends on the feature index alone.  The f32 inputs are widened in
// registers: every product is exact in f64.  The product of the norms commutes, square root and division are the IEEE
// operations (this unit is not built with fast-math, and the epilogue holds no a * b + c for the compiler to contract).
// So s(i, j) has the same bits whichever tile, column split or launch computed it, and whichever set is the A side: a
// threshold taken by one launch compares exactly in the next.  No atomics, no memset, no allocation: partial results of
// column splits go to a caller-provided workspace and a second small launch merges them in split order.
#include "f64_tile.h"

namespace {

constexpr int RTV_TLD = F64T_TILE + 1;          // row stride of the finished score tile in doubles

// the running maximum of the own scores: a NaN, once seen, stays
__device__ __forceinline__ double rtv_best(double best, double s) {
    return (best != best || s != s) ? (double)NAN : fmax(best, s);
}

// MODE 0, own best: out_d[split * na + i] = the largest s(i, j) over this split's rows j with key_b[j] == key_a[i], -inf
// when there is none, NaN when one of them is NaN; with `direct` (one split) the index is i.
// MODE 1, counts: out_i[(split * na + i) * 2 ..] = #{j : key_b[j] != key_a[i], NOT (s(i, j) < thr[i])} over this split's
// rows, and the same count over the rows whose class also differs from cls_a[i] (0 without the class vectors); with
// `direct` they go to out_i[i] / out_m[i] (out_m only with the class vectors).
// blockIdx.x: block of 64 A rows; blockIdx.y: column split (f64t_split_range).
template <int MODE>
__global__ __launch_bounds__(F64T_THREADS) void rtv_kernel(const float* __restrict__ a, int na, int64_t lda,
                                                           const float* __restrict__ b, int nb, int64_t ldb, int D,
                                                           const int32_t* __restrict__ key_a,
                                                           const int32_t* __restrict__ key_b,
                                                           const int32_t* __restrict__ cls_a,
                                                           const int32_t* __restrict__ cls_b,
                                                           const double* __restrict__ thr, double eps, int direct,
                                                           double* __restrict__ out_d, int32_t* __restrict__ out_i,
                                                           int32_t* __restrict__ out_m) {
    __shared__ __attribute__((aligned(16))) float sh[2][F64T_STAGE];
    __shared__ double sh_part[2 * F64T_TILE][8];        // per staged row: the norm partials of its 8 feature groups
    __shared__ double sh_norm[2 * F64T_TILE];
    __shared__ int32_t sh_key[2][F64T_TILE];            // key and class of the tile's B rows
    static_assert(sizeof(double) * F64T_TILE * RTV_TLD <= sizeof(sh), "the score tile lives in the staging buffers");
    double* sh_s = reinterpret_cast<double*>(&sh[0][0]);        // the finished tile, afterwards the partials of a row:
                                                        // over the staging buffers, which are idle by then

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

    const bool masked = MODE == 1 && cls_a && cls_b;
    const int32_t my_key = gi < na ? key_a[gi] : 0;
    const int32_t my_cls = (masked && gi < na) ? cls_a[gi] : 0;
    const double my_thr = (MODE == 1 && gi < na) ? thr[gi] : 0.0;
    double best = -INFINITY;
    int cnt = 0, cnt_m = 0;

    const int chunks = D / F64T_KC;
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * F64T_TILE;
        row[2] = f64t_row(b, nb, ldb, nullptr, nb, j0 + sr);
        row[3] = f64t_row(b, nb, ldb, nullptr, nb, j0 + sr + 32);
        f64x4_t acc[2][2];
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y) acc[x][y] = f64x4_t{0.0, 0.0, 0.0, 0.0};
        double nrm[F64T_VEC];
#pragma unroll
        for (int s = 0; s < F64T_VEC; ++s) nrm[s] = 0.0;
        // the squared norm of the staged rows: slot s of this thread always holds the same 4 features of the same row, so
        // nrm[s] adds those features over the chunks in ascending order (the products are exact, so the fma rounds as the
        // separate multiply and add would)
        const auto norms = [&](int s, const float4& x) {
            const double x0 = (double)x.x, x1 = (double)x.y, x2 = (double)x.z, x3 = (double)x.w;
            nrm[s] = fma(x3, x3, fma(x2, x2, fma(x1, x1, fma(x0, x0, nrm[s]))));
        };

        float4 v[F64T_VEC];
        f64t_fetch(v, row, 0);
        int32_t kv = 0;                 // threads 0 .. 63: key of B row j0 + threadIdx.x; 64 .. 127: its class
        if (threadIdx.x < F64T_TILE) {
            if (j0 + (int)threadIdx.x < nb) kv = key_b[j0 + threadIdx.x];
        } else if (threadIdx.x < 2 * F64T_TILE) {
            if (masked && j0 + (int)threadIdx.x - F64T_TILE < nb) kv = cls_b[j0 + threadIdx.x - F64T_TILE];
        }
        __syncthreads();                // the previous tile's epilogue has read the score tile these buffers held
        f64t_stage(sh[0], v, norms);
        if (threadIdx.x < 2 * F64T_TILE) sh_key[threadIdx.x >> 6][threadIdx.x & 63] = kv;
        __syncthreads();
        for (int c = 0; c < chunks; ++c) {
            const bool more = c + 1 < chunks;
            if (more) f64t_fetch(v, row, (c + 1) * F64T_KC);
            f64t_chunk(sh[c & 1], l, acc);
            if (more) f64t_stage(sh[(c + 1) & 1], v, norms);  // last read in iteration c - 1, which every wave has left
            __syncthreads();
        }

        // squared norms of the 128 staged rows: 8 partials per row, added in feature order
#pragma unroll
        for (int s = 0; s < F64T_VEC; ++s) sh_part[sr + 32 * s][threadIdx.x & 7] = nrm[s];
        __syncthreads();
        if (threadIdx.x < 2 * F64T_TILE) {
            const double* __restrict__ p = sh_part[threadIdx.x];
            sh_norm[threadIdx.x] = ((((((p[0] + p[1]) + p[2]) + p[3]) + p[4]) + p[5]) + p[6]) + p[7];
        }
        __syncthreads();
        f64t_each(l, acc, [&](int i, int j, double g) {
            sh_s[i * RTV_TLD + j] = g / fmax(sqrt(sh_norm[i] * sh_norm[F64T_TILE + j]), eps);
        });
        __syncthreads();

        // row-wise epilogue: thread (er, eq) takes columns 16 eq .. 16 eq + 15 of row er
        if (gi < na) {
#pragma unroll 4
            for (int q = 0; q < 16; ++q) {
                const int j = 16 * eq + q;
                if (j0 + j >= nb) break;
                const double s = sh_s[er * RTV_TLD + j];
                const bool own = sh_key[0][j] == my_key;        // own pairs go by key, never by value
                if (MODE == 0) {
                    if (own) best = rtv_best(best, s);
                } else if (!own) {
                    const int c = !(s < my_thr);                // a tie and a NaN on either side count
                    cnt += c;
                    if (masked && sh_key[1][j] != my_cls) cnt_m += c;
                }
            }
        }
    }

    // the four quarters of a row, merged in quarter order
    __syncthreads();
    if (MODE == 0) {
        sh_s[er * 4 + eq] = best;
    } else {
        reinterpret_cast<int*>(sh_s)[(er * 4 + eq) * 2] = cnt;
        reinterpret_cast<int*>(sh_s)[(er * 4 + eq) * 2 + 1] = cnt_m;
    }
    __syncthreads();
    if (threadIdx.x < F64T_TILE && gi < na) {
        if (MODE == 0) {
            for (int m = 1; m < 4; ++m) best = rtv_best(best, sh_s[er * 4 + m]);
            out_d[direct ? (int64_t)gi : (int64_t)blockIdx.y * na + gi] = best;
        } else {
            const int* __restrict__ p = reinterpret_cast<const int*>(sh_s) + er * 8;
            const int c = p[0] + p[2] + p[4] + p[6], cm = p[1] + p[3] + p[5] + p[7];
            if (direct) {
                out_i[gi] = c;
                if (out_m) out_m[gi] = cm;
            } else {
                out_i[((int64_t)blockIdx.y * na + gi) * 2] = c;
                out_i[((int64_t)blockIdx.y * na + gi) * 2 + 1] = cm;
            }
        }
    }
}

// the split maxima of a row, merged in split order
__global__ __launch_bounds__(256) void rtv_merge_best_kernel(const double* __restrict__ ws, int n, int S,
                                                             double* __restrict__ best) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v = ws[i];
    for (int s = 1; s < S; ++s) v = rtv_best(v, ws[(int64_t)s * n + i]);
    best[i] = v;
}

__global__ __launch_bounds__(256) void rtv_merge_counts_kernel(const int32_t* __restrict__ ws, int n, int S,
                                                               int32_t* __restrict__ above,
                                                               int32_t* __restrict__ above_masked) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int c = 0, cm = 0;
    for (int s = 0; s < S; ++s) {
        c += ws[((int64_t)s * n + i) * 2];
        cm += ws[((int64_t)s * n + i) * 2 + 1];
    }
    above[i] = c;
    if (above_masked) above_masked[i] = cm;
}

inline int rtv_splits(int na, int nb, int splits) {
    return f64t_splits(cdiv(na, F64T_TILE), cdiv(nb, F64T_TILE), splits);
}

// what both entry points check alike; S: the column splits of the launch
inline bool rtv_args_ok(const float* a, int na, int lda, const float* b, int nb, int ldb, int D, const int32_t* key_a,
                        const int32_t* key_b, double eps, int splits, const void* ws, int64_t ws_bytes, int& S) {
    if (!f64t_rows_ok(a, na, D, lda) || !f64t_rows_ok(b, nb, D, ldb)) return false;
    if (!key_a || !key_b || !f64t_aligned(key_a, 4) || !f64t_aligned(key_b, 4)) return false;
    if (!(eps > 0.0) || splits < 0 || splits > F64T_MAX_SPLITS) return false;
    S = rtv_splits(na, nb, splits);
    return S == 1 || (ws && f64t_aligned(ws, 8) && ws_bytes >= sba_retrieval_workspace_bytes(na, nb, splits));
}

}  // namespace

extern "C" int64_t sba_retrieval_workspace_bytes(int na, int nb, int splits) {
    if (na < 1 || nb < 1 || splits < 0 || splits > F64T_MAX_SPLITS) return -1;
    const int s = rtv_splits(na, nb, splits);
    return s == 1 ? 0 : (int64_t)s * na * 8;    // one f64, or two int32, per row and split
}

extern "C" int sba_retrieval_own_best(const float* a, int na, int lda, const float* b, int nb, int ldb, int D,
                                      const int32_t* key_a, const int32_t* key_b, double eps, int splits, double* best,
                                      void* ws, int64_t ws_bytes, void* stream) {
    int S = 0;
    if (!best || !f64t_aligned(best, 8)) return SBA_E_ARG;
    if (!rtv_args_ok(a, na, lda, b, nb, ldb, D, key_a, key_b, eps, splits, ws, ws_bytes, S)) return SBA_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    SBA_LAUNCH(rtv_kernel<0>, dim3(cdiv(na, F64T_TILE), S), dim3(F64T_THREADS), 0, st, a, na, (int64_t)lda, b, nb,
               (int64_t)ldb, D, key_a, key_b, (const int32_t*)nullptr, (const int32_t*)nullptr, (const double*)nullptr,
               eps, S == 1 ? 1 : 0, S == 1 ? best : (double*)ws, (int32_t*)nullptr, (int32_t*)nullptr);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    if (S == 1) return SBA_OK;
    SBA_LAUNCH(rtv_merge_best_kernel, dim3(cdiv(na, 256)), dim3(256), 0, st, (const double*)ws, na, S, best);
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_retrieval_counts(const float* a, int na, int lda, const float* b, int nb, int ldb, int D,
                                    const int32_t* key_a, const int32_t* key_b, const int32_t* cls_a, const int32_t* cls_b,
                                    const double* best, double eps, int splits, int32_t* above, int32_t* above_masked,
                                    void* ws, int64_t ws_bytes, void* stream) {
    int S = 0;
    if (!best || !f64t_aligned(best, 8) || !above || !f64t_aligned(above, 4)) return SBA_E_ARG;
    // the class vectors and the masked count go together: all three or none
    if ((cls_a != nullptr) != (cls_b != nullptr) || (cls_a != nullptr) != (above_masked != nullptr)) return SBA_E_ARG;
    if (!f64t_aligned(cls_a, 4) || !f64t_aligned(cls_b, 4) || !f64t_aligned(above_masked, 4)) return SBA_E_ARG;
    if (!rtv_args_ok(a, na, lda, b, nb, ldb, D, key_a, key_b, eps, splits, ws, ws_bytes, S)) return SBA_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    SBA_LAUNCH(rtv_kernel<1>, dim3(cdiv(na, F64T_TILE), S), dim3(F64T_THREADS), 0, st, a, na, (int64_t)lda, b, nb,
               (int64_t)ldb, D, key_a, key_b, cls_a, cls_b, best, eps, S == 1 ? 1 : 0, (double*)nullptr,
               S == 1 ? above : (int32_t*)ws, S == 1 ? above_masked : (int32_t*)nullptr);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    if (S == 1) return SBA_OK;
    SBA_LAUNCH(rtv_merge_counts_kernel, dim3(cdiv(na, 256)), dim3(256), 0, st, (const int32_t*)ws, na, S, above,
               above_masked);
    return SBA_CHECK_LAUNCH();
}
