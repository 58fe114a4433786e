// FID statistics (sba_fid_accumulate / sba_fid_finalize in sbagan_hip.h): the float64 column sums and Gram matrix X^T X
// of f32 feature rows on the f64 matrix instruction (v_mfma_f64_16x16x4_f64), and the mean / covariance / trace from them.
// The f32 inputs are widened in registers: a product of two f32 values is exact in f64, so the only rounding is the f64
// accumulation.  No atomics, no workspace, a fixed summation order.
#include "f64_tile.h"

namespace {

constexpr int FID_TILE = F64T_TILE;             // gram tile edge: one workgroup per tile pair (ti <= tj)
constexpr int FID_THREADS = F64T_THREADS;       // (lane map and MFMA step of f64_tile.h; the rows are the reduction axis
                                                // here, so the row-major staging below is this file's own)
constexpr int FID_KC = 32;                      // feature rows staged per chunk
constexpr int FID_LD = 2 * FID_TILE + 16;       // LDS row stride in floats: the 4 rows of one MFMA operand read fall
                                                // into 4 distinct groups of 16 banks
constexpr int FID_VEC = FID_KC * 2 * FID_TILE / 4 / FID_THREADS;   // float4 loads per thread and chunk (4)

// rows k0 .. k0 + KC - 1 of the column blocks i0 .. i0 + 63 and j0 .. j0 + 63 -> registers; a row >= n reads as zeros
__device__ __forceinline__ void fid_fetch(float4 (&v)[FID_VEC], const float* __restrict__ x, int n, int64_t ldx, int k0,
                                          int i0, int j0) {
#pragma unroll
    for (int s = 0; s < FID_VEC; ++s) {
        const int e = threadIdx.x + FID_THREADS * s;    // float4 slot: 32 per staged row
        const int r = e >> 5, c = (e & 31) << 2;        // row of the chunk, column of the 128-wide staged row
        const int col = c < FID_TILE ? i0 + c : j0 + c - FID_TILE;
        const int k = k0 + r;
        v[s] = k < n ? *reinterpret_cast<const float4*>(x + (int64_t)k * ldx + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
__device__ __forceinline__ void fid_stage(float* __restrict__ buf, const float4 (&v)[FID_VEC]) {
#pragma unroll
    for (int s = 0; s < FID_VEC; ++s) {
        const int e = threadIdx.x + FID_THREADS * s;
        *reinterpret_cast<float4*>(buf + (e >> 5) * FID_LD + ((e & 31) << 2)) = v[s];
    }
}

// gram[i0 .. i0 + 63][j0 .. j0 + 63] += X[:, i0 ..]^T X[:, j0 ..] for the upper-triangular tile pair of this workgroup;
// the diagonal workgroups also add their 64 column sums.  MFMA operands (lane map of f64_tile.h): A[i][k] = x[k][i],
// B[k][j] = x[k][j], so both are the same kind of read of staged row k.
__global__ __launch_bounds__(FID_THREADS) void fid_accumulate_kernel(const float* __restrict__ x, int n, int D, int64_t ldx,
                                                                     double* __restrict__ sum, double* __restrict__ gram) {
    __shared__ __attribute__((aligned(16))) float sh[2][FID_KC * FID_LD];
    __shared__ double sh_sum[FID_THREADS];

    // triangular decode: block t of row ti covers tile columns ti .. T - 1
    int t = blockIdx.x, ti = 0;
    for (int len = D / FID_TILE; t >= len; --len) {
        t -= len;
        ++ti;
    }
    const int tj = ti + t;
    const int i0 = ti * FID_TILE, j0 = tj * FID_TILE;
    const bool diag = ti == tj;

    const F64Lanes l = f64t_lanes();

    f64x4_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    double csum = 0.0;                                          // diagonal workgroups: column threadIdx & 63, rows
    const int sc = threadIdx.x & 63, sr = (threadIdx.x >> 6) * (FID_KC / 4);   // sr .. sr + 7 of every chunk

    float4 v[FID_VEC];
    const int chunks = (n + FID_KC - 1) / FID_KC;
    fid_fetch(v, x, n, ldx, 0, i0, j0);
    fid_stage(sh[0], v);
    __syncthreads();
    for (int c = 0; c < chunks; ++c) {
        const float* __restrict__ buf = sh[c & 1];
        const bool more = c + 1 < chunks;
        if (more) fid_fetch(v, x, n, ldx, (c + 1) * FID_KC, i0, j0);
        const int rows = min(FID_KC, n - c * FID_KC);
        const int steps = (rows + 3) >> 2;                      // (rows past n inside the last step are staged zeros)
        // (rolled on purpose: the fully unrolled K loop measured 9 % slower, profiles/fid_bench.json)
        for (int s = 0; s < steps; ++s) {
            const float* __restrict__ row = buf + (4 * s + l.lk) * FID_LD;
            f64t_mfma((double)row[l.wi + l.lc], (double)row[l.wi + 16 + l.lc], (double)row[FID_TILE + l.wj + l.lc],
                      (double)row[FID_TILE + l.wj + 16 + l.lc], acc);
        }
        if (diag) {
#pragma unroll
            for (int r = 0; r < FID_KC / 4; ++r) csum += (double)buf[(sr + r) * FID_LD + sc];
        }
        if (more) fid_stage(sh[(c + 1) & 1], v);    // last read in iteration c - 1, which every wave has left
        __syncthreads();
    }

    f64t_each(l, acc, [&](int i, int j, double g) { gram[(int64_t)(i0 + i) * D + (j0 + j)] += g; });
    if (diag) {
        sh_sum[threadIdx.x] = csum;
        __syncthreads();
        if (threadIdx.x < FID_TILE)
            sum[i0 + threadIdx.x] += ((sh_sum[threadIdx.x] + sh_sum[threadIdx.x + 64]) + sh_sum[threadIdx.x + 128]) +
                                     sh_sum[threadIdx.x + 192];
    }
}

// one covariance entry from the upper triangle: the SAME expression for (i, j) and (j, i), so sigma is bitwise symmetric
__device__ __forceinline__ double fid_cov(const double* __restrict__ sum, const double* __restrict__ gram, int D, int i,
                                          int j, double n) {
    const int a = min(i, j), b = max(i, j);
    return (gram[(int64_t)a * D + b] - sum[a] * sum[b] / n) / (n - 1.0);
}

__global__ __launch_bounds__(256) void fid_sigma_kernel(const double* __restrict__ sum, const double* __restrict__ gram,
                                                        double n, int D, double* __restrict__ sigma) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int ib = blockIdx.y * 64 + (threadIdx.x >> 6);
    for (int r = 0; r < 64; r += 4) {
        const int i = ib + r;
        sigma[(int64_t)i * D + j] = fid_cov(sum, gram, D, i, j, n);
    }
}

// mu = sum / n and trace = sum_i sigma_ii: thread t adds i = t, t + 256, ... in order, then a fixed tree over the threads
__global__ __launch_bounds__(256) void fid_mu_trace_kernel(const double* __restrict__ sum, const double* __restrict__ gram,
                                                           double n, int D, double* __restrict__ mu,
                                                           double* __restrict__ trace) {
    __shared__ double sh[256];
    double tr = 0.0;
    for (int i = threadIdx.x; i < D; i += 256) {
        mu[i] = sum[i] / n;
        tr += fid_cov(sum, gram, D, i, i, n);
    }
    sh[threadIdx.x] = tr;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *trace = sh[0];
}

}  // namespace

extern "C" int sba_fid_accumulate(const float* x, int n, int D, int ldx, double* sum, double* gram, void* stream) {
    if (!x || !sum || !gram) return SBA_E_ARG;
    if (n < 1 || D < FID_TILE || D % FID_TILE || ldx < D || ldx % 4) return SBA_E_ARG;
    if (!f64t_aligned(x, 16) || !f64t_aligned(sum, 8) || !f64t_aligned(gram, 8)) return SBA_E_ARG;
    const int T = D / FID_TILE;
    SBA_LAUNCH(fid_accumulate_kernel, dim3(T * (T + 1) / 2), dim3(FID_THREADS), 0, (hipStream_t)stream, x, n, D,
               (int64_t)ldx, sum, gram);
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_fid_finalize(const double* sum, const double* gram, int64_t n, int D, double* mu, double* sigma,
                                double* trace, void* stream) {
    if (!sum || !gram || !mu || !sigma || !trace) return SBA_E_ARG;
    if (n < 2 || D < FID_TILE || D % FID_TILE) return SBA_E_ARG;
    if (!f64t_aligned(sum, 8) || !f64t_aligned(gram, 8) || !f64t_aligned(mu, 8) || !f64t_aligned(sigma, 8) ||
        !f64t_aligned(trace, 8))
        return SBA_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    SBA_LAUNCH(fid_sigma_kernel, dim3(D / 64, D / 64), dim3(256), 0, st, sum, gram, (double)n, D, sigma);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    SBA_LAUNCH(fid_mu_trace_kernel, dim3(1), dim3(256), 0, st, sum, gram, (double)n, D, mu, trace);
    return SBA_CHECK_LAUNCH();
}
