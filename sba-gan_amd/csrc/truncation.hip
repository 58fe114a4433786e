// The truncation trick in W (Karras et al., CVPR 2019, "A Style-Based Generator Architecture for GANs", appendix B;
// the precision / recall curve over psi: Kynkaanniemi et al., NeurIPS 2019): the mean style w_avg of a mapping network and
// w' = w_avg + psi (w - w_avg) (sba_style_mean / sba_style_truncate in sbagan_hip_ext.h; sbagan/truncation.py).
//
// Both kernels are small -- 16 MB read once for the mean at its default size, a few KB per generated batch for the lerp.
// What they supply is a FIXED order of summation and rounding: images and figures are reproducible, a numpy restatement
// matches bit for bit (tests/truncation_ref.py), and psi = 1 is a copy, so that run is exactly the run without the flag.
#include "common.h"
#include "sbagan_hip_ext.h"

namespace {

constexpr int TRUNC_CHUNK = 256;          // rows per partial sum: part of the contract (sbagan_hip_ext.h)
constexpr int TRUNC_COLS = 64;            // one wave per workgroup: lane l reads column 64 bx + l, neighbours coalesce
constexpr int TRUNC_THREADS = 256;
constexpr int TRUNC_MAX_N = 1 << 20;
constexpr int TRUNC_MAX_D = 4096;

// P_c of column d: rows 256 c .. min(256 c + 256, n) - 1 in ascending order, from +0.0.  The loads of the unrolled rows
// are independent (the compiler issues them together); the float64 adds stay in row order.  ONE_CHUNK: P_0 is T, and the
// mean is written here.
template <bool ONE_CHUNK>
__global__ __launch_bounds__(TRUNC_COLS) void style_mean_partial_kernel(const float* __restrict__ w, int n, int D,
                                                                        double* __restrict__ part,
                                                                        double* __restrict__ mean64,
                                                                        float* __restrict__ mean32) {
    const int d = blockIdx.x * TRUNC_COLS + threadIdx.x;
    if (d >= D) return;
    const int c = blockIdx.y;
    const int r0 = c * TRUNC_CHUNK;
    const int r1 = min(r0 + TRUNC_CHUNK, n);
    const float* p = w + (int64_t)r0 * D + d;
    double acc = 0.0;
#pragma unroll 8
    for (int r = r0; r < r1; ++r, p += D) acc += (double)*p;
    if (ONE_CHUNK) {
        const double m = acc / (double)n;
        mean64[d] = m;
        mean32[d] = (float)m;
    } else {
        part[(int64_t)c * D + d] = acc;
    }
}

// T = P_0 + P_1 + ... in ascending c, from +0.0; one thread per column, neighbouring lanes read neighbouring columns
__global__ __launch_bounds__(TRUNC_THREADS) void style_mean_tail_kernel(const double* __restrict__ part, int chunks,
                                                                        int n, int D, double* __restrict__ mean64,
                                                                        float* __restrict__ mean32) {
    const int d = blockIdx.x * TRUNC_THREADS + threadIdx.x;
    if (d >= D) return;
    const double* p = part + d;
    double t = 0.0;
#pragma unroll 8
    for (int c = 0; c < chunks; ++c, p += D) t += *p;
    const double m = t / (double)n;
    mean64[d] = m;
    mean32[d] = (float)m;
}

// three separately rounded f32 operations.  hipcc contracts a * b + c into one fused multiply-add by default, and its
// __fmul_rn / __fadd_rn are plain operators compiled under that default (inlined, they fuse all the same: seen in the
// assembly): the operators are written out here, under a pragma that switches contraction off for this function.
template <bool COPY>
__global__ __launch_bounds__(TRUNC_THREADS) void style_truncate_kernel(const float* w, const float* __restrict__ w_avg,
                                                                       float psi, float* out, int64_t total, int D) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * TRUNC_THREADS + threadIdx.x;
    if (i >= total) return;
    if (COPY) {         // psi == 1: the bits of w (the formula does not give them back in floating point)
        reinterpret_cast<uint32_t*>(out)[i] = reinterpret_cast<const uint32_t*>(w)[i];
        return;
    }
    const float a = w_avg[(int)(i % D)];
    const float diff = w[i] - a;
    const float scaled = psi * diff;
    out[i] = a + scaled;
}

inline bool trunc_bad(const void* q, uintptr_t align_mask) { return !q || ((uintptr_t)q & align_mask) != 0; }

}  // namespace

extern "C" int sba_style_mean(const float* w, int n, int D, double* mean64, float* mean32, void* workspace,
                              void* stream) {
    if (n < 1 || n > TRUNC_MAX_N || D < 1 || D > TRUNC_MAX_D) return SBA_E_ARG;
    if (trunc_bad(w, 3) || trunc_bad(mean32, 3) || trunc_bad(mean64, 7)) return SBA_E_ARG;
    const int chunks = cdiv(n, TRUNC_CHUNK);
    if (chunks > 1 && trunc_bad(workspace, 7)) return SBA_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cdiv(D, TRUNC_COLS), chunks);
    if (chunks == 1) {
        SBA_LAUNCH(style_mean_partial_kernel<true>, grid, dim3(TRUNC_COLS), 0, st, w, n, D, (double*)nullptr, mean64,
                   mean32);
        return SBA_CHECK_LAUNCH();
    }
    double* part = (double*)workspace;
    SBA_LAUNCH(style_mean_partial_kernel<false>, grid, dim3(TRUNC_COLS), 0, st, w, n, D, part, (double*)nullptr,
               (float*)nullptr);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    SBA_LAUNCH(style_mean_tail_kernel, dim3(cdiv(D, TRUNC_THREADS)), dim3(TRUNC_THREADS), 0, st, (const double*)part,
               chunks, n, D, mean64, mean32);
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_style_truncate(const float* w, const float* w_avg, float psi, float* out, int n, int D,
                                  void* stream) {
    if (!__builtin_isfinite(psi) || n < 1 || n > TRUNC_MAX_N || D < 1 || D > TRUNC_MAX_D) return SBA_E_ARG;
    if (trunc_bad(w, 3) || trunc_bad(w_avg, 3) || trunc_bad(out, 3)) return SBA_E_ARG;
    const int64_t total = (int64_t)n * D;
    const dim3 grid((unsigned)((total + TRUNC_THREADS - 1) / TRUNC_THREADS));
    const hipStream_t st = (hipStream_t)stream;
    if (psi == 1.0f) {
        if (out == w) return SBA_OK;        // in place: every row already holds its bits
        SBA_LAUNCH(style_truncate_kernel<true>, grid, dim3(TRUNC_THREADS), 0, st, w, w_avg, psi, out, total, D);
    } else {
        SBA_LAUNCH(style_truncate_kernel<false>, grid, dim3(TRUNC_THREADS), 0, st, w, w_avg, psi, out, total, D);
    }
    return SBA_CHECK_LAUNCH();
}
