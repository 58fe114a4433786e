// The adaptive-augmentation controller (Karras et al., NeurIPS 2020, "Training GANs with Limited Data"): the strength p of
// the gated augmentation (diffaug.hip) follows the overfitting read-out r_t = E[sign(D(real) - 0.5)] of each
// discriminator, entirely on the device (sba_ada_count / sba_ada_adjust in sbagan_hip_ext.h; sbagan/diffaug.py;
// DESIGN.md 7p).  State per discriminator: p, rt (f32) and four int32 counters (pos, neg, cnt, calls).
//
// Both kernels are a few hundred bytes of traffic: what matters is that they are launches like any other -- no host
// read, no atomics, nothing allocated -- so a recorded step holds them and every replay moves p by itself.
#include "common.h"
#include "sbagan_hip_ext.h"

namespace {

constexpr int ADA_THREADS = 256;
constexpr int ADA_MAX_N = 1 << 20;
constexpr int ADA_MAX_D = 8;

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ONE workgroup; integer sums are exact in any order.  0.5 and NaN fail both comparisons: they count in cnt alone.
__global__ __launch_bounds__(ADA_THREADS) void ada_count_kernel(const float* __restrict__ prob, int n,
                                                                int32_t* __restrict__ row) {
    int pos = 0, neg = 0;
    for (int i = threadIdx.x; i < n; i += ADA_THREADS) {
        const float v = prob[i];
        pos += v > 0.5f ? 1 : 0;
        neg += v < 0.5f ? 1 : 0;
    }
    pos = wave_sum_i(pos);
    neg = wave_sum_i(neg);
    __shared__ int sh[2][ADA_THREADS / 64];
    if ((threadIdx.x & 63) == 0) {
        sh[0][threadIdx.x >> 6] = pos;
        sh[1][threadIdx.x >> 6] = neg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        row[0] += sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
        row[1] += sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
        row[2] += n;
        row[3] += 1;
    }
}

// one thread per row.  p + adjust / p - adjust as an add and a subtract (not a multiply by a sign: nothing to contract)
__global__ __launch_bounds__(64) void ada_adjust_kernel(float* __restrict__ p, float* __restrict__ rt,
                                                        int32_t* __restrict__ counters, int nD, int interval,
                                                        float target, float adjust, float p_max) {
    const int r = threadIdx.x;
    if (r >= nD) return;
    int32_t* c = counters + 4 * r;
    if (c[3] < interval) return;
    const int pos = c[0], neg = c[1], cnt = c[2];
    float r_t = 0.f;
    if (cnt != 0) {
        r_t = __fdiv_rn((float)(pos - neg), (float)cnt);
        float v = p[r];
        if (r_t > target) v = __fadd_rn(v, adjust);
        else if (r_t < target) v = __fsub_rn(v, adjust);
        p[r] = fminf(fmaxf(v, 0.f), p_max);
    }
    rt[r] = r_t;
    c[0] = 0, c[1] = 0, c[2] = 0, c[3] = 0;
}

inline bool ada_bad_word(const void* q) { return !q || ((uintptr_t)q & 3) != 0; }

}  // namespace

extern "C" int sba_ada_count(const float* prob, int n, int32_t* counters_row, void* stream) {
    if (n < 1 || n > ADA_MAX_N || ada_bad_word(prob) || ada_bad_word(counters_row)) return SBA_E_ARG;
    SBA_LAUNCH(ada_count_kernel, dim3(1), dim3(ADA_THREADS), 0, (hipStream_t)stream, prob, n, counters_row);
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_ada_adjust(float* p, float* rt, int32_t* counters, int nD, int interval, float target, float adjust,
                              float p_max, void* stream) {
    if (nD < 1 || nD > ADA_MAX_D || interval < 1 || interval > 1024) return SBA_E_ARG;
    if (!(p_max >= 0.f && p_max <= 1.f) || !(adjust >= 0.f) || !__builtin_isfinite(adjust) || target != target) return SBA_E_ARG;
    if (ada_bad_word(p) || ada_bad_word(rt) || ada_bad_word(counters)) return SBA_E_ARG;
    SBA_LAUNCH(ada_adjust_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p, rt, counters, nD, interval, target,
               adjust, p_max);
    return SBA_CHECK_LAUNCH();
}
