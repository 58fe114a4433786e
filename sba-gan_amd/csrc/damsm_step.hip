// The pieces of the DAMSM pre-training update that had to move onto the device before the update could be RECORDED
// (sbagan/damsm.py: DAMSMSlotStep):
//   sba_embed_dropout_fwd / _bwd   Embedding -> Dropout of RNN_ENCODER's training path with the keep mask as a tensor
//                                  (drawn eagerly per batch; a recorded Philox launch would repeat the capture's mask)
//   sba_sqnorm_partials            } clip_grad_norm_ over the text encoder's range of the flat gradient: the norm and
//   sba_clip_adam_prepare          } the clip coefficient stay on the device, with Adam's bias corrections from a
//                                    learning rate READ from device memory (a recording keeps no host float)
// The update that consumes the coefficient is sba_adam_step_dscale (losses_optim.hip, beside sba_adam_step).
// Plain vector loads and stores, no atomics, no host synchronisation: every result is the same bits on every run.
#include "common.h"

namespace {

struct AdamState {          // (losses_optim.hip)
    int32_t step;
    float step_size;       // lr / (1 - beta1^step)
    float inv_sqrt_bc2;    // 1 / sqrt(1 - beta2^step)
    float pad;
};

constexpr int ED_THREADS = 256;
constexpr int ED_MAX_BLOCKS = 2048;
constexpr int EDB_THREADS = 128;
constexpr int ED_MAX_N = 8192;          // ids of one batch held in LDS as int32: 32 KB
constexpr int SQ_THREADS = 256;
constexpr int SQ_MAX_PARTS = 1024;

// out[i][c] = keep[i][c] ? W[ids[i]][c] * scale : 0; 4 columns (16 bytes of W / out, 4 bytes of keep) per thread
__global__ __launch_bounds__(ED_THREADS) void embed_dropout_fwd_kernel(
    const int64_t* __restrict__ ids, const float* __restrict__ W, const uint8_t* __restrict__ keep, float scale,
    float* __restrict__ out, int N, int ntoken, int ninput) {
    const int c4n = ninput >> 2;
    const int64_t n = (int64_t)N * c4n, stride = (int64_t)gridDim.x * ED_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * ED_THREADS + threadIdx.x; e < n; e += stride) {
        const int64_t i = e / c4n;
        const int c = (int)(e - i * c4n) << 2;
        const int64_t id = ids[i];
        f32x4_t o = {0.f, 0.f, 0.f, 0.f};
        if (id >= 0 && id < ntoken) {           // compared BEFORE it indexes: a bad id yields a zero row
            const uint32_t k = *reinterpret_cast<const uint32_t*>(keep + i * ninput + c);
            const f32x4_t w = *reinterpret_cast<const f32x4_t*>(W + id * ninput + c);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if ((k >> (8 * q)) & 0xffu) o[q] = w[q] * scale;
        }
        *reinterpret_cast<f32x4_t*>(out + i * ninput + c) = o;
    }
}

// dW[id][c] += sum_{j: ids[j] == id, increasing j} keep[j][c] * dout[j][c] * scale.  One workgroup per position; the
// FIRST position that holds an id owns that row of dW and adds every later position with the same id, so no two
// workgroups write one address and the order of the sum is fixed.  ids in LDS (int32, -1 = out of range).
__global__ __launch_bounds__(EDB_THREADS) void embed_dropout_bwd_kernel(
    const int64_t* __restrict__ ids, const uint8_t* __restrict__ keep, float scale, const float* __restrict__ dout,
    float* __restrict__ dW, int N, int ntoken, int ninput) {
    __shared__ int32_t sid[ED_MAX_N];
    for (int j = threadIdx.x; j < N; j += EDB_THREADS) {
        const int64_t id = ids[j];
        sid[j] = (id >= 0 && id < ntoken) ? (int32_t)id : -1;
    }
    __syncthreads();
    const int i = blockIdx.x;
    const int32_t my = sid[i];
    if (my < 0) return;                         // (uniform over the workgroup)
    int earlier = 0;
    for (int j = threadIdx.x; j < i; j += EDB_THREADS) earlier |= (sid[j] == my);
    if (__syncthreads_or(earlier)) return;      // an earlier position owns this row
    const int c4n = ninput >> 2;
    for (int c4 = threadIdx.x; c4 < c4n; c4 += EDB_THREADS) {
        const int c = c4 << 2;
        f32x4_t* dst = reinterpret_cast<f32x4_t*>(dW + (int64_t)my * ninput + c);
        f32x4_t acc = *dst;
        for (int j = i; j < N; ++j) {
            if (sid[j] != my) continue;         // (LDS broadcast, uniform branch)
            const uint32_t k = *reinterpret_cast<const uint32_t*>(keep + (int64_t)j * ninput + c);
            const f32x4_t d = *reinterpret_cast<const f32x4_t*>(dout + (int64_t)j * ninput + c);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if ((k >> (8 * q)) & 0xffu) acc[q] += d[q] * scale;
        }
        *dst = acc;
    }
}

// partials[b] = sum over the elements block b visits (grid-stride) of g^2: the square in f32, the sum in f64; the
// workgroup's 256 sums are folded in LDS by a fixed tree
__global__ __launch_bounds__(SQ_THREADS) void sqnorm_partials_kernel(const float* __restrict__ g, int64_t n,
                                                                    double* __restrict__ partials, int vec) {
    __shared__ double sh[SQ_THREADS];
    const int64_t t = (int64_t)blockIdx.x * SQ_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * SQ_THREADS;
    const int64_t n4 = vec ? n >> 2 : 0;
    double acc = 0.0;
    for (int64_t i = t; i < n4; i += stride) {
        const f32x4_t v = reinterpret_cast<const f32x4_t*>(g)[i];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc += (double)(v[q] * v[q]);
    }
    for (int64_t i = n4 * 4 + t; i < n; i += stride) acc += (double)(g[i] * g[i]);
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = SQ_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = sh[0];
}

// one workgroup: the partials in index order (f64), norm and clip coefficient, then adam_prepare_kernel's work with
// the learning rate read from device memory
__global__ void clip_adam_prepare_kernel(AdamState* st, const double* __restrict__ partials, int nparts,
                                         const float* __restrict__ lr_dev, float max_norm, float beta1, float beta2,
                                         float* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s = 0.0;
        for (int p = 0; p < nparts; ++p) s += partials[p];
        const double norm = sqrt(s);
        const double coef = fmin(1.0, (double)max_norm / (norm + 1e-6));
        out[0] = (float)norm;
        out[1] = (float)coef;
        const int step = st->step + 1;
        st->step = step;
        const double bc1 = 1.0 - pow((double)beta1, (double)step);
        const double bc2 = 1.0 - pow((double)beta2, (double)step);
        st->step_size = (float)((double)lr_dev[0] / bc1);
        st->inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    }
}

}  // namespace

extern "C" int sba_embed_dropout_fwd(const int64_t* ids, const float* W, const uint8_t* keep, float scale, float* out,
                                     int N, int ntoken, int ninput, void* stream) {
    if (!ids || !W || !keep || !out) return SBA_E_ARG;
    if (N < 1 || N > ED_MAX_N || ntoken < 1 || ninput < 4 || (ninput & 3)) return SBA_E_ARG;
    if ((((uintptr_t)W | (uintptr_t)out) & 15) || ((uintptr_t)keep & 3) || ((uintptr_t)ids & 7)) return SBA_E_ARG;
    int blocks = cdiv((int64_t)N * (ninput >> 2), ED_THREADS);
    if (blocks > ED_MAX_BLOCKS) blocks = ED_MAX_BLOCKS;
    SBA_LAUNCH(embed_dropout_fwd_kernel, dim3(blocks), dim3(ED_THREADS), 0, (hipStream_t)stream, ids, W, keep, scale,
               out, N, ntoken, ninput);
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_embed_dropout_bwd(const int64_t* ids, const uint8_t* keep, float scale, const float* dout,
                                     float* dW, int N, int ntoken, int ninput, void* stream) {
    if (!ids || !keep || !dout || !dW) return SBA_E_ARG;
    if (N < 1 || N > ED_MAX_N || ntoken < 1 || ninput < 4 || (ninput & 3)) return SBA_E_ARG;
    if ((((uintptr_t)dW | (uintptr_t)dout) & 15) || ((uintptr_t)keep & 3) || ((uintptr_t)ids & 7)) return SBA_E_ARG;
    SBA_LAUNCH(embed_dropout_bwd_kernel, dim3(N), dim3(EDB_THREADS), 0, (hipStream_t)stream, ids, keep, scale, dout,
               dW, N, ntoken, ninput);
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_sqnorm_partials(const float* g, int64_t n, double* partials, int nparts, void* stream) {
    if (!g || !partials || n < 1 || nparts < 1 || nparts > SQ_MAX_PARTS) return SBA_E_ARG;
    if (((uintptr_t)g & 3) || ((uintptr_t)partials & 7)) return SBA_E_ARG;
    const int vec = ((uintptr_t)g & 15) == 0 ? 1 : 0;
    SBA_LAUNCH(sqnorm_partials_kernel, dim3(nparts), dim3(SQ_THREADS), 0, (hipStream_t)stream, g, n, partials, vec);
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_clip_adam_prepare(void* state, const double* partials, int nparts, const float* lr_dev,
                                     float max_norm, float beta1, float beta2, float* out, void* stream) {
    if (!state || !partials || !lr_dev || !out || nparts < 1 || nparts > SQ_MAX_PARTS) return SBA_E_ARG;
    if (((uintptr_t)partials & 7) || ((uintptr_t)state & 3) || ((uintptr_t)lr_dev & 3) || ((uintptr_t)out & 3))
        return SBA_E_ARG;
    SBA_LAUNCH(clip_adam_prepare_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (AdamState*)state, partials,
               nparts, lr_dev, max_norm, beta1, beta2, out);
    return SBA_CHECK_LAUNCH();
}
