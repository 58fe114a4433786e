// BatchNorm(train)+activation, BatchNorm1d+GLU, InstanceNorm/AdaIN kernels (gfx950).
// All are HBM-bound streaming kernels: 16-byte vector accesses along the NHWC
// channel axis, f32 math, per-channel reductions through LDS then global atomics.
//
// Reference: model.py:43-44 (BN+GLU), :62-65,70 (ResBlock BN, residual add),
// :543-544,553-554 (BN+LeakyReLU 0.2), :353-356 (BatchNorm1d+GLU), :324-339 (AdaIN).
#include "common.h"

namespace {

constexpr float LRELU_SLOPE = 0.2f;

// ---- the arithmetic every kernel below shares.  All helpers are forced inline: a kernel that uses one compiles to
// the floating-point operations, in the order, that it had with the expression written out in place ----

// forward element: BatchNorm output n = y * scale + shift of the value channel (and gp of its gate channel under GLU)
// -> activated value.  The residual add stays with the caller.  (sigmoidf_, IEEE division: see common.h)
template <int ACT>
__device__ __forceinline__ float bn_act_elem(float ya, float sca, float sha, float yg, float scg, float shg) {
    const float n = ya * sca + sha;
    if (ACT == SBA_ACT_GLU) return n * sigmoidf_(yg * scg + shg);
    if (ACT == SBA_ACT_LRELU) return n > 0.f ? n : LRELU_SLOPE * n;
    if (ACT == SBA_ACT_RELU) return fmaxf(n, 0.f);
    return n;
}

// backward element: dz = d loss / d (BatchNorm output) and xhat of the value channel (index 0) and, under GLU, of its
// gate channel (index 1) from y, dout and the channels' (scale, shift, mean, rstd); without GLU kg = ka.  The LeakyReLU branch is taken from
// the recomputed forward value; the gate is recomputed with sigmoid_bwd_ (v_rcp_f32: see common.h)
struct ChCoef { float scale, shift, mean, rstd; };
// (loaded in the order the backward math uses them: scale and shift of both channels for the forward value, then mean and
// rstd for xhat -- the load order decides a VGPR or two, and with them a wave of occupancy of bn_bwd_apply_kernel)
__device__ __forceinline__ void ch_coef_pair(const float* __restrict__ scale, const float* __restrict__ shift,
                                             const float* __restrict__ mean, const float* __restrict__ rstd, int ca, int cg,
                                             ChCoef& ka, ChCoef& kg) {
    ka.scale = scale[ca]; ka.shift = shift[ca]; kg.scale = scale[cg]; kg.shift = shift[cg];
    ka.mean = mean[ca]; ka.rstd = rstd[ca]; kg.mean = mean[cg]; kg.rstd = rstd[cg];
}
template <int ACT>
__device__ __forceinline__ void bn_bwd_elem(float ya, float yg, float dd, const ChCoef& ka, const ChCoef& kg,
                                            float (&dz)[2], float (&xh)[2]) {
    if (ACT == SBA_ACT_GLU) {
        const float n = ya * ka.scale + ka.shift;
        const float gp = yg * kg.scale + kg.shift;
        const float s = sigmoid_bwd_(gp);
        dz[0] = dd * s;
        dz[1] = dd * n * s * (1.f - s);
    } else {
        dz[0] = dd;
        if (ACT == SBA_ACT_LRELU) {
            const float n = ya * ka.scale + ka.shift;
            dz[0] = n > 0.f ? dd : LRELU_SLOPE * dd;
        }
    }
    xh[0] = (ya - ka.mean) * ka.rstd;
    if (ACT == SBA_ACT_GLU) xh[1] = (yg - kg.mean) * kg.rstd;
}

// (sum, sumsq) of `count` values -> mean, biased variance, rstd; with gamma and beta -> scale and shift
struct Moments { float mean, var, rstd; };
__device__ __forceinline__ Moments moments_of(float sum, float sumsq, float count, float eps) {
    Moments m;
    m.mean = sum / count;
    m.var = fmaxf(sumsq / count - m.mean * m.mean, 0.f);
    m.rstd = rsqrtf(m.var + eps);
    return m;
}
struct BnCoef { float scale, shift, mean, rstd, var; };
__device__ __forceinline__ BnCoef bn_affine(float mean, float var, float rstd, float gamma, float beta) {
    BnCoef k;
    k.mean = mean; k.var = var; k.rstd = rstd;
    k.scale = gamma * rstd;
    k.shift = beta - mean * k.scale;
    return k;
}
// aux[4][C] = scale, shift, mean, rstd: what the forward leaves for the backward kernels
__device__ __forceinline__ void store_aux(float* __restrict__ aux, int C, int c, const BnCoef& k) {
    aux[c] = k.scale; aux[C + c] = k.shift; aux[2 * C + c] = k.mean; aux[3 * C + c] = k.rstd;
}
// running statistics after one more batch: momentum, unbiased variance
__device__ __forceinline__ void running_update(float& rm, float& rv, float mean, float var, float count, float momentum) {
    const float unb = count > 1.f ? var * count / (count - 1.f) : var;
    rm = (1.f - momentum) * rm + momentum * mean;
    rv = (1.f - momentum) * rv + momentum * unb;
}
// per-channel coefficients of one BatchNorm batch from its replicated (sum, sumsq) statistics
__device__ __forceinline__ BnCoef bn_coef(const float* __restrict__ stats, const float* __restrict__ gamma,
                                          const float* __restrict__ beta, int C, int c, float count, float eps) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int sl = 0; sl < SBA_BN_STAT_SLOTS; ++sl) {            // add the replicas up
        s0 += stats[sl * 2 * C + c];
        s1 += stats[sl * 2 * C + C + c];
    }
    const Moments m = moments_of(s0, s1, count, eps);
    return bn_affine(m.mean, m.var, m.rstd, gamma[c], beta[c]);
}

// The channel-sum tail of the reduction kernels: per-thread partial sums of 2C per-channel values (two halves of C) meet
// in LDS, then go to their destination.  Default mode: acc[2*C], cleared, LDS atomics.  Deterministic mode: one private
// row acc[tr][2*C] per row-group (plain stores, no clearing), the row-groups added in order.  dst(i, v) receives the
// workgroup's sum v of value i < 2C.
struct ChannelSum {
    float* acc;
    int C;
    bool det;
    __device__ __forceinline__ void clear() const {
        if (det) return;
        for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) acc[i] = 0.f;
        __syncthreads();
    }
    // row-group tr adds V consecutive channels from c on: s0 into the first half, s1 into the second
    template <int V>
    __device__ __forceinline__ void add(int tr, int c, const float (&s0)[V], const float (&s1)[V]) const {
        float* row = acc + (det ? tr * 2 * C : 0);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (det) {
                row[c + k] = s0[k];
                row[C + c + k] = s1[k];
            } else {
                atomicAdd(&row[c + k], s0[k]);
                atomicAdd(&row[C + c + k], s1[k]);
            }
        }
    }
    template <typename Dst>
    __device__ __forceinline__ void finish(int rpi, Dst dst) const {
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) {
            float v = det ? 0.f : acc[i];
            if (det)
                for (int r = 0; r < rpi; ++r) v += acc[r * 2 * C + i];
            dst(i, v);
        }
    }
};

// Cross-wave sum of the N (sum, sumsq) pairs a 256-thread workgroup owns: lane 0 of each of the four waves stores its
// wave's sums, interleaved, into s_red[wave]; after a barrier four_wave_sum adds the waves as ((w0 + w1) + w2) + w3.
template <int NV, int V>
__device__ __forceinline__ void wave_sums_to_lds(const float (&s0)[NV][V], const float (&s1)[NV][V],
                                                 float (&s_red)[4][2 * NV * V]) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int h = 0; h < NV; ++h)
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float a0 = wave_sum(s0[h][k]), a1 = wave_sum(s1[h][k]);
            if (lane == 0) { s_red[wid][(h * V + k) * 2] = a0; s_red[wid][(h * V + k) * 2 + 1] = a1; }
        }
    __syncthreads();
}
template <int W>
__device__ __forceinline__ float four_wave_sum(const float (&s_red)[4][W], int i) {
    return s_red[0][i] + s_red[1][i] + s_red[2][i] + s_red[3][i];
}

// ---- batch statistics of an NHWC tensor (used when the conv epilogue cannot provide them:
//      grouped passes, where one conv launch covers several BatchNorm batches); blockIdx.y = group ----
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_kernel(const T* __restrict__ y_all, float* __restrict__ stats_all, int64_t rows, int C,
                                                       float* __restrict__ det_part) {
    constexpr int V = Vec16<T>::N;
    const T* y = y_all + (int64_t)blockIdx.y * rows * C;
    float* stats = stats_all + ((int64_t)blockIdx.y * SBA_BN_STAT_SLOTS + (blockIdx.x & (SBA_BN_STAT_SLOTS - 1))) * 2 * C;
    const int cv = C / V;
    extern __shared__ float s_acc[];                        // [2*C]; deterministic mode: [rows per iteration][2*C]
    const ChannelSum cs{s_acc, C, det_part != nullptr};
    cs.clear();
    const int tpr = cv < (int)blockDim.x ? cv : (int)blockDim.x;
    const int rpi = blockDim.x / tpr;           // (cv not a power of two: the last blockDim.x % tpr threads idle)
    const int tc = threadIdx.x % tpr, tr = threadIdx.x / tpr;
    for (int cvi = tc; cvi < cv && tr < rpi; cvi += tpr) {
        const int c = cvi * V;
        float s0[V], s1[V];
#pragma unroll
        for (int k = 0; k < V; ++k) s0[k] = s1[k] = 0.f;
        for (int64_t row = (int64_t)blockIdx.x * rpi + tr; row < rows; row += (int64_t)gridDim.x * rpi) {
            Vec16<T> a = ld16(y + row * C + c);
#pragma unroll
            for (int k = 0; k < V; ++k) { const float v = a.get(k); s0[k] += v; s1[k] += v * v; }
        }
        cs.add(tr, c, s0, s1);
    }
    // deterministic mode: this workgroup's partial sums go to its own slot; sba_det_fold adds the workgroups
    float* part = det_part ? det_part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * C : nullptr;
    cs.finish(rpi, [&](int i, float v) {
        if (det_part) part[i] = v;
        else atomicAdd(&stats[i], v);
    });
}

// ---- forward: finalize + out = act(y*scale+shift) (+residual) in one launch; blockIdx.y = group.
// Every workgroup derives scale/shift of its group's C channels from the (sum, sumsq) statistics into
// LDS (C rsqrt: noise next to the streaming pass); workgroup (0, g) also stores aux[g] = scale,
// shift, mean, rstd for the backward, and workgroup (0, 0) applies the running-statistics updates
// of all groups in order (momentum, unbiased variance), as consecutive module calls would.
template <typename T, typename YT, int ACT>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const YT* __restrict__ y_all, const float* __restrict__ stats_all,
                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                  float* __restrict__ rmean, float* __restrict__ rvar, int64_t* __restrict__ nbt,
                                  float* __restrict__ aux_all, const T* __restrict__ residual_all,
                                  T* __restrict__ out_all, int64_t rows, int C, int out_cstride, int out_coff,
                                  float eps, float momentum, int training) {
    constexpr int V = Vec16<T>::N;
    extern __shared__ float s_co[];                         // scale[C], shift[C]
    const int g = blockIdx.y;
    const int Co = ACT == SBA_ACT_GLU ? C / 2 : C;
    const float count = (float)rows;
    float* aux = aux_all + (int64_t)g * 4 * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        BnCoef k;
        if (training) {
            k = bn_coef(stats_all + (int64_t)g * SBA_BN_STAT_SLOTS * 2 * C, gamma, beta, C, c, count, eps);
        } else {                                            // inference: running statistics
            k = bn_affine(rmean[c], rvar[c], rsqrtf(rvar[c] + eps), gamma[c], beta[c]);
        }
        s_co[c] = k.scale;
        s_co[C + c] = k.shift;
        if (blockIdx.x == 0) store_aux(aux, C, c, k);
        if (blockIdx.x == 0 && g == 0 && training && rmean) {
            float rm = rmean[c], rv = rvar[c];
            for (int gg = 0; gg < (int)gridDim.y; ++gg) {
                const BnCoef q = bn_coef(stats_all + (int64_t)gg * SBA_BN_STAT_SLOTS * 2 * C, gamma, beta, C, c, count, eps);
                running_update(rm, rv, q.mean, q.var, count, momentum);
            }
            rmean[c] = rm;
            rvar[c] = rv;
        }
    }
    if (blockIdx.x == 0 && g == 0 && threadIdx.x == 0 && training && nbt) *nbt += gridDim.y;
    __syncthreads();
    const float* scale = s_co;
    const float* shift = s_co + C;
    const YT* y = y_all + (int64_t)g * rows * C;
    // (GLU takes no residual: the entry point refuses it)
    const T* residual = ACT != SBA_ACT_GLU && residual_all ? residual_all + (int64_t)g * rows * Co : nullptr;
    T* out = out_all + (int64_t)g * rows * out_cstride;
    const int cv = Co / V;
    const int64_t total = rows * cv;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cv;
        const int c = (int)(i - row * cv) * V;
        Vec16<YT> a = ld16(y + row * C + c);
        Vec16<YT> gt = ACT == SBA_ACT_GLU ? ld16(y + row * C + Co + c) : a;     // the gate channels (GLU only)
        Vec16<T> r, o;
        if (residual) r = ld16(residual + row * Co + c);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int ca = c + k, cg = ACT == SBA_ACT_GLU ? Co + ca : ca;
            float n = bn_act_elem<ACT>(a.get(k), scale[ca], shift[ca], gt.get(k), scale[cg], shift[cg]);
            if (residual) n += r.get(k);
            o.set(k, n);
        }
        st16(out + row * out_cstride + out_coff + c, o);
    }
}

// ---- backward pass 1: per-channel sum(dz), sum(dz*xhat); blockIdx.y = group ----
// (This kernel keeps its element math and its LDS tail written out: with bn_bwd_elem the bf16 LeakyReLU variant took 116
// instead of 112 VGPRs, and with ChannelSum alone its 32x32 row still measured 0.1-0.2 us above the hand-written tail.)
// thread mapping: each thread keeps a fixed set of channel vectors and strides over rows
template <typename T, typename YT, int ACT>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const YT* __restrict__ y_all, const T* __restrict__ dout_all,
                                     const float* __restrict__ aux_all, float* __restrict__ red_all,
                                     int64_t rows, int C, int dcs, int dco, float* __restrict__ det_part) {
    constexpr int V = Vec16<T>::N;
    const int g = blockIdx.y;
    const YT* y = y_all + (int64_t)g * rows * C;
    const T* dout = dout_all + (int64_t)g * rows * dcs;
    const float* scale = aux_all + (int64_t)g * 4 * C;
    const float* shift = scale + C;
    const float* mean = scale + 2 * C;
    const float* rstd = scale + 3 * C;
    // one of SBA_BN_STAT_SLOTS replicas per workgroup (same-address f32 atomics serialise at the memory side)
    float* red = red_all + ((int64_t)g * SBA_BN_STAT_SLOTS + (blockIdx.x & (SBA_BN_STAT_SLOTS - 1))) * 2 * C;
    const int Co = ACT == SBA_ACT_GLU ? C / 2 : C;
    const int cv = Co / V;                                  // power of two
    extern __shared__ float s_acc[];                        // [2*C]; deterministic mode: [rows per iteration][2*C]
    if (!det_part) {
        for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) s_acc[i] = 0.f;
        __syncthreads();
    }
    const int tpr = cv < (int)blockDim.x ? cv : (int)blockDim.x;   // threads per row
    const int rpi = blockDim.x / tpr;                               // rows per iteration
    const int tc = threadIdx.x % tpr, tr = threadIdx.x / tpr;
    for (int cvi = tc; cvi < cv; cvi += tpr) {
        const int c = cvi * V;
        float s0[V], s1[V], g0[V], g1[V];
        float sc[V], sh[V], mn[V], rs[V], scg[V], shg[V], mng[V], rsg[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            s0[k] = s1[k] = g0[k] = g1[k] = 0.f;
            sc[k] = scale[c + k]; sh[k] = shift[c + k]; mn[k] = mean[c + k]; rs[k] = rstd[c + k];
            if (ACT == SBA_ACT_GLU) {
                scg[k] = scale[Co + c + k]; shg[k] = shift[Co + c + k];
                mng[k] = mean[Co + c + k]; rsg[k] = rstd[Co + c + k];
            }
        }
#pragma unroll 2
        for (int64_t row = (int64_t)blockIdx.x * rpi + tr; row < rows; row += (int64_t)gridDim.x * rpi) {
            Vec16<YT> a = ld16(y + row * C + c);
            Vec16<T> d = ld16(dout + row * dcs + dco + c);
            if (ACT == SBA_ACT_GLU) {
                Vec16<YT> gt = ld16(y + row * C + Co + c);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float n = a.get(k) * sc[k] + sh[k];
                    const float gp = gt.get(k) * scg[k] + shg[k];
                    const float s = sigmoid_bwd_(gp), dd = d.get(k);
                    const float dza = dd * s, dzg = dd * n * s * (1.f - s);
                    s0[k] += dza;
                    s1[k] += dza * (a.get(k) - mn[k]) * rs[k];
                    g0[k] += dzg;
                    g1[k] += dzg * (gt.get(k) - mng[k]) * rsg[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    float dz = d.get(k);
                    if (ACT == SBA_ACT_LRELU) {
                        const float n = a.get(k) * sc[k] + sh[k];
                        dz = n > 0.f ? dz : LRELU_SLOPE * dz;
                    }
                    s0[k] += dz;
                    s1[k] += dz * (a.get(k) - mn[k]) * rs[k];
                }
            }
        }
        if (det_part) {
            float* row = s_acc + tr * 2 * C;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                row[c + k] = s0[k];
                row[C + c + k] = s1[k];
                if (ACT == SBA_ACT_GLU) {
                    row[Co + c + k] = g0[k];
                    row[C + Co + c + k] = g1[k];
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                atomicAdd(&s_acc[c + k], s0[k]);
                atomicAdd(&s_acc[C + c + k], s1[k]);
                if (ACT == SBA_ACT_GLU) {
                    atomicAdd(&s_acc[Co + c + k], g0[k]);
                    atomicAdd(&s_acc[C + Co + c + k], g1[k]);
                }
            }
        }
    }
    __syncthreads();
    if (det_part) {
        float* part = det_part + ((int64_t)g * gridDim.x + blockIdx.x) * 2 * C;
        for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) {
            float v = 0.f;
            for (int r = 0; r < rpi; ++r) v += s_acc[r * 2 * C + i];
            part[i] = v;
        }
        return;
    }
    for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) atomicAdd(&red[i], s_acc[i]);
}

// ---- backward pass 2: dy = gamma*rstd*(dz - mean(dz) - xhat*mean(dz*xhat)); blockIdx.y = group ----
// per-channel coefficients live in LDS: A = scale, B = shift, M = mean, R = rstd, P = red0/rows, Q = red1/rows
template <typename T, typename YT, int ACT>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const YT* __restrict__ y_all, const T* __restrict__ dout_all,
                                    const float* __restrict__ aux_all, const float* __restrict__ red_all,
                                    T* __restrict__ dy_all, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                    int64_t rows, int C, int dcs, int dco) {
    constexpr int V = Vec16<T>::N;
    extern __shared__ float s_k[];                          // [6][C]
    const int g = blockIdx.y;
    const float* aux = aux_all + (int64_t)g * 4 * C;
    const float* red = red_all + (int64_t)g * SBA_BN_STAT_SLOTS * 2 * C;
    const float inv = 1.f / (float)rows;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        s_k[c] = aux[c]; s_k[C + c] = aux[C + c]; s_k[2 * C + c] = aux[2 * C + c]; s_k[3 * C + c] = aux[3 * C + c];
        float r0 = 0.f, r1 = 0.f;
#pragma unroll
        for (int sl = 0; sl < SBA_BN_STAT_SLOTS; ++sl) {    // add the replicas up
            r0 += red[(int64_t)sl * 2 * C + c];
            r1 += red[(int64_t)sl * 2 * C + C + c];
        }
        s_k[4 * C + c] = r0 * inv;
        s_k[5 * C + c] = r1 * inv;
        if (blockIdx.x == 0 && dgamma) {                    // groups accumulate into the same parameter
            atomicAdd(&dgamma[c], r1);
            atomicAdd(&dbeta[c], r0);
        }
    }
    __syncthreads();
    const float* scale = s_k;
    const float* shift = s_k + C;
    const float* mean = s_k + 2 * C;
    const float* rstd = s_k + 3 * C;
    const float* P = s_k + 4 * C;
    const float* Q = s_k + 5 * C;
    const YT* y = y_all + (int64_t)g * rows * C;
    const T* dout = dout_all + (int64_t)g * rows * dcs;
    T* dy = dy_all + (int64_t)g * rows * C;
    const int Co = ACT == SBA_ACT_GLU ? C / 2 : C;
    const int cv = Co / V;
    const int64_t total = rows * cv;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cv;
        const int c = (int)(i - row * cv) * V;
        Vec16<YT> a = ld16(y + row * C + c);
        Vec16<T> d = ld16(dout + row * dcs + dco + c);
        Vec16<T> o;
        if (ACT == SBA_ACT_GLU) {
            Vec16<YT> gt = ld16(y + row * C + Co + c);
            Vec16<T> og;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int ca = c + k, cg = Co + c + k;
                float dz[2], xh[2];
                ChCoef ka, kg;
                ch_coef_pair(scale, shift, mean, rstd, ca, cg, ka, kg);
                bn_bwd_elem<ACT>(a.get(k), gt.get(k), d.get(k), ka, kg, dz, xh);
                o.set(k, scale[ca] * (dz[0] - P[ca] - xh[0] * Q[ca]));
                og.set(k, scale[cg] * (dz[1] - P[cg] - xh[1] * Q[cg]));
            }
            st16(dy + row * C + Co + c, og);
        } else {
            // (written out: through bn_bwd_elem the bf16 kernel without activation takes one more VGPR and its 128x128 row
            // measured 0.2-0.3 us above the parent's)
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int ca = c + k;
                float dz = d.get(k);
                if (ACT == SBA_ACT_LRELU) {
                    const float n = a.get(k) * scale[ca] + shift[ca];
                    dz = n > 0.f ? dz : LRELU_SLOPE * dz;
                }
                const float xa = (a.get(k) - mean[ca]) * rstd[ca];
                o.set(k, scale[ca] * (dz - P[ca] - xa * Q[ca]));
            }
        }
        st16(dy + row * C + c, o);
    }
}

// ---- forward of BatchNorm(train) + activation for SMALL tensors whose statistics are not available from
// a conv epilogue (grouped real|fake passes): statistics, finalize, running-stat update and normalise in
// ONE launch.  A workgroup owns V channels (+ their V gate channels for GLU) over all rows and walks
// the groups in order, so the running statistics see the same sequence as consecutive module calls.
template <typename T, typename YT, int ACT>
__global__ __launch_bounds__(256) void bn_fwd_fused_kernel(const YT* __restrict__ y_all, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ rmean,
                                                           float* __restrict__ rvar, int64_t* __restrict__ nbt,
                                                           float* __restrict__ aux_all, T* __restrict__ out_all,
                                                           int64_t rows, int groups, int C, int out_cstride,
                                                           int out_coff, float eps, float momentum) {
    constexpr int V = Vec16<T>::N;
    constexpr int NV = ACT == SBA_ACT_GLU ? 2 : 1;
    __shared__ float s_red[4][2 * NV * V];
    __shared__ float s_co[2 * NV * V];                      // scale, shift per owned channel
    const int tid = threadIdx.x;
    const int Co = ACT == SBA_ACT_GLU ? C / 2 : C;
    const int c = blockIdx.x * V;
    const float count = (float)rows;
    if (blockIdx.x == 0 && tid == 0 && nbt) *nbt += groups;
    for (int g = 0; g < groups; ++g) {
        const YT* y = y_all + (int64_t)g * rows * C;
        T* out = out_all + (int64_t)g * rows * out_cstride;
        float* aux = aux_all + (int64_t)g * 4 * C;
        float s0[NV][V], s1[NV][V];
#pragma unroll
        for (int h = 0; h < NV; ++h)
#pragma unroll
            for (int k = 0; k < V; ++k) { s0[h][k] = 0.f; s1[h][k] = 0.f; }
        for (int64_t row = tid; row < rows; row += 256) {
#pragma unroll
            for (int h = 0; h < NV; ++h) {
                Vec16<YT> a = ld16(y + row * C + c + h * Co);
#pragma unroll
                for (int k = 0; k < V; ++k) { const float v = a.get(k); s0[h][k] += v; s1[h][k] += v * v; }
            }
        }
        wave_sums_to_lds(s0, s1, s_red);
        if (tid < NV * V) {
            const int h = tid / V, k = tid - h * V, ch = c + h * Co + k;
            const Moments m = moments_of(four_wave_sum(s_red, tid * 2), four_wave_sum(s_red, tid * 2 + 1), count, eps);
            const BnCoef q = bn_affine(m.mean, m.var, m.rstd, gamma[ch], beta[ch]);
            s_co[tid * 2] = q.scale;
            s_co[tid * 2 + 1] = q.shift;
            store_aux(aux, C, ch, q);
            if (rmean) running_update(rmean[ch], rvar[ch], q.mean, q.var, count, momentum);
        }
        __syncthreads();
        for (int64_t row = tid; row < rows; row += 256) {
            Vec16<YT> a = ld16(y + row * C + c);
            Vec16<YT> gt = ACT == SBA_ACT_GLU ? ld16(y + row * C + Co + c) : a;     // the gate channels (GLU only)
            Vec16<T> o;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int kg = (NV - 1) * V + k;
                o.set(k, bn_act_elem<ACT>(a.get(k), s_co[k * 2], s_co[k * 2 + 1], gt.get(k), s_co[kg * 2], s_co[kg * 2 + 1]));
            }
            st16(out + row * out_cstride + out_coff + c, o);
        }
        __syncthreads();                                    // s_red / s_co reused by the next group
    }
}

// ---- backward of BatchNorm + activation for SMALL tensors in ONE launch (the 4x4 .. 16x16 maps of
// the discriminator tails and the generator's first stage): a workgroup owns V channels (and, for GLU,
// their V gate channels) over ALL rows of one group, so both the reduction and the apply pass are
// workgroup-local -- no global accumulator, no second launch.  blockIdx.x = channel vector, .y = group.
template <typename T, typename YT, int ACT>
__global__ __launch_bounds__(256) void bn_bwd_fused_kernel(const YT* __restrict__ y_all, const T* __restrict__ dout_all,
                                                           const float* __restrict__ aux_all, T* __restrict__ dy_all,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           int64_t rows, int C, int dcs, int dco) {
    constexpr int V = Vec16<T>::N;
    constexpr int NV = ACT == SBA_ACT_GLU ? 2 : 1;          // channel vectors owned (value [+ gate])
    __shared__ float s_red[4][2 * NV * V];
    __shared__ float s_tot[2 * NV * V];
    const int g = blockIdx.y, tid = threadIdx.x;
    const int Co = ACT == SBA_ACT_GLU ? C / 2 : C;
    const int c = blockIdx.x * V;                           // first owned (value) channel
    const YT* y = y_all + (int64_t)g * rows * C;
    const T* dout = dout_all + (int64_t)g * rows * dcs;
    T* dy = dy_all + (int64_t)g * rows * C;
    const float* aux = aux_all + (int64_t)g * 4 * C;
    ChCoef kc[NV][V];
#pragma unroll
    for (int k = 0; k < V; ++k)
        ch_coef_pair(aux, aux + C, aux + 2 * C, aux + 3 * C, c + k, c + (NV - 1) * Co + k, kc[0][k], kc[NV - 1][k]);
    float s0[NV][V], s1[NV][V];
#pragma unroll
    for (int h = 0; h < NV; ++h)
#pragma unroll
        for (int k = 0; k < V; ++k) { s0[h][k] = 0.f; s1[h][k] = 0.f; }
    // dz of one row for the owned channels
    auto dz_row = [&](int64_t row, float (&dz)[NV][V], float (&xh)[NV][V]) {
        Vec16<YT> a = ld16(y + row * C + c);
        Vec16<T> d = ld16(dout + row * dcs + dco + c);
        Vec16<YT> gt = ACT == SBA_ACT_GLU ? ld16(y + row * C + Co + c) : a;     // the gate channels (GLU only)
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float z[2], x[2];
            bn_bwd_elem<ACT>(a.get(k), gt.get(k), d.get(k), kc[0][k], kc[NV - 1][k], z, x);
#pragma unroll
            for (int h = 0; h < NV; ++h) { dz[h][k] = z[h]; xh[h][k] = x[h]; }
        }
    };
    for (int64_t row = tid; row < rows; row += 256) {
        float dz[NV][V], xh[NV][V];
        dz_row(row, dz, xh);
#pragma unroll
        for (int h = 0; h < NV; ++h)
#pragma unroll
            for (int k = 0; k < V; ++k) { s0[h][k] += dz[h][k]; s1[h][k] += dz[h][k] * xh[h][k]; }
    }
    wave_sums_to_lds(s0, s1, s_red);
    if (tid < 2 * NV * V) s_tot[tid] = four_wave_sum(s_red, tid);
    __syncthreads();
    if (tid < NV * V && dgamma) {                           // groups accumulate into the same parameter
        const int h = tid / V, k = tid - h * V;
        atomicAdd(&dgamma[c + h * Co + k], s_tot[tid * 2 + 1]);
        atomicAdd(&dbeta[c + h * Co + k], s_tot[tid * 2]);
    }
    const float inv = 1.f / (float)rows;
    for (int64_t row = tid; row < rows; row += 256) {
        float dz[NV][V], xh[NV][V];
        dz_row(row, dz, xh);
#pragma unroll
        for (int h = 0; h < NV; ++h) {
            Vec16<T> o;
#pragma unroll
            for (int k = 0; k < V; ++k)
                o.set(k, kc[h][k].scale * (dz[h][k] - s_tot[(h * V + k) * 2] * inv - xh[h][k] * s_tot[(h * V + k) * 2 + 1] * inv));
            st16(dy + row * C + c + h * Co, o);
        }
    }
}

// ---- BatchNorm1d + GLU on [B][F] f32 with the NCHW->NHWC view permutation ----
// feature f' in [0,F/2) pairs with gate f'+F/2; view(B, F/2/16, 4, 4): f' = c*16 + s
// B <= BN1D_BM (the training batch): the B values of a column are loaded ONCE into registers, all loads in flight together
// (three passes of dependent loads took 27 us for 20 x 16384 values at the head of the generator's forward pass); a larger
// batch reads global memory at every use.  Same sums in the same order either way: each kernel's body is written once,
// over sample_at and BN1D_EACH_SAMPLE.  (Plain loops, and the cache filled in the body, on purpose: a lambda that captures
// the register cache, or a helper that fills it, costs bn1d_glu_bwd_kernel 31 VGPRs and a wave of occupancy.)
constexpr int BN1D_BM = 32;
// sample b of a column of p[B][stride]: from the register cache, or p[b * stride + col]
template <bool CACHED, typename T, int N>
__device__ __forceinline__ float sample_at(const float (&cache)[N], const T* __restrict__ p, int stride, int col, int b) {
    if constexpr (CACHED) return cache[b];
    else return to_f<T>(p[(int64_t)b * stride + col]);
}
// for every sample b < B: fully unrolled over the register cache (CACHED, a compile-time constant of the body), one
// iteration at a time otherwise -- `unroll 1` pins the uncached loop, which the compiler was free to unroll before
#define BN1D_EACH_SAMPLE(b, B, CACHED) \
    _Pragma("unroll CACHED ? BN1D_BM : 1") for (int b = 0; b < (CACHED ? BN1D_BM : B); ++b) if (b < B)

template <typename T, bool CACHED>
__device__ __forceinline__ void bn1d_glu_fwd_body(const float* __restrict__ y, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, float* __restrict__ rmean,
                                                  float* __restrict__ rvar, float* __restrict__ mean_o,
                                                  float* __restrict__ rstd_o, T* __restrict__ out, int B, int F, int f,
                                                  float eps, float momentum) {
    const int fh = F / 2, Cg = fh / 16;
    float yv[2][CACHED ? BN1D_BM : 1];
    if constexpr (CACHED) {
#pragma unroll
        for (int b = 0; b < BN1D_BM; ++b) {
            yv[0][b] = b < B ? y[(int64_t)b * F + f] : 0.f;
            yv[1][b] = b < B ? y[(int64_t)b * F + f + fh] : 0.f;
        }
    }
    float sc[2], sh[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ff = f + h * fh;
        float s = 0.f, q = 0.f;
        BN1D_EACH_SAMPLE(b, B, CACHED) s += sample_at<CACHED>(yv[h], y, F, ff, b);
        const float mean = s / B;
        BN1D_EACH_SAMPLE(b, B, CACHED) { const float v = sample_at<CACHED>(yv[h], y, F, ff, b) - mean; q += v * v; }    // centred: two passes
        const float var = q / B, r = rsqrtf(var + eps);
        // (y * scale + shift: the form the step's forward values were validated with.  The backward kernel recomputes the
        // pre-activation as (y - mean) * scale + beta, which does not cancel at a tiny batch variance; see there)
        sc[h] = gamma[ff] * r; sh[h] = beta[ff] - mean * sc[h];
        mean_o[ff] = mean; rstd_o[ff] = r;
        if (rmean) running_update(rmean[ff], rvar[ff], mean, var, (float)B, momentum);
    }
    const int c = f / 16, s16 = f % 16;
    BN1D_EACH_SAMPLE(b, B, CACHED) {
        const float ya = sample_at<CACHED>(yv[0], y, F, f, b), yg = sample_at<CACHED>(yv[1], y, F, f + fh, b);
        // (fmaf: the contraction the compiler made of y * scale + shift while the expression stood here alone; through
        // bn_act_elem the vectoriser pairs the add with one of __expf's and leaves it unfused -- other bits in `out`)
        const float n = fmaf(ya, sc[0], sh[0]), gp = fmaf(yg, sc[1], sh[1]);
        out[((int64_t)b * 16 + s16) * Cg + c] = from_f<T>(n * sigmoidf_(gp));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bn1d_glu_fwd_kernel(const float* __restrict__ y, const float* __restrict__ gamma,
                                    const float* __restrict__ beta, float* __restrict__ rmean,
                                    float* __restrict__ rvar, int64_t* __restrict__ nbt,
                                    float* __restrict__ mean_o, float* __restrict__ rstd_o,
                                    T* __restrict__ out, int B, int F, float eps, float momentum) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f == 0 && nbt) *nbt += 1;
    if (f >= F / 2) return;
    if (B <= BN1D_BM) bn1d_glu_fwd_body<T, true>(y, gamma, beta, rmean, rvar, mean_o, rstd_o, out, B, F, f, eps, momentum);
    else bn1d_glu_fwd_body<T, false>(y, gamma, beta, rmean, rvar, mean_o, rstd_o, out, B, F, f, eps, momentum);
}

// dz of one sample's value and gate feature.  The pre-activations are recomputed as (y - mean) * scale + beta, not
// y * scale + shift: with a tiny batch variance (B = 2, two nearly equal samples: rstd up to 316) y * scale and shift are
// two large numbers that cancel, and the gate's rounding error (4e-5) reaches dgamma / dbeta
struct Bn1dCoef { float scale, beta, mean, rstd; };
__device__ __forceinline__ void bn1d_glu_dz(float ya, float yg, float dd, const Bn1dCoef& ka, const Bn1dCoef& kg,
                                            float& dza, float& dzg) {
    const float n = (ya - ka.mean) * ka.scale + ka.beta, gp = (yg - kg.mean) * kg.scale + kg.beta, s = sigmoidf_(gp);
    dza = dd * s;
    dzg = dd * n * s * (1.f - s);
}

template <typename T, bool CACHED>
__device__ __forceinline__ void bn1d_glu_bwd_body(const float* __restrict__ y, const T* __restrict__ dout,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  const float* __restrict__ mean, const float* __restrict__ rstd,
                                                  float* __restrict__ dy, float* __restrict__ dgamma,
                                                  float* __restrict__ dbeta, int B, int F, int f) {
    const int fh = F / 2, Cg = fh / 16;
    const int fa = f, fg = f + fh, dcol = (f % 16) * Cg + f / 16;       // dout[b][s16][c]: column s16 * Cg + c of 16 * Cg
    const Bn1dCoef ka{gamma[fa] * rstd[fa], beta[fa], mean[fa], rstd[fa]}, kg{gamma[fg] * rstd[fg], beta[fg], mean[fg], rstd[fg]};
    constexpr int NB = CACHED ? BN1D_BM : 1;
    float ya_[NB], yg_[NB], dd_[NB];
    if constexpr (CACHED) {
#pragma unroll
        for (int b = 0; b < BN1D_BM; ++b) {
            ya_[b] = b < B ? y[(int64_t)b * F + fa] : 0.f;
            yg_[b] = b < B ? y[(int64_t)b * F + fg] : 0.f;
            dd_[b] = b < B ? to_f<T>(dout[(int64_t)b * (16 * Cg) + dcol]) : 0.f;
        }
    }
    float a0 = 0.f, a1 = 0.f, g0 = 0.f, g1 = 0.f;
    BN1D_EACH_SAMPLE(b, B, CACHED) {
        const float ya = sample_at<CACHED>(ya_, y, F, fa, b), yg = sample_at<CACHED>(yg_, y, F, fg, b);
        float dza, dzg;
        bn1d_glu_dz(ya, yg, sample_at<CACHED>(dd_, dout, 16 * Cg, dcol, b), ka, kg, dza, dzg);
        a0 += dza; a1 += dza * (ya - ka.mean) * ka.rstd;
        g0 += dzg; g1 += dzg * (yg - kg.mean) * kg.rstd;
    }
    dgamma[fa] += a1; dbeta[fa] += a0;
    dgamma[fg] += g1; dbeta[fg] += g0;
    const float inv = 1.f / B;
    BN1D_EACH_SAMPLE(b, B, CACHED) {
        const float ya = sample_at<CACHED>(ya_, y, F, fa, b), yg = sample_at<CACHED>(yg_, y, F, fg, b);
        float dza, dzg;
        bn1d_glu_dz(ya, yg, sample_at<CACHED>(dd_, dout, 16 * Cg, dcol, b), ka, kg, dza, dzg);
        dy[(int64_t)b * F + fa] = ka.scale * (dza - a0 * inv - (ya - ka.mean) * ka.rstd * a1 * inv);
        dy[(int64_t)b * F + fg] = kg.scale * (dzg - g0 * inv - (yg - kg.mean) * kg.rstd * g1 * inv);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bn1d_glu_bwd_kernel(const float* __restrict__ y, const T* __restrict__ dout,
                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                    float* __restrict__ dy, float* __restrict__ dgamma,
                                    float* __restrict__ dbeta, int B, int F) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F / 2) return;
    if (B <= BN1D_BM) bn1d_glu_bwd_body<T, true>(y, dout, gamma, beta, mean, rstd, dy, dgamma, dbeta, B, F, f);
    else bn1d_glu_bwd_body<T, false>(y, dout, gamma, beta, mean, rstd, dy, dgamma, dbeta, B, F, f);
}

// ---- InstanceNorm statistics / AdaIN ----
// grid (N, splits); threads [rows][C/V]; accumulates (sum, sumsq) into mean/rstd buffers
template <typename T>
__global__ __launch_bounds__(256) void instnorm_accum_kernel(const T* __restrict__ h, float* __restrict__ sum,
                                      float* __restrict__ sumsq, int HW, int C, int det) {
    constexpr int V = Vec16<T>::N;
    const int cv = C / V, n = blockIdx.x;
    const int rpi = blockDim.x / cv;
    const int tc = threadIdx.x % cv, tr = threadIdx.x / cv;
    extern __shared__ float s_acc[];   // [2*C]; deterministic mode (one workgroup per image): [rpi][2*C]
    const ChannelSum cs{s_acc, C, det != 0};
    cs.clear();
    float s0[V], s1[V];
#pragma unroll
    for (int k = 0; k < V; ++k) s0[k] = s1[k] = 0.f;
    if (tr < rpi) {
        for (int p = blockIdx.y * rpi + tr; p < HW; p += gridDim.y * rpi) {
            Vec16<T> a = ld16(h + ((int64_t)n * HW + p) * C + tc * V);
#pragma unroll
            for (int k = 0; k < V; ++k) { const float v = a.get(k); s0[k] += v; s1[k] += v * v; }
        }
        cs.add(tr, tc * V, s0, s1);
    }
    // (deterministic mode, gridDim.y == 1: this workgroup owns image n -- plain stores)
    cs.finish(rpi, [&](int i, float v) {
        float* dst = i < C ? &sum[n * C + i] : &sumsq[n * C + i - C];
        if (det) *dst = v;
        else atomicAdd(dst, v);
    });
}

// The same statistics in ONE launch, no atomics, no clearing, no finalize pass: workgroup (n, tc) owns 16-byte channel vector tc
// of image n over all HW pixels -- each thread sums its pixels (four loads in flight), the 256 partial sums meet in a fixed
// order through LDS, thread 0..V-1 write mean and rstd.  Three launches (clear, accumulate, finalize: 28-35 us alone at the
// entry of a generator stage, serial time of the step) become one; deterministic by construction.
template <typename T>
__global__ __launch_bounds__(256) void instnorm_stats_fused_kernel(const T* __restrict__ h, float* __restrict__ mean,
                                                                   float* __restrict__ rstd, int HW, int C, float eps) {
    constexpr int V = Vec16<T>::N;
    const int n = blockIdx.x, tc = blockIdx.y, tid = threadIdx.x;
    const T* base = h + (int64_t)n * HW * C + tc * V;
    float s0[V], s1[V];
#pragma unroll
    for (int k = 0; k < V; ++k) s0[k] = s1[k] = 0.f;
    int p = tid;
    for (; p + 3 * 256 < HW; p += 4 * 256) {
        Vec16<T> a0 = ld16(base + (int64_t)p * C), a1 = ld16(base + (int64_t)(p + 256) * C);
        Vec16<T> a2 = ld16(base + (int64_t)(p + 512) * C), a3 = ld16(base + (int64_t)(p + 768) * C);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float v0 = a0.get(k), v1 = a1.get(k), v2 = a2.get(k), v3 = a3.get(k);
            s0[k] += (v0 + v1) + (v2 + v3);
            s1[k] += (v0 * v0 + v1 * v1) + (v2 * v2 + v3 * v3);
        }
    }
    for (; p < HW; p += 256) {
        Vec16<T> a = ld16(base + (int64_t)p * C);
#pragma unroll
        for (int k = 0; k < V; ++k) { const float v = a.get(k); s0[k] += v; s1[k] += v * v; }
    }
    __shared__ float s_part[4][2 * V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const float a = wave_sum(s0[k]), b = wave_sum(s1[k]);
        if ((tid & 63) == 0) { s_part[tid >> 6][k] = a; s_part[tid >> 6][V + k] = b; }
    }
    __syncthreads();
    if (tid < V) {
        const float sm = (s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid]);
        const float sq = (s_part[0][V + tid] + s_part[1][V + tid]) + (s_part[2][V + tid] + s_part[3][V + tid]);
        const Moments m = moments_of(sm, sq, (float)HW, eps);
        mean[n * C + tc * V + tid] = m.mean;
        rstd[n * C + tc * V + tid] = m.rstd;
    }
}

__global__ __launch_bounds__(256) void instnorm_finalize_kernel(float* __restrict__ mean, float* __restrict__ rstd, int NC,
                                         float HW, float eps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NC) return;
    const Moments m = moments_of(mean[i], rstd[i], HW, eps);
    mean[i] = m.mean;
    rstd[i] = m.rstd;
}

template <typename T>
__global__ __launch_bounds__(256) void adain_fwd_kernel(const T* __restrict__ h, const float* __restrict__ mean,
                                 const float* __restrict__ rstd, const float* __restrict__ style,
                                 T* __restrict__ out, int N, int HW, int C, int ocs, int oco) {
    constexpr int V = Vec16<T>::N;
    const int cv = C / V;
    const int64_t total = (int64_t)N * HW * cv;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cv;
        const int c = (int)(i - row * cv) * V;
        const int n = (int)(row / HW);
        Vec16<T> a = ld16(h + row * C + c), o;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float xh = (a.get(k) - mean[n * C + c + k]) * rstd[n * C + c + k];
            o.set(k, (style[n * 2 * C + c + k] + 1.f) * xh + style[n * 2 * C + C + c + k]);
        }
        st16(out + row * ocs + oco + c, o);
    }
}

// red[n][c][0] += sum dout*xhat, red[n][c][1] += sum dout
template <typename T>
__global__ __launch_bounds__(256) void adain_bwd_reduce_kernel(const T* __restrict__ h, const T* __restrict__ dout,
                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                        float* __restrict__ red, int HW, int C, int dcs, int dco, int det) {
    constexpr int V = Vec16<T>::N;
    const int cv = C / V, n = blockIdx.x;
    const int rpi = blockDim.x / cv;
    const int tc = threadIdx.x % cv, tr = threadIdx.x / cv;
    extern __shared__ float s_acc[];   // [2*C]; deterministic mode (one workgroup per image): [rpi][2*C]
    const ChannelSum cs{s_acc, C, det != 0};
    cs.clear();
    float s0[V], s1[V];
#pragma unroll
    for (int k = 0; k < V; ++k) s0[k] = s1[k] = 0.f;
    if (tr < rpi) {
        for (int p = blockIdx.y * rpi + tr; p < HW; p += gridDim.y * rpi) {
            const int64_t row = (int64_t)n * HW + p;
            Vec16<T> a = ld16(h + row * C + tc * V);
            Vec16<T> d = ld16(dout + row * dcs + dco + tc * V);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const int c = tc * V + k;
                const float xh = (a.get(k) - mean[n * C + c]) * rstd[n * C + c];
                s0[k] += d.get(k) * xh;
                s1[k] += d.get(k);
            }
        }
        cs.add(tr, tc * V, s0, s1);
    }
    cs.finish(rpi, [&](int i, float v) {
        float* dst = i < C ? &red[(n * C + i) * 2 + 0] : &red[(n * C + i - C) * 2 + 1];
        if (det) *dst += v;
        else atomicAdd(dst, v);
    });
}

template <typename T>
__global__ __launch_bounds__(256) void adain_bwd_apply_kernel(const T* __restrict__ h, const T* __restrict__ dout,
                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                       const float* __restrict__ style, const float* __restrict__ red,
                                       T* __restrict__ dh, float* __restrict__ dstyle, int N, int HW,
                                       int C, int dcs, int dco, int accumulate) {
    constexpr int V = Vec16<T>::N;
    const int cv = C / V;
    const float inv = 1.f / HW;
    if (blockIdx.x == 0 && dstyle) {
        for (int i = threadIdx.x; i < N * C; i += blockDim.x) {
            const int n = i / C, c = i - n * C;
            dstyle[n * 2 * C + c] = red[i * 2 + 0];
            dstyle[n * 2 * C + C + c] = red[i * 2 + 1];
        }
    }
    const int64_t total = (int64_t)N * HW * cv;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cv;
        const int c = (int)(i - row * cv) * V;
        const int n = (int)(row / HW);
        Vec16<T> a = ld16(h + row * C + c);
        Vec16<T> d = ld16(dout + row * dcs + dco + c);
        Vec16<T> o;
        if (accumulate) o = ld16(dh + row * C + c);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int nc = n * C + c + k;
            const float xh = (a.get(k) - mean[nc]) * rstd[nc];
            const float g = (style[n * 2 * C + c + k] + 1.f) * rstd[nc];
            float v = g * (d.get(k) - red[nc * 2 + 1] * inv - xh * red[nc * 2 + 0] * inv);
            if (accumulate) v += o.get(k);
            o.set(k, v);
        }
        st16(dh + row * C + c, o);
    }
}

inline int grid_for(int64_t items, int cap = 4096) {
    int64_t b = (items + 255) / 256;
    if (b < 1) b = 1;
    return (int)(b > cap ? cap : b);
}
inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

inline int vec_width(int dtype) { return dtype != SBA_F32 ? 8 : 4; }       // elements per 16-byte vector
inline int64_t elem_size(int dtype) { return dtype != SBA_F32 ? 2 : 4; }
// a `width` channel slice at `offset` of rows `stride` channels apart, all three in whole vectors
inline bool slice_ok(int stride, int offset, int width, int V) {
    return stride >= width + offset && stride % V == 0 && offset % V == 0;
}
inline int act_width(int C, int act) { return act == SBA_ACT_GLU ? C / 2 : C; }  // channels after the activation

// Grid of the two channel-sum passes (bn_stats_kernel, bn_bwd_reduce_kernel): rpi rows per iteration of a workgroup.
// Every workgroup ends with 2C same-address f32 atomics per replica: measured (tools/bench_bn.py) 85 -> 63 us at
// 256x256 and 64 -> 43 us at 128x128 going from 1024 to 512 workgroups in total (two per CU)
constexpr int BN_RED_WORKGROUPS = 512;                      // over all groups ...
constexpr int BN_RED_WORKGROUPS_PER_GROUP = 64;             // ... but at least this many for each
struct ReduceGrid { int rpi, blocks; };
inline ReduceGrid reduce_grid(int64_t rows, int cv, int groups) {
    ReduceGrid r;
    r.rpi = cv < 256 ? 256 / cv : 1;
    r.blocks = cdiv(rows, (int64_t)r.rpi * 8);
    const int cap = BN_RED_WORKGROUPS / groups > BN_RED_WORKGROUPS_PER_GROUP ? BN_RED_WORKGROUPS / groups
                                                                              : BN_RED_WORKGROUPS_PER_GROUP;
    if (r.blocks > cap) r.blocks = cap;
    if (r.blocks < 1) r.blocks = 1;
    return r;
}
// One channel-sum pass into dst[groups][SBA_BN_STAT_SLOTS][2*C]: launch(lds_bytes, part) starts the kernel.  Deterministic
// mode: each workgroup gets a slot of scratch (`part`) and one LDS row per row-group, and the workgroups' partial sums are
// added in workgroup order into replica 0 (the others stay zero).
template <typename Launch>
int reduce_pass(int groups, ReduceGrid rg, int C, float* dst, hipStream_t st, Launch launch) {
    float* part = nullptr;
    size_t sh = 2 * (size_t)C * sizeof(float);
    if (sba_det_on()) {
        part = sba_det_alloc((int64_t)groups * rg.blocks * 2 * C);
        if (!part) return SBA_E_ARG;
        sh *= rg.rpi;
    }
    const int rc = launch(sh, part);
    if (rc != SBA_OK) return rc;
    if (part) sba_det_fold(part, groups, rg.blocks, 2 * C, dst, (int64_t)SBA_BN_STAT_SLOTS * 2 * C, 0, st);
    return SBA_CHECK_LAUNCH();
}
// A backward launch whose groups add into the same dgamma / dbeta: launch(g0, ng) covers groups [g0, g0 + ng).  All
// groups at once, or in deterministic mode one launch per group, in group order.
template <typename Launch>
int param_grad_pass(int groups, bool param_grads, Launch launch) {
    const int step = sba_det_on() && groups > 1 && param_grads ? 1 : groups;
    for (int g = 0; g < groups; g += step) {
        const int rc = launch(g, step);
        if (rc != SBA_OK) return rc;
    }
    return SBA_CHECK_LAUNCH();
}
// workgroups per image of the two InstanceNorm channel-sum passes (deterministic mode: one, row-groups added in order)
inline int instnorm_splits(int HW, int rpi, bool det) {
    const int splits = cdiv(HW, rpi * 16);
    return det ? 1 : splits > 256 ? 256 : splits;
}

}  // namespace

extern "C" int sba_bn_stats(int dtype, const void* y, float* stats, int64_t rows, int groups, int C,
                            void* stream) {
    const int V = vec_width(dtype);
    if (!y || !stats || rows <= 0 || groups <= 0 || groups > 65535 || C <= 0 || C % V || C > 4096)
        return SBA_E_ARG;
    const ReduceGrid rg = reduce_grid(rows, C / V, groups);
    return reduce_pass(groups, rg, C, stats, (hipStream_t)stream, [&](size_t sh, float* part) -> int {
        SBA_DISPATCH_Y(dtype, SBA_LAUNCH((bn_stats_kernel<YT>), dim3(rg.blocks, groups), dim3(256), sh, (hipStream_t)stream,
                                         (const YT*)y, stats, rows, C, part));
        return SBA_OK;
    });
}

// ACT_SWITCH: the activations that have a backward; ACT_SWITCH_FWD adds ReLU (sba_bn_act_fwd only: the Inception trunk)
#define ACT_CASE(A, ...) case A: { constexpr int ACT = A; __VA_ARGS__; } break;
#define ACT_SWITCH_(act, EXTRA_CASE, ...)                                                                       \
    switch (act) {                                                                                               \
        ACT_CASE(SBA_ACT_NONE, __VA_ARGS__) ACT_CASE(SBA_ACT_GLU, __VA_ARGS__) ACT_CASE(SBA_ACT_LRELU, __VA_ARGS__) \
        EXTRA_CASE                                                                                               \
        default: return SBA_E_ARG;                                                                               \
    }
#define ACT_SWITCH(act, ...) ACT_SWITCH_(act, , __VA_ARGS__)
#define ACT_SWITCH_FWD(act, ...) ACT_SWITCH_(act, ACT_CASE(SBA_ACT_RELU, __VA_ARGS__), __VA_ARGS__)

static bool bn_shape_ok(int dtype, int64_t rows, int groups, int C, int act) {
    return rows > 0 && groups > 0 && groups <= 65535 && C > 0 && pow2(C) && act_width(C, act) % vec_width(dtype) == 0 &&
           C <= 4096;
}

extern "C" int sba_bn_act_fwd(int dtype, const void* y, const float* stats, const float* gamma,
                              const float* beta, float* running_mean, float* running_var,
                              int64_t* num_batches_tracked, float* aux, const void* residual, void* out,
                              int64_t rows, int groups, int C, int act, int out_cstride, int out_coff, float eps,
                              float momentum, int training, void* stream) {
    // (the forward kernel indexes channels generically: any C that is a multiple of the vector width -- the Inception
    // trunk's 80 / 96 / 160 / 192 / 320 / 448 ... channel BatchNorms in the DAMSM pre-training loop)
    const int V = vec_width(dtype), Co = act_width(C, act);
    const bool shape_ok = rows > 0 && groups > 0 && groups <= 65535 && C > 0 && C <= 4096 &&
                          (act == SBA_ACT_GLU ? Co % V == 0 && C % 2 == 0 : C % V == 0);
    if (!y || !gamma || !beta || !aux || !out || !shape_ok) return SBA_E_ARG;
    if (training ? !stats : (!running_mean || !running_var)) return SBA_E_ARG;
    if ((running_mean == nullptr) != (running_var == nullptr)) return SBA_E_ARG;
    if (act == SBA_ACT_GLU && residual) return SBA_E_ARG;
    if (!slice_ok(out_cstride, out_coff, Co, V)) return SBA_E_ARG;
    const int blocks = grid_for(rows * (Co / V));
    const size_t sh = 2 * (size_t)C * sizeof(float);
    SBA_DISPATCH_Y(dtype, ACT_SWITCH_FWD(act, SBA_LAUNCH((bn_act_fwd_kernel<T, YT, ACT>), dim3(blocks, groups),
                                                               dim3(256), sh, (hipStream_t)stream, (const YT*)y, stats,
                                                               gamma, beta, running_mean, running_var,
                                                               num_batches_tracked, aux, (const T*)residual, (T*)out,
                                                               rows, C, out_cstride, out_coff, eps, momentum,
                                                               training)));
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_bn_act_bwd_reduce(int dtype, const void* y, const void* dout, const float* aux, float* red,
                                     int64_t rows, int groups, int C, int act, int dcs, int dco, void* stream) {
    if (!y || !dout || !aux || !red || !bn_shape_ok(dtype, rows, groups, C, act)) return SBA_E_ARG;
    const int V = vec_width(dtype), Co = act_width(C, act);
    if (!slice_ok(dcs, dco, Co, V)) return SBA_E_ARG;
    const ReduceGrid rg = reduce_grid(rows, Co / V, groups);
    return reduce_pass(groups, rg, C, red, (hipStream_t)stream, [&](size_t sh, float* part) -> int {
        SBA_DISPATCH_Y(dtype, ACT_SWITCH(act, SBA_LAUNCH((bn_bwd_reduce_kernel<T, YT, ACT>), dim3(rg.blocks, groups),
                                                               dim3(256), sh, (hipStream_t)stream, (const YT*)y,
                                                               (const T*)dout, aux, red, rows, C, dcs, dco, part)));
        return SBA_OK;
    });
}

extern "C" int sba_bn_act_bwd_apply(int dtype, const void* y, const void* dout, const float* aux,
                                    const float* red, void* dy, float* dgamma, float* dbeta, int64_t rows,
                                    int groups, int C, int act, int dcs, int dco, void* stream) {
    if (!y || !dout || !aux || !red || !dy || !bn_shape_ok(dtype, rows, groups, C, act)) return SBA_E_ARG;
    if ((dgamma == nullptr) != (dbeta == nullptr)) return SBA_E_ARG;
    const int V = vec_width(dtype), Co = act_width(C, act);
    if (!slice_ok(dcs, dco, Co, V)) return SBA_E_ARG;
    const int blocks = grid_for(rows * (Co / V));
    const size_t sh = 6 * (size_t)C * sizeof(float);
    const int64_t esz = elem_size(dtype);
    return param_grad_pass(groups, dgamma != nullptr, [&](int g, int ng) -> int {
        const char* yg = (const char*)y + (int64_t)g * rows * C * esz;
        const char* dg = (const char*)dout + (int64_t)g * rows * dcs * esz;
        char* dyg = (char*)dy + (int64_t)g * rows * C * esz;
        const float* auxg = aux + (int64_t)g * 4 * C;
        const float* redg = red + (int64_t)g * SBA_BN_STAT_SLOTS * 2 * C;
        SBA_DISPATCH_Y(dtype, ACT_SWITCH(act, SBA_LAUNCH((bn_bwd_apply_kernel<T, YT, ACT>), dim3(blocks, ng), dim3(256), sh,
                                                               (hipStream_t)stream, (const YT*)yg, (const T*)dg, auxg, redg,
                                                               (T*)dyg, dgamma, dbeta, rows, C, dcs, dco)));
        return SBA_OK;
    });
}

extern "C" int sba_bn_act_fwd_fused(int dtype, const void* y, const float* gamma, const float* beta,
                                    float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                    float* aux, void* out, int64_t rows, int groups, int C, int act,
                                    int out_cstride, int out_coff, float eps, float momentum, void* stream) {
    if (!y || !gamma || !beta || !aux || !out || !bn_shape_ok(dtype, rows, groups, C, act)) return SBA_E_ARG;
    if ((running_mean == nullptr) != (running_var == nullptr)) return SBA_E_ARG;
    const int V = vec_width(dtype), Co = act_width(C, act);
    if (!slice_ok(out_cstride, out_coff, Co, V)) return SBA_E_ARG;
    SBA_DISPATCH_Y(dtype, ACT_SWITCH(act, SBA_LAUNCH((bn_fwd_fused_kernel<T, YT, ACT>), dim3(Co / V), dim3(256), 0,
                                                           (hipStream_t)stream, (const YT*)y, gamma, beta,
                                                           running_mean, running_var, num_batches_tracked, aux,
                                                           (T*)out, rows, groups, C, out_cstride, out_coff, eps,
                                                           momentum)));
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_bn_act_bwd_fused(int dtype, const void* y, const void* dout, const float* aux, void* dy,
                                    float* dgamma, float* dbeta, int64_t rows, int groups, int C, int act, int dcs,
                                    int dco, void* stream) {
    if (!y || !dout || !aux || !dy || !bn_shape_ok(dtype, rows, groups, C, act)) return SBA_E_ARG;
    if ((dgamma == nullptr) != (dbeta == nullptr)) return SBA_E_ARG;
    const int V = vec_width(dtype), Co = act_width(C, act);
    if (!slice_ok(dcs, dco, Co, V)) return SBA_E_ARG;
    const int64_t esz = elem_size(dtype);
    return param_grad_pass(groups, dgamma != nullptr, [&](int g, int ng) -> int {
        const char* yg = (const char*)y + (int64_t)g * rows * C * esz;
        const char* dg = (const char*)dout + (int64_t)g * rows * dcs * esz;
        char* dyg = (char*)dy + (int64_t)g * rows * C * esz;
        const float* auxg = aux + (int64_t)g * 4 * C;
        SBA_DISPATCH_Y(dtype, ACT_SWITCH(act, SBA_LAUNCH((bn_bwd_fused_kernel<T, YT, ACT>), dim3(Co / V, ng), dim3(256), 0,
                                                               (hipStream_t)stream, (const YT*)yg, (const T*)dg, auxg,
                                                               (T*)dyg, dgamma, dbeta, rows, C, dcs, dco)));
        return SBA_OK;
    });
}

extern "C" int sba_bn1d_glu_fwd(int dtype, const float* y, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, int64_t* nbt, float* mean, float* rstd,
                                void* out, int B, int F, float eps, float momentum, void* stream) {
    if (!y || !gamma || !beta || !mean || !rstd || !out || B <= 0 || F <= 0 || F % 32 != 0) return SBA_E_ARG;
    if ((running_mean == nullptr) != (running_var == nullptr)) return SBA_E_ARG;
    SBA_DISPATCH(dtype, SBA_LAUNCH((bn1d_glu_fwd_kernel<T>), dim3(cdiv(F / 2, 64)), dim3(64), 0,
                                           (hipStream_t)stream, y, gamma, beta, running_mean, running_var, nbt,
                                           mean, rstd, (T*)out, B, F, eps, momentum));
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_bn1d_glu_bwd(int dtype, const float* y, const void* dout, const float* gamma, const float* beta,
                                const float* mean, const float* rstd, float* dy, float* dgamma, float* dbeta,
                                int B, int F, void* stream) {
    if (!y || !dout || !gamma || !beta || !mean || !rstd || !dy || !dgamma || !dbeta || B <= 0 || F <= 0 ||
        F % 32 != 0)
        return SBA_E_ARG;
    SBA_DISPATCH(dtype, SBA_LAUNCH((bn1d_glu_bwd_kernel<T>), dim3(cdiv(F / 2, 64)), dim3(64), 0,
                                           (hipStream_t)stream, y, (const T*)dout, gamma, beta, mean, rstd, dy,
                                           dgamma, dbeta, B, F));
    return SBA_CHECK_LAUNCH();
}

static bool in_shape_ok(int dtype, int N, int HW, int C) {
    // (the dtype is refused HERE, before sba_instnorm_stats clears its outputs: a refused call writes nothing)
    if (dtype != SBA_F32 && dtype != SBA_BF16) return false;
    const int V = vec_width(dtype);
    return N > 0 && HW > 0 && C > 0 && C % V == 0 && C / V <= 256 && pow2(C / V);
}

extern "C" int sba_instnorm_stats(int dtype, const void* h, float* mean, float* rstd, int N, int HW, int C,
                                  float eps, void* stream) {
    if (!h || !mean || !rstd || !in_shape_ok(dtype, N, HW, C)) return SBA_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int V = vec_width(dtype);
    if (N * (C / V) >= 64 && HW >= 1024) {                  // enough workgroups of enough pixels: one launch
        SBA_DISPATCH(dtype, SBA_LAUNCH((instnorm_stats_fused_kernel<T>), dim3(N, C / V), dim3(256), 0, st, (const T*)h, mean,
                                               rstd, HW, C, eps));
        return SBA_CHECK_LAUNCH();
    }
    // small shapes: clear + accumulate + finalize
    sba_zero_f32(mean, rstd, (int64_t)N * C, st);
    const int rpi = 256 / (C / V);
    const bool det = sba_det_on();
    SBA_DISPATCH(dtype, SBA_LAUNCH((instnorm_accum_kernel<T>), dim3(N, instnorm_splits(HW, rpi, det)), dim3(256),
                                           (det ? rpi : 1) * 2 * C * sizeof(float), st, (const T*)h, mean, rstd, HW, C,
                                           (int)det));
    SBA_LAUNCH(instnorm_finalize_kernel, dim3(cdiv(N * C, 256)), dim3(256), 0, st, mean, rstd, N * C,
                       (float)HW, eps);
    return SBA_CHECK_LAUNCH();
}


extern "C" int sba_adain_fwd(int dtype, const void* h, const float* mean, const float* rstd, const float* style,
                             void* out, int N, int HW, int C, int ocs, int oco, void* stream) {
    if (!h || !mean || !rstd || !style || !out || !in_shape_ok(dtype, N, HW, C)) return SBA_E_ARG;
    const int V = vec_width(dtype);
    if (!slice_ok(ocs, oco, C, V)) return SBA_E_ARG;
    const int blocks = grid_for((int64_t)N * HW * (C / V));
    SBA_DISPATCH(dtype, SBA_LAUNCH((adain_fwd_kernel<T>), dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                                           (const T*)h, mean, rstd, style, (T*)out, N, HW, C, ocs, oco));
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_adain_bwd_reduce(int dtype, const void* h, const void* dout, const float* mean,
                                    const float* rstd, float* red, int N, int HW, int C, int dcs, int dco,
                                    void* stream) {
    if (!h || !dout || !mean || !rstd || !red || !in_shape_ok(dtype, N, HW, C)) return SBA_E_ARG;
    const int V = vec_width(dtype);
    if (!slice_ok(dcs, dco, C, V)) return SBA_E_ARG;
    const int rpi = 256 / (C / V);
    const bool det = sba_det_on();
    SBA_DISPATCH(dtype, SBA_LAUNCH((adain_bwd_reduce_kernel<T>), dim3(N, instnorm_splits(HW, rpi, det)), dim3(256),
                                           (det ? rpi : 1) * 2 * C * sizeof(float), (hipStream_t)stream, (const T*)h,
                                           (const T*)dout, mean, rstd, red, HW, C, dcs, dco, (int)det));
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_adain_bwd_apply(int dtype, const void* h, const void* dout, const float* mean,
                                   const float* rstd, const float* style, const float* red, void* dh,
                                   float* dstyle, int N, int HW, int C, int dcs, int dco, int accumulate,
                                   void* stream) {
    if (!h || !dout || !mean || !rstd || !style || !red || !dh || !in_shape_ok(dtype, N, HW, C)) return SBA_E_ARG;
    const int V = vec_width(dtype);
    if (!slice_ok(dcs, dco, C, V)) return SBA_E_ARG;
    const int blocks = grid_for((int64_t)N * HW * (C / V));
    SBA_DISPATCH(dtype, SBA_LAUNCH((adain_bwd_apply_kernel<T>), dim3(blocks), dim3(256), 0,
                                           (hipStream_t)stream, (const T*)h, (const T*)dout, mean, rstd, style,
                                           red, (T*)dh, dstyle, N, HW, C, dcs, dco, accumulate));
    return SBA_CHECK_LAUNCH();
}
