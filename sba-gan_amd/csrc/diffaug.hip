// Differentiable Augmentation (Zhao et al., NeurIPS 2020; policy color,translation,cutout) of the image batch a
// discriminator sees, forward and backward (sba_diffaug_fwd / sba_diffaug_bwd in sbagan_hip.h; sbagan/ops.py: DiffAugFn;
// DESIGN.md 7n).  The forward is the step's [real | fake] concatenation and the augmentation in one pass.
//
// Bandwidth bound: every image element is read once (twice with color on: the per-image sum) and written once.  One
// thread owns four consecutive pixels of the S x S plane in all three channels (the saturation step needs the pixel's
// channel mean): three 16-byte loads -- unaligned by the translation, which a global load tolerates -- and three aligned
// 16-byte stores.  The plane is split over blocks (grid.x), the images over grid.y.
//
// The per-image sums (forward: the input; backward: the visible output gradient) are f64, in two fixed-order stages:
// block p of the sum kernel adds elements [4096 p, 4096 (p + 1)) of the image -- the partition depends on S alone --
// thread by thread, then by the xor butterfly of the wave, then over the four waves in index order, and stores ONE f64;
// the main kernel adds the partials of its image in index order.  No atomics; two calls give the same bits.
//
// The gated entry points (sba_diffaug_gated_fwd / _bwd in sbagan_hip_ext.h) are the SAME kernels with
// per-image flags: every block resolves its image's flags once (da_image_flags) and branches on them block-uniformly.
// An image whose color bit is off leaves the sum kernel before any load; with all bits off the main kernel is a copy.
#include "common.h"
#include "sbagan_hip_ext.h"

namespace {

constexpr int DA_THREADS = 256;
constexpr int DA_ITERS = 4;                                 // 16-byte loads per thread of the sum kernel
constexpr int DA_CHUNK4 = DA_THREADS * DA_ITERS;            // float4 per partial sum: 4096 elements
constexpr int DA_MAX_S = 4096;                              // 3 S^2 stays far inside int32
constexpr float DA_THIRD = 1.f / 3.f;

// integer maps of one parameter row: translation (ty, tx) and the cut rectangle [cy0, cy1) x [cx0, cx1) in OUTPUT
// coordinates, already intersected with the image.  The paper masks a clamped index grid; for cut >= 2 (S >= 8 here,
// cut = S / 2) the clamped indices are exactly the rows and columns of this intersection: the rectangle always overlaps
// the image, and an index clamped to 0 or S - 1 lands on a row the intersection holds already.
struct DaMaps {
    int ty, tx, cy0, cy1, cx0, cx1;
};

__device__ __forceinline__ int da_draw(float u, int n) {    // min(int(u * n), n - 1): u * n in f32 can round up to n
    const int v = (int)(u * (float)n);
    return v < n - 1 ? v : n - 1;
}

__device__ __forceinline__ DaMaps da_maps(const float* __restrict__ p, int S, int flags, int shift, int cut) {
    DaMaps m = {0, 0, 0, 0, 0, 0};
    if (flags & 2) {
        m.ty = da_draw(p[3], 2 * shift + 1) - shift;
        m.tx = da_draw(p[4], 2 * shift + 1) - shift;
    }
    if (flags & 4) {
        const int odd = cut & 1;
        const int oy = da_draw(p[5], S + 1 - odd) - cut / 2, ox = da_draw(p[6], S + 1 - odd) - cut / 2;
        m.cy0 = max(oy, 0), m.cy1 = min(oy + cut, S);
        m.cx0 = max(ox, 0), m.cx1 = min(ox + cut, S);
    }
    return m;
}

// Is output pixel (i, j) fed by a source pixel: its source (i + ty, j + tx) inside the image, and (i, j) not cut
__device__ __forceinline__ bool da_live(const DaMaps& m, int S, int i, int j) {
    const int si = i + m.ty, sj = j + m.tx;
    const bool in = (unsigned)si < (unsigned)S && (unsigned)sj < (unsigned)S;
    const bool cut = i >= m.cy0 && i < m.cy1 && j >= m.cx0 && j < m.cx1;
    return in && !cut;
}

// The flags of image n, once per block.  gates == nullptr && applied == nullptr: the ungated entry points, `flags` as
// given.  applied: the backward of a gated forward, what that forward recorded (masked: never an address).  gates: bit b
// is on iff gates[n][b] < *p_dev -- false for every gate when p is NaN or 0, true for every gate in [0, 1) when p >= 1.
struct DaGate {
    const float* gates;
    const float* p_dev;
    const int32_t* applied;
};

__device__ __forceinline__ int da_image_flags(int flags, const DaGate& g, int n) {
    if (g.applied) return flags & g.applied[n];
    if (!g.gates) return flags;
    const float p = *g.p_dev;
    const float* row = g.gates + (size_t)n * 4;
    const int on = (row[0] < p ? 1 : 0) | (row[1] < p ? 2 : 0) | (row[2] < p ? 4 : 0);
    return flags & on;
}

__device__ __forceinline__ const float* da_image(const float* a, int na, const float* b, int n, size_t img) {
    return n < na ? a + (size_t)n * img : b + (size_t)(n - na) * img;
}

// stage 1 of the per-image sum.  BWD: only the elements of dout that reach an input (da_live) count.
template <bool BWD>
__global__ __launch_bounds__(DA_THREADS) void diffaug_sum_kernel(
    const float* __restrict__ a, int na, const float* __restrict__ b, const float* __restrict__ params,
    double* __restrict__ partials, int S, int flags, int shift, int cut, int P, DaGate gate) {
    const int n = blockIdx.y, p = blockIdx.x;
    flags = da_image_flags(flags, gate, n);
    if (!(flags & 1)) return;               // no color on this image: nobody reads its partials
    const int plane = S * S, total4 = 3 * plane / 4;
    const float* img = da_image(a, na, b, n, (size_t)3 * plane);
    DaMaps m = {0, 0, 0, 0, 0, 0};
    if (BWD) m = da_maps(params + (size_t)n * 8, S, flags, shift, cut);
    double acc = 0.0;
#pragma unroll
    for (int it = 0; it < DA_ITERS; ++it) {
        const int i4 = p * DA_CHUNK4 + it * DA_THREADS + threadIdx.x;
        if (i4 < total4) {
            const float4 v = *reinterpret_cast<const float4*>(img + (size_t)i4 * 4);
            float e[4] = {v.x, v.y, v.z, v.w};
            if (BWD) {
                const int rem = (i4 * 4) % plane;
                int i = rem / S, j = rem - i * S;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (!da_live(m, S, i, j)) e[q] = 0.f;
                    if (++j == S) {
                        j = 0;
                        if (++i == S) i = 0;
                    }
                }
            }
            acc += (((double)e[0] + (double)e[1]) + (double)e[2]) + (double)e[3];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    __shared__ double sh[DA_THREADS / 64];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[(size_t)n * P + p] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// Forward: out[w] = color(in[w + t]) where da_live, else +0.  Backward: dx[w] = color'(G[w]) with G[w] = dout[w - t] where
// that output pixel is live, else 0.  Both gather four pixels at a shifted position, so they share the body.
template <bool BWD>
__global__ __launch_bounds__(DA_THREADS) void diffaug_main_kernel(
    const float* __restrict__ a, int na, const float* __restrict__ b, const float* __restrict__ params,
    float* __restrict__ out, int S, int flags, int shift, int cut, const double* __restrict__ partials, int P,
    DaGate gate, int32_t* __restrict__ applied_out) {
    const int n = blockIdx.y;
    const int plane = S * S;
    flags = da_image_flags(flags, gate, n);
    if (applied_out && blockIdx.x == 0 && threadIdx.x == 0) applied_out[n] = flags;
    const bool color = flags & 1;
    __shared__ float sh_mean;
    if (color) {
        if (threadIdx.x == 0) {
            double acc = 0.0;
            for (int p = 0; p < P; ++p) acc += partials[(size_t)n * P + p];      // stage 2: index order
            sh_mean = (float)(acc / (double)(3 * plane));
        }
        __syncthreads();
    }
    const int g = blockIdx.x * DA_THREADS + threadIdx.x;
    if (g * 4 >= plane) return;
    const float* prm = params + (size_t)n * 8;
    const DaMaps m = da_maps(prm, S, flags, shift, cut);
    const float* src = da_image(a, na, b, n, (size_t)3 * plane);
    float* dst = out + (size_t)n * 3 * plane + (size_t)g * 4;

    // the four pixels of this thread: where each reads from, and whether it reads at all
    const int dy = BWD ? -m.ty : m.ty, dx = BWD ? -m.tx : m.tx;
    int i = (g * 4) / S, j = g * 4 - i * S;
    const bool one_row = j + 3 < S;
    int off[4];
    unsigned live = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ri = i + dy, rj = j + dx;
        // da_live takes OUTPUT coordinates: the written pixel in the forward, the pixel read in the backward
        const bool ok = BWD ? ((unsigned)ri < (unsigned)S && (unsigned)rj < (unsigned)S && da_live(m, S, ri, rj))
                            : da_live(m, S, i, j);
        off[q] = ri * S + rj;
        if (ok) live |= 1u << q;
        if (++j == S) {
            j = 0;
            ++i;
        }
    }
    float x[3][4];
    if (live == 0xFu && one_row) {          // interior: one 16-byte load per channel, aligned to 4 bytes only
#pragma unroll
        for (int c = 0; c < 3; ++c) __builtin_memcpy(x[c], src + (size_t)c * plane + off[0], 16);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) x[c][q] = (live >> q & 1u) ? src[(size_t)c * plane + off[q]] : 0.f;
    }
    if (color) {
        const float s = 2.f * prm[1], k = prm[2] + 0.5f;
        if (!BWD) {
            const float bri = prm[0] - 0.5f;
            const float M = sh_mean + bri;      // saturation keeps the pixel's channel mean: mean_chw after it = this
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float x0 = x[0][q] + bri, x1 = x[1][q] + bri, x2 = x[2][q] + bri;
                const float mc = ((x0 + x1) + x2) * DA_THIRD;
                const float v[3] = {x0, x1, x2};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float sat = (v[c] - mc) * s + mc;
                    x[c][q] = (live >> q & 1u) ? (sat - M) * k + M : 0.f;
                }
            }
        } else {
            const float tail = (1.f - k) * sh_mean;             // goes to EVERY input element
            const float oms = 1.f - s;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float mg = ((x[0][q] + x[1][q]) + x[2][q]) * DA_THIRD;
#pragma unroll
                for (int c = 0; c < 3; ++c) x[c][q] = k * (s * x[c][q] + oms * mg) + tail;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(dst + (size_t)c * plane) = make_float4(x[c][0], x[c][1], x[c][2], x[c][3]);
}

inline bool da_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

inline int da_parts(int S) { return cdiv((int64_t)3 * S * S / 4, DA_CHUNK4); }

// the checks both entry points share; n = number of images written
int da_check(int n, int S, int flags, const void* params, const void* out, const void* workspace) {
    if (S < 8 || (S & 1) || S > DA_MAX_S || flags < 1 || flags > 7 || n < 1 || n > 65535) return SBA_E_ARG;
    if (!params || !out || da_misaligned(out)) return SBA_E_ARG;
    if ((flags & 1) && (!workspace || ((uintptr_t)workspace & 7))) return SBA_E_ARG;
    return SBA_OK;
}

template <bool BWD>
int da_launch(const float* a, int na, const float* b, int n, const float* params, float* out, int S, int flags,
              void* workspace, hipStream_t st, DaGate gate = {nullptr, nullptr, nullptr}, int32_t* applied_out = nullptr) {
    const int shift = (int)(S * 0.125 + 0.5), cut = (int)(S * 0.5 + 0.5);
    const int P = da_parts(S);
    double* partials = (double*)workspace;
    if (flags & 1) {
        SBA_LAUNCH((diffaug_sum_kernel<BWD>), dim3(P, n), dim3(DA_THREADS), 0, st, a, na, b, params, partials, S, flags,
                   shift, cut, P, gate);
        if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    }
    SBA_LAUNCH((diffaug_main_kernel<BWD>), dim3(cdiv(S * S / 4, DA_THREADS), n), dim3(DA_THREADS), 0, st, a, na, b,
               params, out, S, flags, shift, cut, partials, P, gate, applied_out);
    return SBA_CHECK_LAUNCH();
}

}  // namespace

extern "C" int64_t sba_diffaug_workspace_bytes(int n, int S) {
    if (n < 1 || n > 65535 || S < 8 || (S & 1) || S > DA_MAX_S) return 0;
    return (int64_t)n * da_parts(S) * (int64_t)sizeof(double);
}

extern "C" int sba_diffaug_fwd(const float* real, int nr, const float* fake, int nf, const float* params, float* out,
                               int S, int flags, void* workspace, void* stream) {
    if (nr < 0 || nf < 0 || nr > 65535 || nf > 65535) return SBA_E_ARG;
    if (da_check(nr + nf, S, flags, params, out, workspace) != SBA_OK) return SBA_E_ARG;
    if ((nr > 0 && (!real || da_misaligned(real))) || (nf > 0 && (!fake || da_misaligned(fake)))) return SBA_E_ARG;
    return da_launch<false>(real, nr, fake, nr + nf, params, out, S, flags, workspace, (hipStream_t)stream);
}

extern "C" int sba_diffaug_bwd(const float* dout, int n, const float* params, float* dx, int S, int flags,
                               void* workspace, void* stream) {
    if (da_check(n, S, flags, params, dx, workspace) != SBA_OK) return SBA_E_ARG;
    if (!dout || da_misaligned(dout)) return SBA_E_ARG;
    return da_launch<true>(dout, n, nullptr, n, params, dx, S, flags, workspace, (hipStream_t)stream);
}

static inline bool da_bad_word(const void* p) { return !p || ((uintptr_t)p & 3) != 0; }

extern "C" int sba_diffaug_gated_fwd(const float* real, int nr, const float* fake, int nf, const float* params,
                                     const float* gates, const float* p_dev, float* out, int32_t* applied, int S,
                                     int flags, void* workspace, void* stream) {
    if (nr < 0 || nf < 0 || nr > 65535 || nf > 65535) return SBA_E_ARG;
    if (da_check(nr + nf, S, flags, params, out, workspace) != SBA_OK) return SBA_E_ARG;
    if ((nr > 0 && (!real || da_misaligned(real))) || (nf > 0 && (!fake || da_misaligned(fake)))) return SBA_E_ARG;
    if (da_bad_word(gates) || da_bad_word(p_dev) || da_bad_word(applied)) return SBA_E_ARG;
    return da_launch<false>(real, nr, fake, nr + nf, params, out, S, flags, workspace, (hipStream_t)stream,
                            DaGate{gates, p_dev, nullptr}, applied);
}

extern "C" int sba_diffaug_gated_bwd(const float* dout, int n, const float* params, const int32_t* applied, float* dx,
                                     int S, int flags, void* workspace, void* stream) {
    if (da_check(n, S, flags, params, dx, workspace) != SBA_OK) return SBA_E_ARG;
    if (!dout || da_misaligned(dout) || da_bad_word(applied)) return SBA_E_ARG;
    return da_launch<true>(dout, n, nullptr, n, params, dx, S, flags, workspace, (hipStream_t)stream,
                           DaGate{nullptr, nullptr, applied}, nullptr);
}
