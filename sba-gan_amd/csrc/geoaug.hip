// Geometric augmentation (the x-flip, 90-degree rotation, isotropic scaling and rotation of Karras et al., NeurIPS 2020,
// "Training GANs with Limited Data") of the image batch a discriminator sees: sba_geoaug_prepare / _fwd / _bwd in
// sbagan_hip_ext.h; sbagan/ops.py: GeoAugFn; sbagan/geoaug.py; DESIGN.md 7q.
//
// The four parts of one image compose into ONE 2 x 2 matrix M about the image centre c = (S - 1) / 2: output pixel d
// samples the input at src = c + M (d - c), bilinearly, a tap outside the image contributing zero.  sba_geoaug_prepare
// turns a row of uniforms into M (the only transcendentals of the unit; one thread per row, one launch per step); the
// warp kernels read M and have none.
//
// Forward: one thread owns four consecutive output pixels in all three channels -- 16 tap addresses, 48 cached gathers,
// three aligned 16-byte stores.  Backward: the exact adjoint in GATHER form, no atomics, no workspace: one thread owns
// four consecutive INPUT pixels; for each it visits, in row-major order, the output pixels of the bounding box of
// M^-1 ([qx - 1, qx + 1] x [qy - 1, qy + 1]) (at most GEO_WIN candidates per axis) and adds dout * weight in f32 in that
// fixed order: two calls give the same bits.  Whether a candidate counts is decided by the weight itself (geo_weight,
// built on geo_src and geo_taps, the functions the forward takes its sampling position, taps and fractions from -- an
// output pixel has a weight for exactly the pixels the forward reads for it): a candidate on the edge of the box has
// weight 0, so the rounding of the box cannot move the sum by more than the weight's own rounding.
//
// With flip and rot90 alone the arithmetic is exact for even S: d - c and c are half-integers, M holds 0 and +-1, every
// fraction is exactly 0 -- the output is a permutation of the input, bit for bit.  A block whose image has the
// identity matrix copies.
#include "common.h"
#include "sbagan_hip_ext.h"

namespace {

constexpr int GEO_THREADS = 256;
constexpr int GEO_MAX_S = 4096;                             // 3 S^2 stays far inside int32
constexpr int GEO_WIN = 7;                                  // candidates per axis: s sqrt(2) <= 2.144 each way, + the pad

struct GeoMat {
    float m00, m01, m10, m11;
};

__device__ __forceinline__ GeoMat geo_load(const float* __restrict__ mats, int n) {
    const float4 v = *reinterpret_cast<const float4*>(mats + (size_t)n * 4);
    return GeoMat{v.x, v.y, v.z, v.w};
}

__device__ __forceinline__ bool geo_identity(const GeoMat& m) {
    return m.m00 == 1.f && m.m01 == 0.f && m.m10 == 0.f && m.m11 == 1.f;
}

// where output pixel (dx, dy) samples the input; shared by the forward and the backward
__device__ __forceinline__ void geo_src(const GeoMat& m, float c, int dx, int dy, float& sx, float& sy) {
    const float ax = (float)dx - c, ay = (float)dy - c;
    sx = (m.m00 * ax + m.m01 * ay) + c;
    sy = (m.m10 * ax + m.m11 * ay) + c;
}

// One axis of a sampling position: the two taps i0 = floor(s), i0 + 1 and the fraction f = s - i0 (exact in f32), i.e.
// hat(s - i0) = 1 - f and hat(s - (i0 + 1)) = f.  False -- no tap on this axis is inside the image -- for a position
// outside (-1, S) and for a NaN, which fails both comparisons.  Forward AND backward read their taps from here.
__device__ __forceinline__ bool geo_taps(float s, int S, int& i0, float& f) {
    const float fl = floorf(s);
    if (!(fl >= -1.f && fl <= (float)(S - 1))) return false;
    i0 = (int)fl;
    f = s - fl;
    return true;
}

// the hat weight of pixel q on one axis, given that axis's taps: 1 - f, f, or 0 for a pixel that is no tap
__device__ __forceinline__ float geo_axis_weight(int i0, float f, int q) {
    return q == i0 ? 1.f - f : (q == i0 + 1 ? f : 0.f);
}

// the weight of input pixel (qx, qy) in output pixel (dx, dy): hat(sx - qx) hat(sy - qy)
__device__ __forceinline__ float geo_weight(const GeoMat& m, float c, int S, int dx, int dy, int qx, int qy) {
    float sx, sy, fx, fy;
    int x0, y0;
    geo_src(m, c, dx, dy, sx, sy);
    if (!geo_taps(sx, S, x0, fx) || !geo_taps(sy, S, y0, fy)) return 0.f;
    return geo_axis_weight(x0, fx, qx) * geo_axis_weight(y0, fy, qy);
}

__device__ __forceinline__ const float* geo_image(const float* a, int na, const float* b, int n, size_t img) {
    return n < na ? a + (size_t)n * img : b + (size_t)(n - na) * img;
}

// One thread per row.  M = F . Q^k . R(theta) / s with every part that is off contributing the identity.
__global__ __launch_bounds__(GEO_THREADS) void geoaug_prepare_kernel(
    const float* __restrict__ uniforms, const float* __restrict__ gates, const float* __restrict__ p_dev,
    int rows_per_p, int N, int flags, float* __restrict__ mats, int32_t* __restrict__ applied) {
    const int r = blockIdx.x * GEO_THREADS + threadIdx.x;
    if (r >= N) return;
    int on = flags;
    if (gates) {                // bit b iff gates[r][b] < p: false for every gate when p is NaN or 0, true when p >= 1
        const float p = p_dev[r / rows_per_p];
        const float* g = gates + (size_t)r * 4;
        on &= (g[0] < p ? 1 : 0) | (g[1] < p ? 2 : 0) | (g[2] < p ? 4 : 0) | (g[3] < p ? 8 : 0);
    }
    const float* u = uniforms + (size_t)r * 8;
    float a00 = 1.f, a01 = 0.f, a10 = 0.f, a11 = 1.f;
    if (on & 8) {               // R(theta), theta = pi (2 u4 - 1): the argument in half-turns is exact
        const float t = 2.f * u[4] - 1.f;
        const float c = cospif(t), s = sinpif(t);
        a00 = c, a01 = -s, a10 = s, a11 = c;
    }
    if (on & 2) {               // Q A = [[-a10, -a11], [a00, a01]], k times
        const int k4 = (int)(4.f * u[1]);
        const int k = k4 < 3 ? k4 : 3;
        for (int i = 0; i < k; ++i) {
            const float b00 = -a10, b01 = -a11, b10 = a00, b11 = a01;
            a00 = b00, a01 = b01, a10 = b10, a11 = b11;
        }
    }
    if ((on & 1) && u[0] >= 0.5f) a00 = -a00, a01 = -a01;       // F A: the first row negated
    if (on & 4) {               // 1 / s = 2^(-0.2 z), z a standard normal (Box-Muller) clamped to [-3, 3]
        float z = sqrtf(-2.f * logf(1.f - u[2])) * cospif(2.f * u[3]);
        z = fminf(fmaxf(z, -3.f), 3.f);
        const float inv_s = exp2f(-0.2f * z);
        a00 *= inv_s, a01 *= inv_s, a10 *= inv_s, a11 *= inv_s;
    }
    *reinterpret_cast<float4*>(mats + (size_t)r * 4) = make_float4(a00, a01, a10, a11);
    applied[r] = on;
}

__global__ __launch_bounds__(GEO_THREADS) void geoaug_fwd_kernel(
    const float* __restrict__ a, int na, const float* __restrict__ b, const float* __restrict__ mats,
    float* __restrict__ out, int S) {
    const int n = blockIdx.y;
    const int plane = S * S;
    const int g = blockIdx.x * GEO_THREADS + threadIdx.x;
    if (g * 4 >= plane) return;
    const GeoMat m = geo_load(mats, n);
    const float* src = geo_image(a, na, b, n, (size_t)3 * plane);
    float* dst = out + (size_t)n * 3 * plane + (size_t)g * 4;
    if (geo_identity(m)) {      // block-uniform: a copy
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<float4*>(dst + (size_t)c * plane) =
                *reinterpret_cast<const float4*>(src + (size_t)c * plane + (size_t)g * 4);
        return;
    }
    const float c0 = 0.5f * (float)(S - 1);
    int dy = (g * 4) / S, dx = g * 4 - dy * S;
    float y[3][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float sx, sy, fx, fy;
        int x0, y0;
        geo_src(m, c0, dx, dy, sx, sy);
        float acc[3] = {0.f, 0.f, 0.f};
        if (geo_taps(sx, S, x0, fx) && geo_taps(sy, S, y0, fy)) {
            // the four taps, zero outside the image, combined as two lerps along x and one along y: the weights are
            // (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy -- those of geo_weight --, a constant neighbourhood comes
            // back as it is and fx = fy = 0 returns the first tap's bits
            const bool in_x0 = (unsigned)x0 < (unsigned)S, in_x1 = (unsigned)(x0 + 1) < (unsigned)S;
            const bool in_y0 = (unsigned)y0 < (unsigned)S, in_y1 = (unsigned)(y0 + 1) < (unsigned)S;
            const int o00 = y0 * S + x0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* ch = src + (size_t)c * plane;
                const float v00 = in_x0 && in_y0 ? ch[o00] : 0.f, v01 = in_x1 && in_y0 ? ch[o00 + 1] : 0.f;
                const float v10 = in_x0 && in_y1 ? ch[o00 + S] : 0.f, v11 = in_x1 && in_y1 ? ch[o00 + S + 1] : 0.f;
                const float top = v00 + fx * (v01 - v00), bot = v10 + fx * (v11 - v10);
                acc[c] = top + fy * (bot - top);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) y[c][q] = acc[c];
        if (++dx == S) {
            dx = 0;
            ++dy;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(dst + (size_t)c * plane) = make_float4(y[c][0], y[c][1], y[c][2], y[c][3]);
}

// float -> a clamped int bound; a NaN takes `lo` (fmaxf / fminf return the operand that is a number)
__device__ __forceinline__ int geo_bound(float v, int lo, int hi) {
    return (int)fminf(fmaxf(v, (float)lo), (float)hi);
}

__global__ __launch_bounds__(GEO_THREADS) void geoaug_bwd_kernel(
    const float* __restrict__ dout, const float* __restrict__ mats, float* __restrict__ dx_out, int S) {
    const int n = blockIdx.y;
    const int plane = S * S;
    const int g = blockIdx.x * GEO_THREADS + threadIdx.x;
    if (g * 4 >= plane) return;
    const GeoMat m = geo_load(mats, n);
    const float* src = dout + (size_t)n * 3 * plane;
    float* dst = dx_out + (size_t)n * 3 * plane + (size_t)g * 4;
    if (geo_identity(m)) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<float4*>(dst + (size_t)c * plane) =
                *reinterpret_cast<const float4*>(src + (size_t)c * plane + (size_t)g * 4);
        return;
    }
    const float c0 = 0.5f * (float)(S - 1);
    // M^-1 and the half-widths of the box of M^-1 applied to the square of side 2
    const float rdet = 1.f / (m.m00 * m.m11 - m.m01 * m.m10);
    const float i00 = m.m11 * rdet, i01 = -m.m01 * rdet, i10 = -m.m10 * rdet, i11 = m.m00 * rdet;
    const float hx = fabsf(i00) + fabsf(i01), hy = fabsf(i10) + fabsf(i11);
    int qy = (g * 4) / S, qx = g * 4 - qy * S;
    float y[3][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float ax = (float)qx - c0, ay = (float)qy - c0;
        const float ex = (i00 * ax + i01 * ay) + c0, ey = (i10 * ax + i11 * ay) + c0;
        // floor / ceil of the box: its own edge pixels (weight 0) are the pad.  At most GEO_WIN per axis, whatever M holds
        const int x_lo = geo_bound(floorf(ex - hx), 0, S), y_lo = geo_bound(floorf(ey - hy), 0, S);
        const int x_hi = min(geo_bound(ceilf(ex + hx), -1, S - 1), x_lo + GEO_WIN - 1);
        const int y_hi = min(geo_bound(ceilf(ey + hy), -1, S - 1), y_lo + GEO_WIN - 1);
        float acc[3] = {0.f, 0.f, 0.f};
        for (int wy = y_lo; wy <= y_hi; ++wy)
            for (int wx = x_lo; wx <= x_hi; ++wx) {
                const float w = geo_weight(m, c0, S, wx, wy, qx, qy);
                if (w != 0.f) {
                    const float* tap = src + wy * S + wx;
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] += tap[(size_t)c * plane] * w;
                }
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) y[c][q] = acc[c];
        if (++qx == S) {
            qx = 0;
            ++qy;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(dst + (size_t)c * plane) = make_float4(y[c][0], y[c][1], y[c][2], y[c][3]);
}

inline bool geo_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
inline bool geo_bad_word(const void* p) { return !p || ((uintptr_t)p & 3) != 0; }

// the checks the two warp entry points share (those of the diffaug unit); n = number of images written
int geo_check(int n, int S, const void* mats, const void* out) {
    if (S < 8 || (S & 1) || S > GEO_MAX_S || n < 1 || n > 65535) return SBA_E_ARG;
    if (!mats || geo_misaligned(mats) || !out || geo_misaligned(out)) return SBA_E_ARG;
    return SBA_OK;
}

}  // namespace

extern "C" int sba_geoaug_prepare(const float* uniforms, const float* gates, const float* p_dev, int rows_per_p, int N,
                                  int flags, float* mats, int32_t* applied, void* stream) {
    if (N < 1 || N > (1 << 20) || flags < 1 || flags > 15) return SBA_E_ARG;
    if (geo_bad_word(uniforms) || !mats || geo_misaligned(mats) || geo_bad_word(applied)) return SBA_E_ARG;
    if (gates && (((uintptr_t)gates & 3) || geo_bad_word(p_dev) || rows_per_p < 1)) return SBA_E_ARG;
    SBA_LAUNCH(geoaug_prepare_kernel, dim3(cdiv(N, GEO_THREADS)), dim3(GEO_THREADS), 0, (hipStream_t)stream, uniforms,
               gates, p_dev, rows_per_p, N, flags, mats, applied);
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_geoaug_fwd(const float* real, int nr, const float* fake, int nf, const float* mats, float* out, int S,
                              void* stream) {
    if (nr < 0 || nf < 0 || nr > 65535 || nf > 65535) return SBA_E_ARG;
    if (geo_check(nr + nf, S, mats, out) != SBA_OK) return SBA_E_ARG;
    if ((nr > 0 && (!real || geo_misaligned(real))) || (nf > 0 && (!fake || geo_misaligned(fake)))) return SBA_E_ARG;
    SBA_LAUNCH(geoaug_fwd_kernel, dim3(cdiv(S * S / 4, GEO_THREADS), nr + nf), dim3(GEO_THREADS), 0, (hipStream_t)stream,
               real, nr, fake, mats, out, S);
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_geoaug_bwd(const float* dout, int n, const float* mats, float* dx, int S, void* stream) {
    if (geo_check(n, S, mats, dx) != SBA_OK) return SBA_E_ARG;
    if (!dout || geo_misaligned(dout)) return SBA_E_ARG;
    SBA_LAUNCH(geoaug_bwd_kernel, dim3(cdiv(S * S / 4, GEO_THREADS), n), dim3(GEO_THREADS), 0, (hipStream_t)stream, dout,
               mats, dx, S);
    return SBA_CHECK_LAUNCH();
}
