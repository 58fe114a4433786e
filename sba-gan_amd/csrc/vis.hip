// Attention-map overlays (sba_vis_expand, sba_vis_compose in sbagan_hip.h; sbagan/visualize.py).
//
// expand:  out[n] = M x'[n] M^T for every map of a dump in ONE launch, M [V][a] = (Gaussian sigma 20) o (bilinear resize)
//          built on the host in float64, x' = x or x * (x > thresh[n]); plus per-map min / max of the result and
//          conf[n] = sum of the x[n] above 2 thresh[n].  One workgroup per map, no workspace, no atomics, fixed order.
// compose: the finished uint8 HWC canvas (everything but the caption text) in one launch, one thread per pixel.
#include "common.h"

namespace {

constexpr int VE_THREADS = 256;
constexpr int VE_WAVES = VE_THREADS / 64;
constexpr int VE_R = 32;          // output rows per pass of a workgroup
constexpr int VE_RA = 8;          // rows per work item of the first product
constexpr int VE_RB = 16;         // rows per work item of the second product
constexpr int VE_AMAX = 128;      // largest map side: both LDS tiles are VE_R x VE_AMAX f32 = 16 KiB each

// LDS plan at a = 128, V = 256 (the largest case: the third generator stage's 128 x 128 maps at 256 px).  x (64 KiB), T = M x
// (128 KiB) and the output (256 KiB) of ONE map do not fit the 64 KiB a workgroup may declare, and all of x is needed for
// every row of T.  So a workgroup walks the output in bands of VE_R = 32 rows and keeps only the band's operands in LDS:
//     mt [a][VE_R]   the band's rows of M, transposed (a work item reads its 8 row weights of one i as two 16-byte reads)
//     tt [VE_R][aP]  the band of T = M x' (aP = a rounded up to 4: rows are read 16 bytes at a time, all lanes one address)
// = 32 KiB, all the LDS the kernel declares (the final per-map reduction reuses tt): five workgroups fit a CU's 160 KiB.
// x' is read from global memory (coalesced over its columns; a map is read once per band and stays in L2), and in the
// second product every thread reads ITS OWN row of M (16 contiguous bytes per step), so M needs no transposed copy.
// Every output element is one sequential f32 FMA chain over i, then one over j.
__global__ __launch_bounds__(VE_THREADS) void vis_expand_kernel(
    const float* __restrict__ x, const float* __restrict__ thresh, const float* __restrict__ M, float* __restrict__ out,
    float* __restrict__ mn, float* __restrict__ mx, float* __restrict__ conf, int a, int V) {
    __shared__ __attribute__((aligned(16))) float mt[VE_AMAX * VE_R];
    __shared__ __attribute__((aligned(16))) float tt[VE_R * VE_AMAX];
    const int n = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* xn = x + (size_t)n * a * a;
    float* on = out + (size_t)n * V * V;
    const float th = thresh ? thresh[n] : -INFINITY, th2 = 2.f * th;
    const int aP = (a + 3) & ~3;

    float csum = 0.f, lo = INFINITY, hi = -INFINITY;
    for (int e = t; e < a * a; e += VE_THREADS) {
        const float v = xn[e];
        csum += v > th2 ? v : 0.f;
    }

    if (!M) {                                   // V == a: the map itself (masked)
        for (int e = t; e < a * a; e += VE_THREADS) {
            float v = xn[e];
            v = v > th ? v : 0.f;
            on[e] = v;
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    } else {
        const bool vec = (a & 3) == 0;
        for (int r0 = 0; r0 < V; r0 += VE_R) {
            __syncthreads();                    // the previous band's tt reads are done
            for (int e = t; e < a * VE_R; e += VE_THREADS) {
                const int i = e / VE_R, rr = e % VE_R;
                mt[e] = r0 + rr < V ? M[(size_t)(r0 + rr) * a + i] : 0.f;
            }
            for (int e = t; e < VE_R * (aP - a); e += VE_THREADS) {       // zero the padding columns of tt
                const int rr = e / (aP - a), j = a + e % (aP - a);
                tt[rr * aP + j] = 0.f;
            }
            __syncthreads();
            // T[rr][j] = sum_i M[r0 + rr][i] x'[i][j]: item = (j, group of VE_RA rows)
            for (int it = t; it < a * (VE_R / VE_RA); it += VE_THREADS) {
                const int j = it % a, rg = it / a;
                float acc[VE_RA];
#pragma unroll
                for (int k = 0; k < VE_RA; ++k) acc[k] = 0.f;
                for (int i = 0; i < a; ++i) {
                    float v = xn[(size_t)i * a + j];
                    v = v > th ? v : 0.f;
                    const float4 m0 = *reinterpret_cast<const float4*>(&mt[i * VE_R + rg * VE_RA]);
                    const float4 m1 = *reinterpret_cast<const float4*>(&mt[i * VE_R + rg * VE_RA + 4]);
                    acc[0] = fmaf(m0.x, v, acc[0]); acc[1] = fmaf(m0.y, v, acc[1]);
                    acc[2] = fmaf(m0.z, v, acc[2]); acc[3] = fmaf(m0.w, v, acc[3]);
                    acc[4] = fmaf(m1.x, v, acc[4]); acc[5] = fmaf(m1.y, v, acc[5]);
                    acc[6] = fmaf(m1.z, v, acc[6]); acc[7] = fmaf(m1.w, v, acc[7]);
                }
#pragma unroll
                for (int k = 0; k < VE_RA; ++k) tt[(rg * VE_RA + k) * aP + j] = acc[k];
            }
            __syncthreads();
            // out[r0 + rr][o] = sum_j T[rr][j] M[o][j]: item = (o, group of VE_RB rows)
            for (int it = t; it < V * (VE_R / VE_RB); it += VE_THREADS) {
                const int o = it % V, rg = it / V;
                const float* mo = M + (size_t)o * a;
                float acc[VE_RB];
#pragma unroll
                for (int k = 0; k < VE_RB; ++k) acc[k] = 0.f;
                for (int j = 0; j < aP; j += 4) {
                    float4 m;
                    if (vec) {
                        m = *reinterpret_cast<const float4*>(mo + j);
                    } else {
                        m.x = mo[j];
                        m.y = j + 1 < a ? mo[j + 1] : 0.f;
                        m.z = j + 2 < a ? mo[j + 2] : 0.f;
                        m.w = j + 3 < a ? mo[j + 3] : 0.f;
                    }
#pragma unroll
                    for (int k = 0; k < VE_RB; ++k) {
                        const float4 tv = *reinterpret_cast<const float4*>(&tt[(rg * VE_RB + k) * aP + j]);
                        acc[k] = fmaf(tv.x, m.x, acc[k]);
                        acc[k] = fmaf(tv.y, m.y, acc[k]);
                        acc[k] = fmaf(tv.z, m.z, acc[k]);
                        acc[k] = fmaf(tv.w, m.w, acc[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < VE_RB; ++k) {
                    const int r = r0 + rg * VE_RB + k;
                    if (r < V) {
                        on[(size_t)r * V + o] = acc[k];
                        lo = fminf(lo, acc[k]);
                        hi = fmaxf(hi, acc[k]);
                    }
                }
            }
        }
    }
    // per-map reductions: lanes by xor shuffles, then the waves in wave order
    csum = wave_sum(csum);
    lo = -wave_max(-lo);
    hi = wave_max(hi);
    __syncthreads();                            // the last band's tt reads are done: its first 3 VE_WAVES floats are reused
    float* red = tt;
    if (lane == 0) {
        red[wave] = csum;
        red[VE_WAVES + wave] = lo;
        red[2 * VE_WAVES + wave] = hi;
    }
    __syncthreads();
    if (t == 0) {
        float c = 0.f, l = INFINITY, h = -INFINITY;
        for (int w = 0; w < VE_WAVES; ++w) {
            c += red[w];
            l = fminf(l, red[VE_WAVES + w]);
            h = fmaxf(h, red[2 * VE_WAVES + w]);
        }
        conf[n] = c;
        mn[n] = l;
        mx[n] = h;
    }
}

// ---------------------------------------------------------------------------------------------------------------
struct VisImgs {
    const float* p[2];      // two image batches [count][3][S][S] f32 in [-1, 1]
    int count[2], S[2];
};

// align_corners bilinear sample of channel plane `pl` [S][S] at output pixel (ty, tx) of a V x V tile, then the uint8 of
// (v + 1) 127.5.  The source position ty (S - 1) / (V - 1) is split into its integer part and remainder exactly.
__device__ __forceinline__ int vis_img_u8(const float* __restrict__ pl, int S, int V, int ty, int tx) {
    float v;
    if (S == V) {
        v = pl[(size_t)ty * S + tx];
    } else {
        const int d = V - 1 > 0 ? V - 1 : 1;
        const int py = ty * (S - 1), px = tx * (S - 1);
        const int y0 = py / d, x0 = px / d;
        const float fy = (float)(py - y0 * d) / (float)d, fx = (float)(px - x0 * d) / (float)d;
        const int y1 = min(y0 + 1, S - 1), x1 = min(x0 + 1, S - 1);
        const float v00 = pl[(size_t)y0 * S + x0], v01 = pl[(size_t)y0 * S + x1];
        const float v10 = pl[(size_t)y1 * S + x0], v11 = pl[(size_t)y1 * S + x1];
        const float top = v00 + (v01 - v00) * fx, bot = v10 + (v11 - v10) * fx;
        v = top + (bot - top) * fy;
    }
    v = (v + 1.f) * 127.5f;
    v = fminf(fmaxf(v, 0.f), 255.f);
    return (int)v;
}

// The canvas is nS blocks stacked vertically, each a band of `band` rows over nr rows of V x V tiles; horizontally nc
// cells of V + 2 columns (tile + 2 black columns; the band's colour fills the whole cell).  Cell (s, r, c):
//   desc = {kind, image, map, m}: kind 0 black, 1 image tile, 2 map tile, 3 map blended over the image with mask m;
//          image = batch * 65536 + index;   par = {lo, den}: map byte = trunc(clamp(255 (e - lo) / den)), 0 when den <= 0.
__global__ __launch_bounds__(256) void vis_compose_kernel(
    uint8_t* __restrict__ canvas, int W, int H, int V, int band, int nr, int nc, const int32_t* __restrict__ desc,
    const float* __restrict__ par, const uint32_t* __restrict__ band_rgb, const float* __restrict__ E, int nE,
    VisImgs im) {
    const int xpix = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (xpix >= W || y >= H) return;
    const int Hs = band + nr * V;
    const int s = y / Hs, yy = y % Hs, c = xpix / (V + 2), tx = xpix % (V + 2);
    int r = 0, g = 0, b = 0;
    if (yy < band) {
        const uint32_t col = band_rgb[s * nc + c];
        r = col & 255; g = (col >> 8) & 255; b = (col >> 16) & 255;
    } else if (tx < V) {
        const int tr = (yy - band) / V, ty = (yy - band) % V;
        const size_t cell = ((size_t)s * nr + tr) * nc + c;
        const int kind = desc[cell * 4], isel = desc[cell * 4 + 1], mi = desc[cell * 4 + 2], m = desc[cell * 4 + 3];
        int mapv = 0;
        bool ok = kind >= 1 && kind <= 3;
        if (ok && kind >= 2) {
            ok = mi >= 0 && mi < nE;
            if (ok) {
                const float lo = par[cell * 2], den = par[cell * 2 + 1];
                if (den > 0.f) {
                    float v = 255.f * (E[((size_t)mi * V + ty) * V + tx] - lo) / den;
                    v = fminf(fmaxf(v, 0.f), 255.f);
                    mapv = (int)v;
                }
            }
        }
        int iv[3] = {0, 0, 0};
        if (ok && kind != 2) {
            const int which = isel >> 16, idx = isel & 65535;
            ok = (which == 0 || which == 1) && im.p[which] && idx < im.count[which];
            if (ok) {
                const int S = im.S[which];
                const float* base = im.p[which] + (size_t)idx * 3 * S * S;
                for (int ch = 0; ch < 3; ++ch) iv[ch] = vis_img_u8(base + (size_t)ch * S * S, S, V, ty, tx);
            }
        }
        if (ok) {
            if (kind == 1) {
                r = iv[0]; g = iv[1]; b = iv[2];
            } else if (kind == 2) {
                r = g = b = mapv;
            } else {
                // the 8-bit paste with a constant mask: t = map m + img (255 - m) + 128; ((t >> 8) + t) >> 8
                int o[3];
                for (int ch = 0; ch < 3; ++ch) {
                    const int tq = mapv * m + iv[ch] * (255 - m) + 128;
                    o[ch] = ((tq >> 8) + tq) >> 8;
                }
                r = o[0]; g = o[1]; b = o[2];
            }
        }
    }
    uint8_t* px = canvas + ((size_t)y * W + xpix) * 3;
    px[0] = (uint8_t)r; px[1] = (uint8_t)g; px[2] = (uint8_t)b;
}

}  // namespace

extern "C" int sba_vis_expand(const float* x, const float* thresh, const float* M, float* out, float* mn, float* mx,
                              float* conf, int n, int a, int V, void* stream) {
    if (!x || !out || !mn || !mx || !conf) return SBA_E_ARG;
    if (n < 1 || n > 65535 || a < 1 || a > VE_AMAX || V < a || V > 1024) return SBA_E_ARG;
    if (!M && V != a) return SBA_E_ARG;
    if (M && ((uintptr_t)M & 15)) return SBA_E_ARG;
    SBA_LAUNCH(vis_expand_kernel, dim3(n), dim3(VE_THREADS), 0, (hipStream_t)stream, x, thresh, M, out, mn, mx, conf, a,
               V);
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_vis_compose(uint8_t* canvas, int W, int H, int V, int band, int nS, int nr, int nc,
                               const int32_t* desc, const float* par, const uint32_t* band_rgb, const float* E, int nE,
                               const float* img0, int n0, int S0, const float* img1, int n1, int S1, void* stream) {
    if (!canvas || !desc || !par || !band_rgb) return SBA_E_ARG;
    if (V < 1 || V > 1024 || band < 0 || band > 4096 || nS < 1 || nS > 64 || nr < 1 || nr > 8 || nc < 1 || nc > 64)
        return SBA_E_ARG;
    if (W != nc * (V + 2) || H != nS * (band + nr * V) || H > 65535) return SBA_E_ARG;
    if (nE < 0 || (nE > 0 && !E) || n0 < 0 || n1 < 0 || n0 > 65535 || n1 > 65535) return SBA_E_ARG;
    if ((n0 > 0 && (!img0 || S0 < 1 || S0 > 4096)) || (n1 > 0 && (!img1 || S1 < 1 || S1 > 4096))) return SBA_E_ARG;
    VisImgs im;
    im.p[0] = n0 > 0 ? img0 : nullptr; im.p[1] = n1 > 0 ? img1 : nullptr;
    im.count[0] = n0; im.count[1] = n1;
    im.S[0] = n0 > 0 ? S0 : 1; im.S[1] = n1 > 0 ? S1 : 1;
    SBA_LAUNCH(vis_compose_kernel, dim3(cdiv(W, 256), H), dim3(256), 0, (hipStream_t)stream, canvas, W, H, V, band, nr,
               nc, desc, par, band_rgb, E, nE, im);
    return SBA_CHECK_LAUNCH();
}
