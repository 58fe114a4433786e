// Multi-scale structural similarity of image pairs (sba_msssim_pairs in sbagan_hip.h): per pair, channel and scale the
// mean SSIM and the mean contrast-structure term over the valid positions of the 11-tap Gaussian window, in float64.
//
// The kernel reads the uint8 images at every scale and pools while it stages: a pixel of scale s is the mean of a
// 2^s x 2^s block of the original bytes (dropping the odd tail at every level composes to floor(H / 2^s)), an integer
// over 4^s and exact in f64, so no pyramid is ever stored.  One workgroup takes a 16 x 32 tile of window positions of
// one (pair, channel, scale): it stages the 26 x 42 pooled halo tile of both images in LDS, filters mx, my, E[xx],
// E[yy], E[xy] along the rows into LDS (f64 vector FMAs), then every thread filters two vertically adjacent positions
// down the columns (12 rows read for 2 x 11 taps), forms cs and ssim, and the 256 thread sums are halved in one fixed
// order.  No atomics, no memset, no allocation: one (ssim, cs) partial per workgroup goes to the caller's workspace and
// a second small launch adds the partials of a (pair, channel, scale) in tile order and divides by the count.
#include "common.h"

#include <math.h>

namespace {

constexpr int MS_WIN = 11, MS_HALO = MS_WIN - 1;
constexpr int MS_TR = 16, MS_TC = 32, MS_THREADS = 256;         // window positions per tile: rows x columns
constexpr int MS_IR = MS_TR + MS_HALO, MS_IC = MS_TC + MS_HALO; // pooled pixels staged per tile
constexpr int MS_ROWS_PER_THREAD = MS_TR * MS_TC / MS_THREADS;  // 2
constexpr int MS_MAX_SCALES = 5, MS_MAX_SIDE = 1024, MS_MAX_PAIRS = 1 << 20;
static_assert(MS_ROWS_PER_THREAD == 2 && MS_THREADS / MS_TC * MS_ROWS_PER_THREAD == MS_TR, "the column pass layout");

constexpr int MS_STAGE = (MS_IR * MS_IC + MS_THREADS - 1) / MS_THREADS;     // pooled pixels staged per thread: 5
static_assert(2 * MS_THREADS <= MS_IR * MS_IC, "the thread sums are halved in the staged tile's memory");

struct MsWindow { double g[MS_WIN]; };
struct MsScale { int Hs, Ws, tiles_c, tiles, first; };         // pooled size, tile columns, tiles, first partial slot
struct MsPlan {
    MsScale s[MS_MAX_SCALES];
    int scales, total;                                          // total: partial slots per (pair, channel)
};

// the sum of the K bytes at p (K = 1, 2, or a multiple of 4); p is aligned to nothing
template <int K>
__device__ __forceinline__ int ms_row_sum(const uint8_t* __restrict__ p) {
    if constexpr (K == 1) {
        return p[0];
    } else if constexpr (K == 2) {
        uint16_t v;
        __builtin_memcpy(&v, p, 2);
        return (v & 0xff) + (v >> 8);
    } else {
        unsigned s = 0;
#pragma unroll
        for (int k = 0; k < K; k += 4) {
            uint32_t v;
            __builtin_memcpy(&v, p + k, 4);
            s = __builtin_amdgcn_sad_u8(v, 0u, s);              // the four bytes of v, added to s
        }
        return (int)s;
    }
}

// the sum of the K x K block of bytes at p, rows W apart
template <int K>
__device__ __forceinline__ int ms_block_sum(const uint8_t* __restrict__ p, int W) {
    int s = 0;
#pragma unroll
    for (int dy = 0; dy < K; ++dy) s += ms_row_sum<K>(p + (int64_t)dy * W);
    return s;
}

// blockIdx.x = pair * tiles + tile, blockIdx.y = channel.  part[((pair * 3 + ch) * total + first + tile) * 2 + {0, 1}] =
// this workgroup's sums of ssim and cs.  A pair with an image number outside [0, n) reads and writes nothing.
template <int S>
__global__ __launch_bounds__(MS_THREADS) void msssim_kernel(const uint8_t* __restrict__ imgs, int n, int H, int W,
                                                            const int32_t* __restrict__ pairs, MsScale sc, int total,
                                                            MsWindow win, double C1, double C2,
                                                            double* __restrict__ part) {
    constexpr int K = 1 << S;
    __shared__ double sx[MS_IR][MS_IC], sy[MS_IR][MS_IC];
    __shared__ double sh[5][MS_IR][MS_TC];
    double(*red)[MS_THREADS] = reinterpret_cast<double(*)[MS_THREADS]>(&sx[0][0]);  // after the row pass has read sx

    const int tid = threadIdx.x;
    const int pair = blockIdx.x / sc.tiles, tile = blockIdx.x - pair * sc.tiles, ch = blockIdx.y;
    const int ia = pairs[2 * (int64_t)pair], ib = pairs[2 * (int64_t)pair + 1];
    if ((unsigned)ia >= (unsigned)n || (unsigned)ib >= (unsigned)n) return;     // the whole workgroup
    const int r0 = (tile / sc.tiles_c) * MS_TR, c0 = (tile % sc.tiles_c) * MS_TC;
    const int64_t plane = (int64_t)H * W;
    const uint8_t* __restrict__ pa = imgs + ((int64_t)ia * 3 + ch) * plane;
    const uint8_t* __restrict__ pb = imgs + ((int64_t)ib * 3 + ch) * plane;

    // the pooled halo tile; (y << S) + K - 1 <= Hs * K - 1 <= H - 1, columns alike.  All of a thread's loads are
    // issued before the first LDS store.
    int sa[MS_STAGE], sb[MS_STAGE];
#pragma unroll
    for (int q = 0; q < MS_STAGE; ++q) {
        const int i = tid + q * MS_THREADS;
        const int r = i / MS_IC, c = i - r * MS_IC;
        const int y = r0 + r, x = c0 + c;
        sa[q] = sb[q] = 0;
        if (i < MS_IR * MS_IC && y < sc.Hs && x < sc.Ws) {
            const int64_t o = (int64_t)(y << S) * W + (x << S);
            sa[q] = ms_block_sum<K>(pa + o, W);
            sb[q] = ms_block_sum<K>(pb + o, W);
        }
    }
#pragma unroll
    for (int q = 0; q < MS_STAGE; ++q) {
        const int i = tid + q * MS_THREADS;
        if (i < MS_IR * MS_IC) {
            (&sx[0][0])[i] = (double)sa[q] * (1.0 / (K * K));
            (&sy[0][0])[i] = (double)sb[q] * (1.0 / (K * K));
        }
    }
    __syncthreads();

    // along the rows: taps in ascending order
    for (int i = tid; i < MS_IR * MS_TC; i += MS_THREADS) {
        const int r = i / MS_TC, c = i % MS_TC;
        double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < MS_WIN; ++k) {
            const double x = sx[r][c + k], y = sy[r][c + k], g = win.g[k];
            a[0] += g * x;
            a[1] += g * y;
            a[2] += g * (x * x);
            a[3] += g * (y * y);
            a[4] += g * (x * y);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) sh[q][r][c] = a[q];
    }
    __syncthreads();

    // down the columns: this thread's two positions (rows 2 rg and 2 rg + 1 of column c) share 12 staged rows
    const int c = tid % MS_TC, rg = tid / MS_TC;
    double m[MS_ROWS_PER_THREAD][5];
#pragma unroll
    for (int j = 0; j < MS_ROWS_PER_THREAD; ++j)
#pragma unroll
        for (int q = 0; q < 5; ++q) m[j][q] = 0.0;
#pragma unroll
    for (int k = 0; k < MS_WIN + MS_ROWS_PER_THREAD - 1; ++k)
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const double v = sh[q][MS_ROWS_PER_THREAD * rg + k][c];
#pragma unroll
            for (int j = 0; j < MS_ROWS_PER_THREAD; ++j)
                if (k - j >= 0 && k - j < MS_WIN) m[j][q] += win.g[k - j] * v;
        }

    double t_ssim = 0.0, t_cs = 0.0;
#pragma unroll
    for (int j = 0; j < MS_ROWS_PER_THREAD; ++j) {
        const bool on = r0 + MS_ROWS_PER_THREAD * rg + j < sc.Hs - MS_HALO && c0 + c < sc.Ws - MS_HALO;
        const double mx = m[j][0], my = m[j][1];
        const double sxx = m[j][2] - mx * mx, syy = m[j][3] - my * my, sxy = m[j][4] - mx * my;
        const double cs = (2.0 * sxy + C2) / (sxx + syy + C2);
        const double ssim = cs * (2.0 * mx * my + C1) / (mx * mx + my * my + C1);
        t_ssim += on ? ssim : 0.0;
        t_cs += on ? cs : 0.0;
    }

    // the 256 thread sums, halved in one fixed order
    red[0][tid] = t_ssim;
    red[1][tid] = t_cs;
    __syncthreads();
#pragma unroll
    for (int h = MS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            red[0][tid] += red[0][tid + h];
            red[1][tid] += red[1][tid + h];
        }
        __syncthreads();
    }
    if (tid < 2) part[(((int64_t)pair * 3 + ch) * total + sc.first + tile) * 2 + tid] = red[tid][0];
}

// out[((pair * 3 + ch) * scales + s) * 2 + {0, 1}] = the partials of that scale added in tile order, over the count of
// positions; NaN for a pair with an image number outside [0, n)
__global__ __launch_bounds__(256) void msssim_finish_kernel(const double* __restrict__ part,
                                                            const int32_t* __restrict__ pairs, int n, int P, MsPlan plan,
                                                            double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)P * 3 * plan.scales) return;
    const int s = (int)(i % plan.scales);
    const int64_t pc = i / plan.scales, pair = pc / 3;
    const int ia = pairs[2 * pair], ib = pairs[2 * pair + 1];
    double ssim = NAN, cs = NAN;
    if ((unsigned)ia < (unsigned)n && (unsigned)ib < (unsigned)n) {
        const MsScale sc = plan.s[s];
        const double* __restrict__ p = part + (pc * plan.total + sc.first) * 2;
        ssim = p[0];
        cs = p[1];
        for (int t = 1; t < sc.tiles; ++t) {
            ssim += p[2 * t];
            cs += p[2 * t + 1];
        }
        const double count = (double)(sc.Hs - MS_HALO) * (double)(sc.Ws - MS_HALO);
        ssim /= count;
        cs /= count;
    }
    out[2 * i] = ssim;
    out[2 * i + 1] = cs;
}

// false for a refused shape
inline bool msssim_plan(int H, int W, int P, int scales, MsPlan& plan) {
    if (scales < 1 || scales > MS_MAX_SCALES || H < 1 || W < 1 || H > MS_MAX_SIDE || W > MS_MAX_SIDE) return false;
    if (((H < W ? H : W) >> (scales - 1)) < MS_WIN || P < 1 || P > MS_MAX_PAIRS) return false;
    plan.scales = scales;
    plan.total = 0;
    for (int s = 0; s < scales; ++s) {
        MsScale& sc = plan.s[s];
        sc.Hs = H >> s;
        sc.Ws = W >> s;
        sc.tiles_c = cdiv(sc.Ws - MS_HALO, MS_TC);
        sc.tiles = cdiv(sc.Hs - MS_HALO, MS_TR) * sc.tiles_c;
        sc.first = plan.total;
        plan.total += sc.tiles;
    }
    return (int64_t)P * plan.s[0].tiles <= 0x7fffffffLL;        // the largest grid
}

inline bool ms_aligned(const void* p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }

template <int S>
inline void msssim_launch(const uint8_t* imgs, int n, int H, int W, const int32_t* pairs, int P, const MsPlan& plan,
                          const MsWindow& win, double* part, hipStream_t st) {
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    SBA_LAUNCH(msssim_kernel<S>, dim3((unsigned)(P * plan.s[S].tiles), 3), dim3(MS_THREADS), 0, st, imgs, n, H, W, pairs,
               plan.s[S], plan.total, win, C1, C2, part);
}

}  // namespace

extern "C" int64_t sba_msssim_workspace_bytes(int H, int W, int P, int scales) {
    MsPlan plan;
    if (!msssim_plan(H, W, P, scales, plan)) return -1;
    return (int64_t)P * 3 * plan.total * 2 * (int64_t)sizeof(double);
}

extern "C" int sba_msssim_pairs(const uint8_t* imgs, int n, int H, int W, const int32_t* pairs, int P, int scales,
                                double* out, void* ws, int64_t ws_bytes, void* stream) {
    MsPlan plan;
    if (!imgs || n < 1 || !msssim_plan(H, W, P, scales, plan)) return SBA_E_ARG;
    if (!ms_aligned(pairs, 4) || !ms_aligned(out, 8) || !ms_aligned(ws, 8)) return SBA_E_ARG;
    if (ws_bytes < sba_msssim_workspace_bytes(H, W, P, scales)) return SBA_E_ARG;
    MsWindow win;                       // normalised to sum 1 in double, in tap order
    double sum = 0.0;
    for (int k = 0; k < MS_WIN; ++k) {
        win.g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
        sum += win.g[k];
    }
    for (int k = 0; k < MS_WIN; ++k) win.g[k] /= sum;
    const hipStream_t st = (hipStream_t)stream;
    double* part = (double*)ws;
    for (int s = 0; s < scales; ++s) {
        switch (s) {
            case 0: msssim_launch<0>(imgs, n, H, W, pairs, P, plan, win, part, st); break;
            case 1: msssim_launch<1>(imgs, n, H, W, pairs, P, plan, win, part, st); break;
            case 2: msssim_launch<2>(imgs, n, H, W, pairs, P, plan, win, part, st); break;
            case 3: msssim_launch<3>(imgs, n, H, W, pairs, P, plan, win, part, st); break;
            default: msssim_launch<4>(imgs, n, H, W, pairs, P, plan, win, part, st); break;
        }
        if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    }
    SBA_LAUNCH(msssim_finish_kernel, dim3(cdiv((int64_t)P * 3 * scales, 256)), dim3(256), 0, st, (const double*)part, pairs,
               n, P, plan, out);
    return SBA_CHECK_LAUNCH();
}
