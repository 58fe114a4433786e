// Sliced Wasserstein distance of Laplacian-pyramid patch descriptors (Karras et al. 2018, section 5; sbagan/swd.py,
// DESIGN.md 7k): the four entry points sba_swd_descriptors, sba_swd_project, sba_swd_sort_columns and sba_swd_abs_mean of
// sbagan_hip.h.  Float64 throughout, no atomics, no memset, no allocation; every reduction runs in one fixed order, so the
// same arguments give the same bits.
//
// Descriptors.  One workgroup per (image, channel) builds the Gaussian pyramid up to the level after the requested one
// in LDS and never writes it to memory.  Every level is an exact integer over a power of two: with k = (1, 4, 6, 4, 1),
// I_0 = the bytes and I_{l+1}[Y][X] = sum_ij k_i k_j I_l[2Y + i - 2][2X + j - 2] (mirrored), G_l = I_l / 2^(8 l) and
// I_l <= 255 * 2^(8 l).  So level 1 is kept as 16-bit and levels 2 and 3 as 32-bit integers, level 4 (16 x 16 of a 256 px
// image) as f64, 54 KB in all; level 0 is read from the bytes in memory where it is needed.  The arithmetic is f64 on
// those integers: every product and partial sum is an integer below 2^53, hence exact in any order.  The Laplacian value
//   Lap_l = G_l - up(G_{l+1}) = (2^14 I_l - sum_ij k_i k_j Z_{l+1}[y + i - 2][x + j - 2]) / 2^(8 l + 14)
// (Z zero except Z[2Y][2X] = I_{l+1}[Y][X]; mirroring keeps the parity of an index) has at most 46 significant bits.
//
// Projection.  out[d][i] = sum_k (desc[i][k] - mu_c) dir'[k][d], dir' = dir / sigma_c, on the f64 matrix instruction
// through the lane map of f64_tile.h, the directions as the A rows and the descriptors as the B rows of a 64 x 64 tile,
// so that a lane group stores 16 consecutive descriptors of one direction: the result is direction-major.  K is padded
// from 147 to 148 by zeros.  A first small kernel scales the directions from the statistics on the device; the mean is
// taken off while a descriptor tile is staged (subtracting sum_k mu_c dir'[k][d] afterwards instead cancels a digit or
// two at the last level, where |mu| > sigma, in an error common to all projections of a direction).
//
// Sort.  Tiles of SW_SORT_TILE values are sorted by a bitonic network in LDS, then runs are merged pairwise, doubling,
// between the column buffer and a second one: a workgroup takes SW_SORT_TILE consecutive outputs of a merge, finds where
// they start and end in the two runs (merge path, two binary searches in memory), stages both pieces in LDS, ranks
// every value by a binary search in the other piece (ties: the first run first) and writes the ranked tile coalesced.
// Any length m >= 1.  Values compare with <, so the order of NaNs is undefined and -0 and +0 are equal.
#include "common.h"
#include "f64_tile.h"

#include <math.h>

namespace {

constexpr int SW_THREADS = 256;
constexpr int SW_PATCH = 7, SW_PP = SW_PATCH * SW_PATCH, SW_DESC = 3 * SW_PP, SW_K = SW_DESC + 1;   // 49, 147, 148
constexpr int SW_MAX_LEVELS = 5;
constexpr int SW_MAX_PATCHES = 4096, SW_MAX_DIRS = 65535;
constexpr int SW_SORT_TILE = 2048;
constexpr int SW_MEAN_CHUNK = 4096;
constexpr int SW_KC = 32, SW_LD = SW_KC + 2;        // features staged per chunk; LDS row stride in f64 (f64_tile.h: F64T_LD)

static_assert(SW_K % 4 == 0 && SW_KC % 4 == 0, "the MFMA takes 4 values of k a step");
static_assert(SW_SORT_TILE % SW_THREADS == 0 && (SW_SORT_TILE & (SW_SORT_TILE - 1)) == 0, "the bitonic network");

struct SwLds {
    uint16_t g1[128 * 128];     // I_1 <= 255 * 2^8
    uint32_t g2[64 * 64];       // I_2 <= 255 * 2^16
    uint32_t g3[32 * 32];       // I_3 <= 255 * 2^24
    double g4[16 * 16];         // I_4 <= 255 * 2^32
};

__device__ __forceinline__ int sw_mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// I_l at offset o of the level (row-major, side S >> l); level 0: the bytes
template <int LV>
__device__ __forceinline__ double sw_get(const SwLds& s, const uint8_t* __restrict__ img, int o) {
    if constexpr (LV == 0) return (double)img[o];
    else if constexpr (LV == 1) return (double)s.g1[o];
    else if constexpr (LV == 2) return (double)s.g2[o];
    else if constexpr (LV == 3) return (double)s.g3[o];
    else return s.g4[o];
}
template <int LV>
__device__ __forceinline__ void sw_put(SwLds& s, int o, double v) {
    if constexpr (LV == 1) s.g1[o] = (uint16_t)(uint32_t)v;
    else if constexpr (LV == 2) s.g2[o] = (uint32_t)v;
    else if constexpr (LV == 3) s.g3[o] = (uint32_t)v;
    else s.g4[o] = v;
}

// level LS (side Ss) -> level LS + 1 (side Ss / 2), all threads; the caller puts the barrier after it
template <int LS>
__device__ __forceinline__ void sw_down(SwLds& s, const uint8_t* __restrict__ img, int Ss) {
    const int Sd = Ss >> 1;
    for (int o = threadIdx.x; o < Sd * Sd; o += SW_THREADS) {
        const int Y = o / Sd, X = o - Y * Sd;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int yy = sw_mirror(2 * Y + i - 2, Ss);
            const int ki = i == 2 ? 6 : ((i & 1) ? 4 : 1);
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int xx = sw_mirror(2 * X + j - 2, Ss);
                const int kj = j == 2 ? 6 : ((j & 1) ? 4 : 1);
                acc += (double)(ki * kj) * sw_get<LS>(s, img, yy * Ss + xx);
            }
        }
        sw_put<LS + 1>(s, o, acc);
    }
}

// the value of the requested level LV (side Sl) at (y, x): the Laplacian level, or the Gaussian one when `last`
template <int LV>
__device__ __forceinline__ double sw_value(const SwLds& s, const uint8_t* __restrict__ img, int Sl, bool last, int y,
                                           int x) {
    const double g = sw_get<LV>(s, img, y * Sl + x);
    if (last) return g * (1.0 / (double)(1ull << (8 * LV)));
    if constexpr (LV < SW_MAX_LEVELS - 1) {
        const int Sn = Sl >> 1;
        double up = 0.0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int yy = sw_mirror(y + i - 2, Sl);
            const int ki = i == 2 ? 6 : ((i & 1) ? 4 : 1);
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int xx = sw_mirror(x + j - 2, Sl);
                const int kj = j == 2 ? 6 : ((j & 1) ? 4 : 1);
                if (((yy | xx) & 1) == 0) up += (double)(ki * kj) * sw_get<LV + 1>(s, img, (yy >> 1) * Sn + (xx >> 1));
            }
        }
        return (g * 16384.0 - up) * (1.0 / (double)(1ull << (8 * LV + 14)));
    } else {
        return g;           // (not reached: the deepest level is always the last one)
    }
}

// (hi, lo) += v without losing the bits that hi + v rounds away (Knuth's two-sum); hi + lo is the running sum.  The
// channel statistics scale every projection of a side, so their summation error must stay at a rounding or two.
__device__ __forceinline__ void sw_add(double& hi, double& lo, double v) {
    const double s = hi + v, b = s - hi;
    lo += (hi - (s - b)) + (v - b);
    hi = s;
}
// the (hi, lo) sums of the workgroup's threads, halved in one fixed order; the total, rounded once, in thread 0
__device__ __forceinline__ double sw_block_sum(double (&red)[2][SW_THREADS], double hi, double lo) {
    const int tid = threadIdx.x;
    red[0][tid] = hi;
    red[1][tid] = lo;
    __syncthreads();
#pragma unroll
    for (int h = SW_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            sw_add(red[0][tid], red[1][tid], red[0][tid + h]);
            red[1][tid] += red[1][tid + h];
        }
        __syncthreads();
    }
    return red[0][0] + red[1][0];
}

// grid (n, 3).  desc[(img * P + p) * 147 + ch * 49 + dy * 7 + dx]; part[(img * 3 + ch) * 2] = the sum of this workgroup's
// 49 P values
template <int LV>
__global__ __launch_bounds__(SW_THREADS) void swd_desc_kernel(const uint8_t* __restrict__ imgs, int S, int levels,
                                                              const int32_t* __restrict__ centres, int P,
                                                              double* __restrict__ desc, double* __restrict__ part) {
    __shared__ SwLds s;
    __shared__ double red[2][SW_THREADS];
    const int tid = threadIdx.x, ch = blockIdx.y;
    const int64_t im = blockIdx.x;
    const uint8_t* __restrict__ img = imgs + (im * 3 + ch) * ((int64_t)S * S);
    const bool last = LV == levels - 1;
    const int top = last ? LV : LV + 1;                     // the deepest level this workgroup needs
    if (top >= 1) sw_down<0>(s, img, S);
    __syncthreads();
    if constexpr (LV >= 1) {
        if (top >= 2) sw_down<1>(s, img, S >> 1);
        __syncthreads();
    }
    if constexpr (LV >= 2) {
        if (top >= 3) sw_down<2>(s, img, S >> 2);
        __syncthreads();
    }
    if constexpr (LV >= 3) {
        if (top >= 4) sw_down<3>(s, img, S >> 3);
        __syncthreads();
    }
    const int Sl = S >> LV;
    double t_hi = 0.0, t_lo = 0.0;
    for (int e = tid; e < P * SW_PP; e += SW_THREADS) {
        const int p = e / SW_PP, r = e - p * SW_PP;
        const int dy = r / SW_PATCH, dx = r - dy * SW_PATCH;
        const int64_t d = im * P + p;
        const int cx = centres[2 * d], cy = centres[2 * d + 1];
        const double v = sw_value<LV>(s, img, Sl, last, cy - 3 + dy, cx - 3 + dx);
        desc[d * SW_DESC + ch * SW_PP + r] = v;
        sw_add(t_hi, t_lo, v);
    }
    const double total = sw_block_sum(red, t_hi, t_lo);
    if (tid == 0) part[(im * 3 + ch) * 2] = total;
}

// grid (n, 3), after the sums are folded: part[(img * 3 + ch) * 2 + 1] = the sum of (v - mu_ch)^2 over the 49 P values of
// the image and channel, mu_ch = stats[ch] / count
__global__ __launch_bounds__(SW_THREADS) void swd_dev_kernel(const double* __restrict__ desc, int P,
                                                             const double* __restrict__ stats, double count,
                                                             double* __restrict__ part) {
    __shared__ double red[2][SW_THREADS];
    const int tid = threadIdx.x, ch = blockIdx.y;
    const int64_t im = blockIdx.x;
    const double mu = stats[ch] / count;
    double t_hi = 0.0, t_lo = 0.0;
    for (int e = tid; e < P * SW_PP; e += SW_THREADS) {
        const int p = e / SW_PP, r = e - p * SW_PP;
        const double d = desc[(im * P + p) * SW_DESC + ch * SW_PP + r] - mu;
        sw_add(t_hi, t_lo, d * d);
    }
    const double total = sw_block_sum(red, t_hi, t_lo);
    if (tid == 0) part[(im * 3 + ch) * 2 + 1] = total;
}

// stats[q * 3 + ch] = the partials q (0: sums, 1: sums of squared deviations) of the n images added in image order
__global__ void swd_stats_kernel(const double* __restrict__ part, int64_t n, int q, double* __restrict__ stats) {
    const int ch = threadIdx.x;
    if (ch >= 3) return;
    double hi = 0.0, lo = 0.0;
    for (int64_t i = 0; i < n; ++i) sw_add(hi, lo, part[(i * 3 + ch) * 2 + q]);
    stats[q * 3 + ch] = hi + lo;
}

// dirp[d][k] = dirs[k][d] / sigma_c(k) (k < 147; 0 at k = 147), sigma_c = sqrt(stats[3 + c] / count)
__global__ __launch_bounds__(SW_THREADS) void swd_dirs_kernel(const double* __restrict__ dirs, int D,
                                                              const double* __restrict__ stats, double count,
                                                              double* __restrict__ dirp) {
    const int d = blockIdx.x * SW_THREADS + threadIdx.x;
    if (d >= D) return;
    for (int c = 0; c < 3; ++c) {
        const double inv = 1.0 / sqrt(stats[3 + c] / count);
        for (int k = c * SW_PP; k < (c + 1) * SW_PP; ++k)
            dirp[(int64_t)d * SW_K + k] = dirs[(int64_t)k * D + d] * inv;
    }
    dirp[(int64_t)d * SW_K + SW_DESC] = 0.0;
}

// grid (descriptor tiles, direction tiles).  out[d * m + i] for the 64 directions and 64 descriptors of the tile; the
// descriptors are centred (desc - mu_c, mu_c = stats[c] / count) as they are staged
__global__ __launch_bounds__(F64T_THREADS) void swd_project_kernel(const double* __restrict__ desc, int64_t m,
                                                                   const double* __restrict__ dirp,
                                                                   const double* __restrict__ stats, double count, int D,
                                                                   double* __restrict__ out) {
    __shared__ double sa[F64T_TILE * SW_LD], sb[F64T_TILE * SW_LD];
    const F64Lanes l = f64t_lanes();
    const int tid = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * F64T_TILE;     // first descriptor
    const int i0 = blockIdx.y * F64T_TILE;                  // first direction
    const double mu[3] = {stats[0] / count, stats[1] / count, stats[2] / count};
    f64x4_t acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < SW_K; k0 += SW_KC) {
        const int kc = SW_K - k0 < SW_KC ? SW_K - k0 : SW_KC;       // 32, 32, 32, 32, 20
#pragma unroll
        for (int q = 0; q < F64T_TILE * SW_KC / F64T_THREADS; ++q) {
            const int e = tid + q * F64T_THREADS;
            const int row = e / SW_KC, kk = e - row * SW_KC, k = k0 + kk;
            double a = 0.0, b = 0.0;
            if (i0 + row < D && k < SW_K) a = dirp[(int64_t)(i0 + row) * SW_K + k];
            if (j0 + row < m && k < SW_DESC)
                b = desc[(j0 + row) * SW_DESC + k] - (k < SW_PP ? mu[0] : k < 2 * SW_PP ? mu[1] : mu[2]);
            sa[row * SW_LD + kk] = a;
            sb[row * SW_LD + kk] = b;
        }
        __syncthreads();
        for (int st = 0; st < kc / 4; ++st) {
            const int d = 4 * st + l.lk;
            f64t_mfma(sa[(l.wi + l.lc) * SW_LD + d], sa[(l.wi + 16 + l.lc) * SW_LD + d], sb[(l.wj + l.lc) * SW_LD + d],
                      sb[(l.wj + 16 + l.lc) * SW_LD + d], acc);
        }
        __syncthreads();
    }
    f64t_each(l, acc, [&](int i, int j, double v) {
        if (i0 + i < D && j0 + j < m) out[(int64_t)(i0 + i) * m + j0 + j] = v;
    });
}

// grid (tiles, D): tile blockIdx.x of column blockIdx.y, sorted ascending; src == dst is allowed
__global__ __launch_bounds__(SW_THREADS) void swd_tile_sort_kernel(const double* src, double* dst, int64_t m) {
    __shared__ double s[SW_SORT_TILE];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.y * m + (int64_t)blockIdx.x * SW_SORT_TILE;
    const int64_t left = m - (int64_t)blockIdx.x * SW_SORT_TILE;
    const int len = left < SW_SORT_TILE ? (int)left : SW_SORT_TILE;
    for (int e = tid; e < SW_SORT_TILE; e += SW_THREADS) s[e] = e < len ? src[base + e] : INFINITY;
    __syncthreads();
    for (int k = 2; k <= SW_SORT_TILE; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < SW_SORT_TILE / 2; t += SW_THREADS) {
                const int lo = 2 * t - (t & (j - 1)), hi = lo + j;      // the pair whose indices differ in bit j
                const double a = s[lo], b = s[hi];
                const bool asc = (lo & k) == 0;
                if ((b < a) == asc) {
                    s[lo] = b;
                    s[hi] = a;
                }
            }
            __syncthreads();
        }
    for (int e = tid; e < len; e += SW_THREADS) dst[base + e] = s[e];
}

// how many of the first d values of the merge of a[0, na) and b[0, nb) come from a (ties: a first)
__device__ __forceinline__ int64_t sw_merge_path(const double* __restrict__ a, int64_t na, const double* __restrict__ b,
                                                 int64_t nb, int64_t d) {
    int64_t lo = d - nb > 0 ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (!(b[d - 1 - mid] < a[mid])) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// grid (tiles, D): outputs [blockIdx.x * TILE, + TILE) of column blockIdx.y, from the two sorted runs of length R (the
// last ones of a column shorter) that hold them; src != dst
__global__ __launch_bounds__(SW_THREADS) void swd_merge_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                               int64_t m, int64_t R) {
    __shared__ double sin[SW_SORT_TILE], sout[SW_SORT_TILE];
    __shared__ int64_t split[2];
    const int tid = threadIdx.x;
    const double* __restrict__ col = src + (int64_t)blockIdx.y * m;
    const int64_t o0 = (int64_t)blockIdx.x * SW_SORT_TILE, o1 = o0 + SW_SORT_TILE < m ? o0 + SW_SORT_TILE : m;
    const int64_t p0 = o0 / (2 * R) * (2 * R);                      // the pair of runs starts here
    const int64_t na = m - p0 < R ? m - p0 : R, nb = (m - p0 < 2 * R ? m - p0 : 2 * R) - na;
    const double* __restrict__ A = col + p0;
    const double* __restrict__ B = A + na;
    if (tid == 0 || tid == 64) split[tid >> 6] = sw_merge_path(A, na, B, nb, (tid ? o1 : o0) - p0);
    __syncthreads();
    const int64_t a0 = split[0], b0 = o0 - p0 - a0;
    const int ca = (int)(split[1] - a0), cb = (int)(o1 - o0) - ca;  // values taken from each run: ca + cb <= TILE
    for (int e = tid; e < ca + cb; e += SW_THREADS) sin[e] = e < ca ? A[a0 + e] : B[b0 + (e - ca)];
    __syncthreads();
    for (int e = tid; e < ca + cb; e += SW_THREADS) {
        const double v = sin[e];
        int lo, hi;
        if (e < ca) {               // + the values of the second piece below v
            lo = ca, hi = ca + cb;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sin[mid] < v) lo = mid + 1;
                else hi = mid;
            }
            sout[e + (lo - ca)] = v;
        } else {                    // + the values of the first piece not above v
            lo = 0, hi = ca;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (!(v < sin[mid])) lo = mid + 1;
                else hi = mid;
            }
            sout[(e - ca) + lo] = v;
        }
    }
    __syncthreads();
    double* __restrict__ o = dst + (int64_t)blockIdx.y * m + o0;
    for (int e = tid; e < ca + cb; e += SW_THREADS) o[e] = sout[e];
}

// grid (chunks, D): part[d * chunks + chunk] = sum |a - b| over the chunk, the thread sums halved in one fixed order
__global__ __launch_bounds__(SW_THREADS) void swd_abs_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                             int64_t m, double* __restrict__ part) {
    __shared__ double red[SW_THREADS];
    const int tid = threadIdx.x;
    const int64_t col = (int64_t)blockIdx.y * m, c0 = (int64_t)blockIdx.x * SW_MEAN_CHUNK;
    const int64_t c1 = c0 + SW_MEAN_CHUNK < m ? c0 + SW_MEAN_CHUNK : m;
    double t = 0.0;
    for (int64_t e = c0 + tid; e < c1; e += SW_THREADS) t += fabs(a[col + e] - b[col + e]);
    red[tid] = t;
    __syncthreads();
#pragma unroll
    for (int h = SW_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// out[d] = the partials of column d added in chunk order, over m
__global__ __launch_bounds__(SW_THREADS) void swd_mean_kernel(const double* __restrict__ part, int chunks, int D, int64_t m,
                                                              double* __restrict__ out) {
    const int d = blockIdx.x * SW_THREADS + threadIdx.x;
    if (d >= D) return;
    const double* __restrict__ p = part + (int64_t)d * chunks;
    double a = p[0];
    for (int c = 1; c < chunks; ++c) a += p[c];
    out[d] = a / (double)m;
}

inline bool sw_aligned(const void* p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }

// the number of pyramid levels of an S px image, 0 for a size outside {32, 64, 128, 256}
inline int sw_levels(int S) { return S == 32 ? 2 : S == 64 ? 3 : S == 128 ? 4 : S == 256 ? 5 : 0; }

inline bool sw_columns_ok(int D, int64_t m) {
    return D >= 1 && D <= SW_MAX_DIRS && m >= 1 && m <= ((int64_t)1 << 40) / D && (m + 63) / 64 <= 0x7fffffffLL;
}

template <int LV>
inline void sw_desc_launch(const uint8_t* imgs, int64_t n, int S, int levels, const int32_t* centres, int P, double* desc,
                           double* part, hipStream_t st) {
    SBA_LAUNCH(swd_desc_kernel<LV>, dim3((unsigned)n, 3), dim3(SW_THREADS), 0, st, imgs, S, levels, centres, P, desc, part);
}

}  // namespace

extern "C" int sba_swd_descriptors(const uint8_t* imgs, int64_t n, int S, int level, const int32_t* centres, int P,
                                   double* desc, double* stats, void* ws, int64_t ws_bytes, void* stream) {
    const int levels = sw_levels(S);
    if (!imgs || !centres || levels == 0 || level < 0 || level >= levels) return SBA_E_ARG;
    if (n < 1 || n > 0x7fffffffLL || P < 1 || P > SW_MAX_PATCHES) return SBA_E_ARG;
    if (!sw_aligned(centres, 4) || !sw_aligned(desc, 8) || !sw_aligned(stats, 8) || !sw_aligned(ws, 8)) return SBA_E_ARG;
    const int64_t part_bytes = n * 6 * (int64_t)sizeof(double), centre_bytes = n * P * 2 * (int64_t)sizeof(int32_t);
    if (ws_bytes < part_bytes + centre_bytes) return SBA_E_ARG;
    const int Sl = S >> level;
    for (int64_t i = 0; i < n * P * 2; ++i)
        if (centres[i] < 3 || centres[i] > Sl - 4) return SBA_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    double* part = (double*)ws;
    int32_t* dev_centres = (int32_t*)((char*)ws + part_bytes);
    (void)hipGetLastError();
    if (hipMemcpyAsync(dev_centres, centres, (size_t)centre_bytes, hipMemcpyHostToDevice, st) != hipSuccess)
        return SBA_E_LAUNCH;
    switch (level) {
        case 0: sw_desc_launch<0>(imgs, n, S, levels, dev_centres, P, desc, part, st); break;
        case 1: sw_desc_launch<1>(imgs, n, S, levels, dev_centres, P, desc, part, st); break;
        case 2: sw_desc_launch<2>(imgs, n, S, levels, dev_centres, P, desc, part, st); break;
        case 3: sw_desc_launch<3>(imgs, n, S, levels, dev_centres, P, desc, part, st); break;
        default: sw_desc_launch<4>(imgs, n, S, levels, dev_centres, P, desc, part, st); break;
    }
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    SBA_LAUNCH(swd_stats_kernel, dim3(1), dim3(64), 0, st, (const double*)part, n, 0, stats);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    SBA_LAUNCH(swd_dev_kernel, dim3((unsigned)n, 3), dim3(SW_THREADS), 0, st, (const double*)desc, P, (const double*)stats,
               (double)n * (double)P * (double)SW_PP, part);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    SBA_LAUNCH(swd_stats_kernel, dim3(1), dim3(64), 0, st, (const double*)part, n, 1, stats);
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_swd_project(const double* desc, int64_t m, const double* stats, const double* dirs, int D, double* out,
                               void* ws, int64_t ws_bytes, void* stream) {
    if (!sw_columns_ok(D, m)) return SBA_E_ARG;
    if (!sw_aligned(desc, 8) || !sw_aligned(stats, 8) || !sw_aligned(dirs, 8) || !sw_aligned(out, 8) || !sw_aligned(ws, 8))
        return SBA_E_ARG;
    if (ws_bytes < (int64_t)D * SW_K * (int64_t)sizeof(double)) return SBA_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    double* dirp = (double*)ws;
    const double count = (double)m * (double)SW_PP;
    SBA_LAUNCH(swd_dirs_kernel, dim3(cdiv(D, SW_THREADS)), dim3(SW_THREADS), 0, st, dirs, D, stats, count, dirp);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    SBA_LAUNCH(swd_project_kernel, dim3((unsigned)((m + F64T_TILE - 1) / F64T_TILE), cdiv(D, F64T_TILE)), dim3(F64T_THREADS),
               0, st, desc, m, (const double*)dirp, stats, count, D, out);
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_swd_sort_columns(double* data, double* tmp, int D, int64_t m, void* stream) {
    if (!sw_columns_ok(D, m) || !sw_aligned(data, 8)) return SBA_E_ARG;
    int passes = 0;
    for (int64_t R = SW_SORT_TILE; R < m; R *= 2) ++passes;
    if (passes > 0 && (!sw_aligned(tmp, 8) || tmp == data)) return SBA_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((m + SW_SORT_TILE - 1) / SW_SORT_TILE), (unsigned)D);
    double* cur = (passes & 1) ? tmp : data;        // so that the last merge writes `data`
    SBA_LAUNCH(swd_tile_sort_kernel, grid, dim3(SW_THREADS), 0, st, (const double*)data, cur, m);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    for (int64_t R = SW_SORT_TILE; R < m; R *= 2) {
        double* next = cur == data ? tmp : data;
        SBA_LAUNCH(swd_merge_kernel, grid, dim3(SW_THREADS), 0, st, (const double*)cur, next, m, R);
        if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
        cur = next;
    }
    return SBA_OK;
}

extern "C" int sba_swd_abs_mean(const double* a, const double* b, int D, int64_t m, double* out, void* ws, int64_t ws_bytes,
                                void* stream) {
    if (!sw_columns_ok(D, m)) return SBA_E_ARG;
    if (!sw_aligned(a, 8) || !sw_aligned(b, 8) || !sw_aligned(out, 8) || !sw_aligned(ws, 8)) return SBA_E_ARG;
    const int chunks = (int)((m + SW_MEAN_CHUNK - 1) / SW_MEAN_CHUNK);
    if (ws_bytes < (int64_t)D * chunks * (int64_t)sizeof(double)) return SBA_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    SBA_LAUNCH(swd_abs_kernel, dim3((unsigned)chunks, (unsigned)D), dim3(SW_THREADS), 0, st, a, b, m, (double*)ws);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    SBA_LAUNCH(swd_mean_kernel, dim3(cdiv(D, SW_THREADS)), dim3(SW_THREADS), 0, st, (const double*)ws, chunks, D, m, out);
    return SBA_CHECK_LAUNCH();
}
