// Weight packing for the implicit-GEMM convolutions of igemm.hip (row-major, transposed data-gradient and
// fragment-major copies; eval-mode BatchNorm folded into the weights) and 2x2 sum pooling.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------
// weight packing and 2x2 sum pooling
// ---------------------------------------------------------------------------
template <typename T>
__global__ void pack_weight_kernel(const float* __restrict__ w, T* __restrict__ out, int Cout, int KH,
                                   int KW, int Cin, int mode) {
    const int64_t n = (int64_t)Cout * (mode == 3 ? 16 : KH * KW) * Cin;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        // i indexes the OUTPUT (so that writes are coalesced)
        float v;
        if (mode == 0) {
            v = w[i];
        } else if (mode == 1) {
            // out[ci][kh'][kw'][co] = w[co][KH-1-kh'][KW-1-kw'][ci]
            const int co = (int)(i % Cout);
            int64_t t = i / Cout;
            const int kw = (int)(t % KW); t /= KW;
            const int kh = (int)(t % KH);
            const int ci = (int)(t / KH);
            v = w[(((int64_t)co * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw)) * Cin + ci];
        } else if (mode == 3) {
            // data-gradient of (nearest x2 -> conv3x3) as ONE 4x4 stride-2 pad-1 conv over dy:
            // out[ci][dd*4+ee][co] = sum_{kh in S(dd)} sum_{kw in S(ee)} w[co][kh][kw][ci],
            // S(0) = {2}, S(1) = {1,2}, S(2) = {0,1}, S(3) = {0}
            const int co = (int)(i % Cout);
            int64_t t = i / Cout;
            const int sl = (int)(t % 16);
            const int ci = (int)(t / 16);
            const int dd = sl >> 2, ee = sl & 3;
            const int kh0 = dd == 0 ? 2 : (dd == 1 ? 1 : 0), khn = (dd == 1 || dd == 2) ? 2 : 1;
            const int kw0 = ee == 0 ? 2 : (ee == 1 ? 1 : 0), kwn = (ee == 1 || ee == 2) ? 2 : 1;
            v = 0.f;
            for (int a = 0; a < khn; ++a)
                for (int b2 = 0; b2 < kwn; ++b2)
                    v += w[(((int64_t)co * 3 + kh0 + a) * 3 + kw0 + b2) * Cin + ci];
        } else {
            // out[cls][ci][j*2+i2][co], cls = py*2+px, kh = (1-py)+2j, kw = (1-px)+2*i2  (KH=KW=4)
            const int co = (int)(i % Cout);
            int64_t t = i / Cout;
            const int tp = (int)(t % 4); t /= 4;
            const int ci = (int)(t % Cin);
            const int cls = (int)(t / Cin);
            const int py = cls >> 1, px = cls & 1, j = tp >> 1, i2 = tp & 1;
            const int kh = (1 - py) + 2 * j, kw = (1 - px) + 2 * i2;
            v = w[(((int64_t)co * 4 + kh) * 4 + kw) * Cin + ci];
        }
        out[i] = from_f<T>(v);
    }
}

// modes 1 / 2 as tiled transposes: for one (source tap -> destination tap) pair the job is
// out[ci][co] = w[co][ci] with row strides of taps*Cin resp. dtaps*Cout; 32x32 tiles through LDS
// keep both the global reads (along ci) and writes (along co) coalesced.
template <typename T>
__global__ __launch_bounds__(256) void pack_weight_tr_kernel(const float* __restrict__ w, T* __restrict__ out,
                                                             int Cout, int KH, int KW, int Cin, int mode) {
    __shared__ float tile[32][33];
    const int z = blockIdx.z;
    int src_tap, dst_tap, dtaps;
    int64_t dst_base = 0;
    if (mode == 1) {
        const int kh = z / KW, kw = z - kh * KW;
        dst_tap = z;
        src_tap = (KH - 1 - kh) * KW + (KW - 1 - kw);
        dtaps = KH * KW;
    } else {
        const int cls = z >> 2, tp = z & 3;
        const int py = cls >> 1, px = cls & 1, j = tp >> 1, i2 = tp & 1;
        src_tap = ((1 - py) + 2 * j) * 4 + (1 - px) + 2 * i2;
        dst_tap = tp;
        dtaps = 4;
        dst_base = (int64_t)cls * Cin * 4 * Cout;
    }
    const int taps = KH * KW;
    const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
#pragma unroll
    for (int r = ty; r < 32; r += 8) {
        const int co = co0 + r, ci = ci0 + tx;
        tile[r][tx] = (co < Cout && ci < Cin) ? w[((int64_t)co * taps + src_tap) * Cin + ci] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int r = ty; r < 32; r += 8) {
        const int ci = ci0 + r, co = co0 + tx;
        if (ci < Cin && co < Cout) out[dst_base + ((int64_t)ci * dtaps + dst_tap) * Cout + co] = from_f<T>(tile[tx][r]);
    }
}

// every packed copy of one network in one launch: a workgroup owns one 64(co) x 64(ci) tile of one
// source tap of one tensor, reads it once (float4 rows), writes the forward copy (same order) and
// the transposed data-gradient copy (64 co contiguous = full 128-byte lines) through LDS
template <typename T>
__global__ __launch_bounds__(256) void pack_multi_kernel(const sba_pack_desc* __restrict__ descs, int ndesc) {
    __shared__ float tile[64][65];
    int lo = 0, hi = ndesc - 1;
    const int b = blockIdx.x;
    while (lo < hi) {                                   // last desc with tile_begin <= b (uniform)
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].tile_begin <= b) lo = mid; else hi = mid - 1;
    }
    const sba_pack_desc d = descs[lo];
    const int local = b - d.tile_begin;
    const int per_tap = d.co_tiles * d.ci_tiles;
    const int src_tap = local / per_tap;                 // mode 3: the destination tap slot (0..15)
    const int rem = local - src_tap * per_tap;
    const int co0 = (rem / d.ci_tiles) * 64, ci0 = (rem % d.ci_tiles) * 64;
    const int taps = d.KH * d.KW;
    const int slots = d.mode == 3 ? 16 : taps;
    if (src_tap >= slots) return;
    const int tid = threadIdx.x;
    const int c4 = (tid & 15) * 4;
    T* fwd = reinterpret_cast<T*>(d.fwd);
    // mode 3 (data-gradient of nearest x2 -> conv3x3 as one 4x4/s2 conv): slot (dd, ee) sums the source
    // taps kh in S(dd), kw in S(ee);  S(0) = {2}, S(1) = {1,2}, S(2) = {0,1}, S(3) = {0}
    int kh0 = 0, khn = 1, kw0 = 0, kwn = 1;
    if (d.mode == 3) {
        const int dd = src_tap >> 2, ee = src_tap & 3;
        kh0 = dd == 0 ? 2 : (dd == 1 ? 1 : 0); khn = (dd == 1 || dd == 2) ? 2 : 1;
        kw0 = ee == 0 ? 2 : (ee == 1 ? 1 : 0); kwn = (ee == 1 || ee == 2) ? 2 : 1;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (tid >> 4) + 16 * i;
        const int co = co0 + r, ci = ci0 + c4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (co < d.Cout && ci < d.Cin) {
            if (d.mode != 3 || src_tap < taps) {           // forward copy of source tap `src_tap`
                const int64_t o = ((int64_t)co * taps + src_tap) * d.Cin + ci;
                const float4 f = *reinterpret_cast<const float4*>(d.w + o);
                if (fwd) {
                    fwd[o] = from_f<T>(f.x); fwd[o + 1] = from_f<T>(f.y);
                    fwd[o + 2] = from_f<T>(f.z); fwd[o + 3] = from_f<T>(f.w);
                }
                if (d.mode != 3) v = f;
            }
            if (d.mode == 3) {
                for (int a = 0; a < khn; ++a)
                    for (int b2 = 0; b2 < kwn; ++b2) {
                        const float4 f = *reinterpret_cast<const float4*>(
                            d.w + ((int64_t)co * 9 + (kh0 + a) * 3 + kw0 + b2) * d.Cin + ci);
                        v.x += f.x; v.y += f.y; v.z += f.z; v.w += f.w;
                    }
            }
        }
        tile[r][c4] = v.x; tile[r][c4 + 1] = v.y; tile[r][c4 + 2] = v.z; tile[r][c4 + 3] = v.w;
    }
    if (!d.tr) return;
    __syncthreads();
    int dst_tap, dtaps;
    int64_t dst_base = 0;
    if (d.mode == 1) {
        const int kh = src_tap / d.KW, kw = src_tap - kh * d.KW;
        dst_tap = (d.KH - 1 - kh) * d.KW + (d.KW - 1 - kw);
        dtaps = taps;
    } else if (d.mode == 3) {
        dst_tap = src_tap;
        dtaps = 16;
    } else {
        const int kh = src_tap >> 2, kw = src_tap & 3;      // kh = (1-py) + 2j, kw = (1-px) + 2i
        const int py = 1 - (kh & 1), px = 1 - (kw & 1);
        dst_tap = (kh >> 1) * 2 + (kw >> 1);
        dtaps = 4;
        dst_base = (int64_t)(py * 2 + px) * d.Cin * 4 * d.Cout;
    }
    T* tr = reinterpret_cast<T*>(d.tr);
    const int c8 = (tid & 7) * 8;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (tid >> 3) + 32 * i;                  // ci within the tile
        const int ci = ci0 + r, co = co0 + c8;
        if (ci >= d.Cin || co >= d.Cout) continue;
        T* op = tr + dst_base + ((int64_t)ci * dtaps + dst_tap) * d.Cout + co;
        if (co + 8 <= d.Cout && sizeof(T) == 2) {
            uint4 o;
            o.x = (uint32_t)f2bf(tile[c8 + 0][r]) | ((uint32_t)f2bf(tile[c8 + 1][r]) << 16);
            o.y = (uint32_t)f2bf(tile[c8 + 2][r]) | ((uint32_t)f2bf(tile[c8 + 3][r]) << 16);
            o.z = (uint32_t)f2bf(tile[c8 + 4][r]) | ((uint32_t)f2bf(tile[c8 + 5][r]) << 16);
            o.w = (uint32_t)f2bf(tile[c8 + 6][r]) | ((uint32_t)f2bf(tile[c8 + 7][r]) << 16);
            *reinterpret_cast<uint4*>(op) = o;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (co + k < d.Cout) op[k] = from_f<T>(tile[c8 + k][r]);
        }
    }
}

template <typename T>
__global__ void pool2x2_kernel(const T* __restrict__ up, T* __restrict__ dx, int N, int H, int W, int C) {
    constexpr int V = Vec16<T>::N;
    const int cv = C / V;
    const int64_t total = (int64_t)N * H * W * cv;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % cv) * V;
        int64_t p = i / cv;
        const int xx = (int)(p % W); p /= W;
        const int yy = (int)(p % H);
        const int n = (int)(p / H);
        const T* b = up + (((int64_t)n * 2 * H + 2 * yy) * 2 * W + 2 * xx) * C + c;
        Vec16<T> v00 = ld16(b), v01 = ld16(b + C), v10 = ld16(b + (int64_t)2 * W * C),
                 v11 = ld16(b + (int64_t)2 * W * C + C), o;
#pragma unroll
        for (int k = 0; k < V; ++k) o.set(k, v00.get(k) + v01.get(k) + v10.get(k) + v11.get(k));
        st16(dx + (((int64_t)n * H + yy) * W + xx) * C + c, o);
    }
}

// row-major packed conv operand [R][taps][K] (bf16; R a multiple of 32, K of 16) -> fragment-major
// [ceil(R/64)][taps][2][K/16][64 lanes][8]: lane = ((k >> 3) & 1) * 32 + (r & 31).  One thread = 16 bytes.
__global__ __launch_bounds__(256) void pack_frag_kernel(const sba_frag_desc* __restrict__ descs, const int ndesc,
                                                        const int total_units) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= total_units) return;
    int lo = 0, hi = ndesc - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].unit_begin <= u) lo = mid; else hi = mid - 1;
    }
    const sba_frag_desc d = descs[lo];
    const int local = u - d.unit_begin;
    const int k8n = d.K / 8;
    const int k8 = local % k8n, rest = local / k8n;
    const int t = rest % d.taps, r = rest / d.taps;
    const uint4 v = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(d.src) + ((int64_t)r * d.taps + t) * d.K + 8 * k8);
    const int nb = r >> 6, j = (r >> 5) & 1, nn = r & 31, k16 = k8 >> 1, gg = k8 & 1, ks = d.K / 16;
    const int64_t o = (((((int64_t)nb * d.taps + t) * 2 + j) * ks + k16) * 512) + (gg * 32 + nn) * 8;
    *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(d.dst) + o) = v;
}

// Fold the eval-mode BatchNorm of a conv (or dense) layer into its weights and pack them for the forward kernels:
//   out[r][tap][ci] = w[src(r)][tap][ci] * s,  bias[r] = beta - mean * s,  s = gamma / sqrt(var + eps)   (of row src(r))
// the product in f32, rounded ONCE to the storage type.  glu = 0: src(r) = r.  glu = 1: the O = 2C rows are interleaved in
// granules of 32 (tile_epilogue_glu): r = 64 b + q -> value channel 32 b + q (q < 32) or gate channel C + 32 b + q - 32;
// rows of channels >= C are zero.
template <typename T>
__global__ __launch_bounds__(256) void fold_bn_pack_kernel(const float* __restrict__ w, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ mean,
                                                           const float* __restrict__ var, const float eps,
                                                           T* __restrict__ out, float* __restrict__ bias, const int O,
                                                           const int rowlen, const int glu, const int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / rowlen), k = (int)(i - (int64_t)r * rowlen);
        int src = r;
        if (glu) {
            const int C = O / 2, q = r & 63, c = (r >> 6) * 32 + (q & 31);
            src = c < C ? c + (q >= 32 ? C : 0) : -1;
        }
        float v = 0.f, b = 0.f;
        if (src >= 0) {
            const float s = gamma[src] / sqrtf(var[src] + eps);
            v = w[(int64_t)src * rowlen + k] * s;
            b = beta[src] - mean[src] * s;
        }
        out[i] = from_f<T>(v);
        if (k == 0) bias[r] = b;
    }
}

}  // namespace

extern "C" int sba_fold_bn_pack(int dtype, const float* w, const float* gamma, const float* beta,
                                const float* running_mean, const float* running_var, float eps, void* out, float* bias,
                                int O, int taps, int Cin, int glu, void* stream) {
    if (!w || !gamma || !beta || !running_mean || !running_var || !out || !bias) return SBA_E_ARG;
    if (O <= 0 || taps <= 0 || Cin <= 0 || (glu && O % 2)) return SBA_E_ARG;
    const int rows = glu ? 64 * ((O / 2 + 31) / 32) : O;
    const int64_t n = (int64_t)rows * taps * Cin;
    if ((int64_t)taps * Cin > 0x7fffffff) return SBA_E_ARG;
    const int blocks = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    SBA_DISPATCH(dtype, SBA_LAUNCH((fold_bn_pack_kernel<T>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, gamma,
                                   beta, running_mean, running_var, eps, (T*)out, bias, O, taps * Cin, glu, n));
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_pack_weight(int dtype, const float* w, void* out, int Cout, int KH, int KW, int Cin,
                               int mode, void* stream) {
    if (!w || !out || Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0 || mode < 0 || mode > 3) return SBA_E_ARG;
    if (mode == 3 && (KH != 3 || KW != 3)) return SBA_E_ARG;
    if (mode == 2 && (KH != 4 || KW != 4)) return SBA_E_ARG;
    if (mode == 1 || mode == 2) {
        dim3 grid(cdiv(Cin, 32), cdiv(Cout, 32), mode == 1 ? KH * KW : 16);
        if (grid.y > 65535) return SBA_E_ARG;
        SBA_DISPATCH(dtype, SBA_LAUNCH((pack_weight_tr_kernel<T>), grid, dim3(256), 0, (hipStream_t)stream,
                                               w, (T*)out, Cout, KH, KW, Cin, mode));
        return SBA_CHECK_LAUNCH();
    }
    const int64_t n = (int64_t)Cout * (mode == 3 ? 16 : KH * KW) * Cin;
    const int blocks = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    SBA_DISPATCH(dtype, SBA_LAUNCH((pack_weight_kernel<T>), dim3(blocks), dim3(256), 0,
                                           (hipStream_t)stream, w, (T*)out, Cout, KH, KW, Cin, mode));
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_pack_weights_multi(int dtype, const sba_pack_desc* descs, int ndesc, int total_tiles,
                                      void* stream) {
    if (!descs || ndesc <= 0 || total_tiles <= 0) return SBA_E_ARG;
    if (((uintptr_t)descs & 7) != 0) return SBA_E_ARG;
    SBA_DISPATCH(dtype, SBA_LAUNCH((pack_multi_kernel<T>), dim3(total_tiles), dim3(256), 0,
                                           (hipStream_t)stream, descs, ndesc));
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_pack_frag_multi(const sba_frag_desc* descs, int ndesc, int total_units, void* stream) {
    if (!descs || ndesc <= 0 || total_units <= 0 || ((uintptr_t)descs & 7) != 0) return SBA_E_ARG;
    SBA_LAUNCH(pack_frag_kernel, dim3(cdiv(total_units, 256)), dim3(256), 0, (hipStream_t)stream, descs, ndesc, total_units);
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_pool2x2_sum(int dtype, const void* dup, void* dx, int N, int H, int W, int C, void* stream) {
    if (!dup || !dx || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0) return SBA_E_ARG;
    const int64_t total = (int64_t)N * H * W * (C / (dtype == SBA_BF16 ? 8 : 4));
    const int blocks = (int)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    SBA_DISPATCH(dtype, SBA_LAUNCH((pool2x2_kernel<T>), dim3(blocks), dim3(256), 0,
                                           (hipStream_t)stream, (const T*)dup, (T*)dx, N, H, W, C));
    return SBA_CHECK_LAUNCH();
}
