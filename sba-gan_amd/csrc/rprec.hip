// R-precision ranking (sba_rprec_rank in sbagan_hip.h): per generated image, the cosine score of its global code against
// its own caption's sentence embedding and against M mismatched ones gathered BY INDEX from the split's pool, and the
// number of mismatched candidates that are not strictly beaten by the true one.  One launch: gather, reductions, clamp,
// compare and count; no [B][M][nef] intermediate, no atomics, no workspace.
#include "common.h"

namespace {

constexpr int RP_WAVES = 4;
constexpr int RP_THREADS = RP_WAVES * 64;

// lane l of a wave owns the float4 slices l, l + 64, ... of a row (NV of them; a slice past the row reads as zeros)
template <int NV>
__device__ __forceinline__ void rp_load_row(float4 (&v)[NV], const float* __restrict__ row, int nv, int lane) {
    for (int k = 0; k < NV; ++k) {
        const int s = lane + 64 * k;
        v[k] = s < nv ? reinterpret_cast<const float4*>(row)[s] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// One workgroup per image, RP_WAVES waves.  Every wave holds the image row in registers and walks the SAME loop body over
// its candidate sequence: the true caption first (every wave scores it itself: one extra 1 KiB row per wave instead of an
// LDS broadcast and a barrier), then the mismatched candidates wave, wave + RP_WAVES, ...  The lane partition and the
// reduction order are fixed and the true score goes through the code of a candidate's, so byte-identical rows give
// bit-identical scores.  The next candidate's row (and the index after it) is in flight while the current one is reduced.
template <int NV>
__global__ __launch_bounds__(RP_THREADS) void rprec_rank_kernel(
    const float* __restrict__ cnn, const float* __restrict__ true_emb, const float* __restrict__ pool,
    const int32_t* __restrict__ idx, float eps, int32_t* __restrict__ rank, float* __restrict__ scores, int M, int nef) {
    __shared__ int sh_hits[RP_WAVES];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = nef >> 2;
    const int32_t* ib = idx + (size_t)b * M;
    float* sb = scores ? scores + (size_t)b * (M + 1) : nullptr;

    float4 a[NV], cur[NV], nxt[NV];
    rp_load_row<NV>(a, cnn + (size_t)b * nef, nv, lane);
    rp_load_row<NV>(cur, true_emb + (size_t)b * nef, nv, lane);
    float na = 0.f;
    for (int k = 0; k < NV; ++k) {
        na += a[k].x * a[k].x; na += a[k].y * a[k].y; na += a[k].z * a[k].z; na += a[k].w * a[k].w;
    }
    na = sqrtf(wave_sum(na));

    int m = -1, mn = wave;                      // current candidate (-1: the true caption) and the next one
    int32_t in = mn < M ? ib[mn] : 0;           // pool row of the next one
    float s0 = 0.f;
    int hits = 0;
    for (;;) {                                  // (every condition below is wave-uniform)
        const bool more = mn < M;
        if (more) rp_load_row<NV>(nxt, pool + (size_t)in * nef, nv, lane);
        const int mnn = mn + RP_WAVES;
        const int32_t inn = mnn < M ? ib[mnn] : 0;
        float dot = 0.f, nb = 0.f;
        for (int k = 0; k < NV; ++k) {
            dot += a[k].x * cur[k].x; dot += a[k].y * cur[k].y; dot += a[k].z * cur[k].z; dot += a[k].w * cur[k].w;
            nb += cur[k].x * cur[k].x; nb += cur[k].y * cur[k].y; nb += cur[k].z * cur[k].z; nb += cur[k].w * cur[k].w;
        }
        dot = wave_sum(dot);
        nb = wave_sum(nb);
        const float s = dot / fmaxf(na * sqrtf(nb), eps);
        if (m < 0) {
            s0 = s;
            if (sb && wave == 0 && lane == 0) sb[0] = s;
        } else {
            hits += !(s < s0) ? 1 : 0;          // a tie or a NaN on either side counts against the image
            if (sb && lane == 0) sb[m + 1] = s;
        }
        if (!more) break;
        m = mn; mn = mnn; in = inn;
        for (int k = 0; k < NV; ++k) cur[k] = nxt[k];
    }
    if (lane == 0) sh_hits[wave] = hits;
    __syncthreads();
    if (threadIdx.x == 0) {
        int r = 0;
        for (int w = 0; w < RP_WAVES; ++w) r += sh_hits[w];
        rank[b] = r;
    }
}

inline bool rp_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int sba_rprec_rank(const float* cnn, const float* true_emb, const float* pool, const int32_t* idx, float eps,
                              int32_t* rank, float* scores, int B, int M, int nef, int P, void* stream) {
    if (!cnn || !true_emb || !pool || !rank || (M > 0 && !idx)) return SBA_E_ARG;
    if (B < 1 || M < 0 || P < 1 || nef < 4 || nef > 1024 || nef % 4) return SBA_E_ARG;
    if (!rp_aligned16(cnn) || !rp_aligned16(true_emb) || !rp_aligned16(pool)) return SBA_E_ARG;
    const hipStream_t st = (hipStream_t)stream;
    const int NV = (nef / 4 + 63) / 64;
#define RP_GO(N)                                                                                                      \
    SBA_LAUNCH(rprec_rank_kernel<N>, dim3(B), dim3(RP_THREADS), 0, st, cnn, true_emb, pool, idx, eps, rank, scores, M, nef)
    if (NV == 1) RP_GO(1);
    else if (NV == 2) RP_GO(2);
    else if (NV == 3) RP_GO(3);
    else RP_GO(4);
#undef RP_GO
    return SBA_CHECK_LAUNCH();
}
