// BertEncoder forward on the device (model_bert.py:161-189; SURVEY.md 8f-2, second half): the frozen BERT-base
// trunk of the `bert` / `mix` variants' text side.  The dense layers (QKV, attention output, the two feed-forward
// layers, the 1x1 word projection) are M = B*L = 400-row GEMMs and run on the implicit-GEMM kernels as 1x1
// convolutions with a bias epilogue (sba_conv_igemm_bias); this file holds what sits between them:
//   bert_embed_ln     word + position + token-type embedding gather, LayerNorm (eps 1e-12)
//   bert_attention    per (caption, head): softmax(q k^T / sqrt(64)) v for L <= 32 tokens, NO attention mask
//                     (the reference passes none, model_bert.py:181), q / k / v staged in LDS as f32
//   bert_add_ln       LayerNorm(x + residual)
//   bert_gelu         exact (erf) GELU, in place
//   bert_tanh_t       tanh + transpose [B*L][nef] -> [B][nef][L] f32 (words_embs layout of the generator)
// Train mode (pretrain_DAMSM_bert.py: the frozen trunk runs under bert_model.train()): the embedding LayerNorm, the
// attention and the add+LayerNorm kernels take a compile-time DROPOUT flag; the counter-based generator that draws their
// masks is sba_dropout_keep below (definition in include/sbagan_hip.h).  No mask is stored: nothing flows back into the
// trunk.  The heads' backward (the only trained part of the text side):
//   bert_words_head_bwd   dpre = dwords * (1 - y^2), transposed to [B*L][nef] (compute dtype) + its bias sum
//   bert_sent_head_bwd    tanh(fc(tanh(pooler(cls)))) chain: dW / db of fc and pooler, dpooled
// Activations are the compute dtype T (bf16 / f32), statistics and softmax in f32.
#include <math.h>

#include "common.h"

namespace {

// Philox4x32-10 (Salmon et al., SC'11), key = (seed lo, seed hi), counter = (element index, site, offset lo, offset hi);
// an element is dropped when (x0 >> 8) * 2^-24 < p, x0 = the first output word.
__device__ __forceinline__ bool sba_dropout_keep(uint32_t idx, uint32_t site, uint64_t offset, uint64_t seed, float p) {
    uint32_t c0 = idx, c1 = site, c2 = (uint32_t)offset, c3 = (uint32_t)(offset >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return (float)(c0 >> 8) * (1.f / 16777216.f) >= p;
}

struct Dropout {
    float p, scale;          // scale = 1 / (1 - p), applied in f32 to the kept values
    uint64_t seed, offset;
    uint32_t site;
};

// one wave per row of C = 768 values (12 per lane)
template <typename T, bool DROPOUT>
__global__ __launch_bounds__(256) void bert_embed_ln_kernel(const int64_t* __restrict__ tok, const float* __restrict__ we,
                                                            const float* __restrict__ pe, const float* __restrict__ te,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            T* __restrict__ out, int rows, int L, int C, int ntoken,
                                                            float eps, Dropout dp) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    int64_t t = tok[row];
    if (t < 0 || t >= ntoken) t = 0;
    const int pos = row % L;
    float v[16];
    float s = 0.f;
    const int per = C / 64;
    for (int i = 0; i < per; ++i) {
        const int c = lane + 64 * i;
        v[i] = we[t * C + c] + pe[(int64_t)pos * C + c] + te[c];
        s += v[i];
    }
    const float mean = wave_sum(s) / C;
    float q = 0.f;
    for (int i = 0; i < per; ++i) { const float d = v[i] - mean; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) / C + eps);
    for (int i = 0; i < per; ++i) {
        const int c = lane + 64 * i;
        float y = (v[i] - mean) * rstd * gamma[c] + beta[c];
        if (DROPOUT) {                                  // dropout(LayerNorm(emb))
            const bool keep = sba_dropout_keep((uint32_t)((int64_t)row * C + c), dp.site, dp.offset, dp.seed, dp.p);
            y = keep ? y * dp.scale : 0.f;
        }
        out[(int64_t)row * C + c] = from_f<T>(y);
    }
}

template <typename T, bool DROPOUT>
__global__ __launch_bounds__(256) void bert_add_ln_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          T* __restrict__ out, int rows, int C, float eps, Dropout dp) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float v[16];
    float s = 0.f;
    const int per = C / 64;
    for (int i = 0; i < per; ++i) {
        const int64_t o = (int64_t)row * C + lane + 64 * i;
        float xv = to_f<T>(x[o]);
        if (DROPOUT) {                                  // LayerNorm(dropout(x) + residual)
            const bool keep = sba_dropout_keep((uint32_t)o, dp.site, dp.offset, dp.seed, dp.p);
            xv = keep ? xv * dp.scale : 0.f;
        }
        v[i] = xv + to_f<T>(res[o]);
        s += v[i];
    }
    const float mean = wave_sum(s) / C;
    float q = 0.f;
    for (int i = 0; i < per; ++i) { const float d = v[i] - mean; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) / C + eps);
    for (int i = 0; i < per; ++i) {
        const int c = lane + 64 * i;
        out[(int64_t)row * C + c] = from_f<T>((v[i] - mean) * rstd * gamma[c] + beta[c]);
    }
}

// grid (B, heads), block 256: qkv [B*L][3*C] (q | k | v), ctx [B*L][C]; head dim 64, L <= 32
template <typename T, bool DROPOUT>
__global__ __launch_bounds__(256) void bert_attention_kernel(const T* __restrict__ qkv, T* __restrict__ ctx, int L, int C,
                                                             Dropout dp) {
    constexpr int D = 64, LM = 32;
    __shared__ float sq[LM][D + 1], sk[LM][D + 1], sv[LM][D + 1], sp[LM][LM + 1];
    const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < L * D; i += 256) {
        const int t = i / D, d = i - t * D;
        const int64_t o = ((int64_t)b * L + t) * 3 * C + h * D + d;
        sq[t][d] = to_f<T>(qkv[o]);
        sk[t][d] = to_f<T>(qkv[o + C]);
        sv[t][d] = to_f<T>(qkv[o + 2 * C]);
    }
    __syncthreads();
    for (int i = tid; i < L * L; i += 256) {
        const int a = i / L, c = i - a * L;
        float s = 0.f;
#pragma unroll 16
        for (int d = 0; d < D; ++d) s += sq[a][d] * sk[c][d];
        sp[a][c] = s * 0.125f;                     // 1 / sqrt(64)
    }
    __syncthreads();
    if (tid < L) {
        float m = -INFINITY;
        for (int c = 0; c < L; ++c) m = fmaxf(m, sp[tid][c]);
        float z = 0.f;
        for (int c = 0; c < L; ++c) { const float e = expf(sp[tid][c] - m); sp[tid][c] = e; z += e; }
        const float iz = 1.f / z;
        for (int c = 0; c < L; ++c) sp[tid][c] *= iz;
    }
    __syncthreads();
    if (DROPOUT) {                                      // dropout(softmax), element (b, head, query, key)
        const uint32_t base = (uint32_t)((b * gridDim.y + h) * L * L);
        for (int i = tid; i < L * L; i += 256) {
            const int a = i / L, c = i - a * L;
            const bool keep = sba_dropout_keep(base + i, dp.site, dp.offset, dp.seed, dp.p);
            sp[a][c] = keep ? sp[a][c] * dp.scale : 0.f;
        }
        __syncthreads();
    }
    for (int i = tid; i < L * D; i += 256) {
        const int t = i / D, d = i - t * D;
        float s = 0.f;
        for (int c = 0; c < L; ++c) s += sp[t][c] * sv[c][d];
        ctx[((int64_t)b * L + t) * C + h * D + d] = from_f<T>(s);
    }
}

template <typename T>
__global__ void bert_gelu_kernel(T* __restrict__ x, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = to_f<T>(x[i]);
        x[i] = from_f<T>(0.5f * v * (1.f + erff(v * 0.70710678118654752f)));
    }
}

// y[b][c][l] = tanh(x[b*L + l][c])
template <typename T>
__global__ void bert_tanh_t_kernel(const T* __restrict__ x, float* __restrict__ y, int B, int L, int C) {
    const int64_t n = (int64_t)B * L * C;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int64_t r = i / C;
        const int l = (int)(r % L), b = (int)(r / L);
        y[((int64_t)b * C + c) * L + l] = tanhf(to_f<T>(x[i]));
    }
}

}  // namespace

namespace {

Dropout make_dropout(float p, uint64_t seed, uint64_t offset, int site) {
    Dropout d;
    d.p = p;
    d.scale = 1.f / (1.f - p);
    d.seed = seed;
    d.offset = offset;
    d.site = (uint32_t)site;
    return d;
}

template <bool DROPOUT>
int embed_ln(int dtype, const int64_t* tokens, const float* word_emb, const float* pos_emb, const float* type_emb,
             const float* gamma, const float* beta, void* out, int B, int L, int C, int ntoken, float eps, Dropout dp,
             void* stream) {
    if (!tokens || !word_emb || !pos_emb || !type_emb || !gamma || !beta || !out) return SBA_E_ARG;
    if (B <= 0 || L <= 0 || C <= 0 || C % 64 != 0 || C > 1024 || ntoken <= 0) return SBA_E_ARG;
    const int rows = B * L;
    SBA_DISPATCH(dtype, SBA_LAUNCH((bert_embed_ln_kernel<T, DROPOUT>), dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream,
                                   tokens, word_emb, pos_emb, type_emb, gamma, beta, (T*)out, rows, L, C, ntoken, eps, dp));
    return SBA_CHECK_LAUNCH();
}

template <bool DROPOUT>
int add_ln(int dtype, const void* x, const void* residual, const float* gamma, const float* beta, void* out, int rows,
           int C, float eps, Dropout dp, void* stream) {
    if (!x || !residual || !gamma || !beta || !out || rows <= 0 || C <= 0 || C % 64 != 0 || C > 1024) return SBA_E_ARG;
    SBA_DISPATCH(dtype, SBA_LAUNCH((bert_add_ln_kernel<T, DROPOUT>), dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream,
                                   (const T*)x, (const T*)residual, gamma, beta, (T*)out, rows, C, eps, dp));
    return SBA_CHECK_LAUNCH();
}

template <bool DROPOUT>
int attention(int dtype, const void* qkv, void* ctx, int B, int L, int C, int heads, Dropout dp, void* stream) {
    if (!qkv || !ctx || B <= 0 || L <= 0 || L > 32 || heads <= 0 || C != heads * 64) return SBA_E_ARG;
    SBA_DISPATCH(dtype, SBA_LAUNCH((bert_attention_kernel<T, DROPOUT>), dim3(B, heads), dim3(256), 0, (hipStream_t)stream,
                                   (const T*)qkv, (T*)ctx, L, C, dp));
    return SBA_CHECK_LAUNCH();
}

// the dropout entry points: 0 <= p < 1, element indices of a site's tensor within 32 bits
bool dropout_ok(float p, int site, int64_t n) { return p >= 0.f && p < 1.f && site >= 0 && n <= 0xFFFFFFFFll; }

}  // namespace

extern "C" int sba_bert_embed_ln(int dtype, const int64_t* tokens, const float* word_emb, const float* pos_emb,
                                 const float* type_emb, const float* gamma, const float* beta, void* out, int B, int L,
                                 int C, int ntoken, float eps, void* stream) {
    return embed_ln<false>(dtype, tokens, word_emb, pos_emb, type_emb, gamma, beta, out, B, L, C, ntoken, eps,
                           make_dropout(0.f, 0, 0, 0), stream);
}

extern "C" int sba_bert_add_ln(int dtype, const void* x, const void* residual, const float* gamma, const float* beta,
                               void* out, int rows, int C, float eps, void* stream) {
    return add_ln<false>(dtype, x, residual, gamma, beta, out, rows, C, eps, make_dropout(0.f, 0, 0, 0), stream);
}

extern "C" int sba_bert_attention(int dtype, const void* qkv, void* ctx, int B, int L, int C, int heads, void* stream) {
    return attention<false>(dtype, qkv, ctx, B, L, C, heads, make_dropout(0.f, 0, 0, 0), stream);
}

extern "C" int sba_bert_embed_ln_train(float p, uint64_t seed, uint64_t offset, int site, int dtype, const int64_t* tokens,
                                       const float* word_emb, const float* pos_emb, const float* type_emb,
                                       const float* gamma, const float* beta, void* out, int B, int L, int C, int ntoken,
                                       float eps, void* stream) {
    if (!dropout_ok(p, site, (int64_t)B * L * C)) return SBA_E_ARG;
    return embed_ln<true>(dtype, tokens, word_emb, pos_emb, type_emb, gamma, beta, out, B, L, C, ntoken, eps,
                          make_dropout(p, seed, offset, site), stream);
}

extern "C" int sba_bert_add_ln_train(float p, uint64_t seed, uint64_t offset, int site, int dtype, const void* x,
                                     const void* residual, const float* gamma, const float* beta, void* out, int rows,
                                     int C, float eps, void* stream) {
    if (!dropout_ok(p, site, (int64_t)rows * C)) return SBA_E_ARG;
    return add_ln<true>(dtype, x, residual, gamma, beta, out, rows, C, eps, make_dropout(p, seed, offset, site), stream);
}

extern "C" int sba_bert_attention_train(float p, uint64_t seed, uint64_t offset, int site, int dtype, const void* qkv,
                                        void* ctx, int B, int L, int C, int heads, void* stream) {
    if (!dropout_ok(p, site, (int64_t)B * heads * L * L)) return SBA_E_ARG;
    return attention<true>(dtype, qkv, ctx, B, L, C, heads, make_dropout(p, seed, offset, site), stream);
}

extern "C" int sba_bert_gelu(int dtype, void* x, int64_t n, void* stream) {
    if (!x || n <= 0) return SBA_E_ARG;
    const int blocks = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    SBA_DISPATCH(dtype, SBA_LAUNCH((bert_gelu_kernel<T>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, (T*)x, n));
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_bert_tanh_transpose(int dtype, const void* x, float* y, int B, int L, int C, void* stream) {
    if (!x || !y || B <= 0 || L <= 0 || C <= 0) return SBA_E_ARG;
    const int64_t n = (int64_t)B * L * C;
    const int blocks = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
    SBA_DISPATCH(dtype, SBA_LAUNCH((bert_tanh_t_kernel<T>), dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                                   (const T*)x, y, B, L, C));
    return SBA_CHECK_LAUNCH();
}

namespace {

// ---- heads backward --------------------------------------------------------------------------------------------------
// grid (nef / 64), block 256: 64 channels per workgroup, captions in order.  The [64][L] slice of caption b is staged
// in LDS (coalesced reads of dwords[b][c][l] along l, coalesced writes of dpre[b*L + l][c] along c); the bias sums run
// over (b, l) in a fixed order in the first wave's registers: no atomics, bit-reproducible.
template <typename T>
__global__ __launch_bounds__(256) void bert_words_head_bwd_kernel(const float* __restrict__ dwords,
                                                                  const float* __restrict__ y, T* __restrict__ dpre,
                                                                  float* __restrict__ dbias, int B, int L, int nef) {
    __shared__ float s[64][33];
    const int c0 = blockIdx.x * 64, tid = threadIdx.x;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
        for (int i = tid; i < 64 * L; i += 256) {
            const int cl = i / L, l = i - cl * L;
            const int64_t o = ((int64_t)b * nef + c0 + cl) * L + l;
            const float yv = y[o];
            s[cl][l] = dwords[o] * (1.f - yv * yv);
        }
        __syncthreads();
        for (int i = tid; i < 64 * L; i += 256) {
            const int l = i >> 6, cl = i & 63;
            dpre[((int64_t)b * L + l) * nef + c0 + cl] = from_f<T>(s[cl][l]);
        }
        if (tid < 64)
            for (int l = 0; l < L; ++l) acc += s[tid][l];
        __syncthreads();
    }
    if (tid < 64) dbias[c0 + tid] += acc;
}

// Sentence chain, launch 1 (grid nef * C / 256 + B * C / 256 workgroups of 256):
//   dW_fc[n][k] += sum_b g[b][n] pooled[b][k],  db_fc[n] += sum_b g[b][n]     (the k == 0 threads)
//   dpooled[b][k] = sum_n g[b][n] W_fc[n][k]
// with g = dsent * (1 - sent^2) recomputed where it is read (B * nef values).
__global__ __launch_bounds__(256) void bert_sent_fc_bwd_kernel(const float* __restrict__ dsent, const float* __restrict__ sent,
                                                               const float* __restrict__ pooled, const float* __restrict__ wfc,
                                                               float* __restrict__ dwfc, float* __restrict__ dbfc,
                                                               float* __restrict__ dpooled, int B, int C, int nef) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nw = (int64_t)nef * C;
    if (i < nw) {
        const int n = (int)(i / C), k = (int)(i - (int64_t)n * C);
        float acc = 0.f, accb = 0.f;
        for (int b = 0; b < B; ++b) {
            const float sv = sent[b * nef + n];
            const float g = dsent[b * nef + n] * (1.f - sv * sv);
            acc += g * pooled[(int64_t)b * C + k];
            accb += g;
        }
        dwfc[i] += acc;
        if (k == 0) dbfc[n] += accb;
    } else if (i < nw + (int64_t)B * C) {
        const int j = (int)(i - nw), b = j / C, k = j - b * C;
        float acc = 0.f;
        for (int n = 0; n < nef; ++n) {
            const float sv = sent[b * nef + n];
            acc += dsent[b * nef + n] * (1.f - sv * sv) * wfc[(int64_t)n * C + k];
        }
        dpooled[j] = acc;
    }
}

// launch 2 (grid C * C / 256): dW_p[k][j] += sum_b h[b][k] cls[b][j], db_p[k] += sum_b h[b][k],
// h = dpooled * (1 - pooled^2).
__global__ __launch_bounds__(256) void bert_sent_pooler_bwd_kernel(const float* __restrict__ dpooled,
                                                                   const float* __restrict__ pooled,
                                                                   const float* __restrict__ cls, float* __restrict__ dwp,
                                                                   float* __restrict__ dbp, int B, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)C * C) return;
    const int k = (int)(i / C), j = (int)(i - (int64_t)k * C);
    float acc = 0.f, accb = 0.f;
    for (int b = 0; b < B; ++b) {
        const float pv = pooled[b * C + k];
        const float h = dpooled[b * C + k] * (1.f - pv * pv);
        acc += h * cls[b * C + j];
        accb += h;
    }
    dwp[i] += acc;
    if (j == 0) dbp[k] += accb;
}

}  // namespace

extern "C" int sba_bert_words_head_bwd(int dtype, const float* dwords, const float* words, void* dpre, float* dbias, int B,
                                       int L, int nef, void* stream) {
    if (!dwords || !words || !dpre || !dbias || B <= 0 || L <= 0 || L > 32 || nef <= 0 || nef % 64 != 0) return SBA_E_ARG;
    SBA_DISPATCH(dtype, SBA_LAUNCH((bert_words_head_bwd_kernel<T>), dim3(nef / 64), dim3(256), 0, (hipStream_t)stream,
                                   dwords, words, (T*)dpre, dbias, B, L, nef));
    return SBA_CHECK_LAUNCH();
}

extern "C" int sba_bert_sent_head_bwd(const float* dsent, const float* sent, const float* pooled, const float* cls,
                                      const float* w_fc, float* dpooled, float* dw_fc, float* db_fc, float* dw_pool,
                                      float* db_pool, int B, int C, int nef, void* stream) {
    if (!dsent || !sent || !pooled || !cls || !w_fc || !dpooled || !dw_fc || !db_fc || !dw_pool || !db_pool) return SBA_E_ARG;
    if (B <= 0 || B > 64 || C <= 0 || C % 64 != 0 || nef <= 0 || nef % 64 != 0) return SBA_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n1 = (int64_t)nef * C + (int64_t)B * C, n2 = (int64_t)C * C;
    SBA_LAUNCH(bert_sent_fc_bwd_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, dsent, sent, pooled, w_fc,
               dw_fc, db_fc, dpooled, B, C, nef);
    if (SBA_CHECK_LAUNCH() != SBA_OK) return SBA_E_LAUNCH;
    SBA_LAUNCH(bert_sent_pooler_bwd_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, dpooled, pooled, cls,
               dw_pool, db_pool, B, C);
    return SBA_CHECK_LAUNCH();
}
