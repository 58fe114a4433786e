/*
 * sbagan_hip_ext.h -- the second header of libsbagan_hip.so's C ABI: entry points added after sbagan_hip.h was pinned
 * by its tests (tests/test_abi_cpu.py counts its declarations).  Same conventions, same few declaration forms, read by
 * the same parser (sbagan/abi.py: EXT_CONSTANTS, EXT_STRUCTS, EXT_DECLS; a name declared in both headers raises).
 */
#ifndef SBAGAN_HIP_EXT_H
#define SBAGAN_HIP_EXT_H

#include <stdint.h>

#include "sbagan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Gated Differentiable Augmentation: sba_diffaug_fwd / sba_diffaug_bwd (sbagan_hip.h) with PER-IMAGE flags, for an
 * augmentation probability that lives in device memory (csrc/diffaug.hip, sbagan/ops.py: DiffAugGatedFn).
 * Images, params, flags, S, workspace: as for the ungated pair.
 * sba_diffaug_gated_fwd: image n is transformed with f_n = flags & g_n; bit b of g_n (0 color, 1 translation, 2 cutout)
 *   is set iff gates[n][b] < *p_dev, strictly.  gates [n][4] f32: three uniforms in [0, 1), column 3 unused.  p_dev: ONE
 *   f32 in device memory, read when the kernel runs.  A NaN p and p = 0 apply nothing, p >= 1 applies everything.
 *   applied [n] int32 = f_n is written as well.
 * sba_diffaug_gated_bwd: dx [n] for dout [n] with f_n = applied[n] & flags: `applied` is an INPUT, not re-derived from
 *   gates and p, so the backward stays that of its forward whatever has happened to p since.  A value outside 0..7 is
 *   masked with flags, never used as an address.
 * Image n of out / dx has the same bits as sba_diffaug_fwd / _bwd with flags = f_n on that image alone (the same kernel
 * body; the per-image sums never mix images and their partition depends on S alone); f_n = 0: a bit-exact copy.  The
 * per-image sum is skipped, before any load, for an image whose color bit is off.  No atomics; two calls give the
 * same bits.
 * SBA_E_ARG before any launch, nothing written: as for the ungated pair, and on a NULL gates / p_dev / applied or one
 * that is not 4-byte aligned. */
int sba_diffaug_gated_fwd(const float* real, int nr, const float* fake, int nf, const float* params,
                          const float* gates, const float* p_dev, float* out, int32_t* applied, int S, int flags,
                          void* workspace, void* stream);
int sba_diffaug_gated_bwd(const float* dout, int n, const float* params, const int32_t* applied, float* dx, int S,
                          int flags, void* workspace, void* stream);

/* The adaptive-augmentation controller (Karras et al., NeurIPS 2020, "Training GANs with Limited Data"; csrc/ada.hip,
 * sbagan/diffaug.py).  State per discriminator, in device memory: p [nD] f32 (the augmentation
 * probability), rt [nD] f32 (the last overfitting read-out r_t = E[sign(D(real) - 0.5)]), counters [nD][4] int32
 * (pos, neg, cnt, calls).  Neither entry point synchronises with the host, uses atomics or needs a workspace; both
 * are graph-capturable.
 * sba_ada_count: ONE workgroup adds to counters_row (4 int32): pos += #(prob > 0.5), neg += #(prob < 0.5), cnt += n,
 *   calls += 1, over prob [n] f32.  Exactly 0.5 and NaN count in cnt only.  Integer sums: exact in any order.  The row
 *   must be written by this launch alone while it runs.  SBA_E_ARG unless 1 <= n <= 2^20 and both pointers are non-NULL
 *   and 4-byte aligned.
 * sba_ada_adjust: one launch, one thread per row.  For a row with calls >= interval:
 *     cnt == 0: rt = 0, p unchanged;  else rt = (float)(pos - neg) / (float)cnt (one IEEE division) and
 *     p = min(max(p', 0), p_max) with p' = p + adjust when rt > target, p - adjust when rt < target, p otherwise;
 *   then the row's four counters are zeroed.  Rows below the interval are untouched.
 *   SBA_E_ARG unless 1 <= nD <= 8, 1 <= interval <= 1024, 0 <= p_max <= 1, adjust >= 0 and finite, target not NaN, and
 *   all pointers non-NULL and 4-byte aligned. */
int sba_ada_count(const float* prob, int n, int32_t* counters_row, void* stream);
int sba_ada_adjust(float* p, float* rt, int32_t* counters, int nD, int interval, float target, float adjust,
                   float p_max, void* stream);

/* Geometric augmentation: x-flip, 90-degree rotation, isotropic scaling and rotation of the images a discriminator sees
 * (Karras et al., NeurIPS 2020; csrc/geoaug.hip, sbagan/geoaug.py, sbagan/ops.py: GeoAugFn).  Parts, as
 * bits of their OWN namespace (not sba_diffaug_fwd's): 1 flip, 2 rot90, 4 scale, 8 rotate.  Per image the parts compose
 * into one matrix M [m00 m01 m10 m11] about the centre c = (S - 1) / 2, pixel centres on the integers, (x, y) columns:
 *     src - c = M (dst - c),   M = F . Q^k . R(theta) / s,
 *     F = [[-1, 0], [0, 1]] if flipped else I,  Q = [[0, -1], [1, 0]],  R(t) = [[cos t, -sin t], [sin t, cos t]];
 * a part that is off contributes the identity.  All parts fix the centre: M does not depend on S.
 * Sampling is bilinear with zero padding: out[ch, d] = sum over pixels q of x[ch, q] hat(sx - qx) hat(sy - qy),
 * hat(t) = max(0, 1 - |t|).
 * sba_geoaug_prepare: ONE launch, one thread per row, for N rows: uniforms [N][8] f32 in [0, 1) -> mats [N][4] f32 and
 *   applied [N] int32 (the parts that were on).  flip: on a row whose part is on, F is drawn: flipped iff u0 >= 0.5.
 *   rot90: k = min(int(4 u1), 3).  scale: s = 2^(0.2 z), z = sqrt(-2 ln(1 - u2)) cos(2 pi u3) clamped to [-3, 3], so
 *   2^-0.6 <= s <= 2^0.6.  rotate: theta = pi (2 u4 - 1).  u5..u7 unused.
 *   Part b of row r is on iff bit b of `flags` is set and (gates == NULL or gates[r][b] < p_dev[r / rows_per_p],
 *   strictly): nothing when p is NaN or 0, everything when p >= 1.  gates [N][4] f32 uniforms; p_dev f32 in device memory,
 *   at least ceil(N / rows_per_p) values, read when the kernel runs; both ignored (may be NULL) when gates is NULL.
 *   SBA_E_ARG unless 1 <= N <= 2^20, 1 <= flags <= 15, uniforms / applied non-NULL and 4-byte aligned, mats non-NULL and
 *   16-byte aligned, and with gates: gates and p_dev 4-byte aligned, p_dev non-NULL, rows_per_p >= 1.
 * sba_geoaug_fwd: out [nr + nf][3][S][S] = the warp of [real | fake] (in place of a concatenation), image n by mats[n];
 *   nr = 0 or nf = 0 allowed (the pointer of an empty half is ignored).  An image whose M is exactly the identity is copied.
 *   With flip / rot90 alone (entries 0, +-1) the output is a permutation of the input, bit for bit.
 * sba_geoaug_bwd: dx [n][3][S][S] = the exact adjoint, dx[ch, q] = sum over d of dout[ch, d] hat(sx(d) - qx) hat(sy(d) - qy),
 *   gathered: no atomics, no workspace, f32 sums in a fixed order -- two calls give the same bits.  An input pixel looks
 *   at the output pixels of the bounding box of M^-1 ([qx - 1, qx + 1] x [qy - 1, qy + 1]), at most 7 per axis: exact for
 *   every M sba_geoaug_prepare writes; for a matrix that shrinks the image further (singular values below 2^-0.6) the
 *   window is cut there and the result is no longer the adjoint.  A NaN matrix reads nothing.
 * Both: S even, 8..4096; 1 <= number of images <= 65535; images, out / dx and mats 16-byte aligned; SBA_E_ARG before any
 * launch otherwise, nothing written.  No host synchronisation; graph-capturable. */
int sba_geoaug_prepare(const float* uniforms, const float* gates, const float* p_dev, int rows_per_p, int N, int flags,
                       float* mats, int32_t* applied, void* stream);
int sba_geoaug_fwd(const float* real, int nr, const float* fake, int nf, const float* mats, float* out, int S,
                   void* stream);
int sba_geoaug_bwd(const float* dout, int n, const float* mats, float* dx, int S, void* stream);

/* The truncation trick in W (Karras et al., CVPR 2019; csrc/truncation.hip, sbagan/truncation.py): the
 * mean style of a mapping network and the pull of a style towards it.  Neither entry point synchronises with the host
 * or uses atomics; both are graph-capturable.
 * sba_style_mean: the column means of w [n][D] f32, in float64, in an order that is part of the contract.  For column d:
 *     P_c = the float64 sum of rows 256 c .. min(256 c + 256, n) - 1, added in ascending row order;
 *     T   = the float64 sum of the P_c, in ascending c;        (every sum starts from +0.0)
 *     mean64[d] = T / n, one IEEE division;   mean32[d] = (float) mean64[d], round to nearest.
 *   The result does not depend on the grid; two calls give the same bits; a NaN or Inf in a column reaches that column
 *   only.  One launch for the partials and one for the tail; a single launch when n <= 256.
 *   workspace: at least ceil(n / 256) * D * 8 bytes, 8-byte aligned; may be NULL when n <= 256.
 *   SBA_E_ARG unless 1 <= n <= 2^20, 1 <= D <= 4096, w and mean32 non-NULL and 4-byte aligned, mean64 non-NULL and 8-byte
 *   aligned, and workspace as stated.
 * sba_style_truncate: out[r][d] = w_avg[d] + psi * (w[r][d] - w_avg[d]) over w [n][D], w_avg [D], as three separately
 *   rounded f32 operations -- subtract, multiply, add; never a fused multiply-add.  psi == 1.0f exactly: every row is
 *   copied bit for bit (the formula does not give w back in floating point).  out == w (in place) is allowed.
 *   SBA_E_ARG unless psi is finite, 1 <= n <= 2^20, 1 <= D <= 4096, and all pointers are non-NULL and 4-byte aligned.
 * Both: SBA_E_ARG before any launch, nothing written. */
int sba_style_mean(const float* w, int n, int D, double* mean64, float* mean32, void* workspace, void* stream);
int sba_style_truncate(const float* w, const float* w_avg, float psi, float* out, int n, int D, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SBAGAN_HIP_EXT_H */
