"""Float64 reference of the Differentiable Augmentation kernels (csrc/diffaug.hip: sba_diffaug_fwd / sba_diffaug_bwd), from
the definitions in include/sbagan_hip.h, with a per-element error bound, and an f32 emulation of the kernels' operation
chain (numpy float32, one rounding per operation) that the CPU tests mutate.

Per image of side S, parameters u0..u6 (float32 uniforms in [0, 1)), flags 1 color | 2 translation | 4 cutout:
    b = u0 - 0.5, s = 2 u1, k = u2 + 0.5                                    (float64 here, from the float32 u)
    color        x1 = x + b;  m = mean_c x1;  x2 = (x1 - m) s + m;  M = mean_chw(x) + b;  x3 = (x2 - M) k + M
    translation  out[i][j] = in[i + ty][j + tx] inside the image, +0 elsewhere
    cutout       output rows / columns [o - cut // 2, o - cut // 2 + cut) intersected with the image are +0
The integer maps (ty, tx, oy, ox) are taken with numpy.float32 products, as the kernel takes them, so both agree on
every u -- including u * n rounding up to n, which the min() catches.

The error bound of an element is  c * EPS32 * A  with EPS32 = 2^-24 (the unit roundoff of float32) and A the sum of the
absolute intermediate terms of that element in float64.  c is COUNTED from the kernel's chain, not measured:

forward, per live element (every operation rounds once, relative error <= EPS32; gains: |s| <= 2, |1 - s| <= 1, k <= 1.5,
|1 - k| <= 0.5).  Error sources -> (size) x (gain to x3):
    b = u0 - 0.5f           EPS32 |b|       reaches x3 through x1 of the element (gain s k <= 3), through m (|1 - s| k <= 1.5)
                                            and through M (|1 - k| <= 0.5):                             5.0 |b|
    x1 = x + b              EPS32 |x1| <= EPS32 (|x| + |b|), gain s k + |1 - s| k / 3 <= 3.5:            3.5 (|x| + |b|)
    m = ((x1_0 + x1_1) + x1_2) * (1/3 rounded): two additions, one product, one rounded constant, and the x1 roundings
                            of the pixel's three channels: 5 EPS32 mabs, mabs = mean_c |x1_c| (<= mean_c |x_c| + |b|),
                            gain |1 - s| k <= 1.5:                                                        7.5 mabs
    d = x1 - m              EPS32 |d|,  gain s k <= 3:                                                    3.0 |d|
    d s                     EPS32 |d s|, gain k:                                                          1.5 |d s|
    x2 = d s + m            EPS32 |x2|, gain k:                                                           1.5 |x2|
    M0 = float32(sum64 / 3 S^2)   EPS32 |M0|;  M = M0 + b  EPS32 |M|;  gain |1 - k|:                      0.5 (|M0| + |M|)
    e = x2 - M              EPS32 |e|, gain k:                                                            1.5 |e|
    k = u2 + 0.5f and e k   2 EPS32 |e k|:                                                               2.0 |e k|
    x3 = e k + M            EPS32 |x3|:                                                                   1.0 |x3|
  With A = |x| + |b| + mabs + |d| + |d s| + |x2| + |M0| + |M| + |e| + |e k| + |x3| the largest coefficient is the one of
  |b|: 5.0 + 3.5 = 8.5 (mabs is carried with its own |b| inside).  One more for the second-order terms and the float64
  accumulation (3 S^2 additions at 2^-53 each): C_FWD = 10.  A fused multiply-add only removes roundings.

backward, per element:  mg = ((G_0 + G_1) + G_2) * (1/3),  q = s G + (1 - s) mg,  dx = k q + (1 - k) Sg,  Sg = float32(sum64 / 3 S^2)
    mg                      4 EPS32 gabs (gabs = mean_c |G_c|), gain |1 - s| k <= 1.5:                    6.0 gabs
    1 - s                   EPS32 |1 - s| |mg|, gain k:                                                   1.5 |(1 - s) mg|
    s G                     EPS32 |s G|, gain k:                                                          1.5 |s G|
    (1 - s) mg              EPS32, gain k:                                                                1.5 |(1 - s) mg|
    q                       EPS32 |q|, gain k:                                                            1.5 |q|
    k (rounded) and k q     2 EPS32 |k q|:                                                                2.0 |k q|
    1 - k (k's rounding: 1.5 EPS32; its own: EPS32 |1 - k| <= 0.5 EPS32), times |Sg|:                     2.0 |Sg|
    Sg                      EPS32 |Sg|, gain |1 - k| <= 0.5:                                              0.5 |Sg|
    (1 - k) Sg              EPS32:                                                                        1.0 |(1 - k) Sg|
    dx                      EPS32 |dx|:                                                                   1.0 |dx|
  With A = gabs + |s G| + |(1 - s) mg| + |q| + |k q| + |Sg| + |(1 - k) Sg| + |dx| the largest coefficient is 6.0 (gabs);
  |(1 - s) mg| collects 3.0, |Sg| 2.5.  One more for second order and the float64 sum: C_BWD = 7.

With color off nothing is computed: the kernels copy bits, and the tests compare with torch.equal."""
import numpy as np

EPS32 = 2.0 ** -24
C_FWD = 10.0
C_BWD = 7.0
COLOR, TRANSLATION, CUTOUT = 1, 2, 4
BELOW_ONE = np.nextafter(np.float32(1), np.float32(0))      # the largest float32 below 1


def _draw(u, n):
    """min(int(u * n), n - 1) with the product in float32"""
    return min(int(np.float32(u) * np.float32(n)), n - 1)


def shift_of(S):
    return int(S * 0.125 + 0.5)


def cut_of(S):
    return int(S * 0.5 + 0.5)


def int_maps(row, S, flags, shift=None):
    """(ty, tx, oy, ox) of one parameter row; parts that are off give ty = tx = 0 and oy = ox = None"""
    ty = tx = 0
    oy = ox = None
    if flags & TRANSLATION:
        sh = shift_of(S) if shift is None else shift
        ty, tx = _draw(row[3], 2 * sh + 1) - sh, _draw(row[4], 2 * sh + 1) - sh
    if flags & CUTOUT:
        cut = cut_of(S)
        oy, ox = _draw(row[5], S + 1 - cut % 2), _draw(row[6], S + 1 - cut % 2)
    return ty, tx, oy, ox


def cut_mask(S, oy, ox):
    """bool [S][S], True where cut: rows [oy - cut // 2, oy - cut // 2 + cut) and the same columns, inside the image"""
    m = np.zeros((S, S), dtype=bool)
    if oy is None:
        return m
    cut = cut_of(S)
    r0, c0 = oy - cut // 2, ox - cut // 2
    m[max(r0, 0):max(min(r0 + cut, S), 0), max(c0, 0):max(min(c0 + cut, S), 0)] = True
    return m


def gather_plan(row, S, flags, shift=None, cut_first=False):
    """For every OUTPUT pixel: (live bool [S][S], source rows [S][S], source columns [S][S]).  live: the source lies in the
    image and the output pixel is not cut.  cut_first (a mutation): the cut rectangle is applied in source coordinates."""
    ty, tx, oy, ox = int_maps(row, S, flags, shift)
    ii, jj = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    si, sj = ii + ty, jj + tx
    inside = (si >= 0) & (si < S) & (sj >= 0) & (sj < S)
    sic, sjc = np.clip(si, 0, S - 1), np.clip(sj, 0, S - 1)
    cm = cut_mask(S, oy, ox)
    cut = cm[sic, sjc] if cut_first else cm
    return inside & ~cut, sic, sjc


def _scalars(row, dtype):
    """b, s, k in `dtype` arithmetic from the float32 uniforms"""
    u = np.asarray(row, dtype=np.float32).astype(dtype)
    return u[0] - dtype(0.5), dtype(2) * u[1], u[2] + dtype(0.5)


def forward(x, params, flags):
    """x [n][3][S][S], params [n][8] float32 -> (out float64, A float64, live bool [n][S][S]).  A is 0 where not live or
    with color off (those elements are exact)."""
    x = np.asarray(x, dtype=np.float64)
    n, _, S, _ = x.shape
    out, A = np.zeros_like(x), np.zeros_like(x)
    lives = np.zeros((n, S, S), dtype=bool)
    for a in range(n):
        live, si, sj = gather_plan(params[a], S, flags)
        lives[a] = live
        g = x[a][:, si, sj]
        if flags & COLOR:
            b, s, k = _scalars(params[a], np.float64)
            x1 = g + b
            m = x1.mean(0, keepdims=True)
            mabs = np.abs(x1).mean(0, keepdims=True)
            d = x1 - m
            x2 = d * s + m
            M0 = x[a].mean()
            M = M0 + b
            e = x2 - M
            x3 = e * k + M
            g = x3
            A[a] = (np.abs(x[a][:, si, sj]) + abs(b) + mabs + np.abs(d) + np.abs(d * s) + np.abs(x2) + abs(M0) + abs(M)
                    + np.abs(e) + np.abs(e * k) + np.abs(x3)) * live
        out[a] = g * live
    return out, A, lives


def scatter_G(dout_a, row, S, flags, shift=None, cut_first=False):
    """G [3][S][S] in source coordinates: the output gradient of every live output pixel at its source pixel, 0 elsewhere
    (the gather is one to one on its live part, so plain assignment scatters it)"""
    live, si, sj = gather_plan(row, S, flags, shift, cut_first)
    G = np.zeros_like(dout_a)
    G[:, si[live], sj[live]] = dout_a[:, live]
    return G


def backward(dout, params, flags):
    """dout [n][3][S][S] -> (dx float64, A float64); A is 0 with color off"""
    dout = np.asarray(dout, dtype=np.float64)
    n, _, S, _ = dout.shape
    dx, A = np.zeros_like(dout), np.zeros_like(dout)
    for a in range(n):
        G = scatter_G(dout[a], params[a], S, flags)
        if not flags & COLOR:
            dx[a] = G
            continue
        _, s, k = _scalars(params[a], np.float64)
        mg = G.mean(0, keepdims=True)
        gabs = np.abs(G).mean(0, keepdims=True)
        q = s * G + (1 - s) * mg
        Sg = G.sum() / (3 * S * S)
        dx[a] = k * q + (1 - k) * Sg
        A[a] = (gabs + np.abs(s * G) + np.abs((1 - s) * mg) + np.abs(q) + np.abs(k * q) + abs(Sg) + abs((1 - k) * Sg)
                + np.abs(dx[a]))
    return dx, A


def bound_forward(A):
    return C_FWD * EPS32 * A


def bound_backward(A):
    return C_BWD * EPS32 * A


# ---- float32 emulation of the kernels' chain, with the mutations the CPU test must see fail ------------------------
MUTATIONS = ('swap_s_k', 'contrast_per_channel', 'shift_off_by_one', 'drop_sum_term', 'cutout_before_translation')
F = np.float32
THIRD = F(1) / F(3)


def chain_forward(x, params, flags, mutation=None):
    """the forward kernel's operations in float32, one numpy operation per rounding; returns float32"""
    x = np.asarray(x, dtype=np.float32)
    n, _, S, _ = x.shape
    out = np.zeros_like(x)
    shift = shift_of(S) + 1 if mutation == 'shift_off_by_one' else None
    for a in range(n):
        live, si, sj = gather_plan(params[a], S, flags, shift, cut_first=mutation == 'cutout_before_translation')
        g = x[a][:, si, sj]
        if flags & COLOR:
            b, s, k = _scalars(params[a], np.float32)
            if mutation == 'swap_s_k':
                s, k = k, s
            M0 = F(x[a].astype(np.float64).sum() / (3 * S * S))
            if mutation == 'contrast_per_channel':
                M0 = (x[a].astype(np.float64).sum((1, 2)) / (S * S)).astype(np.float32).reshape(3, 1, 1)
            M = M0 + b
            x1 = g + b
            m = ((x1[0] + x1[1]) + x1[2]) * THIRD
            sat = (x1 - m) * s + m
            g = (sat - M) * k + M
        out[a] = np.where(live, g, F(0))
    return out


def chain_backward(dout, params, flags, mutation=None):
    dout = np.asarray(dout, dtype=np.float32)
    n, _, S, _ = dout.shape
    dx = np.zeros_like(dout)
    shift = shift_of(S) + 1 if mutation == 'shift_off_by_one' else None
    for a in range(n):
        G = scatter_G(dout[a], params[a], S, flags, shift, cut_first=mutation == 'cutout_before_translation')
        if not flags & COLOR:
            dx[a] = G
            continue
        _, s, k = _scalars(params[a], np.float32)
        if mutation == 'swap_s_k':
            s, k = k, s
        Sg = F(G.astype(np.float64).sum() / (3 * S * S))
        tail = (F(1) - k) * Sg
        if mutation == 'drop_sum_term':
            tail = F(0)
        mg = ((G[0] + G[1]) + G[2]) * THIRD
        dx[a] = k * (s * G + (F(1) - s) * mg) + tail
    return dx


def corner_params(S, rng, n):
    """n parameter rows (n >= 8): the corners first -- ty, tx = -shift and +shift; oy, ox = 0 and their maximum (the cut
    rectangle partly outside the image); u0..u2 = 0 and the largest float32 below 1 -- then uniform rows"""
    p = rng.random_sample((n, 8)).astype(np.float32)
    lo, hi = np.float32(0), BELOW_ONE
    p[0, 3:5] = lo, lo                  # ty = tx = -shift
    p[1, 3:5] = hi, hi                  # ty = tx = +shift
    p[2, 3:5] = lo, hi
    p[3, 5:7] = lo, lo                  # oy = ox = 0
    p[4, 5:7] = hi, hi                  # oy = ox = max
    p[5, 5:7] = hi, lo
    p[6, 0:3] = lo, lo, lo              # b = -0.5, s = 0, k = 0.5
    p[7, 0:3] = hi, hi, hi
    p[0, 5:7] = hi, hi                  # corners of two parts together
    p[1, 5:7] = lo, lo
    return p
