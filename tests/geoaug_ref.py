"""--geoaug restated in float64 numpy, with the error bounds its tests hold the HIP unit (csrc/geoaug.hip) to.

The definition (include/sbagan_hip_ext.h).  Per image one matrix about the centre c = (S - 1) / 2, pixel centres on the
integers, (x, y) columns:  src - c = M (dst - c),  M = F . Q^k . R(theta) / s,  F = diag(-1, 1) if flipped,
Q = [[0, -1], [1, 0]], R(t) = [[cos t, -sin t], [sin t, cos t]]; from one row of uniforms: flipped iff u0 >= 0.5,
k = min(int(4 u1), 3), s = 2^(0.2 z) with z = sqrt(-2 ln(1 - u2)) cos(2 pi u3) clamped to [-3, 3], theta = pi (2 u4 - 1).
Sampling is bilinear with zero padding: out[ch, d] = sum_q x[ch, q] hat(sx - qx) hat(sy - qy), hat(t) = max(0, 1 - |t|);
the backward is its adjoint, dx[ch, q] = sum_d dout[ch, d] hat(sx(d) - qx) hat(sy(d) - qy).

matrices() is f64 throughout, except that 1 - u2 is taken as its f32-rounded value: it is the one input rounding that ln
amplifies without bound (u2 -> 0), and every f32 evaluation has it.  forward() and backward() take matrices as given
(the tests hand them the kernel's own f32 matrices, so the warp is tested on exactly known inputs).

THE BOUNDS.  None is taken from the HIP kernels' output.  Each is a first-order model of the f32 evaluation with one
constant, and the constant is 4 x the largest ratio |f32 emulation - f64 reference| / model seen on the CPU (the
emulate_* functions below evaluate the formulas in numpy float32, operation by operation, no fused multiply-add; the
factor 4 is for a device whose sinf / cosf / logf / exp2f and fused multiply-adds round differently).  measure() redoes
the measurement; tests/test_geoaug_cpu.py runs it and holds the constants to it.

  matrix entries (MATRIX_BOUND, absolute).  |entry| <= 2^0.6.  Errors: the f32 angle 2 pi u3 (up to 2 pi) is off by up
    to 2^-22, cos by as much, z = r cos by r 2^-22 with r <= 5.8 where |z| <= 3 can still hold, and
    d s / d z = 0.2 ln 2 s <= 0.21: 3e-7; theta = pi (2 u4 - 1) in f32 is off by 2^-23, the entry by 2^-23 s = 1.8e-7; the
    roundings of logf, sqrtf, exp2f and the products add a few 2^-24 each.  Measured over 2 x 10^5 random rows (and the
    edge rows of the tests): 3.96e-7, taken as 4.0e-7.  MATRIX_BOUND = 4 x that.
  forward (forward_bound, per output element).  The sampling position is src = c + M (d - c) with |d - c| < S / 2 and
    row sums of |M| <= 2^0.6 sqrt 2 = 2.15: its f32 value is off by about S 2^-24 x 2.15 / 2 + ulp(S) <= S 2^-23 px.  The
    bilinear interpolant is continuous and piecewise linear in the position, with a slope per axis of at most the
    spread (max - min) of the taps of the cell the position is in -- or of a neighbouring cell when the rounding carries
    it over an integer.  So with `spread` and `maxabs` taken over the 4 x 4 pixels around the position (zeros where
    they are outside the image):   |error| <= FWD_K (S 2^-23 spread + 2^-23 maxabs),
    the second term for the roundings of the three lerps (each result is at most maxabs).  Measured over SHAPES: ratio
    0.453, taken as 0.46.
  backward (backward_bound, per input element).  Each weight hat hat is off by at most the two coordinate errors,
    2 S 2^-23, plus roundings of 2^-23; the sum has at most 49 terms.  With `mass` = sum of |dout| over the output pixels of
    the bounding box of M^-1 applied to the 2 x 2 square around the input pixel, padded by two pixels:
    |error| <= BWD_K (S + 4) 2^-23 mass.  Measured over SHAPES: ratio 0.342, taken as 0.35.
  Where the model is zero -- a constant neighbourhood, an empty box -- the bound asks for the exact value."""
import numpy as np

FLIP, ROT90, SCALE, ROTATE = 1, 2, 4, 8
NAMES = {'flip': FLIP, 'rot90': ROT90, 'scale': SCALE, 'rotate': ROTATE}
BELOW_ONE = np.nextafter(np.float32(1), np.float32(0))
S_MAX = 2.0 ** 0.6                      # the largest scale factor (z = 3)

MEASURED_MATRIX, MEASURED_FWD, MEASURED_BWD = 4.0e-7, 0.46, 0.35      # measure(), see above
MATRIX_BOUND = 4 * MEASURED_MATRIX
FWD_K = 4 * MEASURED_FWD
BWD_K = 4 * MEASURED_BWD

_Q = np.array([[0.0, -1.0], [1.0, 0.0]])
_QK = np.stack([np.linalg.matrix_power(_Q, k) for k in range(4)])


def parts_on(flags, n, gates=None, p=None, rows_per_p=None):
    """int32 [n]: the parts applied to each row -- bit b of flags, and (no gates, or gates[r][b] < p[r // rows_per_p])"""
    on = np.full(n, int(flags), dtype=np.int32)
    if gates is not None:
        pr = np.asarray(p, dtype=np.float32)[np.arange(n) // int(rows_per_p)]
        with np.errstate(invalid='ignore'):
            passed = np.asarray(gates, dtype=np.float32) < pr[:, None]           # (a NaN p: False)
        on &= (passed.astype(np.int32) << np.arange(4)).sum(1).astype(np.int32)
    return on


def draws(u):
    """(flipped, k, s, theta) of rows u [n][8] of f32 uniforms, in f64"""
    u = np.asarray(u, dtype=np.float32)
    flipped = u[:, 0] >= np.float32(0.5)
    k = np.minimum((4.0 * u[:, 1].astype(np.float64)).astype(np.int64), 3)
    one_minus = (np.float32(1) - u[:, 2]).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        z = np.sqrt(-2.0 * np.log(one_minus)) * np.cos(2.0 * np.pi * u[:, 3].astype(np.float64))
    z = np.clip(np.nan_to_num(z, nan=0.0), -3.0, 3.0)
    return flipped, k, 2.0 ** (0.2 * z), np.pi * (2.0 * u[:, 4].astype(np.float64) - 1.0)


def compose(flipped, k, s, theta, on, order='FQR'):
    """f64 [n][4] = (m00, m01, m10, m11) of M = F . Q^k . R(theta) / s, each part the identity where its bit of `on` is
    off.  order 'QRF' is the MUTATION that flips after the rotation."""
    n = len(on)
    eye = np.broadcast_to(np.eye(2), (n, 2, 2))
    th = np.where(on & ROTATE, theta, 0.0)
    R = np.stack([np.stack([np.cos(th), -np.sin(th)], -1), np.stack([np.sin(th), np.cos(th)], -1)], -2)
    R = np.where((on & ROTATE).astype(bool)[:, None, None], R, eye)          # (theta = 0 gives it anyway; keep it exact)
    Qk = _QK[np.where(on & ROT90, k, 0)]
    F = np.where(((on & FLIP) != 0) & flipped, -1.0, 1.0)[:, None, None] * np.array([[1.0, 0.0], [0.0, 0.0]]) \
        + np.array([[0.0, 0.0], [0.0, 1.0]])
    M = F @ Qk @ R if order == 'FQR' else Qk @ R @ F
    M = M / np.where(on & SCALE, s, 1.0)[:, None, None]
    return M.reshape(n, 4)


def matrices(u, flags, gates=None, p=None, rows_per_p=None):
    """(mats f64 [n][4], applied int32 [n]) of sba_geoaug_prepare"""
    on = parts_on(flags, len(u), gates, p, rows_per_p)
    return compose(*draws(u), on), on


def emulate_matrices(u, on, mutate=None):
    """the formulas evaluated in float32, operation by operation.  mutate: 'theta' (negated), 'k' (off by one),
    's' (inverted), 'flip_last' (flip applied after the rotation) -- each must break MATRIX_BOUND."""
    f = np.float32
    u = np.asarray(u, dtype=f)
    flipped = u[:, 0] >= f(0.5)
    k = np.minimum((f(4) * u[:, 1]).astype(np.int64), 3)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.sqrt(f(-2) * np.log(f(1) - u[:, 2]))
        z = r * np.cos(f(2 * np.pi) * u[:, 3])
    z = np.clip(np.nan_to_num(z, nan=0.0), f(-3), f(3)).astype(f)
    s = np.exp2(f(0.2) * z).astype(f)
    theta = (f(np.pi) * (f(2) * u[:, 4] - f(1))).astype(f)
    if mutate == 'theta':
        theta = -theta
    if mutate == 'k':
        k = (k + 1) % 4
    if mutate == 's':
        s = (f(1) / s).astype(f)
    n = len(on)
    rot = (on & ROTATE) != 0
    c, sn = np.where(rot, np.cos(theta), f(1)).astype(f), np.where(rot, np.sin(theta), f(0)).astype(f)
    A = np.stack([c, -sn, sn, c], -1).reshape(n, 2, 2).astype(np.float64)     # (signed permutations below are exact)
    Qk = _QK[np.where(on & ROT90, k, 0)]
    F = np.where(((on & FLIP) != 0) & flipped, -1.0, 1.0)[:, None, None] * np.array([[1.0, 0.0], [0.0, 0.0]]) \
        + np.array([[0.0, 0.0], [0.0, 1.0]])
    M = (F @ Qk @ A if mutate != 'flip_last' else Qk @ A @ F).astype(f)
    return (M / np.where(on & SCALE, s, f(1)).astype(f)[:, None, None]).astype(f).reshape(n, 4)


# ---- the warp ---------------------------------------------------------------------------------------------------------
def _positions(m, S, dtype):
    """(sx, sy) [S][S] of one matrix m (4 values), evaluated in `dtype` in the kernel's order of operations"""
    t = dtype
    c = t(0.5) * t(S - 1)
    ay, ax = np.meshgrid(np.arange(S).astype(t) - c, np.arange(S).astype(t) - c, indexing='ij')
    m = np.asarray(m, dtype=t)
    sx = ((m[0] * ax).astype(t) + (m[1] * ay).astype(t)).astype(t) + c
    sy = ((m[2] * ax).astype(t) + (m[3] * ay).astype(t)).astype(t) + c
    return sx.astype(t), sy.astype(t)


def _taps(s, S):
    """(i0, f, ok): floor, fraction and whether any tap of the axis can be inside the image"""
    with np.errstate(invalid='ignore'):
        fl = np.floor(s)
        ok = (fl >= -1) & (fl <= S - 1)
    fl = np.where(ok, fl, 0)
    return fl.astype(np.int64), (np.where(ok, s, 0) - fl).astype(s.dtype), ok


def _gather(img, yy, xx, S):
    """img [C][S][S] at integer positions, zero outside the image"""
    inside = (yy >= 0) & (yy < S) & (xx >= 0) & (xx < S)
    v = img[:, np.clip(yy, 0, S - 1), np.clip(xx, 0, S - 1)]
    return np.where(inside, v, img.dtype.type(0))


def forward(x, mats):
    """f64 [n][C][S][S]: out[ch, d] = sum over the four taps q of x[ch, q] hat(sx - qx) hat(sy - qy)"""
    x = np.asarray(x, dtype=np.float64)
    S = x.shape[-1]
    out = np.zeros_like(x)
    for n in range(x.shape[0]):
        sx, sy = _positions(np.asarray(mats[n], dtype=np.float64), S, np.float64)
        x0, fx, okx = _taps(sx, S)
        y0, fy, oky = _taps(sy, S)
        ok = okx & oky
        for j, wy in ((0, 1 - fy), (1, fy)):
            for i, wx in ((0, 1 - fx), (1, fx)):
                out[n] += np.where(ok, _gather(x[n], y0 + j, x0 + i, S) * (wx * wy), 0.0)
    return out


def backward(g, mats):
    """f64 [n][C][S][S]: the adjoint, scattered tap by tap with the weights of forward()"""
    g = np.asarray(g, dtype=np.float64)
    S = g.shape[-1]
    dx = np.zeros_like(g)
    for n in range(g.shape[0]):
        sx, sy = _positions(np.asarray(mats[n], dtype=np.float64), S, np.float64)
        x0, fx, okx = _taps(sx, S)
        y0, fy, oky = _taps(sy, S)
        for j, wy in ((0, 1 - fy), (1, fy)):
            for i, wx in ((0, 1 - fx), (1, fx)):
                yy, xx = y0 + j, x0 + i
                live = okx & oky & (yy >= 0) & (yy < S) & (xx >= 0) & (xx < S)
                for ch in range(g.shape[1]):
                    np.add.at(dx[n, ch], (yy[live], xx[live]), (g[n, ch] * wx * wy)[live])
    return dx


def emulate_forward(x, mats, mutate=None):
    """the forward kernel in numpy float32: positions, taps, two lerps along x and one along y.  mutate 'axis': the x
    lerps take the y fraction and the y lerp the x fraction (a tap's weight from the wrong axis)."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    S = x.shape[-1]
    out = np.zeros_like(x)
    for n in range(x.shape[0]):
        sx, sy = _positions(np.asarray(mats[n], dtype=f), S, f)
        x0, fx, okx = _taps(sx, S)
        y0, fy, oky = _taps(sy, S)
        if mutate == 'axis':
            fx, fy = fy, fx
        v00, v01 = _gather(x[n], y0, x0, S), _gather(x[n], y0, x0 + 1, S)
        v10, v11 = _gather(x[n], y0 + 1, x0, S), _gather(x[n], y0 + 1, x0 + 1, S)
        top = (v00 + (fx * (v01 - v00).astype(f)).astype(f)).astype(f)
        bot = (v10 + (fx * (v11 - v10).astype(f)).astype(f)).astype(f)
        out[n] = np.where(okx & oky, (top + (fy * (bot - top).astype(f)).astype(f)).astype(f), f(0))
    return out


def _boxes(m, S, dtype):
    """per input pixel [S][S]: the centre (ex, ey) of M^-1 (q - c) + c and the half-widths (hx, hy) of the box of M^-1
    applied to the square [-1, 1]^2, in `dtype`"""
    t = dtype
    m = np.asarray(m, dtype=t)
    with np.errstate(divide='ignore', invalid='ignore'):
        rdet = t(1) / t(t(m[0] * m[3]) - t(m[1] * m[2]))
        i00, i01, i10, i11 = t(m[3] * rdet), t(-m[1] * rdet), t(-m[2] * rdet), t(m[0] * rdet)
    c = t(0.5) * t(S - 1)
    ay, ax = np.meshgrid(np.arange(S).astype(t) - c, np.arange(S).astype(t) - c, indexing='ij')
    ex = ((i00 * ax).astype(t) + (i01 * ay).astype(t)).astype(t) + c
    ey = ((i10 * ax).astype(t) + (i11 * ay).astype(t)).astype(t) + c
    return ex.astype(t), ey.astype(t), t(abs(i00) + abs(i01)), t(abs(i10) + abs(i11))


WINDOW = 7      # candidates per axis in the kernel: 2 S_MAX sqrt 2 = 4.29 px of box hold at most 5 integers, + 2 of pad


def emulate_backward(g, mats, mutate=None):
    """the backward kernel in numpy float32: per input pixel the candidates floor(e - h) .. ceil(e + h) per axis (at
    most WINDOW), row-major, each with the weight the forward gives it, accumulated in f32 in that order.
    mutate 'window': the window ends one pixel early on both axes."""
    f = np.float32
    g = np.asarray(g, dtype=f)
    S = g.shape[-1]
    dx = np.zeros_like(g)
    qy, qx = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    for n in range(g.shape[0]):
        m = np.asarray(mats[n], dtype=f)
        sx, sy = _positions(m, S, f)
        x0, fx, okx = _taps(sx, S)
        y0, fy, oky = _taps(sy, S)
        ex, ey, hx, hy = _boxes(m, S, f)
        x_lo = np.clip(np.floor(ex - hx), 0, S).astype(np.int64)
        y_lo = np.clip(np.floor(ey - hy), 0, S).astype(np.int64)
        x_hi = np.minimum(np.clip(np.ceil(ex + hx), -1, S - 1).astype(np.int64), x_lo + WINDOW - 1)
        y_hi = np.minimum(np.clip(np.ceil(ey + hy), -1, S - 1).astype(np.int64), y_lo + WINDOW - 1)
        if mutate == 'window':
            x_hi, y_hi = x_hi - 1, y_hi - 1
        acc = np.zeros((g.shape[1], S, S), dtype=f)
        for j in range(WINDOW):
            for i in range(WINDOW):
                wy, wx = y_lo + j, x_lo + i
                live = (wy <= y_hi) & (wx <= x_hi)
                wyc, wxc = np.clip(wy, 0, S - 1), np.clip(wx, 0, S - 1)
                cx0, cfx, cy0, cfy = x0[wyc, wxc], fx[wyc, wxc], y0[wyc, wxc], fy[wyc, wxc]
                ax = np.where(qx == cx0, f(1) - cfx, np.where(qx == cx0 + 1, cfx, f(0))).astype(f)
                ay = np.where(qy == cy0, f(1) - cfy, np.where(qy == cy0 + 1, cfy, f(0))).astype(f)
                w = np.where(live & okx[wyc, wxc] & oky[wyc, wxc], (ax * ay).astype(f), f(0))
                acc = (acc + (g[n][:, wyc, wxc] * w).astype(f)).astype(f)
        dx[n] = acc
    return dx


# ---- the bounds -------------------------------------------------------------------------------------------------------
def forward_model(x, mats):
    """[n][C][S][S]: S 2^-23 spread + 2^-23 maxabs over the 4 x 4 pixels around each sampling position"""
    x = np.asarray(x, dtype=np.float64)
    S = x.shape[-1]
    out = np.zeros_like(x)
    for n in range(x.shape[0]):
        sx, sy = _positions(np.asarray(mats[n], dtype=np.float64), S, np.float64)
        x0 = np.clip(np.floor(np.nan_to_num(sx)), -3, S + 1).astype(np.int64)
        y0 = np.clip(np.floor(np.nan_to_num(sy)), -3, S + 1).astype(np.int64)
        nb = np.stack([_gather(x[n], y0 + j, x0 + i, S) for j in range(-1, 3) for i in range(-1, 3)])
        out[n] = S * 2.0 ** -23 * (nb.max(0) - nb.min(0)) + 2.0 ** -23 * np.abs(nb).max(0)
    return out


def forward_bound(x, mats):
    return FWD_K * forward_model(x, mats)


def backward_model(g, mats):
    """[n][C][S][S]: (S + 4) 2^-23 times the sum of |dout| over the box of each input pixel, padded by two pixels"""
    g = np.abs(np.asarray(g, dtype=np.float64))
    S = g.shape[-1]
    out = np.zeros_like(g)
    for n in range(g.shape[0]):
        ex, ey, hx, hy = _boxes(np.asarray(mats[n], dtype=np.float64), S, np.float64)
        table = np.zeros((g.shape[1], S + 1, S + 1))
        table[:, 1:, 1:] = g[n].cumsum(1).cumsum(2)
        x_lo = np.clip(np.floor(ex - hx) - 2, 0, S).astype(np.int64)
        y_lo = np.clip(np.floor(ey - hy) - 2, 0, S).astype(np.int64)
        x_hi = np.maximum(np.clip(np.ceil(ex + hx) + 3, 0, S).astype(np.int64), x_lo)       # exclusive
        y_hi = np.maximum(np.clip(np.ceil(ey + hy) + 3, 0, S).astype(np.int64), y_lo)
        mass = table[:, y_hi, x_hi] - table[:, y_lo, x_hi] - table[:, y_hi, x_lo] + table[:, y_lo, x_lo]
        out[n] = (S + 4) * 2.0 ** -23 * np.maximum(mass, 0.0)
    return out


def backward_bound(g, mats):
    return BWD_K * backward_model(g, mats)


def ratio(got, want, model):
    """max |got - want| / model, an element with model 0 counting as inf unless it is exact"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / model)
    return float(r.max())


# ---- the inputs the CPU and the GPU tests share -----------------------------------------------------------------------
def edge_rows():
    """uniform rows on the edges of the draws: k = 3 from u1 just below 1; u2 = 0 (z = 0, s = 1); u0 exactly 0.5
    (flipped); both scale extremes (z clamped at +-3); theta = -pi and just below pi"""
    rng = np.random.RandomState(5)
    u = rng.random_sample((8, 8)).astype(np.float32)
    u[0, 1] = BELOW_ONE
    u[1, 2] = 0
    u[2, 0] = 0.5
    u[3, 2], u[3, 3] = BELOW_ONE, 0             # z = +5.77 -> 3
    u[4, 2], u[4, 3] = BELOW_ONE, 0.5           # z -> -3
    u[5, 4] = 0
    u[6, 4] = BELOW_ONE
    u[7, :] = 0
    return u


def rot_scale(theta, s=1.0, k=0, flipped=False):
    """one f32 matrix row from given draws"""
    m = compose(np.array([flipped]), np.array([k]), np.array([float(s)]), np.array([float(theta)]), np.array([15]))
    return m.astype(np.float32)[0]


def case_mats(n):
    """n <= 5 f32 matrices: a 45-degree rotation, the smallest and the largest scale (the largest rotated), a flipped
    90-degree turn and a generic draw"""
    rows = [rot_scale(np.pi / 4), rot_scale(0.0, s=1 / S_MAX), rot_scale(0.3, s=S_MAX), rot_scale(0.0, k=1, flipped=True),
            rot_scale(-2.2, s=1.2, k=3, flipped=True)]
    return np.stack(rows[:n])


def case_images(n, S, seed):
    """[n][3][S][S] f32: standard normal, but image 1 (if any) constant 0.75 and image 2 a one-hot at an odd place"""
    x = np.random.RandomState(seed).standard_normal((n, 3, S, S)).astype(np.float32)
    if n > 1:
        x[1] = 0.75
    if n > 2:
        x[2] = 0
        x[2, :, S // 2 + 1, S // 3] = (1.0, -2.0, 0.5)
    return x


SHAPES = [(8, 1), (10, 3), (64, 5)]         # (S, n): the smallest; rows no multiple of 4 pixels; more than one block


def measure(rows=200000):
    """the three largest ratios of the f32 emulation to its model: (matrix entries, forward, backward)"""
    rng = np.random.RandomState(0)
    u = np.concatenate([rng.random_sample((rows, 8)).astype(np.float32), edge_rows()])
    on = np.full(len(u), 15, dtype=np.int32)
    worst_m = float(np.abs(emulate_matrices(u, on) - matrices(u, 15)[0]).max())
    worst_f = worst_b = 0.0
    for S, n in SHAPES:
        mats, x, g = case_mats(n), case_images(n, S, 1), case_images(n, S, 2)
        worst_f = max(worst_f, ratio(emulate_forward(x, mats), forward(x, mats), forward_model(x, mats)))
        worst_b = max(worst_b, ratio(emulate_backward(g, mats), backward(g, mats), backward_model(g, mats)))
        # and on matrices as the prepare step makes them
        mats = emulate_matrices(rng.random_sample((n, 8)).astype(np.float32), np.full(n, 15, dtype=np.int32))
        worst_f = max(worst_f, ratio(emulate_forward(x, mats), forward(x, mats), forward_model(x, mats)))
        worst_b = max(worst_b, ratio(emulate_backward(g, mats), backward(g, mats), backward_model(g, mats)))
    return worst_m, worst_f, worst_b
