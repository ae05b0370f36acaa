"""References for the environment map of csrc/envmap.hip (fastnerf_env_lookup, fastnerf_env_grad; include/fastnerf.h, "environment
map").  Plain numpy: no GPU, nothing imported from the package.

  F32   taps32 / lookup32 / terms32 / grad32: numpy float32, one np.float32 operation per kernel operation.  The kernels use only
        + - * / and comparisons, each rounded on its own, so they are expected to equal this evaluation bit for bit; the scatter
        adds llrint(term * 2^50) as integers, which numpy restates exactly whatever the order.
  F64   lookup64 / grad64: the same formulas in float64 on the same fp32 inputs, with a bound on the distance of the fp32 result
        accumulated alongside (the running-error pairs RE of tests/rays_ref.py for the coordinates).

The bound of the lookup, per ray and channel (u = 2^-24):
    e = Dx (e_x + u) + Dy (e_y + u) + 6 u sum_k w_k |T_k|
e_x, e_y: the running error of the texel coordinates x, y (the 1-norm, the division, the fold, the affine map: they carry the
factor R), + u for the rounding of the fraction x - floor(x); Dx, Dy: the largest difference, per channel, between two texels that
the interpolation can pair along x / along y, the mirror wrap included -- the Lipschitz constant of the interpolant, which is
continuous across cell borders and across the table's border, so a floor that falls the other way in float64 needs no exclusion
list; 6 u: the weights' three roundings (1-fx, 1-fy, their product), the product with the texel and two levels of sums, 5 in all.
The two decisions that are not continuous in the bits -- s zero or not finite, and the signs sg(px), sg(py) of the fold, which
pick one of two border points that the wrap identifies -- are taken from the float32 evaluation.

The bound of the gradient, per texel word:
    e = sum_terms (7 u w (|a| + |b|) + 2^-51) + u |sum|
a = (1-acc1) g1, b = (1-acc0) g0: seven fp32 roundings per term (three in the weight, two in each of a and b and one in their sum
count as three on |a| + |b|, one in the product), 2^-51 for the term's rounding to a multiple of 2^-50, one final rounding to fp32.
The float64 sums are taken over the cells and fractions of the float32 restatement.  No tolerance here is a measured number."""
import numpy as np

from rays_ref import RE, U, F32

FIX = 2.0 ** 50
GRID = 256 * 256                                   # env_grid's cap: 256 blocks of 256 threads
N_BIG = 70001                                      # past one grid of threads, with a tail
SUB = 2.0 ** -140                                  # an absolute term for fp32 results in the subnormal range (spacing 2^-149)
G7 = 7 * U * (1 + 2.0 ** -20)                      # (1+u)^7 - 1
G6 = 6 * U


# ---- the float32 restatement -------------------------------------------------------------------------------------------------------
def _sg(t):
    return np.where(t >= 0, F32(1), F32(-1)).astype(F32)      # -0 >= 0: +1


def texel(i, j, R):
    """The mirror wrap: flat texel index j*R + i of a neighbour (i, j), either index possibly outside [0, R)."""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    oi, oj = (i < 0) | (i >= R), (j < 0) | (j >= R)
    i, j = np.clip(i, 0, R - 1), np.clip(j, 0, R - 1)
    j = np.where(oi, R - 1 - j, j)
    i = np.where(oj, R - 1 - i, i)
    return j * R + i


def coords32(d, R):
    """-> dict(ok, neg, sx, sy, px, py, x, y): the decisions and the float32 octahedral image and texel coordinates of d [n,3]."""
    d = np.asarray(d, F32)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all='ignore'):
        s = (np.abs(dx) + np.abs(dy)) + np.abs(dz)
        ok = (s != 0) & np.isfinite(s)
        ss = np.where(ok, s, F32(1))
        px = np.where(ok, np.where(ok, dx, F32(0)) / ss, F32(0)).astype(F32)
        py = np.where(ok, np.where(ok, dy, F32(0)) / ss, F32(0)).astype(F32)
        neg = dz < 0
        sx, sy = _sg(px), _sg(py)
        qx = (F32(1) - np.abs(py)) * sx
        qy = (F32(1) - np.abs(px)) * sy
        px, py = np.where(neg, qx, px).astype(F32), np.where(neg, qy, py).astype(F32)
        Rf = F32(R)
        x = ((px * F32(0.5) + F32(0.5)) * Rf) - F32(0.5)
        y = ((py * F32(0.5) + F32(0.5)) * Rf) - F32(0.5)
    assert x.dtype == F32 and y.dtype == F32
    return dict(ok=ok, neg=neg, sx=sx, sy=sy, px=px, py=py, x=x, y=y)


def taps32(d, R):
    """-> (idx [n,4] flat texel indices, w [n,4] float32 weights, (i0, j0, fx, fy)) in the order (i0,j0), (i0+1,j0), (i0,j0+1), (i0+1,j0+1)."""
    c = coords32(d, R)
    i0f, j0f = np.floor(c['x']), np.floor(c['y'])
    fx, fy = (c['x'] - i0f).astype(F32), (c['y'] - j0f).astype(F32)
    i0, j0 = i0f.astype(np.int64), j0f.astype(np.int64)
    idx = np.stack([texel(i0, j0, R), texel(i0 + 1, j0, R), texel(i0, j0 + 1, R), texel(i0 + 1, j0 + 1, R)], 1)
    gx, gy = F32(1) - fx, F32(1) - fy
    w = np.stack([gx * gy, fx * gy, gx * fy, fx * fy], 1)
    assert w.dtype == F32
    return idx, w, (i0, j0, fx, fy)


def lookup32(table, d):
    table = np.asarray(table, F32)
    R = table.shape[0]
    idx, w, _ = taps32(d, R)
    T = table.reshape(R * R, 3)[idx]                   # [n,4,3]
    t = w[:, :, None] * T
    out = (t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])
    assert out.dtype == F32
    return out


def ray_grad32(g1, acc1, g0=None, acc0=None):
    """g [n,3] = (1-acc1) g1 + (1-acc0) g0 in float32."""
    g = (F32(1) - np.asarray(acc1, F32))[:, None] * np.asarray(g1, F32)
    if g0 is not None:
        g = g + (F32(1) - np.asarray(acc0, F32))[:, None] * np.asarray(g0, F32)
    assert g.dtype == F32
    return g


def terms32(d, R, g1, acc1, g0=None, acc0=None):
    """-> (idx [n,4], term [n,4,3] float32): what every ray sends to its four texels."""
    idx, w, _ = taps32(d, R)
    term = w[:, :, None] * ray_grad32(g1, acc1, g0, acc0)[:, None, :]
    assert term.dtype == F32
    return idx, term


def grad32(d, R, g1, acc1, g0=None, acc0=None):
    """d_table [R,R,3] float32 as the kernel forms it: integer sums of llrint(term * 2^50)."""
    idx, term = terms32(d, R, g1, acc1, g0, acc0)
    q = np.rint(term.astype(np.float64) * FIX).astype(np.int64)
    ws = np.zeros((R * R, 3), np.int64)
    np.add.at(ws, idx.reshape(-1), q.reshape(-1, 3))
    return (ws.astype(np.float64) * (1.0 / FIX)).astype(F32).reshape(R, R, 3)


# ---- float64 with the bound --------------------------------------------------------------------------------------------------------
def coords_re(d, R):
    """The texel coordinates as running-error pairs (x, y), the discontinuous decisions taken from coords32."""
    d = np.asarray(d, F32)
    c = coords32(d, R)
    ok, neg = c['ok'], c['neg']
    dd = np.where(ok[:, None], d, F32(0)).astype(np.float64)
    one, half = RE(np.float64(1.0)), RE(np.float64(0.5))
    s = RE(np.abs(dd[:, 0])) + RE(np.abs(dd[:, 1])) + RE(np.abs(dd[:, 2]))
    s = RE(np.where(ok, s.v, 1.0), np.where(ok, s.e, 0.0))
    px, py = RE(dd[:, 0]) / s, RE(dd[:, 1]) / s
    px, py = RE(px.v, px.e + SUB), RE(py.v, py.e + SUB)
    ax, ay = RE(np.abs(px.v), px.e), RE(np.abs(py.v), py.e)
    qx, qy = one - ay, one - ax
    sx, sy = c['sx'].astype(np.float64), c['sy'].astype(np.float64)
    px = RE(np.where(neg, qx.v * sx, px.v), np.where(neg, qx.e, px.e))
    py = RE(np.where(neg, qy.v * sy, py.v), np.where(neg, qy.e, py.e))
    Rc = RE(np.float64(R))
    out = []
    for p in (px, py):
        h = RE(p.v * 0.5, p.e * 0.5 + SUB)
        out.append(((h + half) * Rc) - half)
    return out[0], out[1]


def lipschitz(table):
    """(Dx [3], Dy [3]): the largest |difference| per channel between texels paired along x / along y, the wrap included."""
    T = np.asarray(table, np.float64)
    R = T.shape[0]
    flat = T.reshape(R * R, 3)
    a = np.arange(-1, R)[:, None]                     # the lower index of a pair
    b = np.arange(-1, R + 1)[None, :]                 # the other coordinate, as a neighbour sees it
    Dx = np.abs(flat[texel(a + 1, b, R)] - flat[texel(a, b, R)]).max((0, 1))
    Dy = np.abs(flat[texel(b, a + 1, R)] - flat[texel(b, a, R)]).max((0, 1))
    return Dx, Dy


def bilinear64(table, x, y):
    T = np.asarray(table, np.float64)
    R = T.shape[0]
    flat = T.reshape(R * R, 3)
    i0, j0 = np.floor(x), np.floor(y)
    fx, fy = (x - i0)[:, None], (y - j0)[:, None]
    i0, j0 = i0.astype(np.int64), j0.astype(np.int64)
    return ((1 - fx) * (1 - fy) * flat[texel(i0, j0, R)] + fx * (1 - fy) * flat[texel(i0 + 1, j0, R)]
            + (1 - fx) * fy * flat[texel(i0, j0 + 1, R)] + fx * fy * flat[texel(i0 + 1, j0 + 1, R)])


def lookup64(table, d):
    """-> (v [n,3] float64, e [n,3]): the colours in float64 and the bound on |fp32 result - v|."""
    table = np.asarray(table, F32)
    R = table.shape[0]
    x, y = coords_re(d, R)
    v = bilinear64(table, x.v, y.v)
    Dx, Dy = lipschitz(table)
    idx, w, _ = taps32(d, R)
    mag = (w.astype(np.float64)[:, :, None] * np.abs(table.astype(np.float64).reshape(R * R, 3)[idx])).sum(1)
    e = Dx[None, :] * (x.e + U)[:, None] + Dy[None, :] * (y.e + U)[:, None] + G6 * mag
    return v, e


def grad64(d, R, g1, acc1, g0=None, acc0=None):
    """-> (v [R,R,3] float64, e [R,R,3]): the table gradient summed in float64 over the float32 restatement's cells and fractions,
    and the bound on |fp32 result - v|."""
    idx, _, (_, _, fx, fy) = taps32(d, R)
    fx, fy = fx.astype(np.float64), fy.astype(np.float64)
    w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], 1)
    a = (1.0 - np.asarray(acc1, np.float64))[:, None] * np.asarray(g1, np.float64)
    b = np.zeros_like(a) if g0 is None else (1.0 - np.asarray(acc0, np.float64))[:, None] * np.asarray(g0, np.float64)
    term = w[:, :, None] * (a + b)[:, None, :]
    mag = w[:, :, None] * (np.abs(a) + np.abs(b))[:, None, :]
    v = np.zeros((R * R, 3))
    e = np.zeros((R * R, 3))
    np.add.at(v, idx.reshape(-1), term.reshape(-1, 3))
    np.add.at(e, idx.reshape(-1), (G7 * mag + 2.0 ** -51).reshape(-1, 3))
    e = e + U * (1 + 2.0 ** -20) * np.abs(v)
    return v.reshape(R, R, 3), e.reshape(R, R, 3)


def scatter64(d, R, G):
    """The adjoint of the lookup in float64: sum_r w_k(r) G[r] into the texels, over the float32 restatement's cells and fractions."""
    n = np.asarray(G).shape[0]
    return grad64(d, R, G, np.zeros(n))[0]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def special_directions():
    """The directions at which the map's formulas branch or degenerate, as float32 rows."""
    z, nz = 0.0, -0.0
    rows = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]                    # the six axes
    rows += [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]                    # the eight diagonals
    rows += [(0.3, -0.7, z), (0.3, -0.7, nz), (-2.0, 0.5, z), (-2.0, 0.5, nz)]                      # dz = +-0
    rows += [(z, 0.4, 0.6), (nz, 0.4, 0.6), (z, 0.4, -0.6), (nz, 0.4, -0.6), (0.4, z, -0.6), (0.4, nz, -0.6),
             (nz, nz, -1.0), (z, nz, -1.0), (nz, z, -1.0), (nz, nz, 1.0), (z, 1.0, nz), (nz, -1.0, z)]      # zero and -0 components
    rows += [(z, z, z), (nz, nz, nz), (nz, z, nz)]                                                  # the zero vector
    rows += [(0.3e-20, -0.5e-20, 0.8e-20), (-0.3e-20, 0.5e-20, -0.8e-20), (0.3e20, -0.5e20, 0.8e20), (-0.3e20, 0.5e20, -0.8e20),
             (1e-45, -1e-45, 1e-45), (1e-45, 1e-45, -3e38), (-1e-45, 1e-45, -1.0)]                  # lengths 1e-20 and 1e20, the extremes
    for t in (0.0, 0.25, 0.5, 0.75, 1.0):                                                           # the |x| + |y| = 1 diamond
        for sx in (1, -1):
            for sy in (1, -1):
                rows += [(sx * t, sy * (1 - t), z), (sx * t, sy * (1 - t), nz), (sx * t, sy * (1 - t), 1e-30), (sx * t, sy * (1 - t), -1e-30)]
    for t in (0.125, 0.5, 0.875):                                                                   # the border: the folded image has |px| or |py| = 1
        for s1 in (1, -1):
            for s0 in (z, nz):
                rows += [(s1 * t, s0, -(1 - t)), (s0, s1 * t, -(1 - t))]
    rows += [(1e-8, 1e-8, -1.0), (-1e-8, 1e-8, -1.0), (1e-8, -1e-8, -1.0), (-1e-8, -1e-8, -1.0)]    # next to the corners
    rows += [(1.0, 1e-8, -1e-8), (-1.0, -1e-8, -1e-8), (1e-8, 1.0, -1e-8), (-1e-8, -1.0, -1e-8)]    # next to the border's midpoints
    rows += [(np.inf, 0.0, 1.0), (3e38, 3e38, 3e38), (np.nan, 1.0, 1.0), (1.0, 1.0, -np.inf), (0.0, 0.0, -np.inf)]      # s not finite
    return np.array(rows, F32)


def directions(n, seed):
    """n directions: the special ones first (as many as fit, none for n == 1), Gaussian draws of mixed length behind them."""
    rng = np.random.default_rng(seed)
    d = (rng.standard_normal((n, 3)) * np.exp(rng.uniform(-2, 2, (n, 1)))).astype(F32)
    if n > 1:
        sp = special_directions()[:n]
        d[:len(sp)] = sp
    return d


def table(R, seed):
    return np.random.default_rng(1000 + seed).standard_normal((R, R, 3)).astype(F32)


def grad_inputs(n, seed, two, acc_kind):
    """-> (g1 [n,3], acc1 [n], g0 or None, acc0 or None) float32; acc_kind in ('zero', 'one', 'random')."""
    rng = np.random.default_rng(2000 + seed)

    def acc():
        if acc_kind == 'zero':
            return np.zeros(n, F32)
        if acc_kind == 'one':
            return np.ones(n, F32)
        return rng.uniform(0, 1, n).astype(F32)
    g1 = (rng.standard_normal((n, 3)) / (3 * n)).astype(F32)
    a1 = acc()
    if not two:
        return g1, a1, None, None
    return g1, a1, (rng.standard_normal((n, 3)) / (3 * n)).astype(F32), acc()


def centre_directions(R):
    """[R*R,3] directions that hit the texel centres exactly (weights exactly 1 and 0), in texel order j*R + i: px, py are multiples
    of 1/R, the direction (px, py, 1 - |px| - |py|) of 1-norm 1 above the diamond, the unfolded image below."""
    assert R & (R - 1) == 0, 'a power of two keeps every step exact'
    c = (np.arange(R) + 0.5) * 2.0 / R - 1.0
    px, py = np.meshgrid(c, c)                        # [j,i]
    px, py = px.reshape(-1), py.reshape(-1)
    up = np.abs(px) + np.abs(py) <= 1
    sx, sy = np.where(px >= 0, 1.0, -1.0), np.where(py >= 0, 1.0, -1.0)
    ux, uy = (1 - np.abs(py)) * sx, (1 - np.abs(px)) * sy      # the fold is its own inverse
    dx, dy = np.where(up, px, ux), np.where(up, py, uy)
    dz = np.where(up, 1 - np.abs(px) - np.abs(py), -(1 - np.abs(ux) - np.abs(uy)))
    return np.stack([dx, dy, dz], 1).astype(F32)
