"""References for the ray-side kernels of csrc/rays.hip (gen_rays, gen_rays_pixels, ndc_rays, pack_rays, sample_coarse, posenc,
pp_gen_rays, pp_intersect_sphere, pp_fg_depths, pp_perturb_samples).  Plain numpy: no GPU, nothing imported from the package.

Every formula that uses only + - * / sqrt is written ONCE, in the operation order of rays.hip / depths.h, over a small "kit" of
arithmetic, and evaluated two ways:

  RE   a running-error evaluation: every value is a pair (v, e), v the float64 value of the formula and e a bound on the distance
       of the fp32 result from v.  u = 2^-24; an exact fp32 input has e = 0;
         a +- b   e = e_a + e_b + u |v|
         a * b    e = |a| e_b + |b| e_a + e_a e_b + u |v|
         a / b    e = (e_a + |q| e_b) / (|b| - e_b) + u |q|,  non-finite when |b| <= e_b
         sqrt a   e = e_a / (2 sqrt(max(a - e_a, tiny))) + u |v|
       negation and a product with a power of two add nothing.  The check of a kernel is |got - v| <= e wherever e is finite,
       with no further factor.
  F32  numpy float32, one np.float32 operation per kernel operation.  The library is built with -ffp-contract=off, the kernels use
       __fmul_rn / __fadd_rn, and HIP's fp32 division and square root are correctly rounded: the kernels are expected to equal
       this evaluation bit for bit.

posenc and pp_gen_rays have float64 references of their own (posenc_ref, pp_gen_rays_ref).  The input sets of the GPU tests are
generated here too (the *_inputs functions), so that tests/test_rays_ref_cpu.py can prove on the CPU, on exactly those inputs, that
the bound encloses the fp32 evaluation, that it is finite almost everywhere, and that a wrong formula leaves it."""
import numpy as np

U = 2.0 ** -24
F32 = np.float32
TINY = np.finfo(np.float64).tiny
ONE_BELOW = np.nextafter(F32(1.0), F32(0.0))      # the largest fp32 below 1

GRID = 2048 * 256                                  # grid_for's cap: 2048 blocks of 256 threads
N_RAYS_BIG = GRID + 257                            # one trip past the grid, with a tail block
N_SAMPLE_RAYS = 8200                               # x 64 samples = 524,800 > GRID
IMG_BIG = (725, 724)                               # 524,900 pixels
POSENC_BIG = {10: 8323, 4: 19419}                  # x 63 = 524,349 and x 27 = 524,313 outputs


# ---- the two kits ------------------------------------------------------------------------------------------------------------------
class RE:
    """(v, e): float64 value and bound on |fp32 result - v|, element-wise over numpy arrays."""
    __slots__ = ('v', 'e')

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, dtype=np.float64)

    def __add__(self, o):
        with np.errstate(all='ignore'):
            v = self.v + o.v
            return RE(v, self.e + o.e + U * np.abs(v))

    def __sub__(self, o):
        with np.errstate(all='ignore'):
            v = self.v - o.v
            return RE(v, self.e + o.e + U * np.abs(v))

    def __mul__(self, o):
        with np.errstate(all='ignore'):
            v = self.v * o.v
            return RE(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e + U * np.abs(v))

    def __truediv__(self, o):
        with np.errstate(all='ignore'):
            q = self.v / o.v
            den = np.abs(o.v) - o.e
            e = (self.e + np.abs(q) * o.e) / den + U * np.abs(q)
            return RE(q, np.where(den > 0, e, np.inf))

    def __neg__(self):
        return RE(-self.v, self.e)

    @property
    def shape(self):
        return self.v.shape


class _REKit:
    name = 're'

    @staticmethod
    def inp(a):
        """An exact fp32 input."""
        a = np.asarray(a)
        assert a.dtype == F32 or np.array_equal(a.astype(F32), a), 'inputs must be fp32 values'
        return RE(a)

    @staticmethod
    def const(x):
        """A constant that the kernel receives as fp32: the float64 value of that fp32 number."""
        return RE(np.float64(F32(x)))

    @staticmethod
    def sqrt(a):
        with np.errstate(all='ignore'):
            v = np.sqrt(a.v)
            return RE(v, a.e / (2.0 * np.sqrt(np.maximum(a.v - a.e, TINY))) + U * np.abs(v))

    @staticmethod
    def scale2(a, p):
        assert np.log2(abs(p)) == int(np.log2(abs(p)))
        return RE(a.v * p, a.e * abs(p))

    @staticmethod
    def where(c, a, b):
        return RE(np.where(c, a.v, b.v), np.where(c, a.e, b.e))

    @staticmethod
    def stack(cols):
        shp = np.broadcast_shapes(*[c.shape for c in cols])
        return RE(np.stack([np.broadcast_to(c.v, shp) for c in cols], -1), np.stack([np.broadcast_to(c.e, shp) for c in cols], -1))


class _F32Kit:
    name = 'f32'

    @staticmethod
    def inp(a):
        a = np.asarray(a)
        assert a.dtype == F32 or np.array_equal(a.astype(F32), a), 'inputs must be fp32 values'
        return a.astype(F32)

    @staticmethod
    def const(x):
        return np.asarray(x, dtype=F32)

    @staticmethod
    def sqrt(a):
        with np.errstate(all='ignore'):
            return np.sqrt(a, dtype=F32)

    @staticmethod
    def scale2(a, p):
        return a * F32(p)

    @staticmethod
    def where(c, a, b):
        return np.where(c, a, b).astype(F32)

    @staticmethod
    def stack(cols):
        shp = np.broadcast_shapes(*[c.shape for c in cols])
        out = np.stack([np.broadcast_to(c, shp) for c in cols], -1)
        assert out.dtype == F32
        return out


REK, F32K = _REKit, _F32Kit


def both(formula, *args, **kw):
    """-> (RE result, fp32 result) of one formula."""
    with np.errstate(all='ignore'):
        return formula(REK, *args, **kw), formula(F32K, *args, **kw)


def ratio(got, ref):
    """|got - v| / e where e is finite (0 / 0 counts as 0), and the mask of those elements."""
    fin = np.isfinite(ref.e) & np.isfinite(ref.v)
    with np.errstate(all='ignore'):
        err = np.abs(np.asarray(got, dtype=np.float64) - ref.v)
        r = np.where(err == 0, 0.0, err / ref.e)
        r = np.where(np.isnan(err), np.inf, r)          # a NaN where the reference is finite is outside every bound
    return np.where(fin, r, 0.0), fin


# ---- the formulas, in the kernels' operation order ---------------------------------------------------------------------------------
def pixel_ray(K, row, col, fx, fy, cx, cy, c):
    """pixel_ray of rays.hip.  row, col: integer arrays [n]; c: [12] or [n,12] fp32, a 3x4 pose row-major.  -> [n,3]."""
    c = np.asarray(c, dtype=F32)
    r, cl = K.inp(np.asarray(row).astype(F32)), K.inp(np.asarray(col).astype(F32))
    dx = (cl - K.const(cx)) / K.const(fx)
    dy = -(r - K.const(cy)) / K.const(fy)
    C = [K.inp(c[..., j]) for j in range(12)]
    # fmul(dz, c) with dz = -1 is the exact negation
    return K.stack([(dx * C[4 * k] + dy * C[4 * k + 1]) + (-C[4 * k + 2]) for k in range(3)])


def ndc_scale(dim, focal):
    """-1 / (dim / (2 focal)) in double, then applied as an fp32 scalar."""
    return F32(-1.0 / (float(dim) / (2.0 * float(focal))))


def _ndc_one(K, sx, sy, near, o, d):
    sx, sy, near = K.const(sx), K.const(sy), K.const(near)
    t = -(near + o[2]) / d[2]
    p = [o[k] + t * d[k] for k in range(3)]
    no = [(sx * p[0]) / p[2], (sy * p[1]) / p[2], K.const(1.0) + K.scale2(near, 2.0) / p[2]]
    nd = [sx * (d[0] / d[2] - p[0] / p[2]), sy * (d[1] / d[2] - p[1] / p[2]), K.scale2(near, -2.0) / p[2]]
    return no, nd


def ndc_one(K, sx, sy, near, ro, rd):
    """ndc_one of rays.hip on [n,3] origins and directions -> [n,6] (origin, direction)."""
    o, d = [K.inp(ro[:, k]) for k in range(3)], [K.inp(rd[:, k]) for k in range(3)]
    no, nd = _ndc_one(K, sx, sy, near, o, d)
    return K.stack(no + nd)


def pack_rays(K, ro, rd, near, far, ndc=False, sx=0.0, sy=0.0):
    """pack_rays_kernel -> [n,11]: o, d (NDC'd at near = 1 when ndc), near, far, d / |d| of the un-NDC'd direction."""
    o, d = [K.inp(ro[:, k]) for k in range(3)], [K.inp(rd[:, k]) for k in range(3)]
    nrm = K.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    v = [d[k] / nrm for k in range(3)]
    if ndc:
        o, d = _ndc_one(K, sx, sy, 1.0, o, d)
    return K.stack(o + d + [K.const(near), K.const(far)] + v)


def lin01(K, i, S, wrong=None):
    """lin01 of depths.h: torch.linspace(0, 1, S), start + step i below the midpoint, end - step (S - 1 - i) from it on."""
    i = np.asarray(i)
    step = K.const(1.0) / K.const(float(S if wrong == 'step_1_over_S' else S - 1))
    a = step * K.inp(i.astype(F32))
    if wrong == 'first_branch':
        return a
    b = K.const(1.0) - step * K.inp((S - 1 - i).astype(F32))
    return K.where(i < S // 2, a, b)


def coarse_depth(K, near, far, i, S, lindisp, wrong=None):
    """coarse_depth of depths.h; near, far: kit values [n,1]; i: integers [1,S]."""
    if S == 1:
        return near
    t = lin01(K, i, S, wrong)
    one = K.const(1.0)
    if not lindisp:
        return near * (one - t) + far * t
    return one / ((one / near) * (one - t) + (one / far) * t)


def jitter(K, zc, zl, zu, s, S, u):
    """lower + (upper - lower) u with the mid points to the neighbours zl, zu as borders (the ends keep zc)."""
    half = 0.5
    lower = K.where(s > 0, K.scale2(zc + zl, half), zc)
    upper = K.where(s < S - 1, K.scale2(zu + zc, half), zc)
    return lower + (upper - lower) * K.inp(u)


def sample_coarse(K, near, far, S, lindisp, u=None, wrong=None):
    """sample_coarse_kernel: near, far [n] fp32 (columns 6, 7 of rays11), u None or [n,S] -> [n,S]."""
    nr, fr = K.inp(np.asarray(near, dtype=F32)[:, None]), K.inp(np.asarray(far, dtype=F32)[:, None])
    s = np.arange(S)[None, :]
    w = wrong if wrong in ('first_branch', 'step_1_over_S') else None
    zc = coarse_depth(K, nr, fr, s, S, lindisp, w)
    if u is None:
        return _bcast(K, zc, (len(near), S))
    k = 2 if wrong == 'pm2' else 1
    zl = coarse_depth(K, nr, fr, np.maximum(s - k, 0), S, lindisp, w)
    zu = coarse_depth(K, nr, fr, np.minimum(s + k, S - 1), S, lindisp, w)
    return jitter(K, _bcast(K, zc, (len(near), S)), _bcast(K, zl, (len(near), S)), _bcast(K, zu, (len(near), S)), s, S, u)


def _bcast(K, a, shape):
    if isinstance(a, RE):
        return RE(np.broadcast_to(a.v, shape), np.broadcast_to(a.e, shape))
    return np.broadcast_to(a, shape)


def intersect_sphere(K, rays):
    """intersect_sphere_kernel on [n,11] rays -> (fg_far [n], pn2 [n]); the kernel counts pn2 >= 1 and fg_far is NaN for pn2 > 1."""
    o, d = [K.inp(rays[:, k]) for k in range(3)], [K.inp(rays[:, 3 + k]) for k in range(3)]
    dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    od = (d[0] * o[0] + d[1] * o[1]) + d[2] * o[2]
    d1 = -od / dd
    p = [o[c] + d1 * d[c] for c in range(3)]
    pn2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
    one = K.const(1.0)
    return d1 + K.sqrt(one - pn2) * (one / K.sqrt(dd)), pn2


def fg_depths(K, fg_far, near, S, u=None, wrong=None):
    """fg_depths_kernel: the lattice near + k step, step = (fg_far - near) / (S - 1), jittered when u is given -> [n,S]."""
    far = K.inp(np.asarray(fg_far, dtype=F32)[:, None])
    nr = K.const(near)
    step = (far - nr) / K.const(float(S - 1))
    s = np.arange(S)[None, :]

    def zat(k):
        return nr + K.inp(k.astype(F32)) * step
    zc = zat(s)
    if u is None:
        return zc
    # (the neighbours beyond the ends are never selected)
    return jitter(K, zc, zat(np.maximum(s - 1, 0)), zat(s if wrong == 'zat_s' else s + 1), s, S, u)


def perturb_samples(K, z, u, wrong=None):
    """pp_perturb_kernel on [n,S] depths."""
    z = np.asarray(z, dtype=F32)
    S = z.shape[1]
    s = np.arange(S)[None, :]
    k = 2 if wrong == 'pm2' else 1
    zl = np.concatenate([z[:, :1]] * k + [z[:, :-k]], 1)[:, :S] if S > k else z
    zu = np.concatenate([z[:, k:]] + [z[:, -1:]] * k, 1)[:, -S:] if S > k else z
    return jitter(K, K.inp(z), K.inp(zl), K.inp(zu), s, S, u)


# ---- posenc and pp_gen_rays: float64 references of their own ------------------------------------------------------------------------
def posenc_ref(x, L, dtype=np.float64, wrong=None):
    """[x, sin(2^0 x), cos(2^0 x), ...] of [n,3] fp32 points -> [n, 3 + 6 L].  x 2^k is exact in fp32, so with dtype float64 the
    sine and cosine channels are those of the kernel's exact argument; with float32, numpy's fp32 sin / cos of the same argument."""
    x = np.asarray(x, dtype=F32)
    out = [x.astype(dtype)]
    for k in range(L):
        a = x.astype(dtype) * dtype(2.0 ** (k + 1 if wrong == 'next_band' and k == L - 1 else k))
        out += [np.sin(a), np.cos(a)]
    return np.concatenate(out, -1)


def pp_gen_rays_ref(H, W, intrinsics, c2w, wrong=None):
    """float64 R K^-1 [col + 0.5, row + 0.5, 1] with K^-1 from np.linalg.inv -> (v [H W,3], bound [H W,3], origin fp32 [3]).
    The kernel evaluates in fp64 and rounds once: bound = u |v| + 64 2^-53 A, A the same product with every factor replaced by
    its absolute value (it only matters under a cancellation of about 2^24)."""
    Kinv = np.linalg.inv(np.asarray(intrinsics, dtype=np.float64)[:3, :3])
    R = np.asarray(c2w, dtype=np.float64)[:3, :3]
    half = 0.0 if wrong == 'no_half' else 0.5
    i = np.arange(H * W)
    px = np.stack([(i % W) + half, (i // W) + half, np.ones(H * W)], -1)
    v = px @ (R @ Kinv).T
    A = np.abs(px) @ (np.abs(R) @ np.abs(Kinv)).T
    return v, U * np.abs(v) + 64.0 * 2.0 ** -53 * A, np.asarray(c2w, dtype=np.float64)[:3, 3].astype(F32)


def pp_gen_rays_emu(H, W, intrinsics, c2w):
    """The kernel's own route: cofactor inverse and R K^-1 in float64 on the host, three float64 multiply-adds per component on
    the device (two products, two sums), rounded to fp32 once."""
    K = np.asarray(intrinsics, dtype=np.float64).reshape(4, 4)
    M = np.asarray(c2w, dtype=np.float64).reshape(4, 4)
    a, b, c, d, e, f, g, h, i = K[0, 0], K[0, 1], K[0, 2], K[1, 0], K[1, 1], K[1, 2], K[2, 0], K[2, 1], K[2, 2]
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    inv = np.array([(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det,
                    (f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det,
                    (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det]).reshape(3, 3)
    RK = np.zeros((3, 3))
    for r in range(3):
        for cc in range(3):
            s = 0.0
            for k in range(3):
                s += M[r, k] * inv[k, cc]
            RK[r, cc] = s
    j = np.arange(H * W)
    u, v = (j % W) + 0.5, (j // W) + 0.5
    return np.stack([(RK[k, 0] * u + RK[k, 1] * v + RK[k, 2]) for k in range(3)], -1).astype(F32)


# ---- the input sets of the GPU tests -----------------------------------------------------------------------------------------------
def random_pose(rs, scale=4.0):
    """A random orthonormal 3x4 pose with a translation, rounded to fp32."""
    q, _ = np.linalg.qr(rs.randn(3, 3))
    return np.concatenate([q, scale * rs.randn(3, 1)], 1).astype(F32)


CAMERA = dict(fx=1111.3, fy=987.6, cx=2015.37, cy=1511.81)      # anisotropic, off-centre, non-integer


def gen_rays_inputs(seed=1):
    """-> (H, W, c2w [3,4]) for the sizes 1, 257 and one trip past the grid."""
    rs = np.random.RandomState(seed)
    return [(1, 1, random_pose(rs)), (1, 257, random_pose(rs)), IMG_BIG + (random_pose(rs),)]


def gen_rays_pixels_inputs(n, seed=2, n_img=5):
    """-> (pix [n,3] int32 (image, row, col), rows and columns up to 4031 with the corners present, poses [n_img,3,4])."""
    rs = np.random.RandomState(seed + n % 9973)
    pix = np.stack([rs.randint(0, n_img, n), rs.randint(0, 4032, n), rs.randint(0, 4032, n)], 1).astype(np.int32)
    pix[0, 1:] = (4031, 4031)
    if n > 3:
        pix[1, 1:], pix[2, 1:], pix[3, 1:] = (0, 0), (4031, 0), (0, 4031)
    return pix, np.stack([random_pose(rs) for _ in range(n_img)], 0)


NDC_CAM = (756, 1008, 815.13)          # H, W, focal
NDC_NEARS = (0.1, 1.0, 2.3)


def ndc_inputs(n, seed=3):
    """o ~ N(0, (1, 1, 3)), d_xy in [-0.5, 0.5], d_z in {-1, -1e-2, -1e-4}: d_z enters as a divisor and o_z + t d_z cancels to -near."""
    rs = np.random.RandomState(seed + n % 9973)
    ro = (rs.randn(n, 3) * np.array([1.0, 1.0, 3.0])).astype(F32)
    rd = np.concatenate([rs.rand(n, 2) - 0.5, np.array([-1.0, -1e-2, -1e-4])[rs.randint(0, 3, n)][:, None]], 1).astype(F32)
    return ro, rd


def pack_inputs(n, seed=4):
    """Generic rays for pack_rays without NDC: normal origins, normal directions over four decades of length."""
    rs = np.random.RandomState(seed + n % 9973)
    ro = rs.randn(n, 3).astype(F32)
    rd = (rs.randn(n, 3) * 10.0 ** rs.uniform(-2, 2, (n, 1))).astype(F32)
    return ro, rd


NEAR_FAR = ((2.0, 6.0), (0.05, 50.0), (1e-3, 1.0))
COARSE_S = (1, 2, 3, 64, 65, 192)


def unit_draws(rs, shape):
    """U[0, 1) fp32 draws with exact 0 and the largest fp32 below 1 among them."""
    u = rs.rand(*shape).astype(F32)
    u = np.minimum(u, ONE_BELOW)
    f = u.reshape(-1)
    f[::7] = 0.0
    f[3::11] = ONE_BELOW
    return u


def coarse_inputs(n, S, seed=5):
    """-> (near [n], far [n], u [n,S]): the rays cycle through NEAR_FAR (near > 0 throughout, so every set serves lindisp too)."""
    rs = np.random.RandomState(seed + 131 * S + n % 9973)
    nf = np.array(NEAR_FAR, dtype=F32)[np.arange(n) % len(NEAR_FAR)]
    return nf[:, 0].copy(), nf[:, 1].copy(), unit_draws(rs, (n, S))


def rays11_of(near, far):
    r = np.zeros((len(near), 11), dtype=F32)
    r[:, 6], r[:, 7] = near, far
    return r


def sphere_inputs(n, outside=False, seed=6):
    """-> (rays11 [n,11], planted): cameras inside the unit sphere whose rays pass the origin at distances up to 1 - 1e-6.
    outside: `planted` rays have a closest point ON or beyond the unit sphere, among them o = (1,0,0), d = (0,1,0) and two more
    rays whose fp32 pn2 is exactly 1.0f; rays beyond it (fg_far = NaN) are planted only at n > 1024, one in 1024."""
    rs = np.random.RandomState(seed + n % 9973)
    p = rs.randn(n, 3)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    r = np.where(rs.rand(n) < 0.3, 1.0 - 10.0 ** rs.uniform(-6, -1, n), rs.rand(n))      # |closest point|, up to 1 - 1e-6
    p *= r[:, None]
    t = rs.randn(n, 3)
    t -= p * ((t * p).sum(1) / np.maximum((p * p).sum(1), 1e-30))[:, None]               # a direction orthogonal to p
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    back = rs.uniform(-1, 1, n) * np.sqrt(1.0 - r * r) * 0.98                            # the camera stays inside
    rays = np.zeros((n, 11), dtype=F32)
    rays[:, :3] = p + back[:, None] * t
    rays[:, 3:6] = t * 10.0 ** rs.uniform(-1, 1, (n, 1))
    planted = 0
    if outside:
        exact = np.array([[1, 0, 0, 0, 1, 0], [0, 1, 0, 0, 0, 2], [1, 0.5, 0, 0, 1, 0]], dtype=F32)
        idx = np.arange(5, n, 29 if n <= 1024 else 1024)
        for j, i in enumerate(idx):
            if n > 1024 and j % 2 == 1:
                q = rays[i, :3] / max(np.linalg.norm(rays[i, :3]), 1e-3)
                rays[i, :3] = q * rs.uniform(1.5, 3.0)                                   # far outside: pn2 > 1, fg_far = NaN
                rays[i, 3:6] = np.cross(q, rs.randn(3)).astype(F32)
            else:
                rays[i, :6] = exact[(j // 2) % 3]
        planted = len(idx)
    return rays, planted


FG_S = (2, 3, 64, 65)
FG_NEAR = 1e-4


def fg_inputs(n, S, seed=7):
    """-> (fg_far [n] in (near, 2], u [n,S])."""
    rs = np.random.RandomState(seed + 131 * S + n % 9973)
    return (10.0 ** rs.uniform(-3, np.log10(2.0), n)).astype(F32), unit_draws(rs, (n, S))


def perturb_inputs(n, S, seed=8):
    """-> (z [n,S] sorted depths in (0, 1], u [n,S])."""
    rs = np.random.RandomState(seed + 131 * S + n % 9973)
    return np.sort(1.0 - rs.rand(n, S), axis=1).astype(F32), unit_draws(rs, (n, S))


def posenc_inputs(n, seed=9):
    """|x| log-uniform in [1e-3, 8] with random signs, plus exact 0 and +-8."""
    rs = np.random.RandomState(seed + n % 9973)
    x = (10.0 ** rs.uniform(-3, np.log10(8.0), (n, 3)) * rs.choice([-1.0, 1.0], (n, 3))).astype(F32)
    x = np.clip(x, -8.0, 8.0)
    f = x.reshape(-1)
    f[::97], f[1::101], f[2::103] = 0.0, 8.0, -8.0
    return x


def pp_camera(seed=10):
    """Random intrinsics with skew and an off-centre principal point, a random pose; 4x4 float64 both."""
    rs = np.random.RandomState(seed)
    K = np.eye(4)
    K[0, 0], K[1, 1], K[0, 1], K[0, 2], K[1, 2] = 900.0 + 300 * rs.rand(), 800.0 + 300 * rs.rand(), 3.0 * rs.randn(), 350.0 + 40 * rs.rand(), 370.0 + 40 * rs.rand()
    M = np.eye(4)
    q, _ = np.linalg.qr(rs.randn(3, 3))
    M[:3, :3], M[:3, 3] = q, 0.5 * rs.randn(3)
    return K, M
