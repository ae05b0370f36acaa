"""float32 numpy restatement of fastnerf_occ_ray_bounds (include/fastnerf.h, csrc/ray_bounds.hip): per ray, the part
[near', far'] of [near, far] outside which the occupancy lookup of tests/occ_numpy.py / tests/occ_cascade_numpy.py cannot call a
sample occupied.  The test oracle of the kernel; its own properties -- conservative, tight -- are checked against
occ_numpy.classify in tests/test_ray_bounds_cpu.py.

A cascade here is a list of (mask, lo, hi) and one `outside_occupied`, as in occ_cascade_numpy; a single grid is a cascade of
one level.  Every operation on a depth or a grid coordinate is one fp32 operation, in the order the kernel performs it.

The traversal.  Per level and axis the ray is og + dg * z in grid coordinates (og = (o - lo) * inv, dg = d * inv), and face k is
crossed at t(k) = (k - og) / dg.  The lookup the samples go through rounds differently (x = o + d * z first), so its index along
an axis changes somewhere in [t(k) - e, t(k) + e]: e = delta / |dg|, delta = 2^-20 (B + n + 2) grid units with B the magnitude of
the terms, which bounds both chains' rounding with a factor to spare.  The lookup's index is monotone in z on every axis, so at
a depth z it is the last index the ray has SURELY reached (z >= t + e) or, inside a window, the next one.  The sweep walks the
window starts and ends of the three axes in order of depth; between two events the candidates are a block of 1, 2, 4 or 8 cells,
and the stretch counts as occupied when one of them is.  No fp32 rounding at a face or a corner can then put an occupied sample
outside [near', far'], and the bounds are never more than e (far less than a cell) wider than the cells ask for.
A ray whose terms are too large for delta <= 1/4 keeps its bounds (hit = 1): that is always a valid answer."""
import numpy as np

import occ_numpy as R

F32 = np.float32
INF = F32(np.inf)
ERR_SCALE = F32(2.0 ** -20)
DELTA_MAX = F32(0.25)
Z_LIMIT = F32(2.0 ** 60)


def iteration_cap(shapes):
    """The hard cap of the sweep's events over all levels: two events per face crossed, and some to spare."""
    return 2 * sum(int(s) for sh in shapes for s in sh) + 16 * len(shapes) + 16


class _Bail(Exception):
    """The ray keeps its bounds with hit = 1."""


class _Axis:
    """One axis of one level: geometry, and the sweep's state (c = the last cell surely reached, amb = inside a window)."""

    def __init__(self, o, d, lo, inv, n, zmax):
        self.n = int(n)
        self.og = F32(F32(o - lo) * inv)
        self.dg = F32(d * inv)
        B = F32(F32(F32(abs(o) + abs(lo)) + F32(abs(d) * zmax)) * inv)
        self.delta = F32(ERR_SCALE * F32(F32(B + F32(n)) + F32(2)))
        if not self.delta <= DELTA_MAX:
            raise _Bail
        self.s = 1 if self.dg > 0 else (-1 if self.dg < 0 else 0)
        self.e = F32(self.delta / abs(self.dg)) if self.s else INF
        if self.s:
            kin, kout = (0, self.n) if self.s > 0 else (self.n, 0)
            self.pin, self.pout = self.win_start(kin), self.win_end(kout)      # possibly inside the box
            self.sin, self.sout = self.win_end(kin), self.win_start(kout)      # surely inside the box
        else:
            self.c0 = int(np.floor(F32(self.og - self.delta)))
            self.c1 = int(np.floor(F32(self.og + self.delta)))
            possibly = self.c1 >= 0 and self.c0 <= self.n - 1
            surely = self.c0 >= 0 and self.c1 <= self.n - 1
            self.pin, self.pout = (-INF, INF) if possibly else (INF, -INF)
            self.sin, self.sout = (-INF, INF) if surely else (INF, -INF)

    def t(self, k):
        return F32(F32(F32(k) - self.og) / self.dg)

    def win_start(self, k):
        v = F32(self.t(k) - self.e)
        return v if v == v else -INF

    def win_end(self, k):
        v = F32(self.t(k) + self.e)
        return v if v == v else INF

    def face(self):
        """The next face the ray crosses on this axis."""
        return self.c + 1 if self.s > 0 else self.c

    def start(self, z):
        """The state at depth z (inside the level's 'possibly inside' stretch)."""
        if not self.s:
            self.c, self.amb, self.step, self.tnext = self.c0, self.c1 != self.c0, 1, INF
            return
        self.step = self.s
        est = np.floor(F32(self.og + F32(self.dg * z)))
        self.c = int(min(max(est, F32(-1)), F32(self.n))) if est == est else -1
        for _ in range(4):
            behind = self.c if self.s > 0 else self.c + 1
            movable = self.c > -1 if self.s > 0 else self.c < self.n
            if movable and self.win_end(behind) > z:
                self.c -= self.s
            else:
                break
        else:
            raise _Bail
        for _ in range(4):
            movable = self.c < self.n if self.s > 0 else self.c > -1
            if movable and self.win_end(self.face()) <= z:
                self.c += self.s
            else:
                break
        else:
            raise _Bail
        self.amb = bool(self.win_start(self.face()) <= z)
        self.tnext = self.win_end(self.face()) if self.amb else self.win_start(self.face())

    def advance(self):
        if self.amb:
            self.c += self.s
            self.amb = False
            self.tnext = self.win_start(self.face())
        else:
            self.amb = True
            self.tnext = self.win_end(self.face())

    def candidates(self):
        c = [self.c, self.c + self.step] if self.amb else [self.c]
        return [v for v in c if 0 <= v <= self.n - 1]


def _clip(ta, tb, surely):
    """(min, max) of [ta, tb] without the stretches that surely belong to the levels of `surely`, or None when nothing is left.
    The end points of a removed stretch stay."""
    x, y = ta, tb
    for _ in surely:
        for si, so in surely:
            if si <= x <= so:
                x = so
            if si <= y <= so:
                y = si
    return (x, y) if (x <= tb and y >= ta and x <= y) else None


def ray_bounds_one(levels, outside_occupied, o, d, near, far, cap=None):
    """(near', far', hit) of one ray."""
    o, d, near, far = np.asarray(o, F32), np.asarray(d, F32), F32(near), F32(far)
    if cap is None:
        cap = iteration_cap([np.asarray(m).shape for m, _, _ in levels])
    if not (np.isfinite(o).all() and np.isfinite(d).all() and np.isfinite(near) and np.isfinite(far)) or not near < far:
        return near, far, 1
    zmax = max(abs(near), abs(far))
    if not zmax <= Z_LIMIT:
        return near, far, 1
    best = [INF, -INF]

    def take(ta, tb, surely):
        if ta < best[0] or tb > best[1]:
            r = _clip(ta, tb, surely)
            if r is not None:
                best[0], best[1] = min(best[0], r[0]), max(best[1], r[1])

    try:
        with np.errstate(all='ignore'):
            surely = []
            it = 0
            for mask, lo, hi in levels:
                mask = np.asarray(mask, bool)
                lo3 = np.broadcast_to(np.asarray(lo, F32), (3,))
                inv = R.inv_of(mask.shape, lo, hi)
                ax = [_Axis(o[a], d[a], lo3[a], inv[a], mask.shape[a], zmax) for a in range(3)]
                s0, s1 = max(near, max(x.pin for x in ax)), min(far, min(x.pout for x in ax))
                if s0 <= s1:
                    for x in ax:
                        x.start(s0)
                    tcur = s0
                    while True:
                        it += 1
                        if it > cap:
                            raise _Bail
                        am = min(range(3), key=lambda a: (ax[a].tnext, a))
                        tn = ax[am].tnext
                        tend = max(min(tn, s1), tcur)
                        if tcur < best[0] or tend > best[1]:
                            ci, cj, ck = (x.candidates() for x in ax)
                            if any(mask[i, j, k] for i in ci for j in cj for k in ck):
                                take(tcur, tend, surely)
                        if not tn < s1:
                            break
                        ax[am].advance()
                        tcur = tend
                surely.append((max(x.sin for x in ax), min(x.sout for x in ax)))
            if outside_occupied:
                take(near, far, surely)
    except _Bail:
        return near, far, 1
    if not best[0] <= best[1]:
        return near, far, 0
    n2, f2 = max(near, best[0]), min(far, best[1])
    if not n2 < f2:
        return near, far, 1
    return F32(n2), F32(f2), 1


def ray_bounds(levels, outside_occupied, rays, cap=None):
    """rays [n, >= 8] -> (near' float32 [n], far' float32 [n], hit uint8 [n])."""
    r = np.asarray(rays, F32)
    out = [ray_bounds_one(levels, outside_occupied, q[0:3], q[3:6], q[6], q[7], cap) for q in r]
    return (np.array([v[0] for v in out], F32), np.array([v[1] for v in out], F32), np.array([v[2] for v in out], np.uint8))


def ray_bounds_grid(mask, lo, hi, outside_occupied, rays, cap=None):
    """The single grid: a cascade of one level."""
    return ray_bounds([(mask, lo, hi)], outside_occupied, rays, cap)


# ---- the inputs and the two properties of the tests (CPU and GPU files share them) ------------------------------------------
PROBES = 4096


def random_rays(n=144, seed=3, zero=0):
    """o ~ 1.5 N(0,1), d ~ N(0,1), near = 0.05, far = 4; zero = 1 or 2: that many components of d (per ray, rotating) are exactly 0."""
    r = np.random.RandomState(seed)
    rays = np.zeros((n, 11), F32)
    rays[:, 0:3] = 1.5 * r.randn(n, 3)
    rays[:, 3:6] = r.randn(n, 3)
    rays[:, 6], rays[:, 7] = 0.05, 4.0
    for q in range(n):
        for j in range(zero):
            rays[q, 3 + (q + j) % 3] = 0.0
    rays[:, 8:11] = rays[:, 3:6] / np.linalg.norm(rays[:, 3:6], axis=-1, keepdims=True)
    return rays


def ray_sets(O):
    """name -> [144, 11]: the camera of occ_numpy.scene_rays, random rays, random rays with zero direction components."""
    rnd = random_rays()
    z12 = np.concatenate([random_rays(72, 4, 1), random_rays(72, 5, 2)])
    return {'camera': R.scene_rays(O, side=12), 'random': rnd, 'zeros': z12}


def probe_depths(rays, probes=PROBES):
    """[n, probes] evenly spaced depths over each ray's [near, far], both ends included."""
    r = np.asarray(rays, F32)
    t = np.linspace(0.0, 1.0, probes)
    return (r[:, 6:7].astype(np.float64) * (1.0 - t) + r[:, 7:8].astype(np.float64) * t).astype(F32)


def check_conservative(live, z, near2, far2, hit):
    """Number of exceptions to (C): a live probe outside [near', far'], or on a ray with hit = 0."""
    out = live & ((z < near2[:, None]) | (z > far2[:, None]) | (hit[:, None] == 0))
    return int(out.sum())


def check_tight(live_plus, z, rays, near2, far2, hit, h_max):
    """Number of exceptions to (T) against the probes that are live under the dilated mask: a hit ray without one, or bounds
    further out than s = sqrt(3) h_max / |d| + 2 probe spacings from the first / last of them."""
    r = np.asarray(rays, F32).astype(np.float64)
    spacing = (r[:, 7] - r[:, 6]) / (z.shape[1] - 1)
    s = np.sqrt(3.0) * float(h_max) / np.linalg.norm(r[:, 3:6], axis=-1) + 2.0 * spacing
    bad = 0
    for q in np.nonzero(hit)[0]:
        zz = z[q][live_plus[q]]
        if zz.size == 0:
            bad += 1
            continue
        if near2[q] < zz.min() - s[q] or far2[q] > zz.max() + s[q]:
            bad += 1
    return bad


def cell_edges(shape, lo, hi):
    """float64 [3] cell edge lengths."""
    lo3 = np.broadcast_to(np.asarray(lo, np.float64), (3,))
    hi3 = np.broadcast_to(np.asarray(hi, np.float64), (3,))
    return (hi3 - lo3) / np.asarray(shape, np.float64)


def cascade_fixtures():
    """(levels for (C), levels for (T)): three nested levels, random masks.  The second fixture keeps its occupied cells two
    cells away from every level's faces -- its own, and (in its own cells) those of the boxes inside it -- so that the 3 x 3 x 3
    block around an occupied cell is decided by that cell's level and the seams stay out of the slack of (T)."""
    r = np.random.RandomState(11)
    boxes = [((16, 16, 16), F32(-0.5), F32(0.5)),
             ((20, 24, 28), np.array([-1.5, -1.4, -1.6], F32), np.array([1.5, 1.6, 1.4], F32)),
             ((16, 16, 16), F32(-4.0), F32(4.0))]
    free, kept = [], []
    for l, (shape, lo, hi) in enumerate(boxes):
        m = r.rand(*shape) < 0.3
        free.append((m, lo, hi))
        k = np.zeros(shape, bool)
        k[2:-2, 2:-2, 2:-2] = (r.rand(*shape) < 0.3)[2:-2, 2:-2, 2:-2]
        h = cell_edges(shape, lo, hi)
        lo3 = np.broadcast_to(np.asarray(lo, np.float64), (3,))
        c = np.stack(np.meshgrid(*[lo3[a] + (np.arange(shape[a]) + 0.5) * h[a] for a in range(3)], indexing='ij'), -1)
        for _, lo_j, hi_j in kept[:l]:
            gap = np.maximum(np.broadcast_to(np.asarray(lo_j, np.float64), (3,)) - c, c - np.broadcast_to(np.asarray(hi_j, np.float64), (3,)))
            k &= (gap / h).max(-1) >= 2.5
        kept.append((k, lo, hi))
    return free, kept
