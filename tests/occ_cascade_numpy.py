"""numpy restatement of the occupancy CASCADE of include/fastnerf.h (fn_occ_cascade, fastnerf_occ_*_cascade,
fastnerf_render_rays_fwd_occ_cascade): tests/occ_numpy.py level by level, plus the lookup chain -- the first level whose box
contains the point decides, `outside_occupied` of the cascade when none does.

A cascade here is a list of (mask, lo, hi) -- bool [nx, ny, nz], float32 bounds -- and one `outside_occupied`."""
import numpy as np

import occ_numpy as R

F32 = np.float32


def inside(level, points):
    """bool [..]: the point's cell index in this level lies in 0 .. n-1 on all three axes (the level's own fp32 arithmetic)."""
    mask, lo, hi = level
    f = R.cell_index(points, np.asarray(mask).shape, lo, hi)
    with np.errstate(invalid='ignore'):
        return ((f >= 0) & (f < np.asarray(np.asarray(mask).shape, F32))).all(-1)      # a NaN fails both comparisons


def decided_by(levels, points):
    """int8 [..]: index of the first level that contains the point, -1 when none does."""
    pts = np.asarray(points, F32)
    out = np.full(pts.shape[:-1], -1, np.int8)
    for l in reversed(range(len(levels))):
        out[inside(levels[l], pts)] = l
    return out


def query(levels, outside_occupied, points):
    """bool [..]: the bit a sample at `points` [.., 3] takes."""
    pts = np.asarray(points, F32)
    who = decided_by(levels, pts)
    out = np.full(pts.shape[:-1], bool(outside_occupied))
    for l, (mask, lo, hi) in enumerate(levels):
        # inside level l, occ_numpy.query never reads its `outside` argument: it is the single grid's bit
        out = np.where(who == l, R.query(mask, lo, hi, False, pts), out)
    return out


def classify(levels, outside_occupied, rays11, z):
    """bool [n, S] of the samples of a pass; the live list is np.nonzero(bits.reshape(-1))[0]."""
    return query(levels, outside_occupied, R.sample_points(rays11, z))


def render_rays_masked(O, rays11, sdc, sdf, levels, outside_occupied, N_samples, N_importance, white_bkgd=False, t_rand=None, u=None):
    """occ_numpy.render_rays_masked with a cascade (the oracle's OWN depths, entirely on the CPU); also returns which level
    decided each sample of either pass.  levels None = no cascade."""
    import torch
    rb = torch.as_tensor(rays11)
    z = O.coarse_z(rb[:, 6:7], rb[:, 7:8], N_samples, False, t_rand)
    b0 = np.ones(tuple(z.shape), bool) if levels is None else classify(levels, outside_occupied, rb.numpy(), z.numpy())
    raw0, rgb0, acc0, w0 = R.composite_at(O, sdc, rb, z, b0, white_bkgd)
    z_mid = 0.5 * (z[..., 1:] + z[..., :-1])
    zs = O.sample_pdf(z_mid, w0[..., 1:-1], N_importance, u)
    z1, _ = torch.sort(torch.cat([z, zs], -1), -1)
    b1 = np.ones(tuple(z1.shape), bool) if levels is None else classify(levels, outside_occupied, rb.numpy(), z1.numpy())
    raw1, rgb1, acc1, _ = R.composite_at(O, sdf, rb, z1, b1, white_bkgd)
    res = dict(rgb_map=rgb1, acc_map=acc1, rgb0=rgb0, acc0=acc0, bits0=b0, bits1=b1, raw0=raw0, raw1=raw1)
    if levels is not None:
        res['who0'] = decided_by(levels, R.sample_points(rb.numpy(), z.numpy()))
        res['who1'] = decided_by(levels, R.sample_points(rb.numpy(), z1.numpy()))
    return res


# ---- the scene of the masked-render tests (fixed after the CPU check in tests/test_occupancy_cascade_cpu.py) -----------------
def scene_cascade():
    """(levels, outside_occupied): a ball in 32^3 over +-0.75, a random mask on an anisotropic, off-centre 12 x 16 x 20 box of
    about +-1.2, a half-space in 8^3 over +-2.0; a sample that no box contains counts as occupied.  The test camera's samples reach
    max |x| = 3.1, so every level and the 'no level' outcome decide a share of them: on the CPU oracle 0.16 / 0.38 / 0.40 / 0.05
    of the coarse and 0.13 / 0.40 / 0.37 / 0.09 of the fine samples, 0.64 of the coarse and 0.27 of the fine samples masked."""
    c = (np.arange(32) + 0.5) / 32 * 1.5 - 0.75
    X, Y, Z = np.meshgrid(c, c, c, indexing='ij')
    ball = (X * X + Y * Y + Z * Z) < 0.6 ** 2
    rnd = np.random.RandomState(0).rand(12, 16, 20) < 0.3
    h = (np.arange(8) + 0.5) / 8 * 4.0 - 2.0
    half = np.broadcast_to((h > 0.3)[:, None, None], (8, 8, 8)).copy()
    levels = [(ball, F32(-0.75), F32(0.75)),
              (rnd, np.array([-1.2, -1.12, -1.28], F32), np.array([1.2, 1.28, 1.12], F32)),
              (half, F32(-2.0), F32(2.0))]
    return levels, True


def shares(who, n_levels):
    """Share of the samples each level decides, then the share no level contains."""
    return [float((who == l).mean()) for l in range(n_levels)] + [float((who == -1).mean())]
