"""numpy / torch-CPU restatement of the occupancy-grid contract of include/fastnerf.h (fastnerf_occ_*,
fastnerf_render_rays_fwd_occ), the test oracle of csrc/occupancy.hip and of render_rays(..., occupancy=grid).

A grid here is a plain bool array [nx, ny, nz] plus lo, hi (float32 [3]) and outside_occupied: nothing of the library's packed
words is restated except the documented .npz layout (bit c & 31 of word c >> 5, c = (i * ny + j) * nz + k)."""
import numpy as np

F32 = np.float32


def build(volume, threshold, dilate):
    """Point volume [nx+1, ny+1, nz+1] -> bool [nx, ny, nz]: maximum of the 8 corners > threshold, then dilation."""
    v = np.asarray(volume, dtype=F32)
    m = v[:-1, :-1, :-1]
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                m = np.maximum(m, v[di:v.shape[0] - 1 + di, dj:v.shape[1] - 1 + dj, dk:v.shape[2] - 1 + dk])
    return dilated(m > F32(threshold), dilate)


def dilated(mask, r):
    """Every cell within Chebyshev distance r of a set cell, clipped at the box (brute force over the (2r+1)^3 offsets)."""
    mask = np.asarray(mask, dtype=bool)
    nx, ny, nz = mask.shape
    out = np.zeros_like(mask)
    for a in range(-r, r + 1):
        for b in range(-r, r + 1):
            for c in range(-r, r + 1):
                sx, tx = slice(max(0, a), nx + min(0, a)), slice(max(0, -a), nx + min(0, -a))
                sy, ty = slice(max(0, b), ny + min(0, b)), slice(max(0, -b), ny + min(0, -b))
                sz, tz = slice(max(0, c), nz + min(0, c)), slice(max(0, -c), nz + min(0, -c))
                if sx.start >= sx.stop or sy.start >= sy.stop or sz.start >= sz.stop:
                    continue
                out[tx, ty, tz] |= mask[sx, sy, sz]
    return out


def inv_of(shape, lo, hi):
    """n / (hi - lo) of the fp32 bounds, computed in double precision and rounded to fp32 once."""
    lo, hi = np.asarray(lo, F32).astype(np.float64), np.asarray(hi, F32).astype(np.float64)
    return (np.asarray(shape, np.float64) / (np.broadcast_to(hi, (3,)) - np.broadcast_to(lo, (3,)))).astype(F32)


def cell_index(points, shape, lo, hi):
    """float32 [.., 3] of floor((x - lo) * inv), subtraction and product each rounded to fp32 (may hold NaN / inf)."""
    x = np.asarray(points, dtype=F32)
    lo3 = np.broadcast_to(np.asarray(lo, F32), (3,))
    with np.errstate(invalid='ignore', over='ignore'):
        d = (x - lo3).astype(F32)
        return np.floor((d * inv_of(shape, lo, hi)).astype(F32))


def query(mask, lo, hi, outside_occupied, points):
    """bool [..]: the bit a sample at `points` [.., 3] takes."""
    mask = np.asarray(mask, dtype=bool)
    f = cell_index(points, mask.shape, lo, hi)
    n = np.asarray(mask.shape, F32)
    with np.errstate(invalid='ignore'):
        inside = ((f >= 0) & (f < n)).all(-1)          # a NaN fails both comparisons
    idx = np.where(inside[..., None], f, 0).astype(np.int64)
    return np.where(inside, mask[idx[..., 0], idx[..., 1], idx[..., 2]], bool(outside_occupied))


def sample_points(rays11, z):
    """x = o + d * z in fp32: one rounded multiply, one rounded add.  rays11 [n, >=6], z [n, S] -> [n, S, 3]."""
    r = np.asarray(rays11, dtype=F32)
    z = np.asarray(z, dtype=F32)
    prod = (r[:, None, 3:6] * z[:, :, None]).astype(F32)
    return (r[:, None, 0:3] + prod).astype(F32)


def classify(mask, lo, hi, outside_occupied, rays11, z):
    """bool [n, S] of the samples of a pass; the live list is np.nonzero(bits.reshape(-1))[0]."""
    return query(mask, lo, hi, outside_occupied, sample_points(rays11, z))


def words_to_mask(words, shape):
    """The documented .npz layout, decoded with numpy alone."""
    w = np.asarray(words).astype(np.uint32)
    ncells = int(np.prod(shape))
    bits = (w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & np.uint32(1)
    return bits.reshape(-1)[:ncells].reshape(tuple(int(s) for s in shape)).astype(bool)


# ---- the masked render, on the CPU oracle -----------------------------------------------------------------------------
def masked_raw(O, sd, rays11, z, bits, query_fn=None):
    """Logits of one pass at the given depths: the oracle's MLP at EVERY point, zeros where the bit is clear."""
    import torch
    rb = torch.as_tensor(rays11)
    z = torch.as_tensor(z)
    pts = rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]
    raw = O.run_network(sd, pts, rb[:, 8:11]) if query_fn is None else query_fn(pts)
    return raw * torch.as_tensor(np.asarray(bits))[..., None].to(raw.dtype)


def composite_at(O, sd, rays11, z, bits, white_bkgd, query_fn=None):
    """(raw, rgb_map, acc_map, weights) of one pass restated at given depths and bits."""
    import torch
    raw = masked_raw(O, sd, rays11, z, bits, query_fn)
    rb = torch.as_tensor(rays11)
    rgb, _, acc, w, _ = O.raw2outputs(raw, torch.as_tensor(z), rb[:, 3:6], None, white_bkgd)
    return raw, rgb, acc, w


def render_rays_masked(O, rays11, sdc, sdf, mask, lo, hi, outside_occupied, N_samples, N_importance, white_bkgd=False, t_rand=None,
                       u=None):
    """O.render_rays with the grid, entirely on the CPU (its OWN depths): what the chosen grids and seeds of the GPU tests are
    checked with before they are fixed.  mask None = no grid."""
    import torch
    rb = torch.as_tensor(rays11)
    z = O.coarse_z(rb[:, 6:7], rb[:, 7:8], N_samples, False, t_rand)
    ones = np.ones(tuple(z.shape), bool)
    b0 = ones if mask is None else classify(mask, lo, hi, outside_occupied, rb.numpy(), z.numpy())
    raw0, rgb0, acc0, w0 = composite_at(O, sdc, rb, z, b0, white_bkgd)
    z_mid = 0.5 * (z[..., 1:] + z[..., :-1])
    zs = O.sample_pdf(z_mid, w0[..., 1:-1], N_importance, u)
    z1, _ = torch.sort(torch.cat([z, zs], -1), -1)
    b1 = np.ones(tuple(z1.shape), bool) if mask is None else classify(mask, lo, hi, outside_occupied, rb.numpy(), z1.numpy())
    raw1, rgb1, acc1, _ = composite_at(O, sdf, rb, z1, b1, white_bkgd)
    return dict(rgb_map=rgb1, acc_map=acc1, rgb0=rgb0, acc0=acc0, bits0=b0, bits1=b1, raw0=raw0, raw1=raw1)


# ---- the scenes of the masked-render tests (fixed after the CPU check in tests/test_occupancy_cpu.py) ------------------------
def scene_grids():
    """name -> (mask, lo, hi, outside_occupied): a ball, a random mask on an anisotropic box, a half-space."""
    c = (np.arange(32) + 0.5) / 32 * 3.0 - 1.5
    X, Y, Z = np.meshgrid(c, c, c, indexing='ij')
    ball = (X * X + Y * Y + Z * Z) < 1.2 ** 2
    rnd = np.random.RandomState(0).rand(12, 16, 20) < 0.5
    h = (np.arange(16) + 0.5) / 16 * 4.0 - 2.0
    half = np.broadcast_to((h > 0.7)[:, None, None], (16, 16, 16)).copy()
    return {'ball': (ball, F32(-1.5), F32(1.5), False),
            'random': (rnd, np.array([-1.5, -1.2, -1.0], F32), np.array([1.5, 1.4, 1.6], F32), False),
            'half': (half, F32(-2.0), F32(2.0), True)}


def scene_rays(O, side=8, focal=14.0, near=2.0, far=6.0):
    """[side^2, 11] float32 ray batch of a camera on the sphere of radius 4 looking at the origin."""
    K = O.intrinsics(side, side, focal)
    ro, rd = O.get_rays(side, side, K, O.pose_spherical(30.0, -30.0, 4.0)[:3, :4])
    return O.make_ray_batch(ro.reshape(-1, 3), rd.reshape(-1, 3), near, far).numpy().astype(F32)


def scene_networks(O):
    """Random-init coarse and fine parameters (the oracle's nn.Linear default init, own generator)."""
    import torch
    return O.init_nerf_params(torch.Generator().manual_seed(1)), O.init_nerf_params(torch.Generator().manual_seed(2))


def scene_randoms(n, N_samples, N_importance, perturb):
    if not perturb:
        return None, None
    r = np.random.RandomState(7)
    return r.rand(n, N_samples).astype(F32), r.rand(n, N_importance).astype(F32)
