"""float64 restatement of the early-ray-termination contract of include/fastnerf.h (fastnerf_ert_classify, fastnerf_ert_advance,
fastnerf_render_rays_fwd_ert), on top of tests/occ_numpy.py: the test oracle of render_rays(..., ert=eps, ert_block=B).

Everything here is numpy in float64 on inputs given as float32, except the comparison T > eps of `classify`, which is made on the
float32 transmittance the caller hands in (that IS the contract), and eps itself, which is the float32 value the kernels see."""
import numpy as np

import occ_numpy as R

F32 = np.float32


def segments(S, B):
    """[(s0, s1)] of the segments of B consecutive sample indices."""
    return [(s0, min(s0 + int(B), S)) for s0 in range(0, S, int(B))]


def factors(raw, z, rays11):
    """float64 [n, S]: 1 - alpha + 1e-10 of every sample, alpha = 1 - exp(-relu(sigma) dist), dist = z[i+1] - z[i] (1e10 for the
    last sample) times |d| (render.py:149-192)."""
    raw = np.asarray(raw, F32).astype(np.float64)
    z = np.asarray(z, F32).astype(np.float64)
    d = np.asarray(rays11, F32)[:, 3:6].astype(np.float64)
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((z.shape[0], 1), 1e10)], -1) * np.linalg.norm(d, axis=-1)[:, None]
    with np.errstate(over='ignore', invalid='ignore'):
        alpha = 1.0 - np.exp(-np.maximum(raw[..., 3], 0.0) * dist)
    return 1.0 - alpha + 1e-10


def advance(trans, raw, z, rays11, s0, s1):
    """float64 [n]: trans times the product of the factors of the samples s0 <= s < s1."""
    return np.asarray(trans, np.float64) * np.prod(factors(raw, z, rays11)[:, s0:s1], -1)


def classify(trans, eps, S, s0, s1, bits=None):
    """bool [n, s1 - s0]: the samples of the segment that are evaluated -- trans[ray] > eps as float32 numbers (None: every ray;
    a NaN is not > eps), AND the occupancy bits [n, S] when given.  The list is ray * S + s over the set entries, ascending."""
    n = bits.shape[0] if trans is None else len(trans)
    with np.errstate(invalid='ignore'):
        go = np.ones(n, bool) if trans is None else (np.asarray(trans, F32) > F32(eps))
    keep = np.broadcast_to(go[:, None], (n, s1 - s0)).copy()
    if bits is not None:
        keep &= np.asarray(bits, bool)[:, s0:s1]
    return keep


def live_list(keep, S, s0):
    """int64: the ascending sample indices ray * S + s of a segment's `keep`."""
    r, c = np.nonzero(keep)
    return r * S + s0 + c


def terminate(raw, z, rays11, eps, B, bits=None):
    """The image pass restated on the logits `raw` [n, S, 4] of the call WITHOUT ert (zeros where the grid masks): -> dict of
      keep     bool [n, S], the evaluated samples (the ert call's raw is raw * keep: an evaluated sample keeps its logits),
      t_start  float64 [n, number of segments], T of every ray at the start of every segment, as the ert call carries it (a
               skipped segment multiplies it by its zero logits' factors, (1 + 1e-10)^B),
      t_plain  float64 [n, number of segments], T at the start of every segment from `raw` itself,
      t_final  float64 [n], T after the last segment."""
    n, S = np.asarray(z).shape
    f = factors(raw, z, rays11)
    f0 = factors(np.zeros_like(np.asarray(raw, F32)), z, rays11)
    keep = np.zeros((n, S), bool)
    T = np.ones(n, np.float64)
    Tp = np.ones(n, np.float64)
    t_start, t_plain = [], []
    for s0, s1 in segments(S, B):
        t_start.append(T.copy())
        t_plain.append(Tp.copy())
        go = T > float(F32(eps))
        k = np.broadcast_to(go[:, None], (n, s1 - s0)).copy()
        if bits is not None:
            k &= np.asarray(bits, bool)[:, s0:s1]
        keep[:, s0:s1] = k
        T = T * np.prod(np.where(k, f[:, s0:s1], f0[:, s0:s1]), -1)
        Tp = Tp * np.prod(f[:, s0:s1], -1)
    return dict(keep=keep, t_start=np.stack(t_start, -1), t_plain=np.stack(t_plain, -1), t_final=T)


def weights64(raw, z, rays11):
    """float64 [n, S]: alpha_i prod_{j < i} (1 - alpha_j + 1e-10), the weights of raw2outputs."""
    f = factors(raw, z, rays11)
    T = np.concatenate([np.ones((f.shape[0], 1)), np.cumprod(f, -1)[:, :-1]], -1)
    return (1.0 + 1e-10 - f) * T


# ---- the scene of the GPU tests (validated on the oracle alone in tests/test_ert_cpu.py) ------------------------------------------
NS, NI = 64, 128
BIAS = 40.0      # added to alpha_linear.bias of both networks: random-init networks become opaque within a few samples


def scene_networks(O):
    sdc, sdf = R.scene_networks(O)
    for sd in (sdc, sdf):
        sd['alpha_linear.bias'] = sd['alpha_linear.bias'] + BIAS
    return sdc, sdf


def scene_rays(O):
    return R.scene_rays(O, side=13)      # 169 rays


def oracle_pass(O, rays11, sdc, sdf, grid, N_samples, N_importance):
    """The image pass of the scene without ert on the CPU oracle, at the oracle's own depths (perturb = 0): (raw [n, S, 4] float32
    with zeros where the grid masks, z [n, S], bits [n, S] or None).  The steps of occ_numpy.render_rays_masked, which does not
    hand out its depths."""
    import torch
    mask, lo, hi, oo = (None, None, None, None) if grid is None else grid
    rb = torch.as_tensor(rays11)
    z = O.coarse_z(rb[:, 6:7], rb[:, 7:8], N_samples, False, None)
    cls = lambda zz: None if mask is None else R.classify(mask, lo, hi, oo, rb.numpy(), zz.numpy())      # noqa: E731
    ones = lambda zz: np.ones(tuple(zz.shape), bool)      # noqa: E731
    b = cls(z)
    raw, _, _, w = R.composite_at(O, sdc, rb, z, ones(z) if b is None else b, False)
    if N_importance > 0:
        zs = O.sample_pdf(0.5 * (z[..., 1:] + z[..., :-1]), w[..., 1:-1], N_importance, None)
        z, _ = torch.sort(torch.cat([z, zs], -1), -1)
        b = cls(z)
        raw, _, _, _ = R.composite_at(O, sdf, rb, z, ones(z) if b is None else b, False)
    return raw.numpy().astype(F32), z.numpy().astype(F32), b
