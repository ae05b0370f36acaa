"""tests/rays_ref.py checked on the CPU: the fp32 evaluation against the oracle (bit for bit where the oracle orders its operations
like the kernels) and the goldens, the running-error bound against the goldens, and -- on exactly the input sets that
tests/test_gpu_rays_fp64.py feeds the kernels -- that the bound encloses the fp32 evaluation, is finite on all but 0.1 % of the
elements, and is left by one deliberately wrong evaluation of every formula."""
import os

import numpy as np
import pytest
import torch

import rays_ref as R
from oracle import nerf_oracle as O
from oracle import nerfpp_oracle as PP

F32 = np.float32
NONFINITE_CAP = 1e-3


def L(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def within(got, ref):
    r, fin = R.ratio(got, ref)
    return float(r.max()), float(1.0 - fin.mean())


def grid(H, W):
    i = np.arange(H * W)
    return i // W, i % W


# ---- (b) against the oracle --------------------------------------------------------------------------------------------------------
# Bit for bit: O.ndc_rays, PP.fg_depths, PP.perturb_samples and columns 0-7 of O.make_ray_batch (element-wise operations only).
# Within the running-error bound only, because the oracle orders or groups its operations differently from the kernel:
#   O.get_rays (torch.sum over the three products: its order is the CPU vector path's, not fixed; the goldens recorded from the
#   reference, g1_get_rays, equal the fp32 evaluation bit for bit: test_goldens_lie_within_the_bound)
#   O.ndc_rays columns 2 and 5 when near is no power of two (torch evaluates `2 near / z` as reciprocal(z) * (2 near), the kernel
#   divides 2 near by z; at the near = 1 that pack_rays uses, the product with 2 is exact and the two agree bit for bit)
#   O.coarse_z (torch.linspace on the CPU fills a vector at a time, base + step j from a per-vector base, so its upper half is not
#   the per-element end - step (S - 1 - i) of lin01; it agrees bit for bit below the midpoint and at S <= 5)
#   O.make_ray_batch columns 8-10 (torch.norm is not sqrt((x^2 + y^2) + z^2) rounded per operation)
#   PP.intersect_sphere (torch.sum / torch.norm reductions, and 1 / norm instead of 1 / sqrt(dd) from the kernel's own dd)
def test_emulation_equals_the_oracle():
    rs = np.random.RandomState(0)
    for H, W in ((6, 8), (13, 31)):
        c2w = R.random_pose(rs)
        K = np.array([[37.3, 0, 0.5 * W + 0.37], [0, 29.1, 0.5 * H - 0.81], [0, 0, 1]])
        o, d = O.get_rays(H, W, K, T(c2w))
        row, col = grid(H, W)
        re_, emu = R.both(R.pixel_ray, row, col, K[0][0], K[1][1], K[0][2], K[1][2], c2w.reshape(12))
        worst, nonfinite = within(d.numpy().reshape(-1, 3), re_)
        assert worst <= 1.0 and nonfinite == 0.0 and within(emu, re_)[0] <= 1.0
        assert np.array_equal(o.numpy().reshape(-1, 3), np.broadcast_to(c2w[:, 3], (H * W, 3)))
    ro, rd = R.ndc_inputs(500)
    Hn, Wn, focal = R.NDC_CAM
    for near in R.NDC_NEARS:
        no, nd = O.ndc_rays(Hn, Wn, focal, near, T(ro), T(rd))
        emu = R.ndc_one(R.F32K, R.ndc_scale(Wn, focal), R.ndc_scale(Hn, focal), near, ro, rd)
        ref = np.concatenate([no.numpy(), nd.numpy()], 1)
        same = [0, 1, 2, 3, 4, 5] if near == 1.0 else [0, 1, 3, 4]
        assert np.array_equal(ref[:, same], emu[:, same]), near
        worst, nonfinite = within(ref, R.ndc_one(R.REK, R.ndc_scale(Wn, focal), R.ndc_scale(Hn, focal), near, ro, rd))
        assert worst <= 1.0 and nonfinite == 0.0, near
    for ndc, (a, b) in ((False, R.pack_inputs(500)), (True, (ro, rd))):
        ref = O.make_ray_batch(T(a), T(b), 2.0, 6.0, H=Hn, W=Wn, focal=focal, ndc=ndc).numpy()
        re_, emu = R.both(R.pack_rays, a, b, 2.0, 6.0, ndc, R.ndc_scale(Wn, focal), R.ndc_scale(Hn, focal))
        assert np.array_equal(ref[:, :8], emu[:, :8]), ndc
        assert within(ref[:, 8:], R.RE(re_.v[:, 8:], re_.e[:, 8:]))[0] <= 1.0
    for S in R.COARSE_S:
        near, far, u = R.coarse_inputs(60, S)
        for lindisp in (False, True):
            for t in (None, u):
                ref = O.coarse_z(T(near)[:, None], T(far)[:, None], S, lindisp, None if t is None else T(t)).numpy()
                re_, emu = R.both(R.sample_coarse, near, far, S, lindisp, t)
                worst, nonfinite = within(ref, re_)
                assert worst <= 1.0 and nonfinite == 0.0, (S, lindisp, t is None)
                if S <= 3:
                    assert np.array_equal(ref, emu), (S, lindisp, t is None)
    for S in R.FG_S:
        far, u = R.fg_inputs(60, S)
        z0 = PP.fg_depths(T(far), R.FG_NEAR * torch.ones(60), S)
        assert np.array_equal(z0.numpy(), R.fg_depths(R.F32K, far, R.FG_NEAR, S)), S
        assert np.array_equal(PP.perturb_samples(z0, T(u)).numpy(), R.fg_depths(R.F32K, far, R.FG_NEAR, S, u)), S
    for S in (1,) + R.FG_S:
        z, u = R.perturb_inputs(60, S)
        assert np.array_equal(PP.perturb_samples(T(z), T(u)).numpy(), R.perturb_samples(R.F32K, z, u)), S
    rays, _ = R.sphere_inputs(500)
    (far_re, _), (far_emu, _) = R.both(R.intersect_sphere, rays)
    ref = PP.intersect_sphere(T(rays[:, :3]), T(rays[:, 3:6])).numpy()
    assert within(ref, far_re)[0] <= 1.0 and within(far_emu, far_re)[0] <= 1.0


# ---- (a) and (b) against the goldens recorded from the reference -------------------------------------------------------------------
def test_goldens_lie_within_the_bound(golden_dir):
    g = L(golden_dir, 'g1_get_rays.npz')
    row, col = grid(6, 8)
    re_, emu = R.both(R.pixel_ray, row, col, 10.0, 10.0, 4.0, 3.0, g['c2w'].reshape(12))
    assert within(g['small_d'].reshape(-1, 3), re_)[0] <= 1.0 and np.array_equal(emu, g['small_d'].reshape(-1, 3))
    K = g['K']
    re_, emu = R.both(R.pixel_ray, g['idx'][:, 0], g['idx'][:, 1], K[0][0], K[1][1], K[0][2], K[1][2], g['c2w'].reshape(12))
    assert within(g['big_d'], re_)[0] <= 1.0 and np.array_equal(emu, g['big_d'])
    g = L(golden_dir, 'g2_ndc.npz')
    H, W, focal = int(g['H']), int(g['W']), float(g['focal'])
    re_, emu = R.both(R.ndc_one, R.ndc_scale(W, focal), R.ndc_scale(H, focal), 1.0, g['ro'], g['rd'])
    gold = np.concatenate([g['no'], g['nd']], 1)
    assert within(gold, re_)[0] <= 1.0 and within(gold, re_)[1] == 0.0 and np.array_equal(emu, gold)
    g = L(golden_dir, 'g10_pp_ops.npz')
    rd = PP.get_rays_single_image(6, 8, g['intr'], g['c2w'])[1]
    v, bound, _ = R.pp_gen_rays_ref(6, 8, g['intr'], g['c2w'])
    assert (np.abs(rd.astype(F32) - v) <= bound).all() and (np.abs(g['rd_s'].astype(F32) - v) <= bound).all()
    rays = np.zeros((40, 11), dtype=F32)
    rays[:, :3], rays[:, 3:6] = g['ray_o'], g['ray_d']
    far_re, pn2 = R.intersect_sphere(R.REK, rays)
    assert within(g['fg_far'], far_re)[0] <= 1.0 and (pn2.v < 1).all()
    g = L(golden_dir, 'g3_embed.npz')
    for Lf, key in ((10, 'e10'), (4, 'e4')):
        assert np.abs(g[key] - R.posenc_ref(g['x'], Lf)).max() <= 2e-6
        assert np.array_equal(g[key][:, :3], g['x'])


def test_posenc_and_pp_gen_rays_references():
    """numpy's fp32 sin / cos of the exact argument lies within the 2e-6 cap of the float64 reference on the GPU test's inputs and
    the next band does not; the kernel's own fp64 route for pp_gen_rays lies within the bound and dropping the + 0.5 does not."""
    for Lf, n in R.POSENC_BIG.items():
        x = R.posenc_inputs(n)
        ref = R.posenc_ref(x, Lf)
        assert ref.shape == (n, 3 + 6 * Lf) and ref.size > R.GRID
        assert np.array_equal(ref[:, :3].astype(F32), x) and (x == 0).any() and (x == 8).any() and (x == -8).any()
        assert np.abs(x).max() == 8.0 and np.abs(x[x != 0]).min() >= F32(1e-3)
        err = np.abs(R.posenc_ref(x, Lf, dtype=F32) - ref).max()
        print('POSENC L=%d: numpy fp32 against float64 %.2f u' % (Lf, err / R.U))
        assert err <= 2e-6
        assert np.abs(R.posenc_ref(x, Lf, dtype=F32, wrong='next_band') - ref).max() > 2e-6
    K, M = R.pp_camera()
    for H, W in ((6, 8), R.IMG_BIG):
        v, bound, origin = R.pp_gen_rays_ref(H, W, K, M)
        emu = R.pp_gen_rays_emu(H, W, K, M)
        worst = float((np.abs(emu - v) / bound).max())
        print('PP_GEN_RAYS %dx%d: max |emu - v| / bound = %.3f' % (H, W, worst))
        assert worst <= 1.0 and np.isfinite(bound).all()
        bad = R.pp_gen_rays_ref(H, W, K, M, wrong='no_half')[0].astype(F32)
        assert (np.abs(bad - v) > bound).any()


# ---- the bound on the GPU test's own inputs: enclosure, finiteness, sensitivity ----------------------------------------------------
def coarse_n(S):
    return (R.N_SAMPLE_RAYS,) if S != 64 else (1, 257, R.N_SAMPLE_RAYS)


def formula_cases():
    """(id, thunk -> (RE, fp32 evaluation, a wrong fp32 evaluation or None)) for every input set of tests/test_gpu_rays_fp64.py."""
    cam = R.CAMERA
    Hn, Wn, focal = R.NDC_CAM
    sx, sy = R.ndc_scale(Wn, focal), R.ndc_scale(Hn, focal)
    out = []

    def add(name, formula, args, wrong_args=None, wrong_kw=None, pick=None, **kw):
        def thunk():
            re_, emu = R.both(formula, *args, **kw)
            bad = formula(R.F32K, *(wrong_args or args), **dict(kw, **(wrong_kw or {})))
            return (re_, emu, bad) if pick is None else (re_[pick], emu[pick], bad[pick])
        out.append(pytest.param(thunk, id=name))

    for H, W, c2w in R.gen_rays_inputs():
        row, col = grid(H, W)
        add('gen_rays-%dx%d' % (H, W), R.pixel_ray, (row, col, cam['fx'], cam['fy'], cam['cx'], cam['cy'], c2w.reshape(12)),
            (row, col, cam['fx'], cam['fy'], cam['cy'], cam['cx'], c2w.reshape(12)))
    for n in (1, 257, R.N_RAYS_BIG):
        pix, poses = R.gen_rays_pixels_inputs(n)
        c = poses.reshape(-1, 12)[pix[:, 0]]
        add('gen_rays_pixels-%d' % n, R.pixel_ray, (pix[:, 1], pix[:, 2], cam['fx'], cam['fy'], cam['cx'], cam['cy'], c),
            (pix[:, 1], pix[:, 2], cam['fy'], cam['fx'], cam['cx'], cam['cy'], c))
        ro, rd = R.ndc_inputs(n)
        for near in R.NDC_NEARS:
            add('ndc_rays-%d-near%g' % (n, near), R.ndc_one, (sx, sy, near, ro, rd), (sy, sy, near, ro, rd))
        add('pack_rays-ndc-%d' % n, R.pack_rays, (ro, rd, 0.0, 1.0, True, sx, sy), (ro, rd, 0.0, 1.0, True, sy, sy))
        ro, rd = R.pack_inputs(n)
        add('pack_rays-%d' % n, R.pack_rays, (ro, rd, 2.0, 6.0), (ro, rd[:, [0, 2, 1]], 2.0, 6.0))
        rays, _ = R.sphere_inputs(n)
        add('pp_intersect_sphere-%d' % n, R.intersect_sphere, (rays,), (rays[:, [0, 1, 2, 3, 5, 4, 6, 7, 8, 9, 10]],), pick=0)
        if n > 1:
            rays, _ = R.sphere_inputs(n, outside=True)
            add('pp_intersect_sphere-outside-%d' % n, R.intersect_sphere, (rays,), (rays[:, [0, 1, 2, 3, 5, 4, 6, 7, 8, 9, 10]],),
                pick=0)
    for S in R.COARSE_S:
        for n in coarse_n(S):
            near, far, u = R.coarse_inputs(n, S)
            for lindisp in (False, True):
                add('sample_coarse-S%d-n%d-lindisp%d' % (S, n, lindisp), R.sample_coarse, (near, far, S, lindisp),
                    wrong_kw=dict(wrong='step_1_over_S'))
                add('sample_coarse-S%d-n%d-lindisp%d-jitter' % (S, n, lindisp), R.sample_coarse, (near, far, S, lindisp, u),
                    wrong_kw=dict(wrong='pm2'))
    for S in R.FG_S:
        for n in coarse_n(S):
            far, u = R.fg_inputs(n, S)
            add('pp_fg_depths-S%d-n%d' % (S, n), R.fg_depths, (far, R.FG_NEAR, S), (far, 2 * R.FG_NEAR, S))
            add('pp_fg_depths-S%d-n%d-jitter' % (S, n), R.fg_depths, (far, R.FG_NEAR, S, u), wrong_kw=dict(wrong='zat_s'))
    for S in (1,) + R.FG_S:
        for n in coarse_n(S):
            z, u = R.perturb_inputs(n, S)
            add('pp_perturb_samples-S%d-n%d' % (S, n), R.perturb_samples, (z, u), wrong_kw=dict(wrong='pm2'))
    return out


# where a wrong evaluation cannot differ: one element, or a formula that does not use what the mutation changes
SAME_WHEN_WRONG = ('sample_coarse-S1-', 'sample_coarse-S2-', 'pp_perturb_samples-S1-', 'pp_perturb_samples-S2-')


@pytest.mark.parametrize('thunk', formula_cases())
def test_bound_encloses_the_emulation_and_is_sensitive(thunk, request):
    re_, emu, bad = thunk()
    worst, nonfinite = within(emu, re_)
    med = float(np.median(re_.e[np.isfinite(re_.e) & (re_.v != 0)] / np.abs(re_.v[np.isfinite(re_.e) & (re_.v != 0)])) / R.U) \
        if (re_.v != 0).any() else 0.0
    print('ENCLOSE %s: max |emu - v| / e = %.3f, non-finite e %.4f %%, median e %.1f u |v|' % (
        request.node.callspec.id, worst, 100 * nonfinite, med))
    assert worst <= 1.0
    assert nonfinite <= NONFINITE_CAP
    assert np.array_equal(np.isnan(emu), np.isnan(re_.v))
    if not request.node.callspec.id.startswith(SAME_WHEN_WRONG):
        assert within(bad, re_)[0] > 1.0, 'the wrong evaluation stays within the bound'


def test_lin01_first_branch_is_a_reordering_the_bound_cannot_see():
    """lin01 without its symmetric branch evaluates the same real number in another order: it stays within e, and only the
    bit-equality with the fp32 evaluation tells the two apart (which is how the GPU test catches that mutant)."""
    for S in (64, 192):
        near, far, _ = R.coarse_inputs(257, S)
        for lindisp in (False, True):
            re_, emu = R.both(R.sample_coarse, near, far, S, lindisp)
            bad = R.sample_coarse(R.F32K, near, far, S, lindisp, wrong='first_branch')
            assert within(bad, re_)[0] <= 1.0 and not np.array_equal(bad, emu)
