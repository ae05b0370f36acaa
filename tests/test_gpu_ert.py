"""Early ray termination on the GPU against the float64 restatement of tests/ert_numpy.py: fastnerf_ert_classify bit for bit,
fastnerf_ert_advance within fp32 rounding, and render_rays(..., ert=eps, ert_block=B) against the call without `ert` on the scene
that tests/test_ert_cpu.py validates on the CPU oracle: every row kept bit for bit or zeroed, the coarse pass untouched, the error
bounds of the contract, the two exact cases (eps = 0, one segment), the error paths and the chunked render."""
import numpy as np
import pytest
import torch

import ert_numpy as E
import occ_cascade_numpy as RC
import occ_numpy as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

NS, NI = E.NS, E.NI
SUM_MARGIN = 1.2e-5      # rounding of a 192-term fp32 sum of weights <= 1: 192 * 2^-24


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


def same_bits(a, b):
    """torch.equal on the bit patterns (disp_map may be NaN on a ray without any weight, in the plain render too)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def ball(fn):
    m, lo, hi, oo = R.scene_grids()['ball']
    return fn.occupancy.OccupancyGrid.from_mask(torch.from_numpy(m).cuda(), lo, hi, oo), (m, lo, hi, oo)


def cascade2(fn):
    """The first two levels of the cascade scene; a sample that neither box contains counts as occupied."""
    levels = RC.scene_cascade()[0][:2]
    grids = [fn.occupancy.OccupancyGrid.from_mask(torch.from_numpy(m).cuda(), lo, hi, False) for m, lo, hi in levels]
    return fn.occupancy.OccupancyCascade(grids, outside_occupied=True), levels


def networks(fn, **over):
    """create_nerf's render kwargs with the scene's opaque networks (ert_numpy.scene_networks) loaded."""
    kw = dict(N_importance=NI, N_samples=NS, perturb=0., white_bkgd=False, use_viewdirs=True, no_reload=True)
    kw.update(over)
    _, kte, _, _, _, _ = fn.run_nerf.create_nerf(fn.run_nerf.make_args(**kw))
    sdc, sdf = E.scene_networks(O)
    kte['network_fn'].load_state_dict(sdc)
    if kte.get('network_fine') is not None:
        kte['network_fine'].load_state_dict(sdf)
    return kte


# ---- 1. classify -------------------------------------------------------------------------------------------------------------------
# (169, 192, 32): whole segments, 169 * 32 no multiple of the 1024-entry block, several blocks; (37, 13, 5): a partial last segment and
# a thread's four consecutive entries straddling two rays; (300, 7, 7): one segment, three blocks (the scanned offsets are used);
# (300, 7, 2): segments of 2 and a last one of 1
@pytest.mark.parametrize('n,S,B', [(169, 192, 32), (37, 13, 5), (300, 7, 7), (300, 7, 2)])
@pytest.mark.parametrize('case', ['none', 'ball', 'cascade'])
def test_classify_equals_the_restatement(fn, n, S, B, case):
    rs = np.random.RandomState(S + B)
    rays = R.scene_rays(O, side=13 if n <= 169 else 18)
    rays = rays[np.round(np.linspace(0, rays.shape[0] - 1, n)).astype(int)]
    z = np.sort(2.0 + 4.0 * rs.rand(n, S).astype(np.float32), -1)
    eps = np.float32(1e-2)
    trans = (rs.rand(n) * 0.03).astype(np.float32)      # around eps: about a third of the rays pass
    trans[:6] = [eps, np.nextafter(eps, np.float32(1)), np.nextafter(eps, np.float32(0)), 0.0, 1.0, np.nan]
    trans = trans[rs.permutation(n)]
    cgrid, bits = None, None
    if case == 'ball':
        g, gm = ball(fn)
        cgrid, bits = g._c, R.classify(*gm, rays, z)
    elif case == 'cascade':
        c, levels = cascade2(fn)
        cgrid, bits = c._c, RC.classify(levels, True, rays, z)
    rays_t, z_t, trans_t = (torch.from_numpy(a).cuda() for a in (rays, z, trans))
    seen = 0
    for k, (s0, s1) in enumerate(E.segments(S, B)):
        for tr, tr_t in ((trans, trans_t),) + (((None, None),) if k == 0 else ()):      # trans None: every ray passes
            keep = E.classify(tr, eps, S, s0, s1, bits if bits is not None else np.ones((n, S), bool))
            live = E.live_list(keep, S, s0)
            raw = torch.full((n, S, 4), 7.0, device='cuda')
            idx, cnt = fn.ops.ert_classify(rays_t, z_t, s0, s1, tr_t, float(eps), cgrid, raw)
            assert cnt.tolist() == [live.size, n * (s1 - s0)], (k, cnt.tolist(), live.size)
            assert np.array_equal(idx[:live.size].cpu().numpy(), live), k
            zero = (raw == 0).all(-1).cpu().numpy()
            want = np.zeros((n, S), bool)
            want[:, s0:s1] = ~keep
            assert np.array_equal(zero, want), 'zero logits for the other samples of the segment, and for nothing else'
            assert bool((raw[torch.from_numpy(~want).cuda()] == 7.0).all()), 'nothing else is written'
            idx2, cnt2 = fn.ops.ert_classify(rays_t, z_t, s0, s1, tr_t, float(eps), cgrid)      # raw is optional
            assert torch.equal(cnt, cnt2) and torch.equal(idx[:live.size], idx2[:live.size])
            seen += live.size
    assert seen > 0
    with pytest.raises(RuntimeError):
        fn.ops.ert_classify(rays_t, z_t, 0, S + 1, trans_t, float(eps), cgrid)


# ---- 2. advance --------------------------------------------------------------------------------------------------------------------
def advance_inputs(n, S, seed, huge):
    """sigma chosen so that x = relu(sigma) dist |d| is 0 (sigma <= 0), in (0, 0.2] or (huge) > 200: a factor 1 - alpha + 1e-10 is then
    1, >= 0.81, or exactly 1e-10 in fp32 and 1e-10 (1 + < 1e-70) in float64.  A factor t >= 0.81 carries at most 2^-24 / 0.81 = 7.3e-8
    from the two subtractions, two ulp (1.2e-7) from expf, one rounding (6e-8) of the running product, and 0.2 * 4 * 2^-24 = 4.8e-8 from
    the roundings of x (sigma dist, times |d|, and |d| itself): 3.0e-7, so a segment of up to 32 factors stays within 9.6e-6 < 1e-5
    of the float64 product even if every error has the same sign."""
    rs = np.random.RandomState(seed)
    rays = R.scene_rays(O, side=13 if n <= 169 else 18)
    rays = rays[np.round(np.linspace(0, rays.shape[0] - 1, n)).astype(int)]
    z = np.sort(2.0 + 4.0 * rs.rand(n, S).astype(np.float32), -1)
    dist = np.concatenate([np.diff(z.astype(np.float64), axis=-1), np.full((n, 1), 1e10)], -1) * np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=-1)[:, None]
    x = rs.rand(n, S) * 0.2
    sigma = x / np.maximum(dist, 1e-6)
    sigma[:, -1] = 0.5 + rs.rand(n)      # the last sample: 1e10 |d| times any positive sigma saturates
    sigma[rs.rand(n, S) < 0.3] *= -1.0      # sigma <= 0, exact zeros among them
    sigma[rs.rand(n, S) < 0.05] = 0.0
    if huge:
        sigma[rs.rand(n, S) < 0.02] = 1e9
    raw = (rs.randn(n, S, 4) * 3).astype(np.float32)
    raw[..., 3] = sigma.astype(np.float32)
    return rays, z, raw


FLOOR = 1.2e-38      # below the smallest normal fp32 number a product carries no relative precision


@pytest.mark.parametrize('n,S,B', [(169, 192, 32), (37, 13, 5), (300, 7, 7), (300, 7, 2)])
def test_advance_equals_the_restatement(fn, n, S, B):
    rays, z, raw = advance_inputs(n, S, S * B, huge=True)
    rays_t, z_t, raw_t = (torch.from_numpy(a).cuda() for a in (rays, z, raw))
    rs = np.random.RandomState(1)
    t0 = rs.rand(n).astype(np.float32)
    t0[:3] = [0.0, 1.0, 1e-30]
    worst = 0.0
    for k, (s0, s1) in enumerate(E.segments(S, B)):
        ref = E.advance(t0, raw, z, rays, s0, s1)
        got = fn.ops.ert_advance(raw_t, z_t, rays_t, s0, s1, torch.from_numpy(t0).cuda()).cpu().numpy().astype(np.float64)
        err = np.abs(got - ref) / np.maximum(ref, FLOOR)
        worst = max(worst, float(err[ref > FLOOR].max()))
        assert (np.abs(got - ref) <= 1e-5 * ref + FLOOR).all(), (k, float(err.max()))
        assert got[0] == 0.0, 'an exact zero stays an exact zero'
        first = fn.ops.ert_advance(raw_t, z_t, rays_t, s0, s1, torch.full((n,), 7.0, device='cuda'), first=True).cpu().numpy()
        ones = fn.ops.ert_advance(raw_t, z_t, rays_t, s0, s1, torch.ones(n, device='cuda')).cpu().numpy()
        assert np.array_equal(first, ones), 'first: the old value is not read'
    print('advance (%d, %d, %d): largest relative error of a segment product %.3g' % (n, S, B, worst))
    # the counters: total[0] (0 when first) += seg_count[0], total[1] = n * S
    seg = torch.tensor([5, 99], device='cuda', dtype=torch.int32)
    total = torch.tensor([1000, -1], device='cuda', dtype=torch.int32)
    t = torch.ones(n, device='cuda')
    fn.ops.ert_advance(raw_t, z_t, rays_t, 0, min(B, S), t, first=True, seg_count=seg, total=total)
    assert total.tolist() == [5, n * S]
    fn.ops.ert_advance(raw_t, z_t, rays_t, 0, min(B, S), t, seg_count=seg, total=total)
    assert total.tolist() == [10, n * S]


@pytest.mark.parametrize('n,S,B', [(169, 192, 32), (37, 13, 5)])
def test_chained_segments_are_the_transmittance_of_the_compositing_kernel(fn, n, S, B):
    """T at the start of every segment k >= 1, chained on the GPU over all segments before it, against the transmittance that
    fastnerf_raw2outputs_fwd's weights imply there -- w_i / alpha_i at the segment's first sample, where alpha_i >= 0.1 (alpha in
    float64 from the restatement) -- and against the float64 chain: relative 1e-5, the margin of one segment, for the whole chain."""
    rays, z, raw = advance_inputs(n, S, 7 * S + B, huge=False)
    raw[:, :-1, 3] = np.abs(raw[:, :-1, 3])      # every factor < 1: alpha >= 0.1 is frequent
    rays_t, z_t, raw_t = (torch.from_numpy(a).cuda() for a in (rays, z, raw))
    w = fn.ops.raw2outputs_fwd(raw_t, z_t, rays_t, None, False)[3].cpu().numpy().astype(np.float64)
    alpha = 1.0 + 1e-10 - E.factors(raw, z, rays)
    T = torch.ones(n, device='cuda')
    T64 = np.ones(n)
    checked, worst_w, worst_64 = 0, 0.0, 0.0
    for k, (s0, s1) in enumerate(E.segments(S, B)):
        if k:
            ok = alpha[:, s0] >= 0.1
            got = T.cpu().numpy().astype(np.float64)[ok]
            implied = w[ok, s0] / alpha[ok, s0]
            e_w, e_64 = np.abs(got - implied) / implied, np.abs(got - T64[ok]) / T64[ok]
            worst_w, worst_64 = max(worst_w, float(e_w.max())), max(worst_64, float(e_64.max()))
            print('chain (%d, %d, %d) at segment %d: largest relative error %.3g against the weights, %.3g against float64' % (n, S, B, k, e_w.max(), e_64.max()))
            assert (e_w <= 1e-5).all() and (e_64 <= 1e-5).all(), k
            checked += int(ok.sum())
        fn.ops.ert_advance(raw_t, z_t, rays_t, s0, s1, T, first=(k == 0))
        T64 = E.advance(T64, raw, z, rays, s0, s1)
    assert checked > n // 4 and float(T64.min()) > 1e-30


@pytest.mark.parametrize('n,S,B', [(37, 13, 1), (300, 7, 2)])
def test_advance_in_the_mid_range(fn, n, S, B):
    """x = relu(sigma) dist |d| log-uniform in (0.2, 200), where 1 - alpha has lost its relative precision: a factor t = 1 - alpha + 1e-10 is
    then known absolutely.  alpha = 1 - expf(-x) is rounded to half an ulp of [0.5, 1), 2^-25; expf is within two ulp, 2^-23 e^-x; the
    four roundings of x (sigma dist, times |d|, and |d| itself) move e^-x by at most 4 * 2^-24 x e^-x <= 4 * 2^-24 / e; 1 - alpha is exact:
    under 4 * 2^-24 per factor.  With factors <= 1 a product of B of them, started at T = 1, is within B * 4 * 2^-24 of the float64
    product (its own roundings are relative 2^-24 of a value <= 1 each: + B * 2^-24).  A dist or |d| that is off on an ordinary sample
    moves a factor by a multiple of 1e-2 here."""
    rs = np.random.RandomState(S + B)
    rays = R.scene_rays(O, side=13 if n <= 169 else 18)
    rays = rays[np.round(np.linspace(0, rays.shape[0] - 1, n)).astype(int)]
    z = np.sort(2.0 + 4.0 * rs.rand(n, S).astype(np.float32), -1)
    dist = np.concatenate([np.diff(z.astype(np.float64), axis=-1), np.ones((n, 1))], -1) * np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=-1)[:, None]
    x = 0.2 * 1000.0 ** rs.rand(n, S)
    raw = (rs.randn(n, S, 4) * 3).astype(np.float32)
    raw[..., 3] = (x / np.maximum(dist, 1e-6)).astype(np.float32)
    raw[:, -1, 3] = -1.0      # (the last sample's 1e10 has its own case above)
    rays_t, z_t, raw_t = (torch.from_numpy(a).cuda() for a in (rays, z, raw))
    bound = B * 5 * 2.0 ** -24
    worst = 0.0
    for s0, s1 in E.segments(S, B):
        ref = E.advance(np.ones(n), raw, z, rays, s0, s1)
        got = fn.ops.ert_advance(raw_t, z_t, rays_t, s0, s1, torch.ones(n, device='cuda')).cpu().numpy().astype(np.float64)
        worst = max(worst, float(np.abs(got - ref).max()))
        assert (np.abs(got - ref) <= bound).all(), (s0, float(np.abs(got - ref).max()))
    f = E.factors(raw, z, rays)[:, :-1]
    assert 0.05 < float(((f > 1e-3) & (f < 0.8)).mean()), 'the factors fill the middle of (0, 1)'
    print('advance, mid range (%d, %d, %d): largest absolute error of a segment product %.3g (bound %.3g)' % (n, S, B, worst, bound))


# ---- 3. the render -----------------------------------------------------------------------------------------------------------------
def forward(fn, kte, rays_t, white_bkgd, occupancy=None, ert=None, B=32, NS_=NS, NI_=NI):
    net_c, net_f = kte['network_fn'], kte.get('network_fine') if NI_ > 0 else None
    with torch.no_grad():
        if ert is not None:
            return fn.render._forward_ert(rays_t, net_c, net_f, NS_, NI_, False, 0., white_bkgd, None, None, ert, B, occupancy=occupancy)
        if occupancy is not None:
            return fn.render._forward_occ(rays_t, net_c, net_f, NS_, NI_, False, 0., white_bkgd, None, None, occupancy)
        return fn.render._forward_core(rays_t, net_c, net_f, NS_, NI_, False, 0., white_bkgd, None, None, None, None, False)[0]


def check_contract(fn, plain, out, rays, eps, B, white_bkgd, two):
    """The properties of the contract on the outputs of one call with and one without ert.  Returns the evaluated share."""
    raw_p, raw_e = plain['raw'].cpu(), out['raw'].cpu()
    z = plain['z_vals'].cpu().numpy()
    n, S = z.shape
    e = float(np.float32(eps))
    for k in (('z0', 'raw0', 'rgb0', 'disp0', 'acc0', 'z_std', 'z_vals', 'z_samples', 'depth0', 'weights0') if two else ('z_vals',)):
        if k in plain and k in out:
            assert same_bits(plain[k], out[k]), k + ': the coarse pass and the depths are not touched'
    equal = (raw_p.view(torch.int32) == raw_e.view(torch.int32)).all(-1).numpy()
    zero = (raw_e == 0).all(-1).numpy()
    assert (equal | zero).all(), 'every row is the plain call\'s row bit for bit, or zeros'
    live_p = ~(raw_p == 0).all(-1).numpy()
    t = E.terminate(raw_p.numpy(), z, rays, eps, B)['t_plain']      # float64, from the plain logits
    seg = np.repeat(np.arange(t.shape[1]), B)[:S]
    t_row = t[:, seg]
    skipped, kept = zero & live_p, equal & live_p
    later = t_row[kept & (seg > 0)[None]]      # kept rows of the segments k >= 1 (none when every ray ends within its first segment)
    assert skipped.any() and kept.any()
    print('eps %g B %d: %d of %d live rows skipped; largest T at the start of a skipped row\'s segment %.4g, smallest of a kept row\'s %.4g'
          % (eps, B, skipped.sum(), live_p.sum(), t_row[skipped].max(), later.min() if later.size else float('nan')))
    assert (t_row[skipped] <= e * (1 + 1e-3)).all()
    assert (later > e * (1 - 1e-3)).all()
    d_rgb = float((out['rgb_map'] - plain['rgb_map']).abs().max())
    d_acc = (plain['acc_map'] - out['acc_map']).cpu().numpy()
    d_depth = float((out['depth_map'] - plain['depth_map']).abs().max())
    print('max |d rgb_map| = %.3g, acc_plain - acc_ert in [%.3g, %.3g], max |d depth_map| = %.3g' % (d_rgb, d_acc.min(), d_acc.max(), d_depth))
    assert d_rgb <= e + SUM_MARGIN
    assert -SUM_MARGIN <= d_acc.min() and d_acc.max() <= e + SUM_MARGIN
    assert d_depth <= (e + SUM_MARGIN) * float(z.max())
    # counts: (evaluated, total) of the coarse pass (as without ert), then of the fine pass
    c = out['counts'].tolist()
    img = c[2:] if two else c[:2]
    assert img == [int((~zero).sum()), n * S], 'a row that ran through the network is not all zeros on this scene'
    if two:
        assert c[:2] == (plain['counts'].tolist()[:2] if 'counts' in plain else [n * NS, n * NS])
    return img[0] / img[1]


@pytest.mark.parametrize('white_bkgd', [False, True])
@pytest.mark.parametrize('grid', [None, 'ball'])
@pytest.mark.parametrize('eps,B', [(1e-2, 16), (1e-3, 32)])
def test_render_meets_the_contract(fn, math_mode, grid, white_bkgd, eps, B):
    kte = networks(fn, white_bkgd=white_bkgd)
    rays = E.scene_rays(O)
    rays_t = torch.from_numpy(rays).cuda()
    g = ball(fn)[0] if grid else None
    plain = forward(fn, kte, rays_t, white_bkgd, occupancy=g)
    out = forward(fn, kte, rays_t, white_bkgd, occupancy=g, ert=eps, B=B)
    share = check_contract(fn, plain, out, rays, eps, B, white_bkgd, two=True)
    if (eps, B) == (1e-2, 16):      # the shares that tests/test_ert_cpu.py finds on the oracle
        if g is None:
            assert share <= 0.75
        else:
            assert share < plain['counts'][2].item() / plain['counts'][3].item()
    if g is None:      # (_forward_core does not hand out the coarse logits)
        net = kte['network_fn']
        assert same_bits(out['raw0'], fn.ops.mlp_fwd(rays_t, plain['z0'], net.flat, net.packed()[0]))
        assert float(out['trans'].max()) <= 1e-2, 'every ray of the scene terminates'
    # the public call returns these maps
    args = {k: kte[k] for k in ('network_fn', 'network_fine', 'network_query_fn', 'N_samples', 'N_importance')}
    with torch.no_grad():
        ret = fn.render.render_rays(rays_t, white_bkgd=white_bkgd, retraw=True, retdepth=True, occupancy=g, ert=eps, ert_block=B, **args)
    for k in ('rgb_map', 'disp_map', 'acc_map', 'depth_map', 'raw', 'rgb0', 'disp0', 'acc0', 'z_std', 'depth0'):
        assert same_bits(ret[k], out[k]), k


# ---- 4. the exact cases ------------------------------------------------------------------------------------------------------------
def render_rays(fn, kte, rays_t, **kw):
    args = {k: kte[k] for k in ('network_fn', 'network_fine', 'network_query_fn', 'N_samples', 'N_importance', 'white_bkgd')}
    args.update(kw)
    with torch.no_grad():
        return fn.render.render_rays(rays_t, **args)


@pytest.mark.parametrize('occ', ['none', 'ball', 'cascade'])
def test_eps_zero_and_one_segment_are_exact(fn, math_mode, occ):
    kte = networks(fn, white_bkgd=True)
    rays_t = torch.from_numpy(E.scene_rays(O)).cuda()
    g = {'none': None, 'ball': ball(fn)[0], 'cascade': cascade2(fn)[0]}[occ]
    for retraw in (True, False):
        a = render_rays(fn, kte, rays_t, retraw=retraw, retdepth=True, occupancy=g)
        for B in (32, 16):      # eps = 0: a segment is skipped only once T is exactly 0 -- every map, bit for bit
            b = render_rays(fn, kte, rays_t, retraw=retraw, retdepth=True, occupancy=g, ert=0.0, ert_block=B)
            assert sorted(a) == sorted(b)
            for k in a:
                assert k == 'raw' or same_bits(a[k], b[k]), (k, B, retraw)
        if retraw and occ == 'none':
            skipped = int(((b['raw'] == 0).all(-1) & ~(a['raw'] == 0).all(-1)).sum())
            print('eps = 0, B = 16, %s: %d rows skipped behind T == 0' % (occ, skipped))
            assert skipped > 0, 'T underflows before the last segment of 16 on this scene (on the oracle: on every ray): the case is not empty'
        for B in (NS + NI, 1000):      # one segment: everything, raw included
            b = render_rays(fn, kte, rays_t, retraw=retraw, retdepth=True, occupancy=g, ert=1e-2, ert_block=B)
            assert sorted(a) == sorted(b)
            for k in a:
                assert same_bits(a[k], b[k]), (k, B, retraw)


# ---- 5. one pass -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', [None, 'ball'])
def test_one_pass_render_meets_the_contract(fn, math_mode, grid):
    kte = networks(fn, N_importance=0, N_samples=192)
    rays = E.scene_rays(O)
    rays_t = torch.from_numpy(rays).cuda()
    g = ball(fn)[0] if grid else None
    plain = forward(fn, kte, rays_t, False, occupancy=g, NS_=192, NI_=0)
    out = forward(fn, kte, rays_t, False, occupancy=g, ert=1e-2, B=16, NS_=192, NI_=0)
    share = check_contract(fn, plain, out, rays, 1e-2, 16, False, two=False)
    if g is None:
        assert share <= 0.25
    assert out['counts'].tolist()[2:] == [0, 0]
    exact = forward(fn, kte, rays_t, False, occupancy=g, ert=0.0, B=16, NS_=192, NI_=0)
    one = forward(fn, kte, rays_t, False, occupancy=g, ert=1e-2, B=192, NS_=192, NI_=0)
    for k in ('rgb_map', 'disp_map', 'acc_map', 'depth_map'):
        assert same_bits(exact[k], plain[k]) and same_bits(one[k], plain[k]), k
    assert same_bits(one['raw'], plain['raw'])


# ---- 6. the error paths ------------------------------------------------------------------------------------------------------------
def test_errors(fn):
    kte = networks(fn)
    rays_t = torch.from_numpy(E.scene_rays(O)).cuda()
    args = {k: kte[k] for k in ('network_fn', 'network_fine', 'network_query_fn', 'N_samples', 'N_importance')}
    with torch.no_grad():
        with pytest.raises(ValueError, match='raw_noise_std'):
            fn.render.render_rays(rays_t, raw_noise_std=1.0, ert=1e-2, **args)
        for bad in (dict(ert=1.0), dict(ert=-1e-3), dict(ert=float('nan')), dict(ert=1e-2, ert_block=0), dict(ert=1e-2, ert_block=-4)):
            with pytest.raises(ValueError, match='ert'):
                fn.render.render_rays(rays_t, **bad, **args)
    assert any(p.requires_grad for p in kte['network_fn'].parameters())
    with pytest.raises(ValueError, match='inference feature'):
        fn.render.render_rays(rays_t, ert=1e-2, **args)      # grad mode on, parameters require grad
    tiny = torch.nn.Linear(3, 4).cuda()
    with torch.no_grad():
        with pytest.raises(NotImplementedError):
            fn.render.render_rays(rays_t, tiny, lambda p, v, net: net(p), NS, ert=1e-2)
        ok = fn.render.render_rays(rays_t, tiny, lambda p, v, net: net(p), NS)      # the closure route itself is untouched
    assert ok['rgb_map'].shape == (rays_t.shape[0], 3)


# ---- 7. the surface ----------------------------------------------------------------------------------------------------------------
def test_render_and_render_path_pass_ert_through(fn):
    kte = networks(fn, white_bkgd=True)
    g = ball(fn)[0]
    H = W = 13
    K = np.array([[14.0 * 13 / 8, 0, 6.5], [0, 14.0 * 13 / 8, 6.5], [0, 0, 1]])
    c2w = fn.synthetic.pose_spherical(30.0, -30.0, 4.0)[:3, :4]
    for occ in (None, g):
        kw = dict(kte, near=2.0, far=6.0, ert=1e-2, ert_block=16)
        if occ is not None:
            kw['occupancy'] = occ
        kw.pop('ndc', None)
        with torch.no_grad():
            whole = fn.render.render(H, W, K, chunk=1024, c2w=c2w.cuda(), ndc=False, **kw)
            parts = fn.render.render(H, W, K, chunk=64, c2w=c2w.cuda(), ndc=False, **kw)
            plain = fn.render.render(H, W, K, chunk=64, c2w=c2w.cuda(), ndc=False, **{k: v for k, v in kw.items() if k not in ('ert', 'ert_block')})
        for a, b in zip(whole[:3], parts[:3]):
            assert same_bits(a, b)
        for k in whole[3]:
            assert same_bits(whole[3][k], parts[3][k]), k
        d = float((whole[0] - plain[0]).abs().max())
        assert 0 < d <= float(np.float32(1e-2)) + SUM_MARGIN, 'ert reaches render_rays: the image moves, within the bound'
        rgbs, _ = fn.render.render_path([c2w.numpy()], (H, W, K[0][0]), K, 64, dict(kw, ndc=False))
        assert np.array_equal(rgbs[0], whole[0].cpu().numpy())
