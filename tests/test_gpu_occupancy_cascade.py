"""Occupancy cascade on the GPU against the restatement of tests/occ_cascade_numpy.py: query / classify bit for bit, a cascade of
one level against the single grid, the masked render against the CPU oracle at the GPU's own depths (the bounds of
tests/test_gpu_occupancy.py), from_network level by level, and the public surface."""
import copy

import numpy as np
import pytest
import torch

import occ_cascade_numpy as RC
import occ_numpy as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

TOL_RGB = 1e-4      # test_gpu_occupancy.TOL_RGB
TOL_ACC = 3e-4      # test_gpu_occupancy.TOL_ACC
NS, NI = 64, 128
MIN_SHARE = 0.02    # every level, and the 'no level' outcome, decides at least this share of the samples of each pass


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


def same_bits(a, b):
    """torch.equal on the bit patterns (disp_map is 0 / 0 = NaN on a ray without any weight, in the plain render too)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def grid_of(fn, level, outside=True):
    m, lo, hi = level
    return fn.occupancy.OccupancyGrid.from_mask(torch.from_numpy(m).cuda(), lo, hi, outside)


def cascade_of(fn, levels, outside):
    """The level grids carry the OPPOSITE flag: only the cascade's own `outside_occupied` may be read."""
    return fn.occupancy.OccupancyCascade([grid_of(fn, lv, not outside) for lv in levels], outside_occupied=outside)


def scene(fn):
    levels, oo = RC.scene_cascade()
    return cascade_of(fn, levels, oo), levels, oo


def networks(fn, **over):
    """create_nerf's render kwargs with the scene's random-init parameters loaded into both networks."""
    kw = dict(N_importance=NI, N_samples=NS, perturb=0., white_bkgd=False, use_viewdirs=True, no_reload=True)
    kw.update(over)
    _, kte, _, _, _, _ = fn.run_nerf.create_nerf(fn.run_nerf.make_args(**kw))
    sdc, sdf = R.scene_networks(O)
    kte['network_fn'].load_state_dict(sdc)
    kte['network_fine'].load_state_dict(sdf)
    return kte, sdc, sdf


def render_rays(fn, kte, rays_t, **kw):
    args = {k: kte[k] for k in ('network_fn', 'network_fine', 'network_query_fn', 'N_samples', 'N_importance', 'white_bkgd')}
    args.update(kw)
    with torch.no_grad():
        return fn.render.render_rays(rays_t, **args)


def special_points(levels, rs):
    pts = [(rs.rand(4000, 3) * 7 - 3.5).astype(np.float32)]
    for mask, lo, hi in levels:
        lo3, hi3 = np.broadcast_to(np.asarray(lo, np.float32), (3,)), np.broadcast_to(np.asarray(hi, np.float32), (3,))
        for ax in range(3):      # on every cell face of this level (as fp32 can name it), lo and hi included, and an ulp to either side
            n = mask.shape[ax]
            f = (lo3[ax].astype(np.float64) + (hi3[ax].astype(np.float64) - lo3[ax]) * np.arange(n + 1) / n).astype(np.float32)
            for v in (f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
                p = (lo3 + (hi3 - lo3) * rs.rand(v.size, 3)).astype(np.float32)
                p[:, ax] = v
                pts.append(p)
        pts.append(np.stack([lo3, hi3, np.nextafter(lo3, np.float32(-np.inf)), np.nextafter(hi3, np.float32(-np.inf))]))
    odd = (rs.rand(12, 3) - 0.5).astype(np.float32)
    for i, v in enumerate((np.nan, np.inf, -np.inf, 3e38)):
        for ax in range(3):
            odd[i * 3 + ax, ax] = v
    pts.append(odd)
    return np.concatenate(pts, 0)


# ---- 1. query and classify equal the restatement -----------------------------------------------------------------------------
def cascades_for_lookup():
    levels, _ = RC.scene_cascade()
    rs = np.random.RandomState(21)
    apart = [(rs.rand(3, 4, 5) < 0.5, np.array([0.0, 0.0, 0.0], np.float32), np.array([1.0, 2.0, 3.0], np.float32)),      # overlapping, not nested
             (rs.rand(4, 4, 4) < 0.5, np.array([0.5, -1.0, 1.0], np.float32), np.array([2.5, 1.0, 4.0], np.float32)),
             (rs.rand(33, 2, 9) < 0.5, np.float32(-3.0), np.float32(-0.5))]
    eight = [(rs.rand(3 + l, 5, 4 + l) < 0.5, np.float32(-0.3 * (l + 1)), np.float32(0.35 * (l + 1))) for l in range(8)]
    return {'scene': levels, 'reversed': levels[::-1], 'apart': apart, 'eight levels': eight, 'one level': levels[1:2]}


@pytest.mark.parametrize('outside', [False, True])
def test_query_equals_the_restatement(fn, outside):
    rs = np.random.RandomState(12)
    for name, levels in cascades_for_lookup().items():
        c = cascade_of(fn, levels, outside)
        assert c.levels == len(levels) and c.outside_occupied is outside
        pts = special_points(levels, rs)
        pts_t = torch.from_numpy(pts).cuda()
        got = c.query(pts_t).cpu().numpy()
        ref = RC.query(levels, outside, pts)
        assert np.array_equal(got, ref), (name, np.nonzero(got != ref)[0][:5], pts[got != ref][:5])
        who = c.decided_by(pts_t)
        assert who.dtype == torch.int8 and np.array_equal(who.cpu().numpy(), RC.decided_by(levels, pts)), name
        assert got.any() and not got.all()
    assert c.query(pts_t.reshape(-1, 1, 3)).shape == (pts.shape[0], 1) and c.decided_by(pts_t.reshape(-1, 1, 3)).shape == (pts.shape[0], 1)


# 169 rays: 169 * 64 and 169 * 192 are no multiples of the 1024-point block.  The tails: 37 x 13 = 481 points, one partial block, and
# a thread's four consecutive samples straddle two rays (13 is no multiple of 4); 300 x 7 = 2100 points, three blocks, the last one
# partial, so the scanned block offsets are used
@pytest.mark.parametrize('n,S', [pytest.param(169, 64, id='64'), pytest.param(169, 192, id='192'), pytest.param(37, 13, id='37x13'),
                                 pytest.param(300, 7, id='300x7')])
def test_classify_equals_the_restatement(fn, n, S):
    rs = np.random.RandomState(S)
    rays = R.scene_rays(O, side=13 if n <= 169 else 18)
    rays = rays[np.round(np.linspace(0, rays.shape[0] - 1, n)).astype(int)]      # n rays spread over the image (all 169 of them)
    assert rays.shape[0] == n
    z = np.sort(2.0 + 4.0 * rs.rand(rays.shape[0], S).astype(np.float32), -1)
    rays_t, z_t = torch.from_numpy(rays).cuda(), torch.from_numpy(z).cuda()
    cases = {k: (v, oo) for k, v in cascades_for_lookup().items() for oo in (True,)}
    levels, _ = RC.scene_cascade()
    cases['scene, outside empty'] = (levels, False)
    cases['empty'] = ([(np.zeros((8, 8, 8), bool), np.float32(-1), np.float32(1)), (np.zeros((4, 4, 4), bool), np.float32(-8), np.float32(8))], False)
    cases['full'] = ([(np.ones((8, 8, 8), bool), np.float32(-1), np.float32(1)), (np.ones((4, 4, 4), bool), np.float32(-8), np.float32(8))], False)
    cases['outside only'] = ([(np.zeros((4, 4, 4), bool), np.float32(-0.5), np.float32(0.5)), (np.zeros((2, 2, 2), bool), np.float32(-0.7), np.float32(0.7))], True)
    for name, (lv, oo) in cases.items():
        c = cascade_of(fn, lv, oo)
        raw = torch.full((rays.shape[0], S, 4), 7.0, device='cuda')
        idx, cnt = c.classify(rays_t, z_t, raw)
        bits = RC.classify(lv, oo, rays, z)
        live = np.nonzero(bits.reshape(-1))[0]
        assert cnt.tolist() == [live.size, bits.size], name
        assert np.array_equal(idx[:live.size].cpu().numpy(), live), name
        dead = (raw == 0).all(-1).cpu().numpy()
        assert np.array_equal(dead, ~bits) and bool((raw[torch.from_numpy(bits).cuda()] == 7.0).all()), name
        idx2, cnt2 = c.classify(rays_t, z_t)      # raw is optional; two calls agree
        assert torch.equal(cnt, cnt2) and torch.equal(idx[:live.size], idx2[:live.size])
        if name == 'empty':
            assert live.size == 0
        if name == 'full':
            assert live.size == bits.size
        if name == 'scene':
            pts = torch.from_numpy(R.sample_points(rays, z)).cuda()
            assert np.array_equal(c.decided_by(pts).cpu().numpy(), RC.decided_by(lv, R.sample_points(rays, z)))
            assert min(RC.shares(RC.decided_by(lv, R.sample_points(rays, z)), 3)) >= MIN_SHARE


# ---- 2. one level is the single grid -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', ['ball', 'random', 'half'])
def test_a_cascade_of_one_level_is_the_single_grid_bit_for_bit(fn, math_mode, grid):
    kte, _, _ = networks(fn)
    m, lo, hi, oo = R.scene_grids()[grid]
    g = fn.occupancy.OccupancyGrid.from_mask(torch.from_numpy(m).cuda(), lo, hi, oo)
    c = fn.occupancy.OccupancyCascade([g])
    assert c.outside_occupied is oo and c.grids[0] is g
    rays_t = torch.from_numpy(R.scene_rays(O, side=13)).cuda()
    tr, u = R.scene_randoms(rays_t.shape[0], NS, NI, 1)
    tr, u = torch.from_numpy(tr).cuda(), torch.from_numpy(u).cuda()
    with torch.no_grad():
        for perturb, t, uu in ((0., None, None), (1., tr, u)):
            a = fn.render._forward_occ(rays_t, kte['network_fn'], kte['network_fine'], NS, NI, False, perturb, True, t, uu, g)
            b = fn.render._forward_occ(rays_t, kte['network_fn'], kte['network_fine'], NS, NI, False, perturb, True, t, uu, c)
            assert sorted(a) == sorted(b)
            for k in a:
                assert same_bits(a[k], b[k]), (k, perturb)
    assert 0 < int(a['counts'][0]) < int(a['counts'][1])


# ---- 3. full and all-empty-but-outside cascades are the plain render ---------------------------------------------------------------
def test_full_and_missed_cascades_are_the_plain_render_bit_for_bit(fn, math_mode):
    kte, _, _ = networks(fn, white_bkgd=True)
    rays_t = torch.from_numpy(R.scene_rays(O, side=13)).cuda()
    G = fn.occupancy.OccupancyGrid
    ones = lambda shape, b: G.from_mask(torch.ones(*shape, dtype=torch.bool, device='cuda'), -b, b, outside_occupied=False)      # noqa: E731
    full = fn.occupancy.OccupancyCascade([ones((4, 5, 6), 1.0), ones((3, 3, 3), 3.0), ones((2, 2, 2), 9.0)])
    # all empty, and the boxes miss every ray (the camera looks from radius 4 towards the origin, depths 2 .. 6)
    zeros = lambda lo: G.from_mask(torch.zeros(2, 2, 2, dtype=torch.bool, device='cuda'), lo, lo + 1.0, outside_occupied=False)      # noqa: E731
    missed = fn.occupancy.OccupancyCascade([zeros(50.0), zeros(60.0), zeros(-70.0)], outside_occupied=True)
    pts = torch.from_numpy(R.sample_points(rays_t.cpu().numpy(), np.linspace(2.0, 6.0, 64, dtype=np.float32)[None].repeat(169, 0))).cuda()
    assert bool((missed.decided_by(pts) == -1).all()) and bool((full.decided_by(pts) >= 0).all())
    for retraw in (True, False):
        a = render_rays(fn, kte, rays_t, retraw=retraw)
        for c in (full, missed):
            b = render_rays(fn, kte, rays_t, retraw=retraw, occupancy=c)
            assert sorted(a) == sorted(b)
            for k in a:
                assert same_bits(a[k], b[k]), (k, retraw)


# ---- 4. the masked render is the contract --------------------------------------------------------------------------------------
def restate(sdc, sdf, rays, out, levels, oo, white_bkgd, cascade):
    """The contract at the GPU's own depths (test_gpu_occupancy.restate with the cascade's lookup): bits of o + d * z for the
    returned z0 / z1, the oracle's MLP at every point, zeros where the bit is clear, compositing."""
    res = {}
    for tag, sd, zk, rk, ck, ak in (('0', sdc, 'z0', 'raw0', 'rgb0', 'acc0'), ('1', sdf, 'z_vals', 'raw', 'rgb_map', 'acc_map')):
        z = out[zk].cpu().numpy()
        bits = RC.classify(levels, oo, rays, z)
        who = RC.decided_by(levels, R.sample_points(rays, z))
        raw, rgb, acc, _ = R.composite_at(O, sd, rays, z, bits, white_bkgd)
        got = out[rk].cpu()
        zero = (got == 0).all(-1).numpy()
        sh = RC.shares(who, len(levels))
        print('pass %s: masked %.4f of %d samples, decided per level / none %s, max|raw - ref| / max(1, |ref|) = %.3g, max|rgb - ref| = %.3g, '
              'max|acc - ref| = %.3g' % (tag, 1 - bits.mean(), bits.size, [round(s, 4) for s in sh],
                                         float(((got - raw).abs() / raw.abs().clamp(min=1.0)).max()),
                                         float((out[ck].cpu() - rgb).abs().max()), float((out[ak].cpu() - acc).abs().max())))
        assert np.array_equal(zero, ~bits), 'the pattern of exact zeros is the restated mask'
        assert ((got - raw).abs() <= 2e-5 * raw.abs().clamp(min=1.0)).all()
        assert float((out[ck].cpu() - rgb).abs().max()) < TOL_RGB
        assert float((out[ak].cpu() - acc).abs().max()) < TOL_ACC
        assert 0.2 < 1.0 - bits.mean() < 0.9
        assert min(sh) >= MIN_SHARE, sh
        assert np.array_equal(cascade.decided_by(torch.from_numpy(R.sample_points(rays, z)).cuda()).cpu().numpy(), who)
        res[tag] = bits
    return res


@pytest.mark.parametrize('perturb', [0, 1])
@pytest.mark.parametrize('white_bkgd', [False, True])
def test_masked_render_is_the_contract(fn, math_mode, perturb, white_bkgd):
    kte, sdc, sdf = networks(fn)
    c, levels, oo = scene(fn)
    rays = R.scene_rays(O)
    rays_t = torch.from_numpy(rays).cuda()
    tr, u = R.scene_randoms(rays.shape[0], NS, NI, perturb)
    tr, u = (None if t is None else torch.from_numpy(t).cuda() for t in (tr, u))
    with torch.no_grad():
        out = fn.render._forward_occ(rays_t, kte['network_fn'], kte['network_fine'], NS, NI, False, float(perturb), white_bkgd, tr, u, c)
        plain, _ = fn.render._forward_core(rays_t, kte['network_fn'], kte['network_fine'], NS, NI, False, float(perturb), white_bkgd,
                                           tr, u, None, None, False)
    bits = restate(sdc, sdf, rays, out, levels, oo, white_bkgd, c)
    assert out['counts'].tolist() == [int(bits['0'].sum()), bits['0'].size, int(bits['1'].sum()), bits['1'].size]
    assert float((out['rgb_map'] - plain['rgb_map']).abs().max()) > 1e-2, 'the cascade changes the image: the test is not empty'


# ---- 5. exactness --------------------------------------------------------------------------------------------------------------
def test_occupied_coarse_logits_are_the_plain_ones_bit_for_bit(fn, math_mode):
    kte, _, _ = networks(fn)
    c, levels, oo = scene(fn)
    rays = R.scene_rays(O, side=13)
    rays_t = torch.from_numpy(rays).cuda()
    fwd = lambda: fn.render._forward_occ(rays_t, kte['network_fn'], kte['network_fine'], NS, NI, False, 0., False, None, None, c)      # noqa: E731
    with torch.no_grad():
        out = fwd()
        plain, _ = fn.render._forward_core(rays_t, kte['network_fn'], kte['network_fine'], NS, NI, False, 0., False, None, None, None,
                                           None, False)
        again = fwd()
    assert torch.equal(out['z0'], plain['z0'])
    bits = torch.from_numpy(RC.classify(levels, oo, rays, out['z0'].cpu().numpy())).cuda()
    assert 0 < int(bits.sum()) < bits.numel()
    raw0_plain = fn.ops.mlp_fwd(rays_t, plain['z0'], kte['network_fn'].flat, kte['network_fn'].packed()[0])
    assert torch.equal(out['raw0'][bits], raw0_plain[bits])
    assert bool((out['raw0'][~bits] == 0).all())
    for k in out:      # two calls give bit-identical results
        assert same_bits(out[k], again[k]), k


# ---- 6. from_network -------------------------------------------------------------------------------------------------------------
def test_from_network_builds_every_level_as_the_single_grid_of_its_box(fn):
    kte, _, _ = networks(fn)
    N, bound, growth = 24, 1.2, 2.0
    Cas, G = fn.occupancy.OccupancyCascade, fn.occupancy.OccupancyGrid
    c = Cas.from_network(kte, levels=3, N=N, bound=bound, growth=growth, threshold=0.05, dilate=1)
    assert c.levels == 3 and c.outside_occupied and len(c.occupied_fraction()) == 3
    for l, g in enumerate(c.grids):
        b = bound * growth ** l
        t = torch.linspace(-b, b, N + 1, device='cuda')
        vol = torch.maximum(fn.mesh.density_grid(kte['network_fn'], t, t, t), fn.mesh.density_grid(kte['network_fine'], t, t, t))
        ref = R.build(vol.cpu().numpy(), 0.05, 1)
        assert g.shape == (N, N, N) and np.array_equal(g.to_mask().cpu().numpy(), ref), l
        assert np.array_equal(g.lo, np.full(3, -b, np.float32)) and np.array_equal(g.hi, np.full(3, b, np.float32))
        single = G.from_network(kte, N=N, bound=b, threshold=0.05, dilate=1)
        assert torch.equal(single.words, g.words) and np.array_equal(single.inv, g.inv), l
        assert abs(c.occupied_fraction()[l] - ref.mean()) < 1e-6
    per_level = Cas.from_network(kte, levels=2, N=[24, 12], bound=bound, which='fine')
    assert [g.shape for g in per_level.grids] == [(24, 24, 24), (12, 12, 12)]
    tf = torch.linspace(-2 * bound, 2 * bound, 13, device='cuda')
    assert np.array_equal(per_level.grids[1].to_mask().cpu().numpy(), R.build(fn.mesh.density_grid(kte['network_fine'], tf, tf, tf).cpu().numpy(), 0., 1))


def test_from_network_cascade_only_skips_more_than_the_single_grid(fn):
    """Sample by sample on the test rays, at both passes' depths: what the default-threshold cascade keeps, the single grid of the
    inner box with outside_occupied=True keeps too."""
    kte, _, _ = networks(fn)
    c = fn.occupancy.OccupancyCascade.from_network(kte, levels=3, N=24)
    g = fn.occupancy.OccupancyGrid.from_network(kte, N=24, outside_occupied=True)
    assert torch.equal(c.grids[0].words, g.words)
    rays = R.scene_rays(O, side=13)
    rays_t = torch.from_numpy(rays).cuda()
    with torch.no_grad():
        out = fn.render._forward_occ(rays_t, kte['network_fn'], kte['network_fine'], NS, NI, False, 0., False, None, None, c)
    for z in (out['z0'], out['z_vals']):
        pts = torch.from_numpy(R.sample_points(rays, z.cpu().numpy())).cuda()
        kept_c, kept_g = c.query(pts), g.query(pts)
        who = c.decided_by(pts)
        print('cascade keeps %.4f, single grid keeps %.4f of %d samples; decided per level / none: %s' % (
            float(kept_c.float().mean()), float(kept_g.float().mean()), kept_c.numel(), RC.shares(who.cpu().numpy(), 3)))
        assert not bool((kept_c & ~kept_g).any())
        assert bool((kept_c[who == 0] == kept_g[who == 0]).all()) and bool(kept_g[who != 0].all())
        assert bool((who == 0).any()) and bool((who > 0).any())


# ---- 7. the closure route ------------------------------------------------------------------------------------------------------
class TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(3)
        self.a, self.b = torch.nn.Linear(3, 48), torch.nn.Linear(48, 4)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * 1.5)

    def forward(self, x):
        return self.b(torch.sin(self.a(x)))


@pytest.mark.parametrize('white_bkgd', [False, True])
def test_closure_route_meets_the_contract(fn, white_bkgd):
    coarse, fine = TinyNet(), TinyNet()
    with torch.no_grad():
        fine.b.bias.add_(0.3)
    gc, gf = copy.deepcopy(coarse).cuda(), copy.deepcopy(fine).cuda()
    c, levels, oo = scene(fn)
    rays = R.scene_rays(O)
    rays_t = torch.from_numpy(rays).cuda()
    seen = []

    def query(pts, viewdirs, net):
        assert pts.dim() == 3 and pts.shape[1:] == (1, 3) and viewdirs.shape == (pts.shape[0], 3)
        seen.append(pts.shape[0])
        return net(pts)
    kw = dict(network_fn=gc, network_fine=gf, network_query_fn=query, N_samples=NS, N_importance=NI, white_bkgd=white_bkgd, retraw=True)
    with torch.no_grad():
        ret = fn.render.render_rays(rays_t, occupancy=c, **kw)
        plain = fn.render.render_rays(rays_t, **dict(kw, network_query_fn=lambda p, v, net: net(p)))
        # the same kernels step by step give the depths the route used (deterministic: perturb = 0)
        z0 = fn.ops.sample_coarse(rays_t, NS)
        raw0 = fn.render._query_occupied(lambda p, v, net: net(p), gc, rays_t, z0, rays_t[:, 8:11], c)
        rgb0, _, acc0, w0, _ = fn.ops.raw2outputs_fwd(raw0.contiguous(), z0, rays_t, None, white_bkgd)
        z1, _, _ = fn.ops.sample_pdf_merge(z0, w0, NI, det=True)
        c0, c1 = c.classify(rays_t, z0)[1], c.classify(rays_t, z1)[1]
    assert seen == [int(c0[0]), int(c1[0])]      # exactly as many points as the list is long
    assert torch.equal(ret['rgb0'], rgb0)
    out = {'z0': z0, 'z_vals': z1, 'raw0': raw0, 'raw': ret['raw'], 'rgb0': ret['rgb0'], 'acc0': ret['acc0'], 'rgb_map': ret['rgb_map'],
           'acc_map': ret['acc_map']}
    for sd_net, zk, rk, ck, ak in ((coarse, 'z0', 'raw0', 'rgb0', 'acc0'), (fine, 'z_vals', 'raw', 'rgb_map', 'acc_map')):
        z = out[zk].cpu().numpy()
        bits = RC.classify(levels, oo, rays, z)
        with torch.no_grad():
            raw, rgb, acc, _ = R.composite_at(O, None, rays, z, bits, white_bkgd, query_fn=sd_net)
        got = out[rk].cpu()
        assert np.array_equal((got == 0).all(-1).numpy(), ~bits)
        assert ((got - raw).abs() <= 2e-5 * raw.abs().clamp(min=1.0)).all()
        assert float((out[ck].cpu() - rgb).abs().max()) < TOL_RGB and float((out[ak].cpu() - acc).abs().max()) < TOL_ACC
        assert 0.2 < 1.0 - bits.mean() < 0.9
        assert min(RC.shares(RC.decided_by(levels, R.sample_points(rays, z)), len(levels))) >= MIN_SHARE
    assert float((ret['rgb_map'] - plain['rgb_map']).abs().max()) > 1e-2


@pytest.mark.parametrize('white_bkgd', [False, True])
def test_closure_route_with_an_empty_list(fn, white_bkgd):
    gc, gf = TinyNet().cuda(), TinyNet().cuda()
    rays_t = torch.from_numpy(R.scene_rays(O)).cuda()
    empty = cascade_of(fn, [(np.zeros((8, 8, 8), bool), np.float32(-1), np.float32(1)), (np.zeros((4, 4, 4), bool), np.float32(-3), np.float32(3))], False)
    seen = []

    def query(pts, viewdirs, net):
        seen.append(pts.shape[0])
        assert pts.shape[1:] == (1, 3) and viewdirs.shape == (pts.shape[0], 3)
        return net(pts)
    with torch.no_grad():
        ret = fn.render.render_rays(rays_t, gc, query, NS, retraw=True, N_importance=NI, network_fine=gf, white_bkgd=white_bkgd,
                                    occupancy=empty)
    assert seen == [0, 0]
    bg = 1.0 if white_bkgd else 0.0
    assert bool((ret['rgb_map'] == bg).all()) and bool((ret['acc_map'] == 0).all()) and bool((ret['rgb0'] == bg).all())
    assert ret['raw'].shape == (rays_t.shape[0], NS + NI, 4) and bool((ret['raw'] == 0).all())


# ---- 8. render and render_path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chunk', [25, 50, 40, 64, 1000])      # 100 rays: 25 and 50 divide the image, 40 and 64 do not
def test_render_and_render_path_pass_the_cascade_through(fn, chunk):
    kte, _, _ = networks(fn, white_bkgd=True)
    c, _, _ = scene(fn)
    H = W = 10
    K = np.array([[17.0, 0, 5.0], [0, 17.0, 5.0], [0, 0, 1]])
    c2w = fn.synthetic.pose_spherical(30.0, -30.0, 4.0)[:3, :4]
    kw = dict(kte, near=2.0, far=6.0, occupancy=c)
    kw.pop('ndc', None)
    with torch.no_grad():
        rgb, disp, acc, _ = fn.render.render(H, W, K, chunk=chunk, c2w=c2w.cuda(), ndc=False, **kw)
        ro, rd = fn.run_nerf_helpers.get_rays(H, W, K, c2w.cuda())
        rays11 = fn.ops.pack_rays(ro, rd, 2.0, 6.0)
        parts = [render_rays(fn, kte, rays11[i:i + chunk], occupancy=c) for i in range(0, H * W, chunk)]
        plain, _, _, _ = fn.render.render(H, W, K, chunk=chunk, c2w=c2w.cuda(), ndc=False, **{k: v for k, v in kw.items() if k != 'occupancy'})
    assert torch.equal(rgb.reshape(-1, 3), torch.cat([p['rgb_map'] for p in parts], 0))
    assert torch.equal(acc.reshape(-1), torch.cat([p['acc_map'] for p in parts], 0))
    assert float((rgb - plain).abs().max()) > 1e-2
    rgbs, _ = fn.render.render_path([c2w.numpy()], (H, W, 17.0), K, chunk, dict(kw, ndc=False))
    assert np.array_equal(rgbs[0], rgb.cpu().numpy())


# ---- 9. save and load ------------------------------------------------------------------------------------------------------------
def test_save_and_load_round_trip(fn, tmp_path):
    c, levels, oo = scene(fn)
    p = str(tmp_path / 'cascade.npz')
    c.save(p)
    with np.load(p) as f:      # the documented layout, with numpy alone
        assert int(f['levels']) == 3 and bool(f['outside_occupied']) is oo
        assert sorted(f.files) == sorted(['levels', 'outside_occupied'] + ['l%d_%s' % (i, k) for i in range(3)
                                                                            for k in ('words', 'shape', 'lo', 'hi', 'outside_occupied')])
        for i, (m, lo, hi) in enumerate(levels):
            assert np.array_equal(R.words_to_mask(f['l%d_words' % i], f['l%d_shape' % i]), m)
            assert np.array_equal(f['l%d_lo' % i], np.broadcast_to(np.asarray(lo, np.float32), (3,)))
    d = fn.occupancy.OccupancyCascade.load(p)
    assert d.levels == 3 and d.outside_occupied is oo
    for a, b in zip(c.grids, d.grids):
        assert torch.equal(a.words, b.words) and a.shape == b.shape and np.array_equal(a.lo, b.lo) and np.array_equal(a.hi, b.hi)
        assert np.array_equal(a.inv, b.inv) and a.outside_occupied == b.outside_occupied
    pts = torch.from_numpy(special_points(levels, np.random.RandomState(2))).cuda()
    assert torch.equal(c.query(pts), d.query(pts))
    with pytest.raises(ValueError, match='cascade'):
        fn.occupancy.OccupancyGrid.load(p)
    single = str(tmp_path / 'grid.npz')
    c.grids[0].save(single)
    with pytest.raises(ValueError):
        fn.occupancy.OccupancyCascade.load(single)
    assert torch.equal(fn.occupancy.OccupancyGrid.load(single).words, c.grids[0].words)      # the single grid's file still loads


# ---- 10. errors ------------------------------------------------------------------------------------------------------------------
def test_errors(fn):
    kte, _, _ = networks(fn)
    c, levels, _ = scene(fn)
    rays_t = torch.from_numpy(R.scene_rays(O)).cuda()
    args = {k: kte[k] for k in ('network_fn', 'network_fine', 'network_query_fn', 'N_samples', 'N_importance')}
    with torch.no_grad():
        with pytest.raises(ValueError):
            fn.render.render_rays(rays_t, raw_noise_std=1.0, occupancy=c, **args)
    assert any(p.requires_grad for p in kte['network_fn'].parameters())
    with pytest.raises(ValueError):
        fn.render.render_rays(rays_t, occupancy=c, **args)      # grad mode on, parameters require grad
    tiny = TinyNet().cuda()
    with pytest.raises(ValueError):
        fn.render.render_rays(rays_t, tiny, lambda p, v, n: n(p), NS, occupancy=c)
    with torch.no_grad():
        with pytest.raises(TypeError):      # a fastnerf network paired with another kind, as without a cascade
            fn.render.render_rays(rays_t, kte['network_fn'], lambda p, v, n: n(p), NS, N_importance=NI, network_fine=tiny, occupancy=c)
        with pytest.raises(RuntimeError):
            fn.render.render_rays(rays_t.cpu(), occupancy=c, **args)
    with pytest.raises(RuntimeError):
        c.query(torch.zeros(4, 3))
    with pytest.raises(RuntimeError):
        c.decided_by(torch.zeros(4, 3))
    with pytest.raises(RuntimeError):
        c.classify(rays_t.cpu(), torch.zeros(rays_t.shape[0], 4))
    g = grid_of(fn, levels[0])
    with pytest.raises(ValueError):
        fn.occupancy.OccupancyCascade([g] * 9)
    with pytest.raises(ValueError):
        fn.occupancy.OccupancyCascade([])
    with pytest.raises(TypeError):
        fn.occupancy.OccupancyCascade([g, 'grid'])
    assert fn.occupancy.OccupancyCascade([g] * 8).levels == 8
    # training takes a single grid
    H = W = 8
    K = np.array([[14.0, 0, 4.0], [0, 14.0, 4.0], [0, 0, 1]])
    ktr = fn.run_nerf.create_nerf(fn.run_nerf.make_args(N_importance=NI, N_samples=NS, perturb=1.0, use_viewdirs=True, no_reload=True))[0]
    with pytest.raises(ValueError, match='OccupancyCascade'):
        fn.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, occupancy=c)
