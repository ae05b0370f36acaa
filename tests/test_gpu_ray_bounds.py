"""fastnerf_occ_ray_bounds on the GPU: the kernel's output is conservative (C) and tight (T) against the product's own lookup
(grid.query on 144 x 4096 probe points) on the grids and ray sets of tests/test_ray_bounds_cpu.py, write_back touches columns 6:8
only, a cascade of one level is the grid bit for bit, and `tighten` of render_rays and of the fused Trainer is exactly the render
/ the step on the tightened batch.

(C) every probe that the lookup calls occupied lies in [near', far'] and its ray has hit = 1: zero exceptions.
(T) with M+ the mask dilated by one cell: every hit ray has an occupied probe under M+, near' >= zmin(M+) - s and
    far' <= zmax(M+) + s, s = sqrt(3) h_max / |d| + 2 probe spacings: zero exceptions."""
import copy

import numpy as np
import pytest
import torch

import occ_numpy as R
import ray_bounds_numpy as RB
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
GRIDS = R.scene_grids()
RAYS = RB.ray_sets(O)
NS, NI = 64, 128


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


def G(fn):
    return fn.occupancy.OccupancyGrid


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def grid_of(fn, mask, lo, hi, outside):
    return G(fn).from_mask(torch.from_numpy(np.ascontiguousarray(mask)).cuda(), lo, hi, outside)


def cascade_of(fn, levels, outside):
    return fn.occupancy.OccupancyCascade([grid_of(fn, m, lo, hi, False) for m, lo, hi in levels], outside)


def probes(g, rays, z):
    """bool [n, P]: the product's lookup at the probe points x = o + d * z (one rounded multiply, one rounded add, in torch)."""
    r, zz = torch.from_numpy(rays).cuda(), torch.from_numpy(z).cuda()
    pts = r[:, None, 0:3] + r[:, None, 3:6] * zz[..., None]
    return g.query(pts.contiguous()).cpu().numpy()


def check(fn, g, g_plus, rays, h_max, oracle=None, what=''):
    z = RB.probe_depths(rays)
    n2, f2, hit = (t.cpu().numpy() for t in g.ray_bounds(torch.from_numpy(rays).cuda()))
    hit = hit.astype(np.uint8)
    if oracle is not None:
        print('%s: hit %d of %d; hit differs from the numpy restatement on %d rays, the bounds on %d' % (
            what, hit.sum(), len(hit), int((hit != oracle[2]).sum()), int(((n2 != oracle[0]) | (f2 != oracle[1])).sum())))
    assert (rays[:, 6] <= n2).all() and (n2 < f2).all() and (f2 <= rays[:, 7]).all()
    assert RB.check_conservative(probes(g, rays, z), z, n2, f2, hit) == 0
    if g_plus is not None:
        assert RB.check_tight(probes(g_plus, rays, z), z, rays, n2, f2, hit, h_max) == 0
    miss = hit == 0
    assert (n2[miss] == rays[miss, 6]).all() and (f2[miss] == rays[miss, 7]).all()
    return n2, f2, hit


# ---- 1. the kernel's properties --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rname', sorted(RAYS))
@pytest.mark.parametrize('gname', sorted(GRIDS))
def test_conservative_and_tight(fn, gname, rname):
    mask, lo, hi, outside = GRIDS[gname]
    g, gp = grid_of(fn, mask, lo, hi, outside), grid_of(fn, R.dilated(mask, 1), lo, hi, outside)
    rays = RAYS[rname]
    oracle = RB.ray_bounds_grid(mask, lo, hi, outside, rays)
    _, _, hit = check(fn, g, gp, rays, RB.cell_edges(mask.shape, lo, hi).max(), oracle, '%s / %s' % (gname, rname))
    assert 0 < hit.sum() and (outside or hit.sum() < 144)


@pytest.mark.parametrize('n', [1, 257])
def test_the_tail_of_a_block(fn, n):
    mask, lo, hi, outside = GRIDS['random']
    g, gp = grid_of(fn, mask, lo, hi, outside), grid_of(fn, R.dilated(mask, 1), lo, hi, outside)
    rays = np.concatenate([RAYS['camera'], RAYS['random']])[31:31 + n].copy()
    guard = torch.full((n + 3, 2), -7.0, device='cuda')
    hguard = torch.full((n + 3,), 9, device='cuda', dtype=torch.uint8)
    r = torch.from_numpy(np.concatenate([rays, np.full((3, 11), 5.0, F32)])).cuda()
    before = r.clone()
    fn._lib.check(fn._lib.lib().fastnerf_occ_ray_bounds(g._c, None, n, r.data_ptr(), 1, guard.data_ptr(), hguard.data_ptr(), fn._lib.stream()),
                  'fastnerf_occ_ray_bounds')
    assert (guard[n:] == -7.0).all() and (hguard[n:] == 9).all() and same_bits(r[n:], before[n:])      # nothing beyond row n
    n2, f2, hit = check(fn, g, gp, rays, RB.cell_edges(mask.shape, lo, hi).max())
    assert np.array_equal(guard[:n].cpu().numpy(), np.stack([n2, f2], -1)) and np.array_equal(hguard[:n].cpu().numpy(), hit)


@pytest.mark.parametrize('outside', [False, True])
@pytest.mark.parametrize('rname', sorted(RAYS))
def test_three_level_cascade_is_conservative(fn, rname, outside):
    levels = RB.cascade_fixtures()[0]
    c = cascade_of(fn, levels, outside)
    oracle = RB.ray_bounds(levels, outside, RAYS[rname])
    check(fn, c, None, RAYS[rname], None, oracle, 'cascade (outside_occupied=%s) / %s' % (outside, rname))


@pytest.mark.parametrize('rname', sorted(RAYS))
def test_three_level_cascade_is_tight_away_from_the_seams(fn, rname):
    levels = RB.cascade_fixtures()[1]
    c = cascade_of(fn, levels, False)
    cp = cascade_of(fn, [(R.dilated(m, 1), lo, hi) for m, lo, hi in levels], False)
    h_max = max(RB.cell_edges(m.shape, lo, hi).max() for m, lo, hi in levels)
    _, _, hit = check(fn, c, cp, RAYS[rname], h_max)
    assert 0 < hit.sum() < 144


@pytest.mark.parametrize('gname', sorted(GRIDS))
def test_a_cascade_of_one_level_is_the_grid_bit_for_bit(fn, gname):
    mask, lo, hi, outside = GRIDS[gname]
    g = grid_of(fn, mask, lo, hi, outside)
    c = fn.occupancy.OccupancyCascade([g])
    for rname in sorted(RAYS):
        r = torch.from_numpy(RAYS[rname]).cuda()
        for a, b in zip(g.ray_bounds(r), c.ray_bounds(r)):
            assert same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b)


def test_write_back_rewrites_columns_6_and_7_and_nothing_else(fn):
    mask, lo, hi, outside = GRIDS['ball']
    g = grid_of(fn, mask, lo, hi, outside)
    r0 = torch.from_numpy(RAYS['camera']).cuda()
    r0[:, 8:11] = torch.rand(144, 3, device='cuda')
    bounds, hit = fn.ops.occ_ray_bounds(g._c, r0)
    r1 = r0.clone()
    b1, h1 = fn.ops.occ_ray_bounds(g._c, r1, write_back=True)
    assert same_bits(b1, bounds) and torch.equal(h1, hit)
    assert same_bits(r1[:, :6], r0[:, :6]) and same_bits(r1[:, 8:], r0[:, 8:]) and same_bits(r1[:, 6:8].contiguous(), bounds)
    assert (bounds != r0[:, 6:8]).any()
    # tighten returns a new batch; [n, 8] batches too; the input stays
    keep = r0.clone()
    t11, hit11 = g.tighten(r0)
    t8, hit8 = g.tighten(r0[:, :8].contiguous())
    assert same_bits(r0, keep) and same_bits(t11, r1) and t8.shape == (144, 8) and same_bits(t8, r1[:, :8].contiguous())
    assert torch.equal(hit11, hit.bool()) and torch.equal(hit8, hit11)
    n2, f2, h = g.ray_bounds(r0)
    assert same_bits(torch.stack([n2, f2], -1), bounds) and h.dtype == torch.bool


def test_edge_cases_return_the_input_bounds(fn):
    mask, lo, hi, _ = GRIDS['ball']
    g = grid_of(fn, mask, lo, hi, False)
    base = [0.1, 0.2, -3.0, 0.0, 0.1, 1.0, 0.5, 6.0, 0, 0, 1]
    rows, want_hit = [], []
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(8):
            v = list(base)
            v[col] = bad
            rows.append(v)
            want_hit.append(1)
    for v, h in (([0, 0, -3, 0, 0, 1, 4.0, 4.0, 0, 0, 1], 1), ([0, 0, -3, 0, 0, 1, 5.0, 2.0, 0, 0, 1], 1),      # near >= far
                 ([0, 5, -3, 0, 0, 1, 0.5, 6.0, 0, 0, 1], 0), ([0, 0, -3, 0, 0, -1, 0.5, 6.0, 0, 0, 1], 0),     # misses the box
                 ([0, 0, -9, 0, 0, 1, 0.5, 6.0, 0, 0, 1], 0), ([0, 0, -3e7, 0, 0, 1, 0.5, 6.0, 0, 0, 1], 1),    # ends before it; too far
                 ([0, 0, 0, 0, 0, 0, 0.5, 6.0, 0, 0, 1], 1)):                                                   # d = 0 inside the ball
        rows.append(v)
        want_hit.append(h)
    r = torch.tensor(rows, dtype=torch.float32, device='cuda')
    before = r.clone()
    bounds, hit = fn.ops.occ_ray_bounds(g._c, r, write_back=True)
    assert same_bits(r, before) and same_bits(bounds, before[:, 6:8].contiguous())
    assert hit.tolist() == want_hit
    # parallel to a face, on it: conservative against the lookup, and the restatement's own figures
    rays = np.array([[0, 0, -3, 0, 0, 1, 0.5, 6.0, 0, 0, 1], [-1.5, 0.05, -3, 0, 0, 1, 0.5, 6.0, 0, 0, 1],
                     [0.01, 0.02, -3, 0, 0, 2, 0.25, 3.0, 0, 0, 1]], F32)
    n2, f2, hit = check(fn, g, grid_of(fn, R.dilated(mask, 1), lo, hi, False), rays, RB.cell_edges(mask.shape, lo, hi).max())
    assert hit[0] == 1 and 1.6 < n2[0] < 1.85 and 4.15 < f2[0] < 4.4 and hit[2] == 1 and 0.8 < n2[2] < 0.925 and 2.075 < f2[2] < 2.2


def test_errors(fn):
    mask, lo, hi, _ = GRIDS['ball']
    g = grid_of(fn, mask, lo, hi, False)
    r = torch.from_numpy(RAYS['camera']).cuda()
    with pytest.raises(RuntimeError):
        g.ray_bounds(r.cpu())
    with pytest.raises(ValueError):
        g.ray_bounds(r[:, :7].contiguous())
    with pytest.raises(TypeError):
        fn.ops.occ_ray_bounds(None, r)


# ---- 2. render_rays(..., tighten=True) -----------------------------------------------------------------------------------------------
def networks(fn, **over):
    kw = dict(N_importance=NI, N_samples=NS, perturb=0., white_bkgd=False, use_viewdirs=True, no_reload=True)
    kw.update(over)
    ktr, kte, _, _, _, _ = fn.run_nerf.create_nerf(fn.run_nerf.make_args(**kw))
    sdc, sdf = R.scene_networks(O)
    kte['network_fn'].load_state_dict(sdc)
    kte['network_fine'].load_state_dict(sdf)
    return ktr, kte


def render_rays(fn, kte, rays_t, **kw):
    args = {k: kte[k] for k in ('network_fn', 'network_fine', 'network_query_fn', 'N_samples', 'N_importance', 'white_bkgd')}
    args.update(kw)
    with torch.no_grad():
        return fn.render.render_rays(rays_t, **args)


@pytest.mark.parametrize('perturb', [0., 1.])
@pytest.mark.parametrize('ert', [None, 1e-3])
def test_tighten_is_the_render_of_the_tightened_batch(fn, perturb, ert):
    _, kte = networks(fn)
    mask, lo, hi, outside = GRIDS['ball']
    g = grid_of(fn, mask, lo, hi, outside)
    rays_t = torch.from_numpy(RAYS['camera']).cuda()
    kw = dict(perturb=perturb, pytest=True, retraw=True, retdepth=True, occupancy=g)
    if ert is not None:
        kw['ert'] = ert
    a = render_rays(fn, kte, rays_t, tighten=True, **kw)
    tight, hit = g.tighten(rays_t)
    b = render_rays(fn, kte, tight, **kw)
    assert sorted(a) == sorted(b) and 0 < int(hit.sum()) < 144
    for k in a:
        assert same_bits(a[k], b[k]), k
    # a ray that meets nothing occupied returns exactly what it returns without tighten; the others got other depths
    plain = render_rays(fn, kte, rays_t, **kw)
    for k in a:
        assert same_bits(a[k][~hit], plain[k][~hit]), k
    assert not same_bits(a['rgb_map'][hit], plain['rgb_map'][hit])


class TinyNet(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.a, self.b = torch.nn.Linear(3, 48), torch.nn.Linear(48, 4)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * 1.5)

    def forward(self, x):
        return self.b(torch.sin(self.a(x)))


@pytest.mark.parametrize('perturb', [0., 1.])
def test_tighten_on_the_closure_route(fn, perturb):
    gc, gf = TinyNet(3).cuda(), TinyNet(4).cuda()
    mask, lo, hi, outside = GRIDS['random']
    g = grid_of(fn, mask, lo, hi, outside)
    rays_t = torch.from_numpy(RAYS['camera']).cuda()
    kw = dict(network_fn=gc, network_fine=gf, network_query_fn=lambda p, v, net: net(p), N_samples=16, N_importance=16, retraw=True,
              perturb=perturb, pytest=True, occupancy=g)
    with torch.no_grad():
        a = fn.render.render_rays(rays_t, tighten=True, **kw)
        tight, hit = g.tighten(rays_t)
        b = fn.render.render_rays(tight, **kw)
        plain = fn.render.render_rays(rays_t, **kw)
    assert sorted(a) == sorted(b) and 0 < int(hit.sum()) < 144
    for k in a:
        assert same_bits(a[k], b[k]), k
        assert same_bits(a[k][~hit], plain[k][~hit]), k


def test_render_passes_tighten_through_and_refuses_it_without_a_grid(fn):
    _, kte = networks(fn)
    mask, lo, hi, outside = GRIDS['ball']
    g = grid_of(fn, mask, lo, hi, outside)
    H = W = 12
    K = np.array([[14.0, 0, 6.0], [0, 14.0, 6.0], [0, 0, 1]])
    c2w = torch.as_tensor(O.pose_spherical(30.0, -30.0, 4.0)[:3, :4]).float().cuda()
    kw = dict(kte, near=2.0, far=6.0, ndc=False, occupancy=g, tighten=True)
    with torch.no_grad():
        rgb, _, _, _ = fn.render.render(H, W, K, chunk=50, c2w=c2w, **kw)
        rays11 = fn.ops.pack_rays(*fn.run_nerf_helpers.get_rays(H, W, K, c2w), 2.0, 6.0)
        whole = render_rays(fn, kte, g.tighten(rays11)[0], occupancy=g)
    assert same_bits(rgb.reshape(-1, 3), whole['rgb_map'])
    with pytest.raises(ValueError, match='tighten'):
        render_rays(fn, kte, rays11, tighten=True)


# ---- 3. the fused Trainer ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def compact_on(fn):
    old = fn.render.get_compact()
    fn.render.set_compact('1')
    yield
    fn.render.set_compact(old)


def new_trainer(fn, **extra):
    args = fn.run_nerf.make_args(N_importance=8, N_samples=8, perturb=0., white_bkgd=True, use_viewdirs=True, no_reload=True)
    torch.manual_seed(0)
    ktr, kte, _, _, _, _ = fn.run_nerf.create_nerf(args)
    sdc, sdf = R.scene_networks(O)
    ktr['network_fn'].load_state_dict(sdc)
    ktr['network_fine'].load_state_dict(sdf)
    K = np.array([[14.0, 0, 6.0], [0, 14.0, 6.0], [0, 0, 1]])
    return fn.run_nerf.Trainer(ktr, 12, 12, K, 2.0, 6.0, **extra), ktr, kte


def batch():
    r = torch.from_numpy(RAYS['camera'])
    return r[:, 0:3].contiguous().cuda(), r[:, 3:6].contiguous().cuda(), torch.rand(144, 3, generator=torch.Generator().manual_seed(1)).cuda()


def test_the_fused_step_tightens_between_pack_rays_and_the_forward(fn, compact_on):
    mask, lo, hi, outside = GRIDS['ball']
    g = grid_of(fn, mask, lo, hi, outside)
    tr, ktr, kte = new_trainer(fn, occupancy=g, tighten=True)
    ro, rd, tgt = batch()
    rays11 = fn.ops.pack_rays(ro, rd, 2.0, 6.0)
    n2, f2, hit = g.ray_bounds(rays11)
    assert 0 < int(hit.sum()) < 144 and (n2[hit] > 2.0).any() and (f2[hit] < 6.0).any()
    want = render_rays(fn, ktr, g.tighten(rays11)[0], occupancy=g)      # before the step moves the parameters
    loss2, out = tr.step(ro, rd, tgt)
    assert tr.last_step_live
    assert same_bits(out['z0'][:, 0].contiguous(), n2.contiguous()) and same_bits(out['z0'][:, -1].contiguous(), f2.contiguous())
    for k in ('rgb_map', 'rgb0'):
        err = float((out[k] - want[k]).abs().max())
        print('%s: max |step - render_rays| = %.3g' % (k, err))
        assert err <= 1e-4, k
    occ, total = tr.occupancy_counts.tolist()[:2]
    plain, _, _ = new_trainer(fn, occupancy=g)
    plain.step(ro, rd, tgt)
    print('occupied coarse samples: %d of %d with tighten, %d without' % (occ, total, plain.occupancy_counts.tolist()[0]))
    assert occ > plain.occupancy_counts.tolist()[0]


def test_a_grid_that_cannot_move_the_bounds_leaves_the_step_bit_identical(fn, compact_on):
    res = []
    for tighten in (False, True):
        full = G(fn).from_mask(torch.ones(8, 8, 8, dtype=torch.bool, device='cuda'), -1.5, 1.5, outside_occupied=True)
        tr, _, _ = new_trainer(fn, occupancy=full, tighten=tighten)
        loss2, out = tr.step(*batch())
        res.append((tr.flat.clone(), tr.m.clone(), tr.v.clone(), loss2.clone(), out['z0'].clone()))
    for a, b in zip(*res):
        assert same_bits(a, b)
    assert same_bits(res[1][4][:, 0].contiguous(), torch.full((144,), 2.0, device='cuda'))


def test_the_trainer_refuses_tighten_without_a_grid(fn, compact_on):
    with pytest.raises(ValueError, match='tighten'):
        new_trainer(fn, tighten=True)
    a = fn._lib.StepArgs()      # and so does the C entry point: the bit needs occ
    a.n, a.N_samples, a.math_mode, a.net_floats, a.fwd_flags = 4, 8, 0, fn.ops.NET_PARAMS, fn._lib.STEP_TIGHTEN
    buf = torch.zeros(16, device='cuda')
    a.params = a.grads = a.packed_fwd_c = a.packed_bwd_c = buf.data_ptr()
    import ctypes
    assert fn._lib.lib().fastnerf_train_step(ctypes.byref(a), fn._lib.STEP_FORWARD, None) == -1
    assert b'FN_STEP_TIGHTEN' in fn._lib.lib().fastnerf_last_error()
