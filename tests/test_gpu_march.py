"""The marched render on the GPU (include/fastnerf.h, "marched render"): fastnerf_occ_march bit for bit against the restatement of
tests/march_numpy.py (validated against the contract on the CPU in tests/test_march_cpu.py), render_rays(..., march=K) against the
dense one-pass render through the grid at N_samples = K, early ray termination over the packed rows, K beyond the dense cap against
the float64 composite of the route's own row, and the Python surface.  Networks: ert_numpy.scene_networks (opaque)."""
import numpy as np
import pytest
import torch

import ert_numpy as E
import march_numpy as M
import occ_numpy as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32
U = 2.0 ** -24


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def same_f32(got, want):
    """The same floats bit for bit; NaNs in the same places (a NaN's payload is not part of the contract)."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


def device_grid(fn, grid):
    """march_numpy grid -> OccupancyGrid / OccupancyCascade."""
    G = fn.occupancy
    if grid[0] == 'grid':
        return G.OccupancyGrid.from_mask(torch.from_numpy(grid[1]).cuda(), grid[2], grid[3], grid[4])
    return G.OccupancyCascade([G.OccupancyGrid.from_mask(torch.from_numpy(m).cuda(), lo, hi, False) for m, lo, hi in grid[1]],
                              outside_occupied=grid[2])


def networks(fn, **over):
    kw = dict(N_importance=0, N_samples=64, perturb=0., white_bkgd=False, use_viewdirs=True, no_reload=True)
    kw.update(over)
    _, kte, _, _, _, _ = fn.run_nerf.create_nerf(fn.run_nerf.make_args(**kw))
    sdc, sdf = E.scene_networks(O)
    kte['network_fn'].load_state_dict(sdc)
    if kte.get('network_fine') is not None:
        kte['network_fine'].load_state_dict(sdf)
    return kte


# ---- 1. the kernel against the restatement -------------------------------------------------------------------------------------------
def kernel_rays(n):
    """n rays of the scene camera; the last rows are a NaN origin, an infinite direction, d = 0 outside and inside the object, near == far
    and near > far."""
    rays = R.scene_rays(O, side=13 if n <= 169 else 18)
    rays = rays[np.round(np.linspace(0, rays.shape[0] - 1, n)).astype(int)].copy()
    rays[-1, 0] = np.nan
    rays[-2, 4] = np.inf
    rays[-3, 3:6] = 0.0
    rays[-4, 0:3] = (0.0, 0.0, 0.7)
    rays[-4, 3:6] = 0.0
    rays[-5, 7] = rays[-5, 6]
    rays[-6, 6:8] = (6.0, 2.0)
    return rays


# (193, 256, 64, 16): no multiple of the block or of a wave; (37, 13, 5, 2): a partial last segment, overflow on most rays;
# (300, 2048, 128, 128): K beyond the dense cap, one round
@pytest.mark.parametrize('n,K,C,B', [(193, 256, 64, 16), (37, 13, 5, 2), (300, 2048, 128, 128)])
@pytest.mark.parametrize('scene', ['two_shells', 'cascade', 'cascade_outside'])
@pytest.mark.parametrize('lindisp', [False, True])
def test_kernel_equals_the_restatement(fn, n, K, C, B, scene, lindisp):
    grid = M.cascade2(True) if scene == 'cascade_outside' else M.scene_grids()[scene]
    g = device_grid(fn, grid)
    rays = kernel_rays(n)
    rays_t = torch.from_numpy(rays).cuda()
    zlat = M.lattice(rays, K, lindisp)
    live = M.live_bits(grid, rays, zlat[:, :K])
    # the lattice is the coarse sampler's, bit for bit
    assert same_f32(fn.ops.sample_coarse(rays_t, K, lindisp=lindisp).cpu().numpy(), zlat[:, :K])
    rs = np.random.RandomState(K + C)
    eps = F32(1e-2)
    segs = E.segments(C, B)
    for with_trans in (False, True):
        ref, got = None, (None, None, None, None)
        for j, (s0, s1) in enumerate(segs):
            tr = None
            if with_trans and j > 0:
                tr = (rs.rand(n) * 0.03).astype(F32)      # around eps: about a third of the rays go on
                tr[:5] = [eps, np.nextafter(eps, F32(1)), 0.0, 1.0, np.nan]
                tr = tr[rs.permutation(n)]
            ref = M.march_round(live, zlat, C, s0, s1, ref, tr, eps)
            z, kidx, overflow, state = got
            got = fn.ops.occ_march(g._c, rays_t, K, C, s0, s1, None if tr is None else torch.from_numpy(tr).cuda(), float(eps), lindisp,
                                   state, z, kidx, overflow)
            torch.cuda.synchronize()
            w = s1 + 1 if s1 < C else C      # the slots written so far: the segment and the depth behind it
            assert same_f32(got[0][:, :w].cpu().numpy(), ref[0][:, :w]), (j, 'z')
            assert np.array_equal(got[1][:, :s1].cpu().numpy(), ref[1][:, :s1]), (j, 'kidx')
            assert np.array_equal(got[2].cpu().numpy(), ref[2]), (j, 'overflow')
            assert np.array_equal(got[3].cpu().numpy(), ref[3]), (j, 'state')
            idx, cnt = fn.ops.march_list(got[1], s0, s1)
            want = M.live_list(ref[1], s0, s1)
            assert cnt.tolist() == [want.size, n * (s1 - s0)] and np.array_equal(idx[:want.size].cpu().numpy(), want), (j, 'list')
        if not with_trans:
            cz, ck, co = M.packed(live, zlat, C)      # and the rows are the contract's
            assert same_f32(ref[0], cz) and np.array_equal(ref[1], ck) and np.array_equal(ref[2].astype(bool), co)
            assert (ref[1] >= 0).any()
            assert scene != 'cascade_outside' or co.mean() > 0.9, 'with everything outside the boxes occupied, most rays overflow'
    # the object's methods return one round
    z, kidx, overflow = g.march(rays_t, K, C, lindisp=lindisp)
    one = M.march(live, zlat, C)
    assert same_f32(z.cpu().numpy(), one[0]) and np.array_equal(kidx.cpu().numpy(), one[1])
    assert overflow.dtype == torch.bool and np.array_equal(overflow.cpu().numpy(), one[2].astype(bool))


def test_kernel_argument_errors(fn):
    g = device_grid(fn, M.two_shells())
    rays_t = torch.from_numpy(R.scene_rays(O, side=4)).cuda()
    with pytest.raises(ValueError):
        fn.ops.occ_march(g._c, rays_t, 1, 64)
    with pytest.raises(ValueError):
        fn.ops.occ_march(g._c, rays_t, 64, 513)
    with pytest.raises(ValueError):
        fn.ops.occ_march(g._c, rays_t, 64, 16, 4, 8)      # a later round without the state of the one before
    z, kidx, overflow, state = fn.ops.occ_march(g._c, rays_t, 64, 16, 0, 8)
    with pytest.raises(RuntimeError):
        fn.ops.occ_march(g._c, rays_t, 64, 16, 8, 17, state=state, z=z, kidx=kidx, overflow=overflow)
    with pytest.raises(TypeError):
        fn.ops.occ_march(None, rays_t, 64, 16)


# ---- 2. against the dense one-pass render through the grid ---------------------------------------------------------------------------
def marched(fn, kte, rays_t, grid, K, C, ert=None, B=32):
    with torch.no_grad():
        return fn.render._forward_march(rays_t, kte['network_fn'], K, C, False, False, grid, ert, B)


@pytest.mark.parametrize('K', [256, 512])
@pytest.mark.parametrize('scene', ['two_shells', 'ball'])
def test_march_is_the_dense_render_with_the_empty_samples_dropped(fn, math_mode, scene, K):
    C = 192
    kte = networks(fn, N_samples=K)
    grid = M.scene_grids()[scene]
    g = device_grid(fn, grid)
    rays = E.scene_rays(O)
    rays_t = torch.from_numpy(rays).cuda()
    n = rays.shape[0]
    with torch.no_grad():
        dense = fn.render._forward_occ(rays_t, kte['network_fn'], None, K, 0, False, 0., False, None, None, g)
    out = marched(fn, kte, rays_t, g, K, C)
    kidx = out['march_k'].cpu().numpy()
    over = out['march_overflow'].cpu().numpy()
    # the live set: grid.classify of the dense lattice
    idx, cnt = g.classify(rays_t, dense['z_vals'])
    live = np.zeros((n, K), bool)
    live.reshape(-1)[idx[:int(cnt[0])].cpu().numpy()] = True
    got = np.zeros((n, K), bool)
    r, s = np.nonzero(kidx >= 0)
    got[r, kidx[r, s]] = True
    assert np.array_equal(got[~over], live[~over]), 'the live set of a ray that fits'
    for q in np.nonzero(over)[0]:      # a ray that does not: the first live lattice points, in order, as many as fit
        mine, full = np.nonzero(got[q])[0], np.nonzero(live[q])[0]
        assert mine.size < full.size and np.array_equal(mine, full[:mine.size])
    assert out['counts'].tolist() == [int((kidx >= 0).sum()), n * K]
    # the depths and the logits of the live slots: the dense pass's, bit for bit
    rt, kt = torch.from_numpy(r).cuda(), torch.from_numpy(kidx[r, s].astype(np.int64)).cuda()
    st = torch.from_numpy(s).cuda()
    assert same_bits(out['march_z'][rt, st], dense['z_vals'][rt, kt])
    assert same_bits(out['raw'][rt, st], dense['raw'][rt, kt])
    assert bool((out['raw'][torch.from_numpy(kidx < 0).cuda()] == 0).all()), 'closing entries and padding carry zero logits'
    # the maps of the rays of the consequence: no overflow, lattice point K - 1 empty
    ok = ~over & ~live[:, K - 1]
    assert ok.sum() >= n // 2 and live[ok].any(1).sum() >= n // 8, (int(ok.sum()), int(live[ok].any(1).sum()))
    okt = torch.from_numpy(ok).cuda()
    zK = float(M.lattice(rays, K)[:, K].max())
    bound = 4 * K * U
    d_rgb = float((out['rgb_map'] - dense['rgb_map'])[okt].abs().max())
    d_acc = float((out['acc_map'] - dense['acc_map'])[okt].abs().max())
    d_depth = float((out['depth_map'] - dense['depth_map'])[okt].abs().max())
    solid = okt & (dense['acc_map'] >= 0.5)
    d_disp = float((out['disp_map'] / dense['disp_map'] - 1)[solid].abs().max())
    print('%s K %d %s: |d rgb| %.3g |d acc| %.3g (bound %.3g), |d depth| %.3g (bound %.3g), rel d disp %.3g (bound %.3g); %d of %d rays, %d solid'
          % (scene, K, math_mode, d_rgb, d_acc, bound, d_depth, bound * zK, d_disp, 4 * bound, ok.sum(), n, int(solid.sum())))
    assert int(solid.sum()) >= n // 8
    assert d_rgb <= bound and d_acc <= bound
    assert d_depth <= bound * zK
    assert d_disp <= 4 * bound


# ---- 3. early ray termination over the packed rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize('scene', ['two_shells', 'ball'])
def test_ert_exact_cases_and_bounds(fn, math_mode, scene):
    K, C = 256, 192
    kte = networks(fn, N_samples=K)
    g = device_grid(fn, M.scene_grids()[scene])
    rays_t = torch.from_numpy(E.scene_rays(O)).cuda()
    plain = marched(fn, kte, rays_t, g, K, C)
    maps = ('rgb_map', 'disp_map', 'acc_map', 'depth_map')
    for B in (C, 1000):      # one round: everything, bit for bit
        one = marched(fn, kte, rays_t, g, K, C, ert=1e-2, B=B)
        for k in maps + ('raw', 'march_z', 'weights'):
            assert same_bits(one[k], plain[k]), (k, B)
        assert torch.equal(one['march_k'], plain['march_k']) and torch.equal(one['march_overflow'], plain['march_overflow'])
        assert one['counts'].tolist() == plain['counts'].tolist()
    for B in (16, 32):      # eps = 0: a ray is cut only once its transmittance is exactly 0 -- every map, bit for bit
        zero = marched(fn, kte, rays_t, g, K, C, ert=0.0, B=B)
        for k in maps:
            assert same_bits(zero[k], plain[k]), (k, B)
    zmax = float(plain['march_z'].max())
    for eps, B in ((1e-2, 16), (1e-3, 32)):
        out = marched(fn, kte, rays_t, g, K, C, ert=eps, B=B)
        e = float(F32(eps))
        d_rgb = float((out['rgb_map'] - plain['rgb_map']).abs().max())
        d_acc = (plain['acc_map'] - out['acc_map']).cpu().numpy()
        d_depth = float((out['depth_map'] - plain['depth_map']).abs().max())
        print('%s %s eps %g B %d: |d rgb| %.3g, d acc in [%.3g, %.3g], |d depth| %.3g; evaluated %d of %d'
              % (scene, math_mode, eps, B, d_rgb, d_acc.min(), d_acc.max(), d_depth, out['counts'][0].item(), plain['counts'][0].item()))
        assert d_rgb <= e
        assert 0 <= d_acc.min() and d_acc.max() <= e
        assert d_depth <= e * zmax
        assert out['counts'][0].item() < plain['counts'][0].item(), 'strictly fewer samples are evaluated on the opaque scene'
        assert out['counts'][1].item() == plain['counts'][1].item()
        # what was evaluated keeps its logits; a slot that is live in both rows is the same lattice point
        both = (out['march_k'] >= 0) & (plain['march_k'] >= 0)
        assert torch.equal(out['march_k'][both], plain['march_k'][both]) and same_bits(out['raw'][both], plain['raw'][both])
        assert bool(((out['march_k'] >= 0) <= (plain['march_k'] >= 0)).all())


# ---- 4. K beyond the dense cap --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scene', ['two_shells', 'ball'])
def test_a_fine_lattice_against_the_float64_composite_of_its_own_row(fn, math_mode, scene):
    K, C = 2048, 128
    kte = networks(fn)
    g = device_grid(fn, M.scene_grids()[scene])
    rays = E.scene_rays(O)
    out = marched(fn, kte, torch.from_numpy(rays).cuda(), g, K, C)
    ref = M.composite64(out['raw'].cpu().numpy(), out['march_z'].cpu().numpy(), rays)
    bound = 4 * K * U
    zK = float(M.lattice(rays, K)[:, K].max())
    f64 = lambda t: t.cpu().numpy().astype(np.float64)      # noqa: E731
    d_rgb = np.abs(f64(out['rgb_map']) - ref['rgb']).max()
    d_acc = np.abs(f64(out['acc_map']) - ref['acc']).max()
    d_depth = np.abs(f64(out['depth_map']) - ref['depth']).max()
    solid = ref['acc'] >= 0.5
    d_disp = np.abs(f64(out['disp_map'])[solid] / ref['disp'][solid] - 1).max()
    print('%s %s K 2048: |d rgb| %.3g |d acc| %.3g (bound %.3g), |d depth| %.3g (bound %.3g), rel d disp %.3g (bound %.3g), overflow %.2f'
          % (scene, math_mode, d_rgb, d_acc, bound, d_depth, bound * zK, d_disp, 4 * bound, out['march_overflow'].float().mean().item()))
    assert solid.sum() >= rays.shape[0] // 8
    assert d_rgb <= bound and d_acc <= bound and d_depth <= bound * zK and d_disp <= 4 * bound
    k = out['march_k'].cpu().numpy()
    assert k.max() > 512 and (k[:, C - 1] == -1).all()


# ---- 5. the surface -------------------------------------------------------------------------------------------------------------------
def call(fn, kte, rays_t, **kw):
    args = {k: kte[k] for k in ('network_fn', 'network_fine', 'network_query_fn', 'N_samples', 'N_importance')}
    args.update(kw)
    return fn.render.render_rays(rays_t, **args)


def test_errors(fn):
    kte = networks(fn)
    g = device_grid(fn, M.two_shells())
    rays_t = torch.from_numpy(E.scene_rays(O)).cuda()
    with torch.no_grad():
        with pytest.raises(ValueError, match='occupancy'):
            call(fn, kte, rays_t, march=256)
        with pytest.raises(ValueError, match='perturb'):
            call(fn, kte, rays_t, march=256, occupancy=g, perturb=1.0)
        with pytest.raises(ValueError, match='raw_noise_std'):
            call(fn, kte, rays_t, march=256, occupancy=g, raw_noise_std=1.0)
        for bad in (dict(march=1), dict(march=1 << 24), dict(march=256.5), dict(march=256, march_cap=1), dict(march=256, march_cap=513),
                    dict(march=True)):
            with pytest.raises(ValueError, match='march'):
                call(fn, kte, rays_t, occupancy=g, **bad)
        with pytest.raises(ValueError, match='ert'):
            call(fn, kte, rays_t, march=256, occupancy=g, ert=1.5)
        tiny = torch.nn.Linear(3, 4).cuda()
        with pytest.raises(NotImplementedError):
            fn.render.render_rays(rays_t, tiny, lambda p, v, net: net(p), 64, occupancy=g, march=256)
    assert any(p.requires_grad for p in kte['network_fn'].parameters())
    with pytest.raises(ValueError, match='inference feature'):
        call(fn, kte, rays_t, march=256, occupancy=g)      # grad mode on, parameters require grad


def test_render_rays_keys_network_and_determinism(fn):
    kte = networks(fn, N_importance=128)      # two networks: the marched render takes the fine one
    g = device_grid(fn, M.two_shells())
    rays_t = torch.from_numpy(E.scene_rays(O)).cuda()
    with torch.no_grad():
        a = call(fn, kte, rays_t, march=256, march_cap=96, occupancy=g, retraw=True, retdepth=True)
        b = call(fn, kte, rays_t, march=256, march_cap=96, occupancy=g, retraw=True, retdepth=True)
        small = call(fn, kte, rays_t, march=256, march_cap=96, occupancy=g)
        ref = fn.render._forward_march(rays_t, kte['network_fine'], 256, 96, False, False, g)
        coarse = fn.render._forward_march(rays_t, kte['network_fn'], 256, 96, False, False, g)
        plain = call(fn, kte, rays_t, occupancy=g)
    assert sorted(a) == ['acc_map', 'depth_map', 'disp_map', 'march_k', 'march_overflow', 'march_z', 'raw', 'rgb_map'], 'no coarse-pass keys'
    assert sorted(small) == ['acc_map', 'disp_map', 'march_overflow', 'rgb_map']
    assert a['march_overflow'].dtype == torch.bool and a['march_k'].dtype == torch.int32 and a['raw'].shape == (rays_t.shape[0], 96, 4)
    for k in a:
        same = torch.equal(a[k], b[k]) if a[k].dtype != torch.float32 else same_bits(a[k], b[k])
        assert same, k + ': two calls are bit-identical'
    for k in ('rgb_map', 'disp_map', 'acc_map', 'depth_map', 'raw'):
        assert same_bits(a[k], ref[k]), k
    assert not same_bits(a['rgb_map'], coarse['rgb_map']), 'the image network is network_fine'
    assert sorted(plain) == ['acc0', 'acc_map', 'disp0', 'disp_map', 'rgb0', 'rgb_map', 'z_std'], 'march=None: the hierarchical render'


def test_tighten_render_and_render_path(fn):
    kte = networks(fn, white_bkgd=True)
    g = device_grid(fn, M.two_shells())
    rays_t = torch.from_numpy(E.scene_rays(O)).cuda()
    with torch.no_grad():
        a = call(fn, kte, rays_t, march=256, march_cap=96, occupancy=g, tighten=True, retraw=True, retdepth=True, white_bkgd=True)
        b = call(fn, kte, g.tighten(rays_t)[0], march=256, march_cap=96, occupancy=g, retraw=True, retdepth=True, white_bkgd=True)
        c = call(fn, kte, rays_t, march=256, march_cap=96, occupancy=g, retraw=True, white_bkgd=True)
    for k in a:
        assert (torch.equal(a[k], b[k]) if a[k].dtype != torch.float32 else same_bits(a[k], b[k])), k
    assert not same_bits(a['march_z'], c['march_z']), 'the lattice spans the tightened interval'
    H = W = 13
    K = np.array([[14.0 * 13 / 8, 0, 6.5], [0, 14.0 * 13 / 8, 6.5], [0, 0, 1]])
    c2w = fn.synthetic.pose_spherical(30.0, -30.0, 4.0)[:3, :4]
    kw = dict(kte, near=2.0, far=6.0, occupancy=g, march=256, march_cap=96, ert=1e-2, ert_block=16)
    kw.pop('ndc', None)
    with torch.no_grad():
        whole = fn.render.render(H, W, K, chunk=1024, c2w=c2w.cuda(), ndc=False, **kw)
        parts = fn.render.render(H, W, K, chunk=64, c2w=c2w.cuda(), ndc=False, **kw)
        hier = fn.render.render(H, W, K, chunk=1024, c2w=c2w.cuda(), ndc=False, **{k: v for k, v in kw.items() if k not in ('march', 'march_cap')})
    for x, y in zip(whole[:3], parts[:3]):
        assert same_bits(x, y)
    assert sorted(whole[3]) == ['march_overflow'] and whole[3]['march_overflow'].shape == (H, W)
    assert 'rgb0' not in whole[3] and not same_bits(whole[0], hier[0]), 'march reaches render_rays'
    rgbs, _ = fn.render.render_path([c2w.numpy()], (H, W, K[0][0]), K, 64, dict(kw, ndc=False))
    assert np.array_equal(rgbs[0], whole[0].cpu().numpy())
