"""Training through an occupancy grid: Trainer(..., occupancy=grid), fastnerf_train_step with fn_step_args.occ, and the kernels
that keep the grid (fastnerf_occ_cell_points, fastnerf_occ_update), against numpy / the CPU oracle.

  1. a full grid is the plain compacted step bit for bit;
  2. a masked step is bit-equal to render_rays(..., occupancy=grid) where that is possible (maps, losses, counts, the live list
     a subset of the occupied list) and within the compacted-versus-oracle bound where it is not (the gradients);
  3. an empty grid: zero gradient, background, Adam leaves the parameters alone; the C ABI's refusals;
  4. the grid kernels against a numpy restatement; hysteresis closes a cell after the number of updates decay implies;
  5. save / load with a density, and a file of the earlier layout;
  6. training on the solid-body scene (the grid conditions here; the paired PSNR study is marked slow)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import occ_numpy as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
NS, NI = 64, 128


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


def G(fn):
    return fn.occupancy.OccupancyGrid


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture
def compact_on(fn):
    old = fn.render.get_compact()
    fn.render.set_compact('1')
    yield
    fn.render.set_compact(old)


def new_trainer(fn, occupancy=None, perturb=1.0, white_bkgd=True, **kw):
    """A Trainer over create_nerf's networks with the scene's random-init parameters (tests/occ_numpy.py) loaded."""
    args = fn.run_nerf.make_args(N_importance=NI, N_samples=NS, perturb=perturb, white_bkgd=white_bkgd, use_viewdirs=True, no_reload=True)
    torch.manual_seed(0)
    ktr, kte, _, _, _, _ = fn.run_nerf.create_nerf(args)
    sdc, sdf = R.scene_networks(O)
    ktr['network_fn'].load_state_dict(sdc)
    ktr['network_fine'].load_state_dict(sdf)
    K = np.array([[14.0, 0, 4.0], [0, 14.0, 4.0], [0, 0, 1]])
    extra = {} if occupancy is None else dict(occupancy=occupancy, **kw)
    return fn.run_nerf.Trainer(ktr, 8, 8, K, 2.0, 6.0, **extra), ktr, kte, (sdc, sdf)


def region(tr, out, name):
    off, shape = tr._regions[name]
    return out._block[off:off + int(np.prod(shape))].view(shape)


def batch(n, seed):
    """n rays of cameras on the sphere of radius 4 looking at the origin, and random targets."""
    rays = np.concatenate([R.scene_rays(O, side=16), R.scene_rays(O, side=16, focal=20.0)], 0)
    gen = torch.Generator().manual_seed(seed)
    sel = torch.randint(0, rays.shape[0], (n,), generator=gen)
    r = torch.from_numpy(rays)[sel]
    return r[:, 0:3].contiguous().cuda(), r[:, 3:6].contiguous().cuda(), torch.rand(n, 3, generator=gen).cuda()


# ---- 1. a full grid is the plain compacted step ----------------------------------------------------------------------------
def test_a_full_grid_is_the_plain_compacted_step_bit_for_bit(fn, math_mode, compact_on):
    n, steps = 300, 8
    res = {}
    for tag in ('plain', 'grid'):
        grid = G(fn).for_training(N=16, bound=1.2) if tag == 'grid' else None
        tr, _, _, _ = new_trainer(fn, grid, occupancy_warmup=10 ** 9)
        losses = []
        gen = torch.Generator().manual_seed(5)
        for it in range(steps):
            ro, rd, tgt = batch(n, 100 + it)
            t_rand, u = torch.rand(n, NS, generator=gen).cuda(), torch.rand(n, NI, generator=gen).cuda()
            loss2, out = tr.step(ro, rd, tgt, t_rand=t_rand, u=u)
            losses.append(loss2.clone())
            assert tr.last_step_live
        res[tag] = (tr.flat.clone(), tr.m.clone(), tr.v.clone(), torch.stack(losses), tr.grad.clone(), tr.live_counts.clone())
        if grid is not None:
            assert tr.occupancy_counts.tolist() == [n * NS, n * NS, n * (NS + NI), n * (NS + NI)]
            assert grid.updates == 0 and grid.occupied_fraction() == 1.0
    for a, b, what in zip(res['plain'], res['grid'], ('parameters', 'adam m', 'adam v', 'losses', 'gradient', 'live counts')):
        assert torch.equal(a, b), what
    assert float(res['grid'][3][-1, 0]) != float(res['grid'][3][0, 0])      # the steps did something


# ---- 2. the masked step ----------------------------------------------------------------------------------------------------
def masks():
    h = (np.arange(16) + 0.5) / 16 * 4.0 - 2.0
    half = np.broadcast_to((h > -0.3)[:, None, None], (16, 16, 16)).copy()
    i, j, k = np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing='ij')
    checker = ((i // 2 + j // 2 + k // 2) % 2) == 0
    return {'half': (half, F32(-2.0), F32(2.0)), 'checker': (checker, F32(-1.5), F32(1.5))}


def oracle_grads(sdc, sdf, rays11, z0, z1, bits0, bits1, target, white_bkgd):
    """Autograd of mse(fine) + mse(coarse) on the CPU oracle at the GPU's depths, with the grid's mask applied to raw."""
    rb = torch.from_numpy(rays11)
    leaves = []
    rgbs = []
    for sd, z, bits in ((sdc, z0, bits0), (sdf, z1, bits1)):
        sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        leaves.append(sd)
        z = torch.from_numpy(z)
        pts = rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]
        raw = O.run_network(sd, pts, rb[:, 8:11]) * torch.from_numpy(bits)[..., None].float()
        rgbs.append(O.raw2outputs(raw, z, rb[:, 3:6], None, white_bkgd)[0])
    tgt = torch.from_numpy(target)
    loss0, loss1 = ((rgbs[0] - tgt) ** 2).mean(), ((rgbs[1] - tgt) ** 2).mean()
    (loss0 + loss1).backward()
    names = [nm for nm, _ in O.nerf_param_shapes()]
    return [(('coarse.' if i == 0 else 'fine.') + nm, leaves[i][nm].grad.reshape(-1)) for i in (0, 1) for nm in names], float(loss1), float(loss0)


@pytest.mark.parametrize('mask', ['half', 'checker'])
@pytest.mark.parametrize('perturb', [0, 1])
def test_masked_step_is_exact_where_it_can_be_and_bounded_where_it_cannot(fn, math_mode, compact_on, mask, perturb):
    m, lo, hi = masks()[mask]
    grid = G(fn).from_mask(torch.from_numpy(m).cuda(), lo, hi, outside_occupied=False)
    tr, ktr, kte, (sdc, sdf) = new_trainer(fn, grid, perturb=float(perturb), white_bkgd=True)
    n = 96
    ro, rd, tgt = batch(n, 7)
    rays11 = fn.ops.pack_rays(ro, rd, 2.0, 6.0)
    t_rand = u = None
    if perturb:
        gen = torch.Generator().manual_seed(11)
        t_rand, u = torch.rand(n, NS, generator=gen).cuda(), torch.rand(n, NI, generator=gen).cuda()
    # the render through the same grid on the same weights, BEFORE the step moves them
    with torch.no_grad():
        if perturb:
            ref = fn.render._forward_occ(rays11, tr.net_c, tr.net_f, NS, NI, False, 1.0, True, t_rand, u, grid, skip_dead_rgb=True)
        else:
            ref = fn.render.render_rays(rays11, kte['network_fn'], kte['network_query_fn'], NS, N_importance=NI,
                                        network_fine=kte['network_fine'], white_bkgd=True, occupancy=grid)
        ref_loss, _, _ = fn.ops.mse_leafmax(ref['rgb_map'], ref['rgb0'], tgt)
    loss2, out = tr.step(ro, rd, tgt, t_rand=t_rand, u=u)
    assert same_bits(out['rgb_map'], ref['rgb_map']) and same_bits(out['rgb0'], ref['rgb0'])
    assert same_bits(out['acc_map'], ref['acc_map']) and same_bits(out['disp_map'], ref['disp_map'])
    assert torch.equal(loss2, ref_loss)
    # the counters are grid.query on the sample points (o + d * z: one rounded multiply, one rounded add)
    r11 = rays11.cpu().numpy()
    z0, z1 = out['z0'].cpu().numpy(), out['z_vals'].cpu().numpy()
    q0 = grid.query(torch.from_numpy(R.sample_points(r11, z0)).cuda())
    q1 = grid.query(torch.from_numpy(R.sample_points(r11, z1)).cuda())
    occ = tr.occupancy_counts.tolist()
    assert occ == [int(q0.sum()), n * NS, int(q1.sum()), n * (NS + NI)]
    assert 0.1 * occ[1] < occ[0] < 0.9 * occ[1] and 0.1 * occ[3] < occ[2] < 0.9 * occ[3]
    assert np.array_equal(q0.cpu().numpy(), R.classify(m, lo, hi, False, r11, z0))
    # an unoccupied sample has raw = 0, and the live list of each pass is a subset of its occupied list
    live = tr.live_counts.tolist()      # (live, total) fine, then coarse
    for zk, rk, gk, q, lv in (('z0', 'raw0', 'g_rgb0', q0, live[2]), ('z_vals', 'raw1', 'g_rgb', q1, live[0])):
        raw = region(tr, out, rk)
        assert bool((raw[~q] == 0).all())
        draw = fn.ops.raw2outputs_bwd(raw.contiguous(), out[zk].contiguous(), rays11, region(tr, out, gk).contiguous(), None, True)
        idx, cnt = fn.ops.compact_live(draw)
        k = int(cnt[0])
        assert k == lv and 0 < k
        assert bool(q.reshape(-1)[idx[:k].long()].all()), 'a live sample in an empty cell'
    # gradients against the oracle's autograd with the same mask on raw; bound: tests/test_gpu_compact.py:129
    ref_g, l1, l0 = oracle_grads(sdc, sdf, r11, z0, z1, q0.cpu().numpy(), q1.cpu().numpy(), tgt.cpu().numpy(), True)
    print('losses (fine, coarse): gpu %s oracle (%.8f, %.8f)' % (loss2.tolist(), l1, l0))
    got = tr.grad.cpu()
    off, worst = 0, (0.0, None)
    for name, r in ref_g:
        kk = r.numel()
        err = (got[off:off + kk] - r).abs().max().item()
        scale = max(1.0, r.abs().max().item())
        print('%-36s max|grad - oracle| = %.3g   max|oracle| = %.3g' % (name, err, r.abs().max().item()))
        worst = max(worst, (err / scale, name))
        assert err < 2e-5 * scale, (name, err)
        off += kk
    assert off == got.numel()
    assert float(got.abs().max()) > 0
    print('worst err / max(1, |ref|) = %.3g (%s) under %s' % (worst[0], worst[1], math_mode))


# ---- 3. the empty grid, and what the C ABI refuses ------------------------------------------------------------------------------
@pytest.mark.parametrize('white_bkgd', [False, True])
def test_an_empty_grid_trains_nothing(fn, math_mode, compact_on, white_bkgd):
    empty = G(fn).from_mask(torch.zeros(8, 8, 8, dtype=torch.bool, device='cuda'), -1.0, 1.0, outside_occupied=False)
    tr, _, _, _ = new_trainer(fn, empty, white_bkgd=white_bkgd)
    n = 96
    before = tr.flat.clone()
    tr.grad.fill_(float('nan'))
    for it in range(2):
        ro, rd, tgt = batch(n, 30 + it)
        loss2, out = tr.step(ro, rd, tgt)
        assert torch.count_nonzero(tr.grad) == 0 and bool(torch.isfinite(tr.grad).all())
        bg = 1.0 if white_bkgd else 0.0
        assert bool((out['rgb_map'] == bg).all()) and bool((out['rgb0'] == bg).all()) and bool((out['acc_map'] == 0).all())
        assert tr.occupancy_counts.tolist() == [0, n * NS, 0, n * (NS + NI)]
        assert tr.live_counts.tolist() == [0, n * (NS + NI), 0, n * NS]
    # Adam with a zero gradient and zero moments: the update is lr * 0 / (sqrt(0) + eps) = 0
    assert torch.equal(tr.flat, before) and torch.count_nonzero(tr.m) == 0 and torch.count_nonzero(tr.v) == 0


def test_the_step_refuses_a_grid_it_cannot_honour(fn, compact_on):
    """Returned error codes only: the checks run on the host before anything is enqueued."""
    full = G(fn).for_training(N=4)
    tr, _, _, _ = new_trainer(fn, full, occupancy_warmup=10 ** 9)
    ro, rd, tgt = batch(64, 1)
    tr.step(ro, rd, tgt)
    a = tr._sa
    lib = fn._lib.lib()
    stream = fn._lib.stream()
    torch.cuda.synchronize()
    a.live = 0
    rc = lib.fastnerf_train_step(ctypes.byref(a), 1, stream)
    assert rc == -1 and b'plain backward has no list' in lib.fastnerf_last_error()
    a.live = 1
    noise = torch.zeros(64, NS + NI, device='cuda')
    a.noise1 = noise.data_ptr()
    rc = lib.fastnerf_train_step(ctypes.byref(a), 1, stream)
    assert rc == -1 and b'sigma noise' in lib.fastnerf_last_error()
    a.noise1 = None
    torch.cuda.synchronize()
    # the Python surface says the same, earlier
    args = fn.run_nerf.make_args(N_importance=NI, N_samples=NS, raw_noise_std=1.0, no_reload=True)
    ktr = fn.run_nerf.create_nerf(args)[0]
    K = np.array([[14.0, 0, 4.0], [0, 14.0, 4.0], [0, 0, 1]])
    with pytest.raises(ValueError):
        fn.run_nerf.Trainer(ktr, 8, 8, K, 2.0, 6.0, occupancy=full)
    fn.render.set_compact('0')
    with pytest.raises(ValueError):
        new_trainer(fn, full)
    fn.render.set_compact('1')
    with pytest.raises(ValueError):
        tr.forward_backward(ro, rd, tgt)
    with pytest.raises(ValueError):      # a grid without a density cannot be updated
        G(fn).from_mask(torch.ones(2, 2, 2, dtype=torch.bool, device='cuda'), -1.0, 1.0).update({})
    # render_rays with gradients enabled keeps refusing a grid (tests/test_gpu_occupancy.py::test_errors pins it)
    rays11 = fn.ops.pack_rays(ro, rd, 2.0, 6.0)
    with pytest.raises(ValueError):
        fn.render.render_rays(rays11, tr.net_c, None, NS, N_importance=NI, network_fine=tr.net_f, occupancy=full)


# ---- 4. the grid kernels against numpy -----------------------------------------------------------------------------------------
BOXES = [((16, 16, 16), -1.0, 1.0),
         ((7, 33, 12), np.array([-1.5, 0.1, -3.0], F32), np.array([2.0, 0.7, 5.0], F32)),
         ((1, 1, 1), 0.0, 1.0),
         ((129, 3, 65), -0.3, 0.9),
         ((5, 9, 70), np.array([1000.3, -0.1, 1e-3], F32), np.array([1001.1, 0.2, 3e-3], F32)),      # coarse fp32 steps, tiny cells
         ((3, 3, 3), np.array([-1e-3, 16777.0, -7.7], F32), np.array([2e-3, 16778.0, -7.1], F32)),
         ((128, 128, 4), -1.2, 1.2)]


def cells_ijk(shape):
    return np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), -1).reshape(-1, 3)


@pytest.mark.parametrize('box', range(len(BOXES)))
def test_cell_points_lie_in_their_cells(fn, box):
    shape, lo, hi = BOXES[box]
    rs = np.random.RandomState(box)
    m = rs.rand(*shape) < 0.5
    g = G(fn).from_mask(torch.from_numpy(m).cuda(), lo, hi, outside_occupied=False)
    inv = ~m
    gi = G(fn).from_mask(torch.from_numpy(inv).cuda(), lo, hi, outside_occupied=False)
    ncells = int(np.prod(shape))
    ijk = cells_ijk(shape)
    lo3 = np.broadcast_to(np.asarray(lo, F32), (3,))
    pts = {}
    for seed in (0, 1, 2, 2 ** 40 + 12345):
        rays = torch.full((ncells, 11), 9.0, device='cuda')
        fn.ops.occ_cell_points(g._c, 0, rays, seed)
        again = torch.full((ncells, 11), -9.0, device='cuda')
        fn.ops.occ_cell_points(g._c, 0, again, seed)
        assert torch.equal(rays, again), 'the same seed gives the same bits'
        assert bool((rays[:, 3:] == 0).all())
        p = rays[:, 0:3].cpu().numpy()
        pts[seed] = p
        # its own cell: by the restated arithmetic, and through fastnerf_occ_query under a random mask and its complement
        assert np.array_equal(R.cell_index(p, shape, lo, hi), ijk.astype(F32)), (seed, shape)
        assert np.array_equal(g.query(rays[:, 0:3].contiguous()).cpu().numpy(), m.reshape(-1))
        assert np.array_equal(gi.query(rays[:, 0:3].contiguous()).cpu().numpy(), inv.reshape(-1))
        # a sub-range is the slice of the whole
        c0, k = ncells // 3, max(1, ncells // 2)
        k = min(k, ncells - c0)
        part = torch.empty(k, 11, device='cuda')
        fn.ops.occ_cell_points(g._c, c0, part, seed)
        assert torch.equal(part, rays[c0:c0 + k])
    # seed 0: the centres, lo + (index + 0.5) / inv with every operation rounded to fp32
    centre = (lo3 + ((ijk.astype(F32) + F32(0.5)) / R.inv_of(shape, lo, hi)).astype(F32)).astype(F32)
    assert np.array_equal(pts[0], centre)
    if ncells >= 512:
        assert not np.array_equal(pts[1], pts[2]) and not np.array_equal(pts[1], pts[0])
        # the jitter is uniform over the cell: mean offset 1/2, standard deviation 1/sqrt(12) (5 standard errors)
        frac = ((pts[1].astype(np.float64) - lo3) * R.inv_of(shape, lo, hi).astype(np.float64) - ijk)
        if box not in (4, 5):      # (where a coordinate has only a few fp32 steps per cell the offsets are quantised)
            assert np.abs(frac.mean(0) - 0.5).max() < 5.0 / math.sqrt(12 * ncells)
            assert frac.min() >= -1e-3 and frac.max() <= 1 + 1e-3
    with pytest.raises(RuntimeError):
        fn._lib.check(fn._lib.lib().fastnerf_occ_cell_points(g._c, ncells, 1, 0, 0, None), 'a cell past the end')


def update_ref(dens, raw_c, raw_f, c0, n, decay, thr, dilate, shape):
    """numpy restatement of fastnerf_occ_update -> (dens, mask)."""
    d = dens.copy()
    if n > 0:
        s = raw_c[:n, 3]
        s = np.where(s > 0, s, F32(0))
        if raw_f is not None:
            t = raw_f[:n, 3]
            s = np.where(t > s, t, s)
        old = (d[c0:c0 + n] * F32(decay)).astype(F32)
        d[c0:c0 + n] = np.where(s > old, s, old)
    return d, R.dilated((d > F32(thr)).reshape(shape), dilate)


@pytest.mark.parametrize('shape', [(5, 7, 3), (33, 20, 47), (2, 2, 2), (9, 9, 9), (64, 1, 1), (1, 1, 1), (4, 8, 10)])
@pytest.mark.parametrize('dilate', [0, 1, 2])
def test_update_equals_the_restatement(fn, shape, dilate):
    rs = np.random.RandomState(sum(shape) * 3 + dilate)
    ncells = int(np.prod(shape))
    decay, thr = 0.9, 0.25
    dens = np.zeros(ncells, F32)
    d_gpu = torch.zeros(ncells, device='cuda')
    words = torch.full((fn.ops.occ_words(*shape),), -1, device='cuda', dtype=torch.int32)
    g = G(fn)(words, shape, -1.0, 1.0, True, dens=d_gpu, decay=decay, threshold=thr, dilate=dilate)
    slices = [(0, ncells), (ncells // 3, ncells - ncells // 3 - ncells // 5), (0, 0), (ncells - 1, 1), (0, min(ncells, 37)), (0, ncells),
              (min(ncells - 1, 31), min(ncells - min(ncells - 1, 31), 34))]
    for it, (c0, n) in enumerate(slices):
        raw_c = (rs.randn(max(n, 1), 4) * 0.6).astype(F32)
        raw_c[rs.rand(max(n, 1)) < 0.7, 3] = -1.0      # mostly empty space
        raw_f = (rs.randn(max(n, 1), 4) * 0.6).astype(F32) if it % 2 == 0 else None
        if n > 2:
            raw_c[1, 3] = np.nan
            raw_c[2, 3] = thr      # equal to the threshold: not occupied (unless the old density is)
        fn.ops.occ_update(torch.from_numpy(raw_c).cuda(), None if raw_f is None else torch.from_numpy(raw_f).cuda(), c0, n, shape, decay,
                          thr, dilate, g.dens, g.words)
        dens, mask = update_ref(dens, raw_c, raw_f, c0, n, decay, thr, dilate, shape)
        assert np.array_equal(g.dens.cpu().numpy(), dens), (it, shape)
        assert np.array_equal(g.to_mask().cpu().numpy(), mask), (it, shape)
        assert torch.equal(g.words, fn.ops.occ_from_mask(torch.from_numpy(mask).cuda())), 'bits past the last cell stay clear'
    # the density alone (words = None), then the bits alone (n = 0): what one call does
    d2, w2 = g.dens.clone(), torch.zeros_like(g.words)
    rc = torch.from_numpy((rs.randn(ncells, 4) * 0.6).astype(F32)).cuda()
    fn.ops.occ_update(rc, None, 0, ncells, shape, decay, thr, dilate, d2, None)
    assert torch.equal(w2, torch.zeros_like(w2))
    fn.ops.occ_update(None, None, 0, 0, shape, decay, thr, dilate, d2, w2)
    fn.ops.occ_update(rc, None, 0, ncells, shape, decay, thr, dilate, g.dens, g.words)
    assert torch.equal(d2, g.dens) and torch.equal(w2, g.words)
    assert 0 < mask.sum() or ncells < 8


@pytest.mark.parametrize('decay,thr,d0', [(0.5, 0.1, 1.0), (0.95, 0.01, 1.0), (0.9, 0.5, 8.0)])
def test_a_cell_closes_after_the_updates_decay_implies(fn, decay, thr, d0):
    shape = (6, 5, 7)
    ncells = int(np.prod(shape))
    # open while d0 * decay^k > thr: closed from k = ceil(log(thr / d0) / log(decay)) on (the cases keep d0 * decay^k off thr)
    k_close = math.ceil(math.log(thr / d0) / math.log(decay))
    assert d0 * decay ** (k_close - 1) > thr * 1.01 and d0 * decay ** k_close < thr * 0.99
    c = 97
    dens = torch.zeros(ncells, device='cuda')
    g = G(fn)(torch.zeros(fn.ops.occ_words(*shape), device='cuda', dtype=torch.int32), shape, -1.0, 1.0, True, dens=dens, decay=decay,
              threshold=thr, dilate=0)
    raw = torch.full((ncells, 4), -1.0, device='cuda')
    raw[c, 3] = d0
    fn.ops.occ_update(raw, None, 0, ncells, shape, decay, thr, 0, g.dens, g.words)
    assert int(g.to_mask().sum()) == 1 and bool(g.to_mask().reshape(-1)[c])
    raw[c, 3] = -1.0
    for k in range(1, k_close + 1):
        fn.ops.occ_update(raw, raw, 0, ncells, shape, decay, thr, 0, g.dens, g.words)
        assert bool(g.to_mask().reshape(-1)[c]) == (k < k_close), (k, k_close, float(g.dens[c]))
    assert int(g.to_mask().sum()) == 0


def test_update_from_the_networks(fn, math_mode):
    """grid.update: the jittered points through both networks, the larger sigma, decay, threshold, dilation -- restated with
    the plain forward on the same points; a rotating slice refreshes only its cells."""
    tr, ktr, kte, (sdc, _) = new_trainer(fn)
    shape = (11, 13, 9)
    ncells = int(np.prod(shape))
    g = G(fn).for_training(N=shape, bound=1.3, threshold=0.02, dilate=1, decay=0.8)
    assert g.occupied_fraction() == 1.0 and int(g.dens.count_nonzero()) == 0
    dens = np.zeros(ncells, F32)

    def sigma_at(seed, c0, n):
        rays = torch.empty(n, 11, device='cuda')
        fn.ops.occ_cell_points(g._c, c0, rays, seed)
        z = torch.zeros(n, 1, device='cuda')
        return [fn.ops.mlp_fwd(rays, z, net.flat, net.packed()[0]).reshape(n, 4).cpu().numpy() for net in (tr.net_c, tr.net_f)]

    # the coarse network's sigma bias is moved so that each network is the larger one on part of the grid: the maximum matters
    rc, rf = sigma_at(1, 0, ncells)
    key = [k for k in sdc if k.startswith('alpha_linear') and k.endswith('bias')][0]
    moved = dict(sdc)
    moved[key] = sdc[key] + float(np.median(rf[:, 3] - rc[:, 3]))
    tr.net_c.load_state_dict(moved)
    rc, rf = sigma_at(1, 0, ncells)
    thr = g.threshold = float(np.median(np.maximum(rc[:, 3], rf[:, 3])))      # about half of the cells lie above it
    g.update(kte, cells_per_call=100)      # the first update takes every cell whatever the slice
    rc, rf = sigma_at(1, 0, ncells)
    assert (rc[:, 3] > rf[:, 3]).mean() > 0.1 and (rf[:, 3] > rc[:, 3]).mean() > 0.1
    dens, mask = update_ref(dens, rc, rf, 0, ncells, 0.8, thr, 1, shape)
    assert np.array_equal(g.dens.cpu().numpy(), dens) and np.array_equal(g.to_mask().cpu().numpy(), mask)
    assert 0.3 < (dens > F32(thr)).mean() < 0.7 and g.updates == 1 and g.cursor == 0
    cur = 0
    for call in range(12):      # 12 slices of 200 cells wrap around the 1287 cells
        g.update(kte, cells_per_call=200)
        for c0, n in ((cur, min(200, ncells - cur)),) + (((0, cur + 200 - ncells),) if cur + 200 > ncells else ()):
            rc, rf = sigma_at(2 + call, c0, n)
            dens, mask = update_ref(dens, rc, rf, c0, n, 0.8, thr, 1, shape)
        cur = (cur + 200) % ncells
        assert g.cursor == cur
        assert np.array_equal(g.dens.cpu().numpy(), dens) and np.array_equal(g.to_mask().cpu().numpy(), mask), call
    g.update(kte, seed=0)      # centres, everything
    rc, rf = sigma_at(0, 0, ncells)
    dens, mask = update_ref(dens, rc, rf, 0, ncells, 0.8, thr, 1, shape)
    assert np.array_equal(g.dens.cpu().numpy(), dens) and np.array_equal(g.to_mask().cpu().numpy(), mask)


# ---- 5. save / load ------------------------------------------------------------------------------------------------------------
def test_save_and_load_keep_the_density(fn, tmp_path):
    tr, ktr, kte, _ = new_trainer(fn)
    g = G(fn).for_training(N=(9, 10, 11), bound=1.1, threshold=0.03, dilate=2, decay=0.7, outside_occupied=False)
    g.update(kte)
    g.update(kte, cells_per_call=123)
    p = str(tmp_path / 'train_grid.npz')
    g.save(p)
    h = G(fn).load(p)
    assert torch.equal(h.words, g.words) and torch.equal(h.dens, g.dens) and h.shape == g.shape
    assert (h.decay, h.threshold, h.dilate, h.updates, h.cursor, h.primed, h.outside_occupied) == (0.7, 0.03, 2, 2, 123, True, False)
    assert np.array_equal(h.lo, g.lo) and np.array_equal(h.hi, g.hi) and np.array_equal(h.inv, g.inv)
    g.update(kte, cells_per_call=123)
    h.update(kte, cells_per_call=123)      # the loaded grid goes on exactly where the saved one stood
    assert torch.equal(h.words, g.words) and torch.equal(h.dens, g.dens)
    # a file of the layout before there was a density: the documented fields, written here
    m = np.random.RandomState(3).rand(5, 6, 7) < 0.4
    c = np.arange(m.size)
    words = np.zeros((m.size + 31) // 32, np.uint32)
    np.bitwise_or.at(words, c[m.reshape(-1)] >> 5, (np.uint32(1) << (c[m.reshape(-1)] & 31).astype(np.uint32)))
    old = str(tmp_path / 'old_grid.npz')
    with open(old, 'wb') as fh:
        np.savez(fh, words=words, shape=np.asarray(m.shape, np.int64), lo=np.array([-1, -2, 0.5], F32), hi=np.array([1, 0.25, 3], F32),
                 outside_occupied=np.asarray(False))
    o = G(fn).load(old)
    assert o.dens is None and o.decay is None and np.array_equal(o.to_mask().cpu().numpy(), m) and o.outside_occupied is False
    with pytest.raises(ValueError):
        o.update(kte)
    o.save(str(tmp_path / 'again.npz'))
    with np.load(str(tmp_path / 'again.npz')) as f:
        assert sorted(f.files) == ['hi', 'lo', 'outside_occupied', 'shape', 'words']


# ---- 6. training on the solid-body scene ---------------------------------------------------------------------------------------
CUTOFF = 1.5


def solid_scene(fn, n_rays):
    from fastnerf import synthetic
    dev = torch.device('cuda')
    focal = 0.5 * 800 / np.tan(0.5 * 0.6911112070083618)
    K = np.array([[focal, 0, 400.0], [0, focal, 400.0], [0, 0, 1]])
    poses = torch.stack([synthetic.pose_spherical(-180.0 + 3.6 * k, -30.0, 4.0)[:3, :4] for k in range(100)], 0).to(dev)

    def draw(gen):
        pix = torch.stack([torch.randint(0, 100, (n_rays,), generator=gen), torch.randint(0, 800, (n_rays,), generator=gen),
                           torch.randint(0, 800, (n_rays,), generator=gen)], 1).int().to(dev)
        ro, rd = fn.ops.gen_rays_pixels(pix, poses, K)
        return ro, rd, synthetic.render_rays(ro, rd, cutoff=CUTOFF).contiguous()

    def held_out(kte, n=8192):
        """PSNR of the trained networks (rendered WITHOUT a grid) on rays of views between the training azimuths, at another elevation."""
        gen = torch.Generator().manual_seed(4242)
        views = torch.stack([synthetic.pose_spherical(-180.0 + 36.0 * k + 1.8, -20.0, 4.0)[:3, :4] for k in range(10)], 0).to(dev)
        pix = torch.stack([torch.randint(0, 10, (n,), generator=gen), torch.randint(0, 800, (n,), generator=gen),
                           torch.randint(0, 800, (n,), generator=gen)], 1).int().to(dev)
        ro, rd = fn.ops.gen_rays_pixels(pix, views, K)
        gt = synthetic.render_rays(ro, rd, cutoff=CUTOFF)
        with torch.no_grad():
            out = fn.render.render_rays(fn.ops.pack_rays(ro, rd, 2.0, 6.0), kte['network_fn'], kte['network_query_fn'], NS, N_importance=NI,
                                        network_fine=kte['network_fine'], white_bkgd=True)
        return -10.0 * math.log10(float(((out['rgb_map'] - gt) ** 2).mean()))
    return K, draw, held_out


def train_run(fn, seed, steps, n_rays, grid_kw):
    """-> (held-out PSNR, grid or None, occupied share of the samples per refresh period)."""
    K, draw, held_out = solid_scene(fn, n_rays)
    args = fn.run_nerf.make_args(N_importance=NI, N_samples=NS, perturb=1.0, white_bkgd=True, no_reload=True, lrate=5e-4, lrate_decay=500)
    torch.manual_seed(seed)
    ktr, kte, _, _, _, _ = fn.run_nerf.create_nerf(args)
    grid = None if grid_kw is None else G(fn).for_training(**grid_kw.get('grid', {}))
    extra = {} if grid is None else dict(occupancy=grid, occupancy_every=grid_kw.get('every', 16), occupancy_warmup=grid_kw.get('warmup', 256))
    tr = fn.run_nerf.Trainer(ktr, 800, 800, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500, **extra)
    gen = torch.Generator().manual_seed(1000 + seed)
    shares = []
    for it in range(steps):
        tr.step(*draw(gen))
        if grid is not None and it % 64 == 63:
            c = tr.occupancy_counts.tolist()
            shares.append(((c[0] + c[2]) / (c[1] + c[3]), grid.occupied_fraction()))
    return held_out(kte), grid, shares


def support_cells(grid):
    """bool [nx, ny, nz]: cells whose centre lies within CUTOFF standard deviations of a body's centre (the analytic scene)."""
    from fastnerf import synthetic
    axes = [grid.lo[a] + (np.arange(grid.shape[a]) + 0.5) * (grid.hi[a] - grid.lo[a]) / grid.shape[a] for a in range(3)]
    X, Y, Z = np.meshgrid(*axes, indexing='ij')
    inside = np.zeros(grid.shape, bool)
    for c, s, _, _ in synthetic.BLOBS:
        inside |= ((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) <= (CUTOFF * s) ** 2
    return inside


def check_grid(grid, shares):
    inside = support_cells(grid)
    mask = grid.to_mask().cpu().numpy()
    print('occupied share of the samples / of the cells, every 64 steps:', ' '.join('%.3f/%.3f' % s for s in shares))
    print('cells inside a body\'s %.1f-sigma support: %d, clear among them: %d; occupied cells %.4f' % (
        CUTOFF, int(inside.sum()), int((inside & ~mask).sum()), mask.mean()))
    assert shares[0][0] == 1.0, 'the grid is full through the warm-up'
    assert shares[-1][0] < 1.0 and shares[-1][1] < 1.0, 'the occupied share falls below 1 after the warm-up'
    assert inside.sum() > 0 and not (inside & ~mask).any(), 'a cell inside a body is clear'


def test_training_through_the_grid_on_the_solid_body_scene(fn):
    old = fn.ops.get_math()
    fn.ops.set_math('bf16x6')
    try:
        psnr, grid, shares = train_run(fn, 0, 640, 1024, dict(grid=dict(N=64), warmup=256, every=16))
        print('held-out PSNR after 640 steps of 1024 rays: %.2f dB' % psnr)
        assert grid.updates == (640 - 256 + 15) // 16
        check_grid(grid, shares)
    finally:
        fn.ops.set_math(old)


@pytest.mark.slow
def test_psnr_with_and_without_the_grid_over_seeds(fn):
    """A study (marked slow: not part of a plain -m gpu run; its figures belong in profiles/occupancy_train.md): paired held-out PSNR of Trainer with and without the grid over 8 seeds.  Free
    runs are chaotic, so the yardstick is the no-grid Trainer's own spread over the same seeds (existing behaviour): the
    standard error of a difference of two such runs' means, se = sqrt(2) * std(no-grid PSNR) / sqrt(seeds).  The mean paired
    difference must lie within 2 se + 0.1 dB (the north star's bound) of zero."""
    seeds = int(os.environ.get('OCC_TRAIN_SEEDS', 8))
    steps = int(os.environ.get('OCC_TRAIN_STEPS', 1000))
    assert seeds >= 8
    old = fn.ops.get_math()
    fn.ops.set_math('bf16x6')
    try:
        plain, with_grid = [], []
        for seed in range(seeds):
            p, _, _ = train_run(fn, seed, steps, 4096, None)
            q, grid, shares = train_run(fn, seed, steps, 4096, dict(grid=dict(N=128), warmup=256, every=16))
            check_grid(grid, shares)
            plain.append(p)
            with_grid.append(q)
            print('seed %d: no grid %.3f dB, grid %.3f dB, difference %+.3f dB' % (seed, p, q, q - p), flush=True)
        plain, with_grid = np.array(plain), np.array(with_grid)
        d = with_grid - plain
        se_null = math.sqrt(2.0) * plain.std(ddof=1) / math.sqrt(seeds)
        print('no grid: mean %.3f dB, std over seeds %.3f dB; grid: mean %.3f dB, std %.3f dB' % (
            plain.mean(), plain.std(ddof=1), with_grid.mean(), with_grid.std(ddof=1)))
        print('mean paired difference %+.3f dB, its own standard error %.3f dB; yardstick se %.3f dB, bound 2 se + 0.1 = %.3f dB' % (
            d.mean(), d.std(ddof=1) / math.sqrt(seeds), se_null, 2 * se_null + 0.1))
        assert abs(d.mean()) <= 2 * se_null + 0.1
    finally:
        fn.ops.set_math(old)
