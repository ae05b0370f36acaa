"""Training through an occupancy cascade: the own cells of a level (fastnerf_occ_cascade_own), the refresh over their concatenation
(fastnerf_occ_cascade_points / _update) against each level's own OccupancyGrid.update, the budget's cursor, and the fused, tightened
and marched steps through a cascade (fastnerf_train_step_cascade / _march_cascade) against the step through a grid, the plain
compacted step and the cascade's own classify / march.  Every check is an equality of bits or integers.  The restatement of the
covered rule and of the cursor is tests/occ_cascade_train_numpy.py, pinned on the CPU by tests/test_cascade_train_cpu.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

import occ_cascade_train_numpy as T
import occ_numpy as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
NS = NI = 8
N_RAYS = 300
CAM = np.array([[14.0, 0, 4.0], [0, 14.0, 4.0], [0, 0, 1]])
SCENES = T.scenes()


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


@pytest.fixture
def compact_on(fn):
    old = fn.render.get_compact()
    fn.render.set_compact('1')
    yield
    fn.render.set_compact(old)


@pytest.fixture(params=['fp32', 'bf16x6'])
def math2(request, fn):
    old = fn.ops.get_math()
    fn.ops.set_math(request.param)
    yield request.param
    fn.ops.set_math(old)


def level_grid(fn, level, mask=None, outside=True, dilate=1, decay=0.95, threshold=0.):
    """A training grid over the level's box, built by hand through the constructor: bits (and the density) from `mask`, all set
    with a zero density when there is none -- OccupancyGrid.for_training over any box."""
    shape, lo, hi = level
    m = torch.ones(shape, dtype=torch.bool, device='cuda') if mask is None else torch.from_numpy(mask).cuda()
    dens = torch.zeros(int(np.prod(shape)), device='cuda') if mask is None else m.reshape(-1).float().contiguous()
    return fn.occupancy.OccupancyGrid(fn.ops.occ_from_mask(m), shape, lo, hi, outside, dens=dens, decay=decay, threshold=threshold,
                                      dilate=dilate)


def cascade_of(fn, levels, masks=None, outside=True, **kw):
    grids = [level_grid(fn, L, None if masks is None else masks[l], outside, **kw) for l, L in enumerate(levels)]
    return fn.occupancy.OccupancyCascade(grids, outside)


def copy_grid(fn, g):
    c = fn.occupancy.OccupancyGrid(g.words.clone(), g.shape, g.lo, g.hi, g.outside_occupied, dens=g.dens.clone(), decay=g.decay,
                                   threshold=g.threshold, dilate=g.dilate)
    c.updates, c.cursor, c.primed = g.updates, g.cursor, g.primed
    return c


def checker(shape, period=2):
    i, j, k = np.meshgrid(*[np.arange(s) for s in shape], indexing='ij')
    return ((i // period + j // period + k // period) % 2) == 0


def new_trainer(fn, occupancy=None, perturb=1.0, white_bkgd=True, **kw):
    args = fn.run_nerf.make_args(N_importance=NI, N_samples=NS, perturb=perturb, white_bkgd=white_bkgd, use_viewdirs=True, no_reload=True)
    torch.manual_seed(0)
    ktr = fn.run_nerf.create_nerf(args)[0]
    sdc, sdf = R.scene_networks(O)
    ktr['network_fn'].load_state_dict(sdc)
    ktr['network_fine'].load_state_dict(sdf)
    extra = {} if occupancy is None else dict(occupancy=occupancy, **kw)
    return fn.run_nerf.Trainer(ktr, 8, 8, CAM, 2.0, 6.0, **extra), ktr


_POOL = []


def batch(n, seed):
    """n rays of cameras on the sphere of radius 4 looking at the origin, and random targets."""
    if not _POOL:
        _POOL.append(torch.from_numpy(np.concatenate([R.scene_rays(O, side=16), R.scene_rays(O, side=16, focal=20.0)], 0)))
    gen = torch.Generator().manual_seed(seed)
    r = _POOL[0][torch.randint(0, _POOL[0].shape[0], (n,), generator=gen)]
    return r[:, 0:3].contiguous().cuda(), r[:, 3:6].contiguous().cuda(), torch.rand(n, 3, generator=gen).cuda()


def region(tr, out, name):
    off, shape = tr._regions[name]
    return out._block[off:off + int(np.prod(shape))].view(shape)


def run_steps(tr, steps, march=False, first=0):
    """`steps` steps on fixed batches and injected draws -> (losses [steps, 2], counts per step)."""
    losses, counts = [], []
    for it in range(first, first + steps):
        ro, rd, tgt = batch(N_RAYS, 100 + it)
        gen = torch.Generator().manual_seed(500 + it)
        if march:
            loss2, _ = tr.step(ro, rd, tgt, march_u=torch.rand(N_RAYS, generator=gen).cuda())
            counts.append(tr.march_counts.tolist())
        else:
            loss2, _ = tr.step(ro, rd, tgt, t_rand=torch.rand(N_RAYS, NS, generator=gen).cuda(), u=torch.rand(N_RAYS, NI, generator=gen).cuda())
            counts.append(tr.occupancy_counts.tolist() if tr.occupancy_counts is not None else None)
        losses.append(loss2.clone())
    return torch.stack(losses), counts


# ---- 1. own lists ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dilate', [0, 1, 2])
@pytest.mark.parametrize('name', sorted(SCENES))
def test_own_lists_equal_the_restatement(fn, name, dilate):
    levels = SCENES[name]
    c = cascade_of(fn, levels, dilate=dilate)
    want, off = T.concatenation(levels, dilate)
    assert c.offsets == off.tolist()
    for l in range(len(levels)):
        got = c.own_cells(l)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), T.own_cells(levels, l, dilate)), (name, l)
        again = fn.ops.occ_cascade_own(c._c, l, dilate, 'cuda')
        assert torch.equal(got, again), 'twice in a row gives the same bits'
    assert np.array_equal(c._own.cpu().numpy(), want)


def test_for_training(fn):
    c = fn.occupancy.OccupancyCascade.for_training(levels=3, N=16)
    assert c.levels == 3 and c.outside_occupied is True and c.dens is not None and (c.updates, c.cursor, c.primed) == (0, 0, False)
    levels = SCENES['concentric']
    for l, g in enumerate(c.grids):
        assert g.shape == (16, 16, 16) and np.array_equal(g.lo, levels[l][1]) and np.array_equal(g.hi, levels[l][2])
        assert g.occupied_fraction() == 1.0 and int(torch.count_nonzero(g.dens)) == 0
        assert np.array_equal(c.own_cells(l).cpu().numpy(), T.own_cells(levels, l, 1))
    assert [c.own_cells(l).numel() for l in range(3)] == [4096, 4088, 4088]
    d = fn.occupancy.OccupancyCascade.for_training(levels=3, N=[(6, 5, 7), (5, 5, 4), (4, 6, 3)], outside_occupied=False, dilate=0)
    assert [g.shape for g in d.grids] == [(6, 5, 7), (5, 5, 4), (4, 6, 3)] and d.outside_occupied is False
    assert np.array_equal(d._own.cpu().numpy(), T.concatenation(SCENES['noncubic'], 0)[0])
    e = fn.occupancy.OccupancyCascade.for_training(levels=2, N=[8, 4], growth=1.5)
    assert [g.shape for g in e.grids] == [(8, 8, 8), (4, 4, 4)] and np.array_equal(e.grids[1].hi, np.full(3, 1.2 * 1.5, F32))
    m = fn.occupancy.OccupancyCascade.for_training(levels=2, N=[16, (5, 5, 4)])      # a count for one level, a triple for another
    assert [g.shape for g in m.grids] == [(16, 16, 16), (5, 5, 4)]
    # by hand: one dilate, and a level without a density makes a rendering cascade
    g0, g1 = level_grid(fn, levels[0], dilate=1), level_grid(fn, levels[1], dilate=2)
    with pytest.raises(ValueError, match='dilate'):
        fn.occupancy.OccupancyCascade([g0, g1])
    plain = fn.occupancy.OccupancyGrid.from_mask(torch.ones(4, 4, 4, dtype=torch.bool, device='cuda'), -3.0, 3.0)
    r = fn.occupancy.OccupancyCascade([g0, plain])
    assert r.dens is None
    with pytest.raises(ValueError, match='for_training'):
        r.update({})
    with pytest.raises(ValueError, match='OccupancyCascade'):
        new_trainer(fn, r)


# ---- 2. the refresh against each level's own update --------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['both', 'fine'])
@pytest.mark.parametrize('name', sorted(SCENES))
def test_refresh_equals_each_levels_own_update(fn, name, which):
    levels = SCENES[name]
    _, kw = new_trainer(fn)
    # Thresholds that close most of the cells, so that the bits -- dilation at the seams included -- can differ: the scene networks' sigma
    # is positive everywhere, and a refresh leaves the same density whatever the threshold, so each level takes the 0.95 quantile of
    # its own fully refreshed density (a test input; thresholds may differ from level to level, dilate may not).
    probe = [level_grid(fn, L, outside=False, decay=0.9) for L in levels]
    for g in probe:
        g.update(kw, seed=5, which=which)
    thr = [float(torch.quantile(g.dens, 0.95)) for g in probe]
    c = fn.occupancy.OccupancyCascade([level_grid(fn, L, outside=False, decay=0.9, threshold=t) for L, t in zip(levels, thr)], False)
    c.CHUNK = 777 if name == 'concentric' else 97      # smaller than a level: launches span level boundaries
    refs = [copy_grid(fn, g) for g in c.grids]
    pts = torch.from_numpy(T.points(levels, 100000, seed=3)).cuda()
    for seed in (5, 6):      # the second refresh decays what the first one left
        c.update(kw, seed=seed, which=which)
        for g in refs:
            g.update(kw, seed=seed, which=which)
        nonzero = 0
        for l, (g, ref) in enumerate(zip(c.grids, refs)):
            own = c.own_cells(l).long()
            cov = torch.ones(g.ncells, dtype=torch.bool, device='cuda')
            cov[own] = False
            assert torch.equal(g.dens[own].view(torch.int32), ref.dens[own].view(torch.int32)), (name, l, seed)
            assert int(torch.count_nonzero(g.dens[cov])) == 0
            assert np.array_equal(cov.cpu().numpy(), T.covered(levels, l, 1).reshape(-1))
            nonzero += int(torch.count_nonzero(g.dens))
        assert nonzero > 0, 'the networks are positive somewhere'
        fracs = [ref.occupied_fraction() for ref in refs]
        print('%s seed %d: occupied fraction of the fully refreshed levels %s' % (name, seed, fracs))
        if seed == 5:      # set and clear bits on every level of a useful size
            assert all(0.0 < f < 1.0 for f, L in zip(fracs, levels) if np.prod(L[0]) >= 100), fracs
        full = fn.occupancy.OccupancyCascade(refs, False)
        assert torch.equal(c.query(pts), full.query(pts))
    assert c.updates == 2 and c.primed and c.cursor == 0
    q = c.query(pts)
    assert 0 < int(q.sum()) < q.numel()


def test_default_seed_follows_the_updates(fn):
    levels = SCENES['noncubic']
    _, kw = new_trainer(fn)
    a, b = cascade_of(fn, levels), cascade_of(fn, levels)
    a.update(kw)
    a.update(kw)
    b.update(kw, seed=1)
    b.update(kw, seed=2)
    for g, h in zip(a.grids, b.grids):
        assert torch.equal(g.dens, h.dens) and torch.equal(g.words, h.words)


# ---- 3. the budget ----------------------------------------------------------------------------------------------------------------------
def test_budget_refreshes_the_restatements_slices(fn):
    levels = SCENES['noncubic']
    _, kw = new_trainer(fn)
    c = cascade_of(fn, levels, decay=0.5)
    c.CHUNK = 64
    own, off = T.concatenation(levels, 1)
    total, k = int(off[-1]), 101
    assert total % k != 0 and total > 2 * k
    c.update(kw, cells_per_call=k)      # the first call takes everything
    assert c.primed and c.cursor == 0
    for g in c.grids:
        g.dens.fill_(2.0 ** 20)           # a sentinel above every sigma: a refreshed cell halves, nothing else moves
    times = [np.zeros(int(np.prod(L[0])), np.int64) for L in levels]
    cursor = 0
    calls = math.ceil(total / k)
    for call in range(calls):
        before = [g.dens.clone() for g in c.grids]
        pos, cursor = T.refresh_slice(cursor, True, total, k)
        c.update(kw, cells_per_call=k)
        assert c.cursor == cursor
        lv, _ = T.level_of(off, pos)
        for l, g in enumerate(c.grids):
            want = np.zeros(g.ncells, bool)
            want[own[pos[lv == l]]] = True
            changed = (g.dens != before[l]).cpu().numpy()
            assert np.array_equal(changed, want), (call, l)
            assert bool((g.dens[torch.from_numpy(want).cuda()] == before[l][torch.from_numpy(want).cuda()] * 0.5).all())
            times[l] += want
    # ceil(total / k) calls of k positions: every own cell once, the k * calls - total positions the last call wrapped onto twice
    pos_times = np.concatenate([times[l][own[off[l]:off[l + 1]]] for l in range(len(levels))])
    wrapped = k * calls - total
    assert (pos_times[:wrapped] == 2).all() and (pos_times[wrapped:] == 1).all()
    for l, L in enumerate(levels):
        cov = T.covered(levels, l, 1).reshape(-1)
        assert (times[l][cov] == 0).all()
        assert bool((c.grids[l].dens[torch.from_numpy(cov).cuda()] == 2.0 ** 20).all())
    assert c.updates == 1 + calls


# ---- 4. one level is the grid -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['fused', 'tighten', 'march'])
def test_one_level_cascade_is_its_grid_bit_for_bit(fn, math2, compact_on, route):
    steps = 6
    kw = dict(occupancy_warmup=1, occupancy_every=2, occupancy_cells=1500)
    if route != 'fused':
        kw['tighten'] = True
    if route == 'march':
        kw.update(march=16, march_cap=24)
    res = {}
    for tag in ('grid', 'cascade'):
        # (threshold: the scene networks' sigma is 0.06 .. 0.08 everywhere, so this closes part of the cells and the bits matter)
        g = fn.occupancy.OccupancyGrid.for_training(N=16, bound=1.2, threshold=0.07, outside_occupied=(route == 'fused'))
        occ = g if tag == 'grid' else fn.occupancy.OccupancyCascade([g])
        tr, _ = new_trainer(fn, occ, **kw)
        losses, counts = run_steps(tr, steps, march=(route == 'march'))
        res[tag] = (tr.flat.clone(), tr.m.clone(), losses, counts, g.dens.clone(), g.words.clone(), (occ.updates, occ.cursor, occ.primed))
        if tag == 'cascade':
            assert route == 'march' or tr._sa.occ is None      # the cascade travels beside fn_step_args, not in it
    for a, b, what in zip(res['grid'], res['cascade'], ('parameters', 'adam m', 'losses', 'counts', 'density', 'bits', 'cursor')):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b, what
    assert res['grid'][6] == (3, 3000 % 4096, True)
    assert 0 < int(torch.count_nonzero(res['grid'][4])) and res['grid'][3][-1][0] < res['grid'][3][-1][1]      # the refresh closed cells
    assert float(res['grid'][2][-1, 0]) != float(res['grid'][2][0, 0])


# ---- 5. several levels -----------------------------------------------------------------------------------------------------------------
def test_an_all_ones_cascade_is_the_plain_compacted_step(fn, math2, compact_on):
    steps = 4
    res = {}
    for tag in ('plain', 'cascade'):
        occ = cascade_of(fn, SCENES['concentric'], outside=True) if tag == 'cascade' else None
        tr, _ = new_trainer(fn, occ, occupancy_warmup=10 ** 9)
        losses, counts = run_steps(tr, steps)
        assert tr.last_step_live
        res[tag] = (tr.flat.clone(), tr.m.clone(), tr.v.clone(), losses, tr.grad.clone(), tr.live_counts.clone())
        if occ is not None:
            assert counts[-1] == [N_RAYS * NS, N_RAYS * NS, N_RAYS * (NS + NI), N_RAYS * (NS + NI)] and occ.updates == 0
    for a, b, what in zip(res['plain'], res['cascade'], ('parameters', 'adam m', 'adam v', 'losses', 'gradient', 'live counts')):
        assert torch.equal(a, b), what
    assert float(res['cascade'][3][-1, 0]) != float(res['cascade'][3][0, 0])


def checker_cascade(fn, outside=False):
    levels = SCENES['concentric']
    return cascade_of(fn, levels, [checker(L[0], 2 + l) for l, L in enumerate(levels)], outside)


@pytest.mark.parametrize('tighten', [False, True])
def test_counts_are_the_cascades_classify_and_empty_samples_are_zero(fn, math2, compact_on, tighten):
    c = checker_cascade(fn)
    tr, _ = new_trainer(fn, c, occupancy_warmup=10 ** 9, tighten=tighten)
    ro, rd, tgt = batch(N_RAYS, 7)
    gen = torch.Generator().manual_seed(11)
    loss2, out = tr.step(ro, rd, tgt, t_rand=torch.rand(N_RAYS, NS, generator=gen).cuda(), u=torch.rand(N_RAYS, NI, generator=gen).cuda())
    rays11 = fn.ops.pack_rays(ro, rd, 2.0, 6.0)
    if tighten:
        rays11 = c.tighten(rays11)[0].contiguous()
        assert not torch.equal(rays11[:, 6:8], fn.ops.pack_rays(ro, rd, 2.0, 6.0)[:, 6:8])
    occ = tr.occupancy_counts.tolist()
    for zk, rk, pair, S in (('z0', 'raw0', occ[0:2], NS), ('z_vals', 'raw1', occ[2:4], NS + NI)):
        z = out[zk].contiguous()
        idx, cnt = c.classify(rays11, z)
        assert pair == cnt.tolist() == [int(cnt[0]), N_RAYS * S]
        assert 0.05 * pair[1] < pair[0] < 0.95 * pair[1]
        live = torch.zeros(N_RAYS * S, dtype=torch.bool, device='cuda')
        live[idx[:int(cnt[0])].long()] = True
        raw = region(tr, out, rk).reshape(-1, 4)
        assert int(torch.count_nonzero(raw[~live])) == 0, 'an empty sample has raw = (0, 0, 0, 0) exactly'
        assert int(torch.count_nonzero(raw[live])) > 0
        who = c.decided_by((rays11[:, None, 0:3] + rays11[:, None, 3:6] * z[..., None]).reshape(-1, 3))
        assert all(int((who == l).sum()) > 0 for l in range(3)) or tighten
    assert int(torch.count_nonzero(tr.grad)) > 0


def test_an_all_empty_cascade_trains_nothing(fn, math2, compact_on):
    levels = SCENES['concentric']
    c = cascade_of(fn, levels, [np.zeros(L[0], bool) for L in levels], False)
    tr, _ = new_trainer(fn, c, occupancy_warmup=10 ** 9)
    before = tr.flat.clone()
    tr.grad.fill_(float('nan'))
    for it in range(2):
        ro, rd, tgt = batch(N_RAYS, 30 + it)
        _, out = tr.step(ro, rd, tgt)
        assert int(torch.count_nonzero(tr.grad)) == 0 and bool(torch.isfinite(tr.grad).all())
        assert bool((out['rgb_map'] == 1.0).all()) and bool((out['acc_map'] == 0).all())
        assert tr.occupancy_counts.tolist() == [0, N_RAYS * NS, 0, N_RAYS * (NS + NI)]
    assert torch.equal(tr.flat, before) and int(torch.count_nonzero(tr.m)) == 0


def test_marched_rows_are_the_cascades_march(fn, math2, compact_on):
    c = checker_cascade(fn)
    K, C = 32, 20      # about half the rows of this cascade hold more than 20 entries
    tr, _ = new_trainer(fn, c, occupancy_warmup=10 ** 9, march=K, march_cap=C)
    ro, rd, tgt = batch(N_RAYS, 9)
    u = torch.rand(N_RAYS, generator=torch.Generator().manual_seed(4)).cuda()
    before = tr.flat.clone()
    _, out = tr.step(ro, rd, tgt, march_u=u)
    z, kidx, overflow = c.march(fn.ops.pack_rays(ro, rd, 2.0, 6.0), K, C, u=u)
    assert torch.equal(out['march_k'], kidx) and torch.equal(out['march_overflow'], overflow)
    assert torch.equal(out['z_vals'].view(torch.int32), z.view(torch.int32))
    assert tr.march_counts.tolist() == [int((kidx >= 0).sum()), N_RAYS * K]
    assert 0 < int(overflow.sum()) < N_RAYS and 0 < tr.march_counts.tolist()[0]
    assert not torch.equal(tr.flat, before)
    with pytest.raises(ValueError, match='outside_occupied'):
        new_trainer(fn, checker_cascade(fn, outside=True), march=K, march_cap=C)


# ---- 6. refusals: return codes only, before anything is enqueued ---------------------------------------------------------------------
def test_the_step_refuses(fn, compact_on):
    c = checker_cascade(fn)
    tr, _ = new_trainer(fn, c, occupancy_warmup=10 ** 9)
    ro, rd, tgt = batch(64, 1)
    tr.step(ro, rd, tgt)
    torch.cuda.synchronize()
    a, lib, stream = tr._sa, fn._lib.lib(), fn._lib.stream()
    call = lambda cc: lib.fastnerf_train_step_cascade(ctypes.byref(a), None, None, None, None, ctypes.byref(cc), 1, stream)      # noqa: E731
    assert a.occ is None
    a.occ = ctypes.addressof(c.grids[0]._c)
    assert call(c._c) == -1 and b'occ == NULL' in lib.fastnerf_last_error()
    a.occ = None
    bad = fn._lib.OccCascade()
    ctypes.memmove(ctypes.byref(bad), ctypes.byref(c._c), ctypes.sizeof(bad))
    bad.level[1].words = None
    assert call(bad) == -1 and b'non-null words' in lib.fastnerf_last_error()
    bad.level[1].words = c._c.level[1].words
    bad.levels = 9
    assert call(bad) == -1
    a.live = 0
    assert call(c._c) == -1 and b'plain backward has no list' in lib.fastnerf_last_error()
    a.live = 1
    x = fn._lib.StepMarch()
    x.K, x.C = 16, 16
    a.occ = ctypes.addressof(c.grids[0]._c)
    rc = lib.fastnerf_train_step_march_cascade(ctypes.byref(a), ctypes.byref(x), None, None, None, ctypes.byref(c._c), 1, stream)
    assert rc == -1 and b'occ == NULL' in lib.fastnerf_last_error()
    a.occ = None
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        tr.forward_backward(ro, rd, tgt)


# ---- 7. save, load, continue -------------------------------------------------------------------------------------------------------------
def test_save_load_continue(fn, compact_on, tmp_path):
    kw = dict(occupancy_warmup=1, occupancy_every=1, occupancy_cells=3000)
    make = lambda: fn.occupancy.OccupancyCascade.for_training(levels=3, N=16, outside_occupied=False, decay=0.9)      # noqa: E731
    whole = make()
    tr, _ = new_trainer(fn, whole, **kw)
    run_steps(tr, 6)
    first = make()
    tr2, _ = new_trainer(fn, first, **kw)
    run_steps(tr2, 3)
    p = str(tmp_path / 'cascade.npz')
    first.save(p)
    saved = first.grids[2].dens.clone()
    loaded = fn.occupancy.OccupancyCascade.load(p)
    assert (loaded.updates, loaded.cursor, loaded.primed) == (first.updates, first.cursor, first.primed) == (2, 3000, True)
    assert loaded.dens is not None and torch.equal(loaded._own, first._own) and loaded.offsets == first.offsets
    tr2.occupancy = loaded
    run_steps(tr2, 3, first=3)
    assert torch.equal(tr.flat, tr2.flat) and torch.equal(tr.m, tr2.m)
    for g, h in zip(whole.grids, loaded.grids):
        assert torch.equal(g.dens, h.dens) and torch.equal(g.words, h.words)
    assert (loaded.updates, loaded.cursor) == (whole.updates, whole.cursor) == (5, (4 * 3000) % (4096 + 2 * 4088))
    # a file from before cascades were trained through: the levels' fields alone
    with np.load(p) as f:
        old = {k: f[k] for k in f.files if k not in ('updates', 'cursor', 'primed')}
    q = str(tmp_path / 'old.npz')
    with open(q, 'wb') as fh:
        np.savez(fh, **old)
    o = fn.occupancy.OccupancyCascade.load(q)
    assert (o.updates, o.cursor, o.primed) == (0, 0, False) and torch.equal(o.grids[2].dens, saved)
