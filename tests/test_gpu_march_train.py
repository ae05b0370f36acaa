"""Marched training on the GPU (include/fastnerf.h, "marched training"): fastnerf_occ_march_jitter bit for bit against fastnerf_occ_march
and the restatement of tests/march_train_numpy.py, fastnerf_train_step_march against its parts called by hand through ops, the marched
gradient against the dense one-pass step through the grid (no jitter) and against float64 autograd of its own row (jitter), the
overflow mask, and run_nerf.Trainer(..., march=K).  Networks: ert_numpy.scene_networks (opaque)."""
import ctypes

import numpy as np
import pytest
import torch

import ert_numpy as E
import march_numpy as M
import march_train_numpy as MT
import occ_numpy as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32
CAM = np.array([[14.0, 0, 4.0], [0, 14.0, 4.0], [0, 0, 1]])


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


def same_f32(got, want):
    """The same floats bit for bit; NaNs in the same places (a NaN's payload is not part of the contract)."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


def bits(t):
    return t.contiguous().view(torch.int32)


def device_grid(fn, grid):
    """march_numpy grid -> OccupancyGrid / OccupancyCascade."""
    G = fn.occupancy
    if grid[0] == 'grid':
        return G.OccupancyGrid.from_mask(torch.from_numpy(grid[1]).cuda(), grid[2], grid[3], grid[4])
    return G.OccupancyCascade([G.OccupancyGrid.from_mask(torch.from_numpy(m).cuda(), lo, hi, False) for m, lo, hi in grid[1]],
                              outside_occupied=grid[2])


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------------
def kernel_rays(n):
    """n rays of the scene camera (tests/test_gpu_march.py), every one finite with near < far: what the zero-shift identity is stated for."""
    rays = R.scene_rays(O, side=13 if n <= 169 else 18)
    return rays[np.round(np.linspace(0, rays.shape[0] - 1, n)).astype(int)].copy()


# (37, 13, 5): a partial block, overflow on most rays; (193, 256, 64): a block boundary; (300, 2048, 128): a long walk
@pytest.mark.parametrize('n,K,C', [(37, 13, 5), (193, 256, 64), (300, 2048, 128)])
@pytest.mark.parametrize('scene', ['two_shells', 'cascade', 'cascade_outside'])
@pytest.mark.parametrize('lindisp', [False, True])
def test_jitter_kernel(fn, n, K, C, scene, lindisp):
    grid = M.cascade2(True) if scene == 'cascade_outside' else M.scene_grids()[scene]
    g = device_grid(fn, grid)
    rays = kernel_rays(n)
    rays_t = torch.from_numpy(rays).cuda()
    ops = fn.ops

    def rounds(B, **kw):
        got = (None, None, None, None)
        for s0, s1 in E.segments(C, B):
            z, kidx, overflow, state = got
            got = ops.occ_march_jitter(g._c, rays_t, K, C, s0=s0, s1=s1, lindisp=lindisp, state=state, z=z, kidx=kidx, overflow=overflow, **kw)
        return [t.cpu().numpy() for t in got]

    # zero shift, given or implied, is fastnerf_occ_march bit for bit
    plain = [t.cpu().numpy() for t in ops.occ_march(g._c, rays_t, K, C, lindisp=lindisp)]
    for kw in (dict(u=torch.zeros(n, device='cuda')), dict(u=None, seed=0)):
        got = rounds(C, **kw)
        assert same_f32(got[0], plain[0]), kw
        assert all(np.array_equal(a, b) for a, b in zip(got[1:], plain[1:])), kw
    # an injected shift and two seeds: the restatement bit for bit, in one round and in rounds
    u = np.random.RandomState(K + C).rand(n).astype(F32)
    u[:3] = [0.0, np.nextafter(F32(1), F32(0)), 0.5]
    seen = []
    for kw, uu in ((dict(u=torch.from_numpy(u).cuda()), u), (dict(seed=7), MT.draw_u(n, 7)), (dict(seed=2 ** 40 + 3), MT.draw_u(n, 2 ** 40 + 3))):
        want, live = MT.march(grid, rays, K, C, uu, lindisp)      # one round; rounds reproduce it (tests/test_march_train_cpu.py)
        for B in (C, 2, 16):
            got = rounds(B, **kw)
            assert same_f32(got[0], want[0]), (list(kw), B, 'z')
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (list(kw), B)
            if B == C:
                assert np.array_equal(got[3], want[3]), 'state'
        assert (want[1] >= 0).any()
        seen.append(want[0])
    assert not np.array_equal(seen[1], seen[2]), 'two seeds, two sets of rows'
    assert not same_f32(seen[0], plain[0]), 'a shift moves the depths'
    # the object's method passes the shift through
    z, kidx, overflow = g.march(rays_t, K, C, lindisp=lindisp, seed=7)
    want, _ = MT.march(grid, rays, K, C, MT.draw_u(n, 7), lindisp)
    assert same_f32(z.cpu().numpy(), want[0]) and np.array_equal(kidx.cpu().numpy(), want[1])
    assert overflow.dtype == torch.bool and np.array_equal(overflow.cpu().numpy(), want[2].astype(bool))


def test_kernel_argument_errors(fn):
    g = device_grid(fn, M.two_shells())
    rays_t = torch.from_numpy(R.scene_rays(O, side=4)).cuda()
    u = torch.zeros(16, device='cuda')
    with pytest.raises(ValueError):
        fn.ops.occ_march_jitter(g._c, rays_t, 1, 64, u=u)
    with pytest.raises(ValueError):
        fn.ops.occ_march_jitter(g._c, rays_t, 64, 513, u=u)
    with pytest.raises(ValueError):
        fn.ops.occ_march_jitter(g._c, rays_t, 64, 16, u=u, s0=4, s1=8)      # a later round without the state of the one before
    with pytest.raises(AssertionError):
        fn.ops.occ_march_jitter(g._c, rays_t, 64, 16, u=u[:15])
    z, kidx, overflow, state = fn.ops.occ_march_jitter(g._c, rays_t, 64, 16, u=u, s0=0, s1=8)
    with pytest.raises(RuntimeError):
        fn.ops.occ_march_jitter(g._c, rays_t, 64, 16, u=u, s0=8, s1=17, state=state, z=z, kidx=kidx, overflow=overflow)
    with pytest.raises(TypeError):
        fn.ops.occ_march_jitter(None, rays_t, 64, 16, u=u)
    with pytest.raises(ValueError):
        g.march(rays_t, 64, 16, u=u[:15])
    with pytest.raises(RuntimeError):
        g.march(rays_t, 64, 16, u=np.zeros(16, F32))


# ---- trainers ------------------------------------------------------------------------------------------------------------------------
def new_trainer(fn, grid, N_samples=16, N_importance=16, perturb=0., white_bkgd=True, **kw):
    """A Trainer over create_nerf's networks with the opaque scene networks loaded; N_importance = 0: one network."""
    args = fn.run_nerf.make_args(N_importance=N_importance, N_samples=N_samples, perturb=perturb, white_bkgd=white_bkgd, use_viewdirs=True,
                                 no_reload=True)
    torch.manual_seed(0)
    ktr = fn.run_nerf.create_nerf(args)[0]
    sdc, sdf = E.scene_networks(O)
    ktr['network_fn'].load_state_dict(sdc)
    if ktr.get('network_fine') is not None:
        ktr['network_fine'].load_state_dict(sdf)
    return fn.run_nerf.Trainer(ktr, 8, 8, CAM, 2.0, 6.0, occupancy=grid, **kw), ktr, (sdc, sdf)


def batch(n, seed, pool=None):
    """n rays of cameras on the sphere of radius 4 looking at the origin (rows of `pool` when given), and random targets."""
    if pool is None:
        pool = np.concatenate([R.scene_rays(O, side=16), R.scene_rays(O, side=16, focal=20.0)], 0)
        pool = pool[np.round(np.linspace(0, pool.shape[0] - 1, n)).astype(int)]
    assert pool.shape[0] == n
    gen = torch.Generator().manual_seed(seed)
    r = torch.from_numpy(pool)
    return r[:, 0:3].contiguous().cuda(), r[:, 3:6].contiguous().cuda(), torch.rand(n, 3, generator=gen).cuda()


def block_view(tr, name):
    off, shape = tr._march_regions[name]
    return tr._march_block[off:off + int(np.prod(shape))].view(shape)


def by_hand(fn, tr, grid, ro, rd, tgt, u, K, C, which, tighten=False, grad_scale=1.0, seed=0):
    """The launches of fastnerf_train_step_march through ops, on copies of the trainer's state: dict of the gradient and, after the
    update, the marched half of flat / m / v and its packed pair."""
    ops = fn.ops
    Nn = ops.NET_PARAMS
    n = ro.shape[0]
    sl = slice(which * Nn, (which + 1) * Nn)
    params, m, v = tr.flat[sl].clone(), tr.m[sl].clone(), tr.v[sl].clone()
    pf, pb = ops.mlp_pack(params)      # (a copy of the trainer's pair: the same bits from the same parameters)
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip((pf, pb), tr.pf if which else tr.pc))
    rays11 = ops.pack_rays(ro, rd, 2.0, 6.0)
    if tighten:
        ops.occ_ray_bounds(grid._c, rays11, write_back=True)
    z, kidx, overflow, _ = ops.occ_march_jitter(grid._c, rays11, K, C, u=u, seed=seed)
    raw = torch.empty(n, C, 4, device='cuda')
    counts = torch.zeros(2, device='cuda', dtype=torch.int32)
    idx, cnt = ops.march_list(kidx, 0, C, raw=raw, total=counts, lattice=n * K)
    ops.mlp_fwd_list(rays11, z, params, pf, raw, idx, cnt, flags=1 if tr.skip_dead_rgb else 0)
    maps = ops.raw2outputs_fwd(raw, z, rays11, None, bool(tr.white_bkgd))
    rgb = maps[0]
    loss2, g, _ = ops.mse_leafmax(rgb, None, tgt, grad_scale=grad_scale)
    g_unmasked = g.clone()
    ops.march_mask(overflow, g)
    P = n * C
    ws = torch.empty(ops.dact_floats(P), device='cuda')
    draw = torch.empty(P * 4, device='cuda')
    act = torch.empty(ops.act_floats(P), device='cuda')
    partial = torch.empty(ops.mlp_bwd_partial_floats(), device='cuda')
    live_ws = torch.empty(ops.live_ws_ints(P), device='cuda', dtype=torch.int32)
    grad = torch.full((Nn,), float('nan'), device='cuda')
    ops.render_rays_bwd_live(rays11, bool(tr.white_bkgd), g, None, None, None, z, raw, None, None, params, (pf, pb), None, None, draw, act,
                             ws, partial, live_ws, grad, None, C, 0)
    res = dict(grad=grad.clone(), z=z, kidx=kidx, overflow=overflow, rgb=rgb, loss2=loss2, g=g, g_unmasked=g_unmasked, counts=counts,
               rays11=rays11, raw=raw)
    ops.adam_step(params, grad, m, v, tr.lr, tr.adam_t + 1, tr.beta1, tr.beta2, tr.eps)
    ops.mlp_pack(params, pf, pb)
    res.update(flat=params, m=m, v=v, pf=pf, pb=pb)
    return res


# ---- 2. one step is its parts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tighten', [False, True])
def test_one_step_is_its_parts(fn, math_mode, compact_on, tighten):
    n, K, C = 193, 64, 32
    grid = device_grid(fn, M.two_shells())
    assert not grid.outside_occupied
    Nn = fn.ops.NET_PARAMS
    ro, rd, tgt = batch(n, 3)
    u = torch.from_numpy(np.random.RandomState(9).rand(n).astype(F32)).cuda()
    tr, _, _ = new_trainer(fn, grid, march=K, march_cap=C, tighten=tighten)
    tr.m.uniform_(-1e-3, 1e-3)      # moments that an update has to read
    tr.v.uniform_(0, 1e-6)
    which = 1
    other = slice(0, Nn)
    hand = by_hand(fn, tr, grid, ro, rd, tgt, u, K, C, which, tighten)
    before = [t.clone() for t in (tr.flat[other], tr.m[other], tr.v[other], tr.pc[0], tr.pc[1])]
    state0 = [t.clone() for t in (tr.flat, tr.m, tr.v)]
    loss2, out = tr.step(ro, rd, tgt, march_u=u, decay=False)
    torch.cuda.synchronize()
    # (the tightened lattice is denser on the shells: some of its rows overflow 32 slots, and the mask is part of the comparison)
    assert int((hand['kidx'] >= 0).sum()) > 4 * n and bool(hand['overflow'].any()) == tighten and not bool(hand['overflow'].all())
    assert torch.equal(out['march_k'], hand['kidx']) and torch.equal(bits(out['z_vals']), bits(hand['z']))
    assert torch.equal(bits(out['rgb_map']), bits(hand['rgb'])) and torch.equal(bits(loss2[:1]), bits(hand['loss2'][:1]))
    assert tr.march_counts.tolist() == hand['counts'].tolist() == [int((hand['kidx'] >= 0).sum()), n * K]
    sl = slice(Nn, 2 * Nn)
    assert torch.equal(bits(tr.grad[sl]), bits(hand['grad'])), 'gradient of the marched half'
    assert float(hand['grad'].abs().max()) > 0
    for name, mine in (('flat', tr.flat[sl]), ('m', tr.m[sl]), ('v', tr.v[sl]), ('pf', tr.pf[0]), ('pb', tr.pf[1])):
        assert torch.equal(bits(mine), bits(hand[name])), name
    assert not torch.equal(tr.flat[sl], state0[0][sl]), 'the update moved the marched network'
    for name, mine, was in zip(('flat', 'm', 'v', 'packed_fwd', 'packed_bwd'), (tr.flat[other], tr.m[other], tr.v[other], tr.pc[0], tr.pc[1]), before):
        assert torch.equal(bits(mine), bits(was)), 'the other network: ' + name
    # FORWARD | BWD, then UPDATE, as two calls: the same bits
    tr2, _, _ = new_trainer(fn, grid, march=K, march_cap=C, tighten=tighten)
    tr2.m.copy_(state0[1])
    tr2.v.copy_(state0[2])
    tr2.adam_t += 1
    a, x, out2, _ = tr2._march_prepare(K, C, ro, rd, tgt, None, None, 0, u, None)
    a.lr, a.adam_t = float(tr2.lr), int(tr2.adam_t)
    L = fn._lib
    tr2._march_call(a, x, L.STEP_FORWARD | L.STEP_BWD_FINE | L.STEP_BWD_COARSE)
    torch.cuda.synchronize()
    assert torch.equal(bits(tr2.grad[sl]), bits(tr.grad[sl])) and torch.equal(bits(tr2.flat), bits(state0[0])), 'no update yet'
    tr2._march_call(a, x, L.STEP_UPDATE)
    torch.cuda.synchronize()
    for name, p, q in (('flat', tr2.flat, tr.flat), ('m', tr2.m, tr.m), ('v', tr2.v, tr.v), ('pf', tr2.pf[0], tr.pf[0]), ('pb', tr2.pf[1], tr.pf[1]),
                       ('pc', tr2.pc[0], tr.pc[0])):
        assert torch.equal(bits(p), bits(q)), name


# ---- 3 / 4. the gradient: against the dense one-pass step, and against float64 -------------------------------------------------------------
K3, C3, N3 = 256, 128, 128


def entries(live):
    """Length of the packed sequence of every ray: its live lattice points and one closing entry per run."""
    lv = np.concatenate([np.zeros((live.shape[0], 1), bool), live], 1)
    return live.sum(1) + (lv[:, 1:] & ~lv[:, :-1]).sum(1)


def chosen_rays(u_seed):
    """128 rays of two cameras on the ball scene that fit C3 slots and leave lattice point K3 - 1 empty, unshifted and under the shifts
    of `u_seed` alike (decided on the restatement; the tests assert it again from the kernel's outputs): 112 that cross the ball -- the
    centre of the image does not fit, the chord there is 154 lattice points long -- and 16 that miss it.  -> (rays [128, 11], u [128])."""
    pool = np.concatenate([R.scene_rays(O, side=24, focal=30.0), R.scene_rays(O, side=24, focal=20.0)], 0)
    grid = M.scene_grids()['ball']
    u = np.random.RandomState(u_seed).rand(pool.shape[0]).astype(F32)
    ok = np.ones(pool.shape[0], bool)
    hit = np.ones(pool.shape[0], bool)
    for uu in (np.zeros_like(u), u):
        live = M.live_bits(grid, pool, MT.jittered_lattice(pool, K3, uu)[:, :K3])
        ok &= (entries(live) <= C3) & ~live[:, K3 - 1]
        hit &= live.sum(1) >= 8
    a, b = np.nonzero(ok & hit)[0], np.nonzero(ok & ~hit & (entries(live) == 0))[0]
    assert a.size >= 112 and b.size >= 16
    sel = np.sort(np.concatenate([a[np.round(np.linspace(0, a.size - 1, 112)).astype(int)], b[np.round(np.linspace(0, b.size - 1, 16)).astype(int)]]))
    assert np.unique(sel).size == N3
    return pool[sel].copy(), u[sel].copy()


def march_and_dense(fn, u=None):
    """One marched step (network_fn, which = 0) and one step of today's Trainer(N_samples = K3, N_importance = 0, occupancy = grid,
    perturb = 0) on the same network and batch: (marched trainer, its out, dense trainer, its out, rays, targets, the network's state)."""
    grid = device_grid(fn, M.scene_grids()['ball'])
    rays, u_sel = chosen_rays(21)
    ro, rd, tgt = batch(N3, 4, pool=rays)
    trm, _, (sdc, _) = new_trainer(fn, grid, N_samples=K3, N_importance=0, march=K3, march_cap=C3)
    _, outm = trm.step(ro, rd, tgt, march_u=None if u is None else torch.from_numpy(u_sel).cuda())
    trd, _, _ = new_trainer(fn, grid, N_samples=K3, N_importance=0)
    _, outd = trd.step(ro, rd, tgt)
    torch.cuda.synchronize()
    # the condition, from the kernel's own outputs: no ray overflows, no ray has lattice point K - 1 live
    assert not bool(outm['march_overflow'].any()) and int(outm['march_k'].max()) < K3 - 1
    assert int((outm['march_k'] >= 0).any(1).sum()) >= 112
    return trm, outm, trd, outd, rays, tgt, sdc, grid


def test_no_jitter_equals_the_dense_one_pass_step(fn, math_mode, compact_on):
    trm, outm, trd, outd, _, _, _, grid = march_and_dense(fn)
    Nn = fn.ops.NET_PARAMS
    assert trm.grad.numel() == trd.grad.numel() == Nn
    # the marched samples are the dense step's occupied samples
    assert trm.march_counts.tolist() == [trd.occupancy_counts.tolist()[0], N3 * K3]
    gm, gd = trm.grad, trd.grad
    err, scale = float((gm - gd).abs().max()), float(gd.abs().max())
    print('%s: max|g_march - g_dense| = %.3g, max|g_dense| = %.3g, ratio %.3g (bar 3e-6)' % (math_mode, err, scale, err / scale))
    assert scale > 0
    assert err < 3e-6 * scale


_F64 = {}


def f64_grad(sd, rays11, z, live, target, white_bkgd):
    """float64 autograd of the mean squared error of a row: the network at o + d * z of the slots `live`, zero logits elsewhere, the
    reference's raw2outputs over the whole row.  -> the flat gradient in parameter order (tests/test_gpu_occupancy_train.py, oracle_grads)."""
    sd = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    rb = torch.from_numpy(rays11).double()
    z = torch.from_numpy(z).double()
    lv = torch.from_numpy(live)
    pts = (rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None])[lv]
    dirs = rb[:, None, 8:11].expand(z.shape[0], z.shape[1], 3)[lv]
    x = torch.cat([O.posenc(pts, 10), O.posenc(dirs, 4)], -1)
    raw = torch.zeros(z.shape[0], z.shape[1], 4, dtype=torch.float64)
    raw[lv] = O.nerf_forward(sd, x)
    rgb = O.raw2outputs(raw, z, rb[:, 3:6], None, white_bkgd)[0]
    ((rgb - torch.from_numpy(target).double()) ** 2).mean().backward()
    return torch.cat([sd[nm].grad.reshape(-1) for nm, _ in O.nerf_param_shapes()])


def test_jittered_gradient_against_float64(fn, math_mode, compact_on):
    """Figures (max|g - g64| / max|g64|, marched against the dense twin) are printed per math mode; profiles/march_train.md holds them."""
    trm, outm, trd, outd, rays, tgt, sdc, grid = march_and_dense(fn, u=True)
    r11 = fn.ops.pack_rays(*batch(N3, 4, pool=rays)[:2], 2.0, 6.0).cpu().numpy()
    zm, km = outm['z_vals'].cpu().numpy(), outm['march_k'].cpu().numpy()
    zd = outd['z_vals'].cpu().numpy()
    qd = grid.query(torch.from_numpy(R.sample_points(r11, zd)).cuda()).cpu().numpy()
    if 'ref' not in _F64:      # computed once: depths and live sets do not depend on the math mode
        t = tgt.cpu().numpy()
        _F64['ref'] = (zm, km, zd, qd, f64_grad(sdc, r11, zm, km >= 0, t, True), f64_grad(sdc, r11, zd, qd, t, True))
    zm0, km0, zd0, qd0, ref_m, ref_d = _F64['ref']
    assert np.array_equal(zm, zm0) and np.array_equal(km, km0) and np.array_equal(zd, zd0) and np.array_equal(qd, qd0)
    assert not np.array_equal(zm[km >= 0], M.lattice(r11, K3)[np.nonzero(km >= 0)[0], km[km >= 0]]), 'the rows are shifted'
    em = float((trm.grad.cpu().double() - ref_m).abs().max() / ref_m.abs().max())
    ed = float((trd.grad.cpu().double() - ref_d).abs().max() / ref_d.abs().max())
    print('%s: marched |g - g64| / max|g64| = %.3g, dense twin %.3g, ratio %.3g (bar 2)' % (math_mode, em, ed, em / ed))
    assert float(ref_m.abs().max()) > 0 and ed > 0
    assert em <= 2 * ed


# ---- 5. overflow ------------------------------------------------------------------------------------------------------------------------
def test_overflowed_rays_do_not_train_the_field(fn, math_mode, compact_on):
    n, K, C = 96, 13, 5
    grid = device_grid(fn, M.two_shells())
    ro, rd, tgt = batch(n, 6)
    u = torch.from_numpy(np.random.RandomState(5).rand(n).astype(F32)).cuda()
    tr, _, _ = new_trainer(fn, grid, march=K, march_cap=C)
    hand = by_hand(fn, tr, grid, ro, rd, tgt, u, K, C, 1)
    loss2, out = tr.step(ro, rd, tgt, march_u=u)
    torch.cuda.synchronize()
    ov = out['march_overflow']
    assert ov.dtype == torch.bool and 4 <= int(ov.sum()) <= n - 4 and int(((out['march_k'] >= 0).any(1) & ~ov).sum()) >= 8
    g = block_view(tr, 'g_rgb')
    assert bool((g[ov] == 0).all()), 'rows of the overflowed rays'
    assert torch.equal(bits(g[~ov]), bits(hand['g_unmasked'][~ov])) and bool((hand['g_unmasked'][ov] != 0).any())
    assert torch.equal(bits(g), bits(torch.from_numpy(MT.mask(ov.cpu().numpy(), hand['g_unmasked'].cpu().numpy())).cuda()))
    # the loss is that of the unmasked call: the mean over all n rays
    want, _, _ = fn.ops.mse_leafmax(out['rgb_map'], None, tgt)
    assert torch.equal(bits(loss2[:1]), bits(want[:1]))
    assert abs(float(loss2[0]) - float(((out['rgb_map'] - tgt) ** 2).mean())) < 1e-6
    # the gradient is that of the rays that fit alone, both divided by the same n
    keep = ~ov
    tr2, _, _ = new_trainer(fn, grid, march=K, march_cap=C)
    tr2.step(ro[keep].contiguous(), rd[keep].contiguous(), tgt[keep].contiguous(), march_u=u[keep].contiguous(), n_global=n)
    Nn = fn.ops.NET_PARAMS
    g1, g2 = tr.grad[Nn:], tr2.grad[Nn:]
    err, scale = float((g1 - g2).abs().max()), float(g2.abs().max())
    print('%s: max|g_all - g_fitting| = %.3g, max|g| = %.3g' % (math_mode, err, scale))
    assert scale > 0 and err < 3e-6 * scale


# ---- 6. the trainer ---------------------------------------------------------------------------------------------------------------------
def test_trainer_routing_counts_and_determinism(fn, compact_on):
    n, K, C, NS, NI = 96, 64, 32, 16, 16
    G = fn.occupancy.OccupancyGrid
    mask = torch.from_numpy(M.two_shells()[1]).cuda()

    def fresh():      # a training grid over the two shells, warm from the start (the bits are kept until the first refresh)
        g = G.for_training(N=32, bound=1.5, outside_occupied=False)
        g.words.copy_(fn.ops.occ_from_mask(mask))
        return g

    def run(march, steps=4):
        torch.manual_seed(123)
        kw = dict(march=K, march_cap=C, march_after=2) if march else {}
        tr, _, _ = new_trainer(fn, fresh(), N_samples=NS, N_importance=NI, perturb=1.0, occupancy_warmup=10 ** 9, **kw)
        log = []
        for it in range(steps):
            ro, rd, tgt = batch(n, 40 + it)
            loss2, out = tr.step(ro, rd, tgt)
            log.append((tr.grad.clone(), tr.occupancy_counts.clone(), tr.flat.clone(), loss2.clone(), out))
        return tr, log

    tr_g, log_g = run(False, steps=2)
    tr_m, log_m = run(True)
    for it in range(2):      # before march_after: today's step through the grid
        assert 'march_overflow' not in log_m[it][4]
        for a, b, what in zip(log_g[it][:4], log_m[it][:4], ('grad', 'occupancy_counts', 'flat', 'loss2')):
            assert torch.equal(bits(a), bits(b)), (it, what)
    assert tr_m.occupancy_steps == 4
    out = log_m[3][4]
    assert set(('rgb_map', 'disp_map', 'acc_map', 'depth_map', 'march_overflow')) <= set(out.keys())
    assert out['rgb_map'].shape == (n, 3) and out['depth_map'].shape == (n,) and out['march_overflow'].shape == (n,)
    assert tr_m.march_counts.tolist() == [int((out['march_k'] >= 0).sum()), n * K] and tr_m.march_counts.tolist()[0] > n
    # perturb draws the shift from the 'mrch' stream of the step's seed
    seed = int(tr_m._ma[1].seed)
    assert seed != 0
    ro, rd, _ = batch(n, 43)
    want, _ = MT.march(M.two_shells(), fn.ops.pack_rays(ro, rd, 2.0, 6.0).cpu().numpy(), K, C, MT.draw_u(n, seed))
    assert same_f32(out['z_vals'].cpu().numpy(), want[0]) and np.array_equal(out['march_k'].cpu().numpy(), want[1])
    # a marched step leaves the coarse network alone
    Nn = fn.ops.NET_PARAMS
    assert torch.equal(bits(log_m[3][2][:Nn]), bits(log_m[1][2][:Nn])) and not torch.equal(log_m[3][2][Nn:], log_m[1][2][Nn:])
    # the same seeds, the same bits
    tr_r, log_r = run(True)
    for it in range(4):
        for a, b, what in zip(log_r[it][:4], log_m[it][:4], ('grad', 'occupancy_counts', 'flat', 'loss2')):
            assert torch.equal(bits(a), bits(b)), (it, what)
    assert torch.equal(bits(tr_r.m), bits(tr_m.m)) and torch.equal(bits(tr_r.v), bits(tr_m.v))
    # the settings are read on every step
    tr_m.march = None
    _, out = tr_m.step(*batch(n, 50))
    assert 'march_overflow' not in out
    tr_m.march, tr_m.march_cap, tr_m.perturb = 32, 16, 0.
    _, out = tr_m.step(*batch(n, 51))
    assert out['march_k'].shape == (n, 16) and tr_m.march_counts.tolist()[1] == n * 32 and int(tr_m._ma[1].seed) == 0


def test_trainer_refusals(fn, compact_on):
    grid = device_grid(fn, M.two_shells())
    n = 32
    ro, rd, tgt = batch(n, 1)
    with pytest.raises(ValueError, match='needs occupancy'):
        new_trainer(fn, None, march=64)
    inside_out = fn.occupancy.OccupancyGrid.from_mask(torch.from_numpy(M.two_shells()[1]).cuda(), -1.5, 1.5, True)
    with pytest.raises(ValueError, match='outside_occupied=False'):
        new_trainer(fn, inside_out, march=64)
    with pytest.raises(ValueError, match='2 <= march'):
        new_trainer(fn, grid, march=1)
    with pytest.raises(ValueError, match='2 <= march'):
        new_trainer(fn, grid, march=64, march_cap=513)
    # depth / opacity terms that are on
    tr, ktr, _ = new_trainer(fn, grid, march=64, march_cap=32, lambda_depth=0.1, lambda_acc=0.1)
    tr.step(ro, rd, tgt)      # no target: no term is on
    with pytest.raises(ValueError, match='depth / opacity'):
        tr.step(ro, rd, tgt, depth=torch.ones(n, device='cuda'))
    with pytest.raises(ValueError, match='depth / opacity'):
        tr.step(ro, rd, tgt, acc=torch.ones(n, device='cuda'))
    with pytest.raises(ValueError, match='forward_backward'):
        tr.forward_backward(ro, rd, tgt)
    # a grid set to something the march cannot walk, after construction: refused at the next step
    tr.occupancy = inside_out
    with pytest.raises(ValueError, match='outside_occupied=False'):
        tr.step(ro, rd, tgt)
    # sigma noise, and a trainer off the fused step
    args = fn.run_nerf.make_args(N_importance=16, N_samples=16, raw_noise_std=1.0, use_viewdirs=True, no_reload=True)
    with pytest.raises(ValueError, match='raw_noise_std'):
        fn.run_nerf.Trainer(fn.run_nerf.create_nerf(args)[0], 8, 8, CAM, 2.0, 6.0, occupancy=grid, march=64)
    args = fn.run_nerf.make_args(N_importance=16, N_samples=16, use_viewdirs=False, no_reload=True)
    with pytest.raises(ValueError, match='fused step'):
        fn.run_nerf.Trainer(fn.run_nerf.create_nerf(args)[0], 8, 8, CAM, 2.0, 6.0, occupancy=grid, march=64)
    # the C ABI says the same where it can be asked
    tr, _, _ = new_trainer(fn, grid, march=64, march_cap=32)
    tr.step(ro, rd, tgt)
    torch.cuda.synchronize()
    a, x = tr._ma
    lib = fn._lib.lib()
    a.live = 0
    assert lib.fastnerf_train_step_march(ctypes.byref(a), ctypes.byref(x), 1, fn._lib.stream()) == -1
    assert b'live' in lib.fastnerf_last_error()
    a.live, a.occ = 1, None
    assert lib.fastnerf_train_step_march(ctypes.byref(a), ctypes.byref(x), 1, fn._lib.stream()) == -1
    assert b'occ' in lib.fastnerf_last_error()


def test_update_which(fn, math_mode):
    """update(which='both') is update(); which='fine' / 'coarse' follow that network alone (the restatement of
    tests/test_gpu_occupancy_train.py with the other term dropped)."""
    G = fn.occupancy.OccupancyGrid
    tr, ktr, _ = new_trainer(fn, None)
    shape = (11, 13, 9)
    ncells = int(np.prod(shape))
    # random-init networks, the coarse one's sigma bias moved so that each network is the larger one on part of the grid
    sdc, sdf = R.scene_networks(O)
    tr.net_f.load_state_dict(sdf)
    tr.net_c.load_state_dict(sdc)

    def sigma_at(g, seed, net):
        rays = torch.empty(ncells, 11, device='cuda')
        fn.ops.occ_cell_points(g._c, 0, rays, seed)
        return fn.ops.mlp_fwd(rays, torch.zeros(ncells, 1, device='cuda'), net.flat, net.packed()[0]).reshape(ncells, 4)[:, 3].cpu().numpy()

    probe = G.for_training(N=shape, bound=1.3)
    rc, rf = sigma_at(probe, 1, tr.net_c), sigma_at(probe, 1, tr.net_f)
    key = [k for k in sdc if k.startswith('alpha_linear') and k.endswith('bias')][0]
    tr.net_c.load_state_dict(dict(sdc, **{key: sdc[key] + float(np.median(rf - rc))}))
    rc = sigma_at(probe, 1, tr.net_c)
    assert (rc > rf).mean() > 0.1 and (rf > rc).mean() > 0.1
    thr = float(np.median(np.maximum(rc, rf)))
    grids = {w: G.for_training(N=shape, bound=1.3, threshold=thr, dilate=1, decay=0.8) for w in (None, 'both', 'fine', 'coarse')}
    dens = {w: np.zeros(ncells, F32) for w in ('fine', 'coarse')}
    for it in range(2):
        for w, g in grids.items():
            g.update(ktr) if w is None else g.update(ktr, which=w)
        assert torch.equal(grids[None].dens, grids['both'].dens) and torch.equal(grids[None].words, grids['both'].words)
        for w, net in (('fine', tr.net_f), ('coarse', tr.net_c)):
            g = grids[w]
            s = sigma_at(g, it + 1, net)
            s = np.where(s > 0, s, F32(0))
            old = (dens[w] * F32(0.8)).astype(F32)
            dens[w] = np.where(s > old, s, old)
            assert np.array_equal(g.dens.cpu().numpy(), dens[w]), (w, it)
            assert np.array_equal(g.to_mask().cpu().numpy(), R.dilated((dens[w] > F32(thr)).reshape(shape), 1)), (w, it)
    assert not torch.equal(grids['fine'].dens, grids['coarse'].dens) and not torch.equal(grids['fine'].dens, grids['both'].dens)
    with pytest.raises(ValueError):
        grids['fine'].update(ktr, which='finest')
