"""A step on an empty batch (the shard of a data-parallel tail batch that holds no ray), on one GPU and on every route of
run_nerf.Trainer.step: it renders nothing, leaves the host RNG where a step on rays leaves it, zeroes the gradient of the slice the
step would have trained, takes Adam over that slice with the zero gradient, repacks, and touches neither the grid nor -- on the marched
routes -- the other network."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CAM = np.array([[14.0, 0, 4.0], [0, 14.0, 4.0], [0, 0, 1]])
N = 32


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


def bits(t):
    return t.contiguous().view(torch.int32)


def small_grid(fn):
    """5 x 6 x 7 cells over [-1.5, 1.5)^3, about half of them set, with a density: a grid that a step on rays refreshes at once
    (occupancy_warmup = 0 below)."""
    g = torch.Generator().manual_seed(4)
    shape = (5, 6, 7)
    words = fn.ops.occ_from_mask((torch.rand(shape, generator=g) < 0.5).cuda())
    dens = torch.rand(shape[0] * shape[1] * shape[2], generator=g).cuda()
    return fn.occupancy.OccupancyGrid(words, shape, -1.5, 1.5, outside_occupied=False, dens=dens, decay=0.95)


# route -> (make_args keywords, Trainer keywords, fused, a march_u is given, seeds a step on rays draws)
ROUTES = {
    'fused': (dict(), None, True, False, 2),
    'fused_noise': (dict(raw_noise_std=1.0), None, True, False, 3),
    'call_by_call': (dict(), None, False, False, 2),
    'march': (dict(), dict(march=32, march_cap=16, march_after=0, occupancy_warmup=0), True, False, 1),
    'march_u': (dict(), dict(march=32, march_cap=16, march_after=0, occupancy_warmup=0), True, True, 0),
}


def new_trainer(fn, route):
    akw, tkw, fused, _, _ = ROUTES[route]
    args = fn.run_nerf.make_args(N_importance=8, N_samples=8, perturb=1.0, white_bkgd=True, use_viewdirs=True, no_reload=True, **akw)
    torch.manual_seed(3)
    ktr = fn.run_nerf.create_nerf(args)[0]
    grid = None if tkw is None else small_grid(fn)
    tr = fn.run_nerf.Trainer(ktr, 8, 8, CAM, 2.0, 6.0, occupancy=grid, **(tkw or {}))
    assert tr.fused
    tr.fused = fused
    tr.m.uniform_(-1e-3, 1e-3)      # moments that an update has to read
    tr.v.uniform_(0, 1e-6)
    torch.manual_seed(7)
    return tr, grid


@pytest.fixture(scope='module')
def rays(fn):
    g = torch.Generator().manual_seed(11)
    ro, rd = fn.run_nerf_helpers.get_rays(8, 8, CAM, fn.synthetic.pose_spherical(20.0, -30.0, 4.0)[:3, :4])
    sel = torch.randint(0, 64, (N,), generator=g)
    ro, rd = ro.reshape(-1, 3)[sel].contiguous().cuda(), rd.reshape(-1, 3)[sel].contiguous().cuda()
    return ro, rd, torch.rand(N, 3, generator=g).cuda(), torch.rand(N, generator=g).cuda()


@pytest.mark.parametrize('route', list(ROUTES))
def test_empty_step(fn, compact_on, rays, route):
    ops = fn.ops
    Nn = ops.NET_PARAMS
    ro, rd, tgt, mu = rays
    _, _, _, with_u, n_seeds = ROUTES[route]
    marched = route.startswith('march')
    # A: the step on rays, and where it leaves the host stream of seeds
    tr, _ = new_trainer(fn, route)
    kw = dict(march_u=mu) if with_u else {}
    tr.step(ro, rd, tgt, **kw)
    torch.cuda.synchronize()
    seed_a = fn.render._next_seed()
    # B: the step on no rays
    tr, grid = new_trainer(fn, route)
    assert tr.flat.numel() == 2 * Nn
    sl = slice(Nn, 2 * Nn) if marched else slice(0, 2 * Nn)
    other = slice(0, Nn)
    tr.grad.fill_(1.0)               # (what the step has to zero)
    want = [t[sl].clone() for t in (tr.flat, tr.m, tr.v)]
    ops.adam_step(want[0], torch.zeros_like(want[0]), want[1], want[2], tr.lr, 1, tr.beta1, tr.beta2, tr.eps)
    before = [t.clone() for t in (tr.flat[other], tr.m[other], tr.v[other], tr.pc[0], tr.pc[1])]
    if grid is not None:
        words, dens, steps, updates = grid.words.clone(), grid.dens.clone(), tr.occupancy_steps, grid.updates
    kw = dict(march_u=mu[:0]) if with_u else {}
    loss2, out = tr.step(ro[:0], rd[:0], tgt[:0], **kw)
    torch.cuda.synchronize()
    seed_b = fn.render._next_seed()
    assert seed_a == seed_b, 'an empty step draws the %d seed(s) of a step on rays' % n_seeds
    assert out == {} and loss2.tolist() == [0.0, 0.0] and tr.aux_losses.tolist() == [0.0] * 4 and tr.adam_t == 1
    if grid is not None:
        assert tr.occupancy_steps == steps and grid.updates == updates
        assert torch.equal(grid.words, words) and torch.equal(bits(grid.dens), bits(dens))
    assert int(torch.count_nonzero(bits(tr.grad[sl]))) == 0, 'the trained slice of the gradient'
    for name, mine, w in zip(('flat', 'm', 'v'), (tr.flat, tr.m, tr.v), want):
        assert torch.equal(bits(mine[sl]), bits(w)), name
    pairs = [(tr.pf, tr.flat[Nn:])] + ([] if marched else [(tr.pc, tr.flat[:Nn])])
    for mine, params in pairs:
        pf, pb = ops.mlp_pack(params.clone())
        assert torch.equal(bits(mine[0]), bits(pf)) and torch.equal(bits(mine[1]), bits(pb)), 'packed pair'
    if marched:
        for name, mine, was in zip(('flat', 'm', 'v', 'packed_fwd', 'packed_bwd'), (tr.flat[other], tr.m[other], tr.v[other], tr.pc[0], tr.pc[1]),
                                   before):
            assert torch.equal(bits(mine), bits(was)), 'the other network: ' + name
