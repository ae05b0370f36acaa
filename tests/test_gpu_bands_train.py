"""Training with band weights: Trainer(bands=BandSchedule) on every step route, in the math modes fp32 and bf16x6.

Setting: that of tests/test_gpu_env_train.py (67 rays of a 24 x 24 synthetic set, N_samples = N_importance = 16, two freshly initialised
networks with loosened density heads), with t_rand / u / march_u injected.  Routes: 'fused' (compacted), 'fused-plain', 'grid', 'march',
'call' (FASTNERF_FUSED_STEP=0) and 'pose' (rays from pix).
(3) the scaled-network identity per route: trainer A has the parameters theta and constant weights w, trainer B no bands and the
    parameters band_apply(theta); every output map and the loss are bitwise equal, and A's parameter gradient is band_grad of B's, bitwise;
(4) the update: after one step the parameters and moments are within tests/train_ref.py's Adam bounds of the float64 step on the
    parameter gradient (and have the bits of ops.adam_step by hand); net.flat == band_apply(parameters) and net.packed(refresh=False)
    == a fresh pack of net.flat, bitwise;
(5) a closed band is neither read nor moved: w = 0 on the point bands >= 4, those parameter columns overwritten with 1e30: outputs bitwise
    those of the run without the overwrite over 5 steps, the columns bit-unchanged, their moments exactly 0;
(6) w = 1: an all-ones schedule, and all-ones weights set by hand (which do take the banded update), reproduce the plain trainer bit for
    bit over 3 steps; past the end of a ramp the trainer is the plain trainer: a fresh plain trainer loaded from its state takes bitwise
    identical steps, and the step arguments point at the parameters again;
(8) a mid-ramp checkpoint round trip (save_checkpoint; networks, optimizer, schedule) continues bitwise; a post-ramp checkpoint loads into a
    plain create_nerf pair with strict=True;
(9) every ValueError, before any launch; run_nerf.train(args.band_window) ramps."""
import os

import numpy as np
import pytest
import torch

import bands_ref as B
import test_gpu_env_train as ET
import test_gpu_pose_train as PT
import train_ref as T

pytestmark = pytest.mark.gpu

ROUTES = ['fused', 'fused-plain', 'grid', 'march', 'call', 'pose']


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


@pytest.fixture(params=['fp32', 'bf16x6'])
def mode(request, fn):
    old = fn.ops.get_math()
    fn.ops.set_math(request.param)
    yield request.param
    fn.ops.set_math(old)


@pytest.fixture
def on_route(fn, monkeypatch):
    """on_route(name) -> the Trainer keywords of that route ('call', 'pose' and 'fused-plain' pin the plain backward)."""
    old = fn.render.get_compact()

    def go(route):
        G = fn.occupancy.OccupancyGrid
        if route in ('call', 'pose'):
            monkeypatch.setenv('FASTNERF_FUSED_STEP', '0')
            fn.render.set_compact('0')
        elif route == 'fused-plain':
            fn.render.set_compact('0')
        elif route == 'grid':
            return dict(occupancy=G.for_training(N=16, bound=1.5, device='cuda'), occupancy_warmup=10 ** 9)
        elif route == 'march':
            return dict(occupancy=G.for_training(N=16, bound=1.5, outside_occupied=False, device='cuda'), occupancy_warmup=10 ** 9,
                        march=24, march_cap=32)
        return {}
    yield go
    fn.render.set_compact(old)


def ramp_weights(closed_from=10):
    """Mid-ramp column weights (host, fp32); the point bands >= closed_from at 0."""
    per = [1.0, 0.9, 0.75, 0.6, 0.5, 0.35, 0.25, 0.125, 0.05, 0.0]
    per = [w if k < closed_from else 0.0 for k, w in enumerate(per)]
    return torch.from_numpy(B.columns_from_bands(per)), torch.from_numpy(B.columns_from_bands([1.0, 0.7, 0.3, 0.0]))


def randoms(n=ET.N_RAYS):
    g = torch.Generator().manual_seed(21)
    return dict(t_rand=torch.rand(n, PT.N_S, generator=g).cuda(), u=torch.rand(n, PT.N_I, generator=g).cuda()), \
        dict(march_u=torch.rand(n, generator=g).cuda())


def step(fn, tr, route, **kw):
    pix, img, target, ro, rd = ET.rays(fn)
    dense, marched = randoms()
    if route == 'pose':
        return tr.step(None, None, target, pix=pix, **dense, **kw)
    return tr.step(ro, rd, target, **(marched if route == 'march' else dense), **kw)


def nets_of(tr):
    return [tr.net_c, tr.net_f]


def apply_both(fn, w, flat):
    N = fn.ops.NET_PARAMS
    return torch.cat([fn.ops.band_apply(w[0].cuda(), w[1].cuda(), flat[i * N:(i + 1) * N].contiguous()) for i in range(flat.numel() // N)])


def grad_both(fn, w, grad):
    N = fn.ops.NET_PARAMS
    return torch.cat([fn.ops.band_grad(w[0].cuda(), w[1].cuda(), grad[i * N:(i + 1) * N].clone()) for i in range(grad.numel() // N)])


def same_outputs(out_a, out_b, need=('rgb_map', 'disp_map', 'acc_map', 'depth_map')):
    both = [k for k in out_b if k in out_a and torch.is_tensor(out_b[k])]
    assert set(need) <= set(both), both
    for k in both:
        assert ET.same(out_a[k], out_b[k]), k


def trainer(fn, route, on_route, **kw):
    base = PT.data(fn)[1] if route == 'pose' else None
    return ET.new_trainer(fn, poses=base, **on_route(route), **kw)


@pytest.mark.parametrize('route', ROUTES)
def test_scaled_network_identity(fn, mode, on_route, route):
    """(3)"""
    w = ramp_weights()
    a, _ = trainer(fn, route, on_route, bands=fn.bands.BandSchedule.constant(*w))
    b, _ = trainer(fn, route, on_route)
    theta = a.flat.clone()
    assert torch.equal(theta, b.flat) and a.fused == (route not in ('call', 'pose')) and a._banded() and not b._banded()
    b.flat.copy_(apply_both(fn, w, theta))
    b.repack()
    assert not torch.equal(b.flat, theta)
    for net_a, net_b in zip(nets_of(a), nets_of(b)):
        assert torch.equal(net_a.flat, net_b.flat) and net_a.flat.data_ptr() != net_a.param_flat.data_ptr()
    assert a.net_c.flat.data_ptr() + 4 * fn.ops.NET_PARAMS == a.net_f.flat.data_ptr()       # one effective buffer, one gradient buffer
    assert a.net_c.flat_grad.data_ptr() + 4 * fn.ops.NET_PARAMS == a.net_f.flat_grad.data_ptr()
    loss_a, out_a = step(fn, a, route)
    loss_b, out_b = step(fn, b, route)
    assert torch.equal(loss_a, loss_b) and torch.isfinite(loss_a).all() and float(loss_a[0]) > 0
    same_outputs(out_a, out_b)
    want = grad_both(fn, w, b.grad)
    assert torch.equal(a.grad, want) and float(want.abs().max()) > 0 and not torch.equal(a.grad, b.grad)
    if route == 'march':
        assert int(a.march_counts[0]) > 0 and torch.equal(a.march_counts, b.march_counts)
    if a.fused:      # the step ran on the effective buffers, without the update phase
        sa = a._ma[0] if route == 'march' else a._sa
        assert sa.params == a.net_c.flat.data_ptr() != a.flat.data_ptr() and sa.grads == a.net_c.flat_grad.data_ptr()
    # the parameters moved, and the kernels' network is the weighted one of the parameters as they are now
    assert not torch.equal(a.flat, theta)
    assert torch.equal(torch.cat([n.flat for n in nets_of(a)]), apply_both(fn, w, a.flat))


@pytest.mark.parametrize('route', ['fused', 'march', 'call'])
def test_update_rule(fn, mode, on_route, route):
    """(4)"""
    w = ramp_weights()
    a, _ = trainer(fn, route, on_route, bands=fn.bands.BandSchedule.constant(*w))
    p0, lr = a.flat.clone(), a.lr
    step(fn, a, route)
    N = fn.ops.NET_PARAMS
    sl = slice(N, 2 * N) if route == 'march' else slice(0, 2 * N)      # the marched step trains the fine network alone
    g = a.grad[sl]
    assert float(g.abs().max()) > 0
    got = [x[sl].cpu().numpy() for x in (a.flat, a.m, a.v)]
    zeros = np.zeros(sl.stop - sl.start, np.float32)
    p64, m64, v64, bp, bm, bv = T.adam_bounds(p0[sl].cpu().numpy(), g.cpu().numpy(), zeros, zeros, lr, a.beta1, a.beta2, a.eps, 1)
    assert (np.abs(got[0].astype(np.float64) - p64) <= bp).all()
    assert (np.abs(got[1].astype(np.float64) - m64) <= bm).all()
    assert (np.abs(got[2].astype(np.float64) - v64) <= bv).all()
    p, m, v = p0[sl].clone(), torch.zeros_like(g), torch.zeros_like(g)
    fn.ops.adam_step(p, g.clone(), m, v, lr, 1, a.beta1, a.beta2, a.eps)
    assert torch.equal(a.flat[sl], p) and torch.equal(a.m[sl], m) and torch.equal(a.v[sl], v) and not torch.equal(p, p0[sl])
    if route == 'march':      # the other network, its moments: untouched
        assert torch.equal(a.flat[:N], p0[:N]) and not a.m[:N].any() and not a.v[:N].any()
    eff = apply_both(fn, w, a.flat)
    for i, net in enumerate(nets_of(a)):
        assert torch.equal(net.flat, eff[i * N:(i + 1) * N])
        fresh = fn.ops.mlp_pack(net.flat)
        kept = net.packed(refresh=False)
        assert torch.equal(kept[0], fresh[0]) and torch.equal(kept[1], fresh[1])
    assert a.pc is a.net_c.packed(refresh=False) and a.pf is a.net_f.packed(refresh=False)


def test_closed_band_is_neither_read_nor_moved(fn, mode, on_route):
    """(5)"""
    w = ramp_weights(closed_from=4)
    index, which = B.column_map(0)
    closed = torch.from_numpy((which == 1) & (index >= 3 + 6 * 4)).cuda()
    assert int(closed.sum()) == 2 * 256 * 36
    a, _ = trainer(fn, 'fused', on_route, bands=fn.bands.BandSchedule.constant(*w))
    c, _ = trainer(fn, 'fused', on_route, bands=fn.bands.BandSchedule.constant(*w))
    N = fn.ops.NET_PARAMS
    both = torch.cat([closed, closed])
    c.flat[both] = 1e30
    c.repack()
    for it in range(5):
        loss_a, out_a = step(fn, a, 'fused')
        loss_c, out_c = step(fn, c, 'fused')
        assert torch.equal(loss_a, loss_c) and torch.isfinite(loss_c).all(), it
        same_outputs(out_a, out_c)
        assert torch.equal(a.grad, c.grad) and not c.grad[both].any()
    assert bool((c.flat[both] == 1e30).all()) and ET.same(c.flat[both], torch.full_like(c.flat[both], 1e30))
    assert not c.m[both].any() and not c.v[both].any() and not a.m[both].any()
    assert torch.equal(a.flat[~both], c.flat[~both]) and torch.equal(a.m, c.m) and torch.equal(a.v, c.v)
    assert float(c.m[~both].abs().max()) > 0
    for net in nets_of(c):      # and the kernels' network holds zeros there
        assert not net.flat[closed].any()


def same_trainers(a, b):
    assert torch.equal(a.flat, b.flat) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and torch.equal(a.grad, b.grad)


@pytest.mark.parametrize('route', ['fused', 'march', 'call'])
def test_all_ones_is_the_plain_trainer(fn, mode, on_route, route):
    """(6), first half"""
    ones = (torch.ones(63), torch.ones(27))
    a, _ = trainer(fn, route, on_route, bands=fn.bands.BandSchedule.constant(*ones))
    h, _ = trainer(fn, route, on_route)
    for net in nets_of(h):      # weights of 1 set by hand: the banded update, on numbers that are the plain trainer's
        net.set_bands(*ones)
    h.repack()
    b, _ = trainer(fn, route, on_route)
    assert not a._banded() and h._banded() and not b._banded()
    for it in range(3):
        outs = [step(fn, t, route) for t in (a, h, b)]
        for loss, out in outs[:2]:
            assert torch.equal(loss, outs[2][0]), it
            same_outputs(out, outs[2][1])
        same_trainers(a, b)
        same_trainers(h, b)
        assert a.lr == b.lr == h.lr
    assert h._banded() and float(b.m.abs().max()) > 0


@pytest.mark.parametrize('route', ['fused', 'march'])
def test_end_of_the_ramp(fn, mode, on_route, route):
    """(6), second half: a ramp over the steps 0 .. T = 2"""
    T_END = 2
    a, _ = trainer(fn, route, on_route, bands=fn.bands.BandSchedule('cosine', 0, T_END))
    assert a._banded() and not a.net_c.flat[:256 * 63].view(256, 63)[:, 3:].any()       # step 0: every band closed
    before = a.flat.clone()
    for it in range(T_END):
        assert a._banded()
        step(fn, a, route)
    assert not a._banded() and not torch.equal(a.flat, before)
    for net in nets_of(a):
        assert net.flat.data_ptr() == net.param_flat.data_ptr() and net.flat_grad.data_ptr() == net.param_grad.data_ptr()
    p, _ = trainer(fn, route, on_route)
    p.flat.copy_(a.flat)
    p.load_state_dict(a.state_dict())
    p.repack()
    if route == 'march':
        p.occupancy_steps = a.occupancy_steps
    for it in range(2):
        (loss_a, out_a), (loss_p, out_p) = step(fn, a, route), step(fn, p, route)
        assert torch.equal(loss_a, loss_p), it
        same_outputs(out_a, out_p)
        assert torch.equal(a.flat, p.flat) and torch.equal(a.m, p.m) and torch.equal(a.v, p.v)
        sa = a._ma[0] if route == 'march' else a._sa
        assert sa.params == a.flat.data_ptr() and sa.grads == a.grad.data_ptr()            # the one-call route, on the parameters
    assert a.adam_t == T_END + 2 and a.bands.done(a.adam_t)


def test_checkpoint_round_trip(fn, tmp_path):
    """(8)"""
    sched = lambda: fn.bands.BandSchedule('linear', 0, 5, view=False)      # noqa: E731
    a, ktr = ET.new_trainer(fn, bands=sched())
    for _ in range(2):
        step(fn, a, 'fused')
    assert a._banded()
    args = fn.run_nerf.make_args(basedir=str(tmp_path), expname='bands')
    path = fn.run_nerf.save_checkpoint(args, 1, a, ktr, PT._NoTrees())
    ckpt = torch.load(path, map_location='cuda', weights_only=False)
    assert ckpt['band_schedule'] == {'window': 'linear', 'start': 0.0, 'end': 5.0, 'view': False}
    assert all(torch.equal(x.cpu(), y) for x, y in zip(ckpt['band_weights'], a.bands.weights(2)))
    # the state dicts are the parameters, not the effective networks
    N = fn.ops.NET_PARAMS
    sd = fn.flat_params.strip_prefix(ckpt['network_fn_state_dict'])
    assert torch.equal(torch.cat([sd[name].reshape(-1) for name, _, _ in fn.model.param_slices()]), a.flat[:N])
    assert not torch.equal(a.net_c.flat, a.flat[:N])
    for adopt in (False, True):      # a trainer made with the schedule, and one that takes it from the checkpoint
        c, kc = ET.new_trainer(fn, **({} if adopt else dict(bands=sched())))
        kc['network_fn'].load_state_dict(ckpt['network_fn_state_dict'])
        kc['network_fine'].load_state_dict(ckpt['network_fine_state_dict'])
        c.load_torch_optimizer(ckpt['optimizer_state_dict'])
        c.global_iter = ckpt['global_iter']
        if adopt:
            assert c.load_band_checkpoint(path) and c.bands.settings() == a.bands.settings()
        else:
            c.repack()
        assert c.adam_t == 2 and c._banded() and torch.equal(c.flat, a.flat) and torch.equal(c.m, a.m)
        assert torch.equal(c.net_c.flat, a.net_c.flat) and torch.equal(c.net_f.flat, a.net_f.flat)
        twin, _ = ET.new_trainer(fn, bands=sched())      # a's own continuation, from a copy of its state
        twin.flat.copy_(a.flat)
        twin.load_state_dict(a.state_dict())
        (loss_c, out_c), (loss_t, out_t) = step(fn, c, 'fused'), step(fn, twin, 'fused')
        assert torch.equal(loss_c, loss_t)
        same_outputs(out_c, out_t)
        same_trainers(c, twin)
    for _ in range(4):      # past the ramp: a plain checkpoint of the reference's format
        step(fn, a, 'fused')
    assert not a._banded() and a.adam_t == 6
    post = fn.run_nerf.save_checkpoint(fn.run_nerf.make_args(basedir=str(tmp_path), expname='post'), 2, a, ktr, PT._NoTrees())
    ck2 = torch.load(post, map_location='cuda', weights_only=False)
    args = fn.run_nerf.make_args(N_importance=PT.N_I, N_samples=PT.N_S, no_reload=True)
    plain = fn.run_nerf.create_nerf(args, device='cuda')[0]
    plain['network_fn'].load_state_dict(ck2['network_fn_state_dict'], strict=True)
    plain['network_fine'].load_state_dict(ck2['network_fine_state_dict'], strict=True)
    assert torch.equal(plain['network_fn']._flat_all, a.flat)
    b, _ = ET.new_trainer(fn)
    assert not b.load_band_checkpoint(fn.run_nerf.save_checkpoint(fn.run_nerf.make_args(basedir=str(tmp_path), expname='plain'), 1, b,
                                                                  ET.new_trainer(fn)[1], PT._NoTrees()))


def test_refusals(fn, monkeypatch):
    """(9)"""
    sched = fn.bands.BandSchedule('cosine', 0, 100)
    monkeypatch.setattr(fn.parallel, 'world_size', lambda: 2)
    with pytest.raises(ValueError, match='data parallel'):
        ET.new_trainer(fn, bands=sched)
    monkeypatch.undo()
    images, base, K = PT.data(fn)
    args = fn.run_nerf.make_args(N_importance=PT.N_I, N_samples=PT.N_S, perturb=0., no_reload=True)
    ktr = fn.run_nerf.create_nerf(args, device='cuda')[0]
    flat = ktr['network_fn']._flat_all.clone()
    shared = dict(ktr, network_fine=ktr['network_fn'])
    with pytest.raises(ValueError, match='shared'):
        fn.run_nerf.Trainer(shared, PT.H, PT.W, K, 2.0, 6.0, bands=sched)
    assert ktr['network_fn']._bands is None and torch.equal(ktr['network_fn']._flat_all, flat)
    noview = fn.run_nerf.create_nerf(fn.run_nerf.make_args(N_importance=PT.N_I, N_samples=PT.N_S, use_viewdirs=False, no_reload=True),
                                     device='cuda')[0]
    with pytest.raises(ValueError, match='view directions'):
        fn.run_nerf.Trainer(noview, PT.H, PT.W, K, 2.0, 6.0, bands=sched)
    with pytest.raises(ValueError, match='nerf\\+\\+'):
        fn.nerfpp.CascadeTrainer([], bands=sched)
    # band weights on one of the two networks only
    b, kb = ET.new_trainer(fn)
    kb['network_fn'].set_bands(*ramp_weights())
    pix, img, target, ro, rd = ET.rays(fn)
    state = b.flat.clone()
    with pytest.raises(ValueError, match='one of the two'):
        b.step(ro, rd, target)
    torch.cuda.synchronize()
    assert b.adam_t == 0 and torch.equal(b.flat, state) and not b.grad.any()
    # a trainer's schedule made data parallel later is refused on the step, untouched
    a, _ = ET.new_trainer(fn, bands=sched)
    state = a.flat.clone()
    monkeypatch.setattr(a, 'world', 2)
    with pytest.raises(ValueError, match='data parallel'):
        a.step(ro, rd, target)
    assert a.adam_t == 0 and torch.equal(a.flat, state)


def test_train_driver_ramps(fn, tmp_path):
    """(9): run_nerf.train(args.band_window): the trainer carries the schedule, is mid-ramp after the run, and the checkpoint holds it."""
    imgs, poses, focal = fn.synthetic.make_dataset(n_images=3, H=32, W=32)
    torch.manual_seed(0)
    np.random.seed(0)
    args = fn.run_nerf.make_args(N_importance=16, N_samples=16, perturb=1.0, white_bkgd=False, no_reload=True, N_rand=256, n_epoch=2,
                                 init_level=2, subdivide_every=1, subdivide_thres=0.05, lrate=5e-4, lrate_decay=500, band_window='cosine',
                                 band_start=2, band_end=40, band_view=False, save_ckpt=True, basedir=str(tmp_path), expname='bands')
    ret = fn.run_nerf.train(imgs, poses, 32, 32, focal, args, log=lambda s: None, max_iters_per_epoch=3)
    torch.cuda.synchronize()
    tr, hist = ret[2], ret[4]
    assert isinstance(tr.bands, fn.bands.BandSchedule) and tr.bands.settings() == {'window': 'cosine', 'start': 2.0, 'end': 40.0, 'view': False}
    assert tr.adam_t == 9 and tr._banded() and len(hist) == 2 and all(np.isfinite(h[2]) for h in hist)
    w = tr.bands.weights(tr.adam_t)
    assert all(torch.equal(x.cpu(), y) for x, y in zip(tr.net_c._bands, w)) and 0 < float(w[0][3]) and float(w[0][-1]) == 0
    ckpt = torch.load(os.path.join(str(tmp_path), 'bands', '002.tar'), map_location='cuda', weights_only=False)
    assert ckpt['band_schedule'] == tr.bands.settings() and torch.equal(ckpt['band_weights'][0].cpu(), w[0])
