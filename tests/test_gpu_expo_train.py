"""Training with an exposure table: Trainer(exposure=table).step(..., img=) on every step route, in the math modes fp32 and bf16x6.

Setting: that of tests/test_gpu_pose_train.py -- a 24 x 24 synthetic set, 67 rays over 3 images of which image 1 has none, N_samples =
N_importance = 16, perturb = 0, two freshly initialised networks with the density head lifted.  Routes: 'fused' (one call), 'grid' (one
call through an occupancy grid), 'march' (the marched step, 24 lattice depths in rows of 32 slots: no row overflows) and 'call' (call by
call, FASTNERF_FUSED_STEP=0 with the plain backward).
(1) a fresh table, lambda = 2: loss, maps, network gradients, parameters and moments after the step are bit-identical to a trainer
    without exposure= on the same route; expo_grad = (-sum G rgb, -sum G) of G = 2 (rgb - t) / (3 n) within the kernels' cap
    (tests/expo_ref.py), the empty image's row exactly zero, expo_loss = 0;
(2) a table with a in +-[0.3, 1.5], shift in +-0.1: the one-call step equals the call-by-call step bit for bit, and on the grid and marched
    routes the loss part equals the three ops called by hand on the step's own maps; trainer.expo_grad and the network gradients against
    the float64 oracle (oracle.nerf_oracle.render_rays and the formulas of include/fastnerf.h) by the project's rule: relative L2 <=
    RG.FACTOR x the float32 oracle's own error;
(3) ab after the step is ops.adam_step by hand, bit for bit; the empty image keeps its row;
(4) combined with bkgd='random' (colours injected), an alpha, lambda_dist, depth / opacity targets, and with poses= (pix supplies img):
    the one-call bits equal the call-by-call bits;
(5) behaviour: the images re-exposed by known s_i in [0.7, 1.3], o_i in +-0.05 (t_i = (c - o_i) / s_i); after 300 steps the mean error of
    log(scale_i / scale_j) over image pairs is below where it starts (all zeros); printed, recorded in profiles/exposure.md;
(6) a checkpoint round trip; (7) the refusals, with the trainer's state untouched; (8) run_nerf.train with args.optim_autoexpo steps the
    table; (9) nerfpp.CascadeTrainer: a fresh table is bit-identical to none, a non-trivial one equals the hand composition of the ops."""
import os

import numpy as np
import pytest
import torch

import expo_ref as E
import test_gpu_pose_train as PT
import test_gpu_ray_grad as RG
import test_ray_grad_cpu as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

N_S, N_I, N_RAYS = PT.N_S, PT.N_I, PT.N_RAYS
AB = torch.tensor([[0.8, 0.05], [-1.2, -0.1], [-0.4, 0.08]])
LAM = 0.3
ROUTES = ['fused', 'grid', 'march', 'call']


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
    """on_route(name) -> the Trainer keywords of that route; 'call' and 'fused-plain' pin the plain backward, so that their bits agree."""
    old = fn.render.get_compact()

    def go(route):
        G = fn.occupancy.OccupancyGrid
        if route == 'call':
            monkeypatch.setenv('FASTNERF_FUSED_STEP', '0')
            fn.render.set_compact('0')
        elif route == 'fused-plain':
            monkeypatch.delenv('FASTNERF_FUSED_STEP', raising=False)
            fn.render.set_compact('0')
        elif route == 'grid':
            return dict(occupancy=G.for_training(N=16, bound=1.5, device='cuda'), occupancy_warmup=10 ** 9)
        elif route == 'march':
            return dict(occupancy=G.for_training(N=16, bound=1.5, outside_occupied=False, device='cuda'), occupancy_warmup=10 ** 9,
                        march=24, march_cap=32)
        return {}
    yield go
    fn.render.set_compact(old)


def rays(fn):
    images, base, K = PT.data(fn)
    pix, target = PT.batch(fn)
    ro, rd = fn.ops.gen_rays_pixels(pix, base, K)
    return pix, pix[:, 0].contiguous(), target, ro, rd


def table(fn, ab=None):
    t = fn.exposure.ExposureTable(3).cuda()
    if ab is not None:
        t.ab.data.copy_(ab)
    return t


def same_outputs(out_a, out_b):
    """Every tensor both steps hand out (the call-by-call route names a few more than the one-call step)."""
    both = [k for k in out_b if k in out_a and torch.is_tensor(out_b[k])]
    assert {'rgb_map', 'disp_map', 'acc_map'} <= set(both)
    for k in both:
        assert torch.equal(out_a[k], out_b[k]), k


def same_state(a, b):
    assert torch.equal(a.grad, b.grad) and float(a.grad.abs().max()) > 0
    assert torch.equal(a.flat, b.flat) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)


def adam_by_hand(fn, tr, ab0, lr, t=1):
    ab, m, v = ab0.clone().cuda(), torch.zeros(3, 2, device='cuda'), torch.zeros(3, 2, device='cuda')
    fn.ops.adam_step(ab, tr.expo_grad, m, v, lr, t, tr.beta1, tr.beta2, tr.eps)
    return ab, m, v


@pytest.mark.parametrize('route', ROUTES)
def test_fresh_table_changes_nothing(fn, mode, on_route, route):
    """(1), and (3) on the fresh table."""
    kw = on_route(route)
    pix, img, target, ro, rd = rays(fn)
    a, _ = PT.new_trainer(fn, exposure=table(fn), lambda_autoexpo=2.0, **kw)
    b, _ = PT.new_trainer(fn, **on_route(route))
    assert a.fused == (route != 'call') and torch.equal(a.flat, b.flat)
    loss_a, out_a = a.step(ro, rd, target, img=img)
    loss_b, out_b = b.step(ro, rd, target)
    assert torch.equal(loss_a, loss_b)
    same_outputs(out_a, out_b)
    same_state(a, b)
    if route == 'march':
        assert not out_a['march_overflow'].any() and int(a.march_counts[0]) > 0
    # the table's gradient from the step's own maps
    t64 = target.double().cpu()
    G = [2.0 * (out_a[k].double().cpu() - t64) / (3.0 * N_RAYS) for k in ('rgb_map', 'rgb0') if k in out_a]
    rgbs = [out_a[k].double().cpu() for k in ('rgb_map', 'rgb0') if k in out_a]
    assert len(G) == (1 if route == 'march' else 2)
    got = a.expo_grad.double().cpu()
    idx = img.long().cpu()
    for i in (0, 2):
        rows = idx == i
        m = int(rows.sum())
        want = [-sum(float((g[rows] * x[rows]).sum()) for g, x in zip(G, rgbs)), -sum(float(g[rows].sum()) for g in G)]
        B = [sum(float((g[rows] * x[rows]).abs().sum()) for g, x in zip(G, rgbs)), sum(float(g[rows].abs().sum()) for g in G)]
        for c in (0, 1):
            assert abs(float(got[i, c]) - want[c]) <= E.bound_factor(m) * B[c], (i, c)
        assert abs(want[1]) > 0
    assert np.array_equal(a.expo_grad[1].cpu().numpy().view(np.uint32), np.zeros(2, np.uint32))
    assert a.expo_counts.tolist() == [int((idx == i).sum()) for i in range(3)] and a.expo_counts[1] == 0
    assert float(a.expo_loss) == 0.0 and b.expo_grad is None
    ab, m, v = adam_by_hand(fn, a, torch.tensor([[0.5, 0.0]]).repeat(3, 1), a.lrate)
    assert torch.equal(a.exposure.ab.data, ab) and torch.equal(a.expo_m, m) and torch.equal(a.expo_v, v)
    assert torch.equal(a.exposure.ab.data[1].cpu(), torch.tensor([0.5, 0.0]))


def oracle_grads(fn, sd_c, sd_f, ab, img, ro, rd, target, dtype):
    """d(mse(e1, t) + mse(e0, t) + LAM * mean_r(|scale - 1| + |shift|)) / d(ab, coarse parameters, fine parameters) in `dtype`."""
    sd_c = {k: v.clone().requires_grad_(True) for k, v in sd_c.items()}
    sd_f = {k: v.clone().requires_grad_(True) for k, v in sd_f.items()}
    ab = ab.to(dtype).clone().requires_grad_(True)
    rb = O.make_ray_batch(ro, rd, 2.0, 6.0).to(dtype)
    ret = O.render_rays(rb, sd_c, sd_f, N_S, N_I, white_bkgd=True)
    scale, shift = torch.abs(ab[:, 0]) + 0.5, ab[:, 1]
    idx = img.long()
    t = target.to(dtype)
    e = lambda x: (x - shift[idx][:, None]) / scale[idx][:, None]      # noqa: E731
    loss = O.img2mse(e(ret['rgb_map']), t) + O.img2mse(e(ret['rgb0']), t) + LAM * (torch.abs(scale - 1.0) + torch.abs(shift))[idx].mean()
    leaves = [ab] + list(sd_c.values()) + list(sd_f.values())
    g = torch.autograd.grad(loss, leaves, allow_unused=True)
    return [torch.zeros_like(x).double() if y is None else y.double() for x, y in zip(leaves, g)]


_ORACLE = {}


def test_table_step_against_call_by_call_and_float64(fn, mode, on_route):
    """(2) on the fused route, (3)."""
    pix, img, target, ro, rd = rays(fn)
    a, ktr = PT.new_trainer(fn, exposure=table(fn, AB), lambda_autoexpo=LAM, **on_route('fused-plain'))
    assert a.fused
    b, _ = PT.new_trainer(fn, exposure=table(fn, AB), lambda_autoexpo=LAM, **on_route('call'))
    assert not b.fused
    if 'g' not in _ORACLE:
        names = ['ab'] + ['c.' + k for k in ktr['network_fn'].state_dict()] + ['f.' + k for k in ktr['network_fine'].state_dict()]
        gs = [oracle_grads(fn, RG.state(ktr['network_fn'], dt), RG.state(ktr['network_fine'], dt), AB, img.cpu(), ro.cpu(), rd.cpu(), target.cpu(), dt)
              for dt in (torch.float64, torch.float32)]
        _ORACLE['g'] = (names, gs[0], gs[1])
    names, g64, g32 = _ORACLE['g']
    loss_a, out_a = a.step(ro, rd, target, img=img)
    loss_b, out_b = b.step(ro, rd, target, img=img)
    assert torch.equal(loss_a, loss_b)
    same_outputs(out_a, out_b)
    same_state(a, b)
    for x, y in ((a.expo_grad, b.expo_grad), (a.expo_counts, b.expo_counts), (a.expo_loss, b.expo_loss), (a.exposure.ab.data, b.exposure.ab.data),
                 (a.expo_m, b.expo_m), (a.expo_v, b.expo_v)):
        assert torch.equal(x, y)
    # the float64 oracle: the table's gradient column by column, then every parameter tensor of both networks
    got = a.expo_grad.double().cpu()
    assert (got[1] == 0).all() and (g64[0][1] == 0).all()
    for c, name in ((0, 'd_a'), (1, 'd_shift')):
        err, e32 = R.rel_l2(got[:, c], g64[0][:, c]), R.rel_l2(g32[0][:, c], g64[0][:, c])
        print('\nexpo step %-6s %-8s err %.3e  E32 %.3e  bound %.3e' % (mode, name, err, e32, RG.FACTOR * e32))
        assert err <= RG.FACTOR * e32, (name, err, e32)
    Nn = fn.ops.NET_PARAMS
    nets = ktr['network_fn'].param_grads_from(b.grad[:Nn]) + ktr['network_fine'].param_grads_from(b.grad[Nn:])
    assert len(nets) == len(names) - 1
    worst = 0.0
    for name, x, r64, r32 in zip(names[1:], nets, g64[1:], g32[1:]):
        if float(r64.norm()) == 0:
            assert float(x.abs().max()) == 0, name
            continue
        err, e32 = R.rel_l2(x.double().cpu(), r64), R.rel_l2(r32, r64)
        worst = max(worst, err / (RG.FACTOR * e32))
        assert torch.isfinite(x).all() and err <= RG.FACTOR * e32, (name, err, e32)
    print('expo step %-6s network gradients: worst err / bound %.3f' % (mode, worst))
    assert abs(float(a.expo_loss) - float((torch.abs(AB[:, 0].abs() + 0.5 - 1) + AB[:, 1].abs())[img.long().cpu()].mean())) <= 1e-6
    # (3)
    ab, m, v = adam_by_hand(fn, a, AB, a.lrate)
    assert torch.equal(a.exposure.ab.data, ab) and torch.equal(a.expo_m, m) and torch.equal(a.expo_v, v)
    assert torch.equal(a.exposure.ab.data[1].cpu(), AB[1]) and not torch.equal(a.exposure.ab.data[0].cpu(), AB[0])


@pytest.mark.parametrize('route', ['grid', 'march'])
def test_table_step_through_a_grid_equals_the_ops_by_hand(fn, mode, on_route, route):
    """(2) on the routes that have no call-by-call twin: the loss launches of the one call against apply -> mse_leafmax -> grad by hand on
    the step's own maps, bit for bit; the network's gradient differs from the step without the table."""
    pix, img, target, ro, rd = rays(fn)
    a, _ = PT.new_trainer(fn, exposure=table(fn, AB), lambda_autoexpo=LAM, **on_route(route))
    b, _ = PT.new_trainer(fn, **on_route(route))
    loss_a, out_a = a.step(ro, rd, target, img=img)
    b.step(ro, rd, target)
    ab = AB.cuda()
    two = 'rgb0' in out_a
    e1, e0 = fn.ops.expo_apply(out_a['rgb_map'].contiguous(), img, ab, rgb0=out_a['rgb0'].contiguous() if two else None)
    loss2, g1, g0 = fn.ops.mse_leafmax(e1, e0, target)
    d_ab, counts, reg = fn.ops.expo_grad(img, ab, LAM, 1.0, e1, g1, e0=e0, g0=g0)
    view = lambda name: fn.run_nerf._region(*a._last, name)      # noqa: E731
    assert torch.equal(loss_a[:2 if two else 1], loss2[:2 if two else 1])
    assert torch.equal(a.expo_grad, d_ab) and torch.equal(a.expo_counts, counts) and torch.equal(a.expo_loss, reg)
    assert torch.equal(view('expo.e1'), e1) and torch.equal(view('g_rgb'), g1)
    if two:
        assert torch.equal(view('expo.e0'), e0) and torch.equal(view('g_rgb0'), g0)
    assert not torch.equal(a.grad, b.grad) and torch.isfinite(a.grad).all()
    ab1, m, v = adam_by_hand(fn, a, AB, a.lrate)
    assert torch.equal(a.exposure.ab.data, ab1)


def test_table_step_takes_the_other_terms(fn, mode, on_route):
    """(4)."""
    images, base, K = PT.data(fn)
    pix, img, target, ro, rd = rays(fn)
    gen = torch.Generator().manual_seed(6)
    step_kw = dict(depth=(torch.rand(N_RAYS, generator=gen) * 4 + 2).cuda(), acc=torch.rand(N_RAYS, generator=gen).cuda(),
                   alpha=torch.rand(N_RAYS, generator=gen).cuda(), bkgd=torch.rand(N_RAYS, 3, generator=gen).cuda(),
                   leaf_tag=torch.stack([pix[:, 0], pix[:, 1] % 4], 1).int().contiguous(), max_leaves=4)
    kw = dict(lambda_depth=0.1, lambda_acc=0.1, lambda_dist=0.01, bkgd='random', lambda_autoexpo=LAM)
    new = lambda route, **more: PT.new_trainer(fn, exposure=table(fn, AB), kw_update={'white_bkgd': False}, **kw, **more, **on_route(route))[0]      # noqa: E731
    a, b = new('fused-plain'), new('call')
    assert a.fused and not b.fused
    ta, tb = torch.zeros(12, device='cuda', dtype=torch.int32), torch.zeros(12, device='cuda', dtype=torch.int32)
    loss_a, out_a = a.step(ro, rd, target, img=img, table=ta, **step_kw)
    loss_b, out_b = b.step(ro, rd, target, img=img, table=tb, **step_kw)
    assert torch.equal(loss_a, loss_b) and torch.equal(ta, tb) and int(ta.max()) > 0
    same_outputs(out_a, out_b)
    same_state(a, b)
    assert torch.equal(a.expo_grad, b.expo_grad) and torch.equal(a.exposure.ab.data, b.exposure.ab.data)
    assert torch.equal(a.aux_losses, b.aux_losses) and torch.equal(a.dist_losses, b.dist_losses) and float(a.expo_grad.abs().max()) > 0
    # the pose step: pix supplies img; its network and table gradients are those of the call-by-call step on the rays the poses generate
    c = new('call', poses=base)
    tc = torch.zeros(12, device='cuda', dtype=torch.int32)
    c.step(None, None, target, pix=pix, table=tc, **step_kw)
    assert torch.equal(c.grad, b.grad) and torch.equal(c.expo_grad, b.expo_grad) and torch.equal(tc, tb)
    assert torch.equal(c.exposure.ab.data, b.exposure.ab.data) and float(c.pose_grad.abs().max()) > 0


def test_table_recovers_known_exposures(fn, mode):
    """(5).  Eight views; image i is seen as t_i = (c - o_i) / s_i, so the table that explains the set has scale_i = k s_i for one k: the
    ratios scale_i / scale_j are s_i / s_j whatever the field makes of k.  The choices left to this test: lambda_autoexpo = 1e-3 (the L1
    pull has a dead zone: a weight near the colour loss's own gradient, about 1e-2 here, would pin the table at the identity), the table's
    rate 2e-3 (Adam moves a row by about its rate per step: 300 steps can cover the +-0.3 the scales are off), 1024 rays per step."""
    n_img, n_steps, n_rays = 8, 300, 1024
    images, poses, K = PT.data(fn, n_img)
    gen = torch.Generator().manual_seed(5)
    s = (0.7 + 0.6 * torch.rand(n_img, generator=gen)).cuda()
    o = ((torch.rand(n_img, generator=gen) - 0.5) * 0.1).cuda()
    seen = (images - o[:, None, None, None]) / s[:, None, None, None]
    args = fn.run_nerf.make_args(N_importance=N_I, N_samples=N_S, perturb=1., white_bkgd=True, no_reload=True)
    torch.manual_seed(0)
    ktr = fn.run_nerf.create_nerf(args, device='cuda')[0]
    t = fn.exposure.ExposureTable(n_img).cuda()
    tr = fn.run_nerf.Trainer(ktr, PT.H, PT.W, K, 2.0, 6.0, lrate=1e-3, exposure=t, lambda_autoexpo=1e-3, exposure_lrate=2e-3)

    def pair_error():
        i, j = torch.triu_indices(n_img, n_img, 1)
        ls, lt = torch.log(t.table()[0].detach().cpu().double()), torch.log(s.cpu().double())
        return float(((ls[i] - ls[j]) - (lt[i] - lt[j])).abs().mean())
    start = pair_error()
    for _ in range(n_steps):
        pix = torch.stack([torch.randint(0, n_img, (n_rays,), generator=gen), torch.randint(0, PT.H, (n_rays,), generator=gen),
                           torch.randint(0, PT.W, (n_rays,), generator=gen)], 1).int().cuda()
        p = pix.long()
        loss2, _ = tr.step(*fn.ops.gen_rays_pixels(pix, poses, K), seen[p[:, 0], p[:, 1], p[:, 2]].contiguous(), img=pix[:, 0].contiguous())
    end = pair_error()
    print('\nexposure recovery %-6s mse %.5f | mean |log(scale_i / scale_j) - truth| %.4f -> %.4f' % (mode, float(loss2[0]), start, end))
    assert torch.isfinite(t.ab).all() and end < start, (start, end)


def test_checkpoint_round_trip(fn, tmp_path):
    """(6)."""
    pix, img, target, ro, rd = rays(fn)
    a, ktr = PT.new_trainer(fn, exposure=table(fn, AB))
    for _ in range(2):
        a.step(ro, rd, target, img=img)
    args = fn.run_nerf.make_args(basedir=str(tmp_path), expname='expo')
    path = fn.run_nerf.save_checkpoint(args, 1, a, ktr, PT._NoTrees())
    ckpt = torch.load(path, map_location='cuda', weights_only=False)
    assert torch.equal(ckpt['expo_ab'], a.exposure.ab.data) and torch.equal(ckpt['expo_m'], a.expo_m) and float(a.expo_m.abs().max()) > 0
    c, _ = PT.new_trainer(fn, exposure=table(fn))
    assert c.load_expo_checkpoint(path)
    assert torch.equal(c.exposure.ab.data, a.exposure.ab.data) and torch.equal(c.expo_m, a.expo_m) and torch.equal(c.expo_v, a.expo_v)
    d, _ = PT.new_trainer(fn, exposure=table(fn))
    sd = a.state_dict()
    assert 'expo_m' in sd and 'expo_v' in sd
    d.load_state_dict(sd)
    assert torch.equal(d.expo_m, a.expo_m) and torch.equal(d.expo_v, a.expo_v) and d.expo_lr == a.expo_lr
    b, kb = PT.new_trainer(fn)
    assert 'expo_m' not in b.state_dict()
    plain = fn.run_nerf.save_checkpoint(fn.run_nerf.make_args(basedir=str(tmp_path), expname='plain'), 1, b, kb, PT._NoTrees())
    assert 'expo_ab' not in torch.load(plain, map_location='cuda', weights_only=False)
    ab = c.exposure.ab.data.clone()
    assert not c.load_expo_checkpoint(plain) and torch.equal(c.exposure.ab.data, ab) and not b.load_expo_checkpoint(path)
    e, _ = PT.new_trainer(fn, exposure=fn.exposure.ExposureTable(4).cuda())
    with pytest.raises(ValueError, match='images'):
        e.load_expo_checkpoint(path)


def test_refusals(fn, monkeypatch):
    """(7)."""
    pix, img, target, ro, rd = rays(fn)
    a, _ = PT.new_trainer(fn, exposure=table(fn, AB))
    b, _ = PT.new_trainer(fn)
    with pytest.raises(ValueError, match='img='):
        a.step(ro, rd, target)
    with pytest.raises(ValueError, match='exposure='):
        b.step(ro, rd, target, img=img)
    with pytest.raises(ValueError, match='integer'):
        a.step(ro, rd, target, img=img.float())
    with pytest.raises(ValueError, match='rows'):
        a.step(ro, rd, target, img=img[:-1].contiguous())
    with pytest.raises(ValueError, match='img='):
        a.forward_backward(ro, rd, target)
    for bad in (-1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='lambda_autoexpo'):
            PT.new_trainer(fn, exposure=table(fn), lambda_autoexpo=bad)
        a.lambda_autoexpo = bad
        with pytest.raises(ValueError, match='lambda_autoexpo'):
            a.step(ro, rd, target, img=img)
        a.lambda_autoexpo = 1.0
    monkeypatch.setattr(fn.parallel, 'world_size', lambda: 2)
    with pytest.raises(ValueError, match='data parallel'):
        PT.new_trainer(fn, exposure=table(fn))
    monkeypatch.undo()
    # the step's C entry point: a struct that is not whole is refused before the first launch
    a.step(ro, rd, target, img=img)
    ex, args = a._exp, a._sa
    lib = fn._lib.lib()
    import ctypes
    flat, ab = a.flat.clone(), a.exposure.ab.data.clone()
    for name, value in (('n_img', 0), ('lambda', -1.0), ('lambda', float('nan')), ('img', None), ('ab', None), ('e1', None), ('e0', None), ('ws', None),
                        ('d_ab', None), ('counts', None), ('loss_reg', None)):
        old = getattr(ex, name)
        setattr(ex, name, value)
        rc = lib.fastnerf_train_step_expo(ctypes.byref(args), None, None, None, ctypes.byref(ex), 15, fn._lib.stream())
        setattr(ex, name, old)
        assert rc == -1 and b'fastnerf_train_step_expo' in lib.fastnerf_last_error(), name
    torch.cuda.synchronize()
    assert torch.equal(a.flat, flat) and torch.equal(a.exposure.ab.data, ab)
    assert a.adam_t == 1 and b.adam_t == 0 and b.expo_grad is None


@pytest.mark.parametrize('compat_rng', [False, True], ids=['device_rays', 'host_rays'])
def test_train_driver_fits_the_table(fn, monkeypatch, tmp_path, compat_rng):
    """(8): run_nerf.train(args.optim_autoexpo): the warm-up and every epoch step get the image of their rows; the table is
    trainer.exposure and the checkpoint carries it."""
    imgs, poses, focal = fn.synthetic.make_dataset(n_images=3, H=32, W=32)
    seen = []
    step = fn.run_nerf.Trainer.step

    def spy(self, rays_o, rays_d, target, *a, **kw):
        seen.append((target.clone(), kw['img'].clone()))
        return step(self, rays_o, rays_d, target, *a, **kw)
    monkeypatch.setattr(fn.run_nerf.Trainer, 'step', spy)
    torch.manual_seed(0)
    np.random.seed(0)
    args = fn.run_nerf.make_args(N_importance=16, N_samples=16, perturb=1.0, white_bkgd=True, no_reload=True, N_rand=256, n_epoch=2,
                                 init_level=2, subdivide_every=1, subdivide_thres=0.05, lrate=5e-4, lrate_decay=500, optim_autoexpo=True,
                                 lambda_autoexpo=0.5, save_ckpt=True, basedir=str(tmp_path), expname='expo')
    ret = fn.run_nerf.train(imgs, poses, 32, 32, focal, args, log=lambda s: None, compat_rng=compat_rng, max_iters_per_epoch=3)
    torch.cuda.synchronize()
    trainer, hist = ret[2], ret[4]
    t = trainer.exposure
    assert isinstance(t, fn.exposure.ExposureTable) and t.n_images == 3 and trainer.lambda_autoexpo == 0.5
    assert len(hist) == 2 and all(np.isfinite(h[2]) for h in hist) and len(seen) >= 7
    images = imgs.float().cuda()
    for target, img in seen:
        assert img.dtype == torch.int32 and img.shape == (target.shape[0],) and int(img.min()) >= 0 and int(img.max()) < 3
        # the colours of the rows' own images: every target row is a pixel of the image its img names
        flat = images[img.long()].reshape(target.shape[0], -1, 3)
        assert bool((flat == target[:, None, :]).all(-1).any(-1).all())
    assert torch.isfinite(t.ab).all() and not torch.equal(t.ab.data.cpu(), torch.tensor([[0.5, 0.0]]).repeat(3, 1)) and trainer.expo_grad.shape == (3, 2)
    ckpt = torch.load(os.path.join(str(tmp_path), 'expo', '002.tar'), map_location='cuda', weights_only=False)
    assert torch.equal(ckpt['expo_ab'], t.ab.data) and torch.equal(ckpt['expo_m'], trainer.expo_m)


def test_cascade_trainer(fn):
    """(9): nerfpp.CascadeTrainer, two levels of 8 samples, 67 rays towards the unit sphere."""
    pp = fn.nerfpp
    n, S = N_RAYS, 8
    gen = torch.Generator().manual_seed(12)
    ro = (torch.randn(n, 3, generator=gen) * 0.2).cuda()
    rd = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1).cuda()
    target = torch.rand(n, 3, generator=gen).cuda()
    img = (torch.arange(n) % 2 * 2).int().cuda()      # images 0 and 2 of 3

    def trainer(**kw):
        torch.manual_seed(777)
        nets = [pp.NerfNet(device='cuda') for _ in range(2)]
        return pp.CascadeTrainer(nets, (S, S), perturb=False, **kw)
    plain = trainer()
    fresh = trainer(exposure=[fn.exposure.ExposureTable(3).cuda() for _ in range(2)], lambda_autoexpo=2.0)
    la, rgb_a = fresh.step(ro, rd, target, img=img)
    lb, rgb_b = plain.step(ro, rd, target)
    assert torch.equal(la, lb) and torch.equal(rgb_a, rgb_b)
    for x, y in zip(fresh.nets, plain.nets):
        assert torch.equal(x.flat, y.flat) and torch.equal(x.flat_grad, y.flat_grad) and float(x.flat_grad.abs().max()) > 0
    assert all(float(r) == 0.0 for r in fresh.expo_loss) and all((g[1] == 0).all() and float(g.abs().max()) > 0 for g in fresh.expo_grad)
    # a non-trivial table per level: the level's loss part is the three ops by hand on the level's colours
    tabs = [table(fn, AB), table(fn, AB.flip(0))]
    ab0 = [t.ab.data.clone() for t in tabs]
    tr = trainer(exposure=tabs, lambda_autoexpo=LAM)
    ref = trainer()
    sums, counts = torch.zeros(6, device='cuda', dtype=torch.float64), torch.zeros(6, device='cuda', dtype=torch.int32)
    tags = torch.stack([img, torch.zeros_like(img)], 1).contiguous()
    lc, rgb_c = tr.step(ro, rd, target, img=img, update=False, leaf_tag=tags, max_leaves=2, sumcount=(sums, counts))
    lr_, rgb_r = ref.step(ro, rd, target, update=False)
    # update=False: the depths of the last level hang on the first level's weights alone, so both trainers render the same colours; the
    # returned colours are the last level's, and its loss part is the three ops on them with ITS table
    assert torch.equal(rgb_c, rgb_r)
    e, _ = fn.ops.expo_apply(rgb_c.contiguous(), img, ab0[1])
    loss2, g, _ = fn.ops.mse_leafmax(e, None, target)
    d_ab, _, reg = fn.ops.expo_grad(img, ab0[1], LAM, 1.0, e, g)
    assert torch.equal(lc[1], loss2[0]) and torch.equal(tr.expo_grad[1], d_ab) and torch.equal(tr.expo_loss[1], reg)
    assert not torch.equal(lc[0], lr_[0]) and not torch.equal(tr.expo_grad[0], tr.expo_grad[1])      # one table per level
    for x, y in zip(tr.nets, ref.nets):
        assert not torch.equal(x.flat_grad, y.flat_grad) and torch.isfinite(x.flat_grad).all()
    want = torch.zeros(6, dtype=torch.float64).index_add_(0, (img.long() * 2).cpu(), (e - target).double().abs().sum(-1).cpu())
    assert torch.allclose(sums.cpu(), want, rtol=1e-6, atol=n * 2.0 ** -29)      # the leaf errors see e (a ray's term is rounded to 2^-30)
    assert torch.equal(tabs[0].ab.data, ab0[0]) and int(counts.sum()) == n      # update=False: the table stays
    tr.step(ro, rd, target, img=img)
    assert not torch.equal(tabs[0].ab.data, ab0[0]) and torch.equal(tabs[0].ab.data[1], ab0[0][1]) and tr.t == [1, 1]
    with pytest.raises(ValueError, match='img='):
        tr.step(ro, rd, target)
    with pytest.raises(ValueError, match='exposure='):
        plain.step(ro, rd, target, img=img)
    with pytest.raises(ValueError, match='per level'):
        trainer(exposure=[tabs[0]])
    # the reference's per-image parameters on the network
    net = pp.NerfNetWithAutoExpo(optim_autoexpo=True, img_names=['/data/scene/train/rgb/0001.png', '/data/scene/train/rgb/0002.png'], device='cuda')
    assert list(net.autoexpo_params.keys()) == ['train/rgb/0001-png', 'train/rgb/0002-png']      # (a parameter's name may hold no dot)
    assert 'autoexpo_params.train/rgb/0001-png' in net.state_dict() and 'module.autoexpo_params.train/rgb/0002-png' in net.reference_state_dict()
    assert torch.equal(net.state_dict()['autoexpo_params.train/rgb/0001-png'].cpu(), torch.tensor([0.5, 0.0]))
    z = pp.intersect_sphere(ro, rd)
    fg = torch.linspace(0, 1, S, device='cuda')[None, :] * z[:, None]
    bg = torch.linspace(0, 1, S, device='cuda').expand(n, S).contiguous()
    with torch.no_grad():
        known = net(ro, rd, z, fg.contiguous(), bg, img_name='/elsewhere/scene/train/rgb/0002.png')
        other = net(ro, rd, z, fg.contiguous(), bg, img_name='/data/scene/train/rgb/0003.png')
    scale, shift = known['autoexpo']
    assert float(scale) == 1.0 and float(shift.detach()) == 0.0 and 'autoexpo' not in other and torch.equal(known['rgb'], other['rgb'])
    with pytest.raises(ValueError, match='img_names'):
        pp.NerfNetWithAutoExpo(optim_autoexpo=True)
