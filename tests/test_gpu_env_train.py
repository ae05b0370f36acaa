"""Training and rendering with an environment map: Trainer(envmap=env) on every step route, render_rays / render(envmap=env), in the
math modes fp32 and bf16x6.

Setting: that of tests/test_gpu_pose_train.py -- a 24 x 24 synthetic set, 67 rays, N_samples = N_importance = 16, perturb = 0, two freshly
initialised networks, white_bkgd off -- and an 8 x 8 map of random colours.  The density heads are loosened on the batch's rays
(tests/test_gpu_aux_maps.py: steepened and centred, so that half of the coarse samples are dead): with the heads as they are born, or
lifted, every ray ends on a live sample of infinite width, acc = 1 and the background shows nowhere; loosened, the dense routes must
have at least 16 of the 67 rays with acc inside (0.02, 0.98) in either pass.  Routes: 'fused' (one call per
phase group, compacted), 'fused-plain', 'grid' and 'tighten' (through an occupancy grid), 'march', 'call' (FASTNERF_FUSED_STEP=0), 'pose'
(rays from pix) and 'expo' (with an exposure table).
(1) every route: loss, maps, network gradients, parameters and moments are those of a trainer without the map whose step gets
    bkgd=env(rays_d) injected, bit for bit; trainer.env_grad is within the bound (tests/env_ref.py) of the float64 evaluation from the
    step's own g_rgb / g_rgb0 (mse_leafmax by hand on the step's maps, the exposure rescale and the march mask included), acc maps and
    directions, and has the bits of the float32 restatement;
(2) the dense routes: trainer.env_grad agrees with plain-torch autograd of the loop
        out = render_rays(rays); rgb = out['rgb_map'] + (1 - out['acc_map'])[:, None] * env(rays[:, 3:6]); the same for rgb0
    under torch's mse, within 4 e, e the bound of (1): e for the trainer's side, 3 e for autograd's -- its chain has at most 14 fp32
    roundings per term where the kernel has 7 (torch's own mse gradient instead of the kernel's: 3 on either side of the true value; the
    rest alike), and it adds two float32 tables, |final roundings| <= u (|v1| + |v2| + |v|), which 3 e covers.  Through a grid
    render_rays refuses gradients for the networks; the table's are taken with the maps under no_grad.  The marched route the same way,
    against render_rays(march=) with the step's lattice (perturb = 0: no shift), one pass, with rows of 32 slots (none overflows) and
    of 12 (most do): an overflowed row's colour is detached, as the step zeroes its colour gradient;
(3) the marched step: a row forced to overflow (march_cap too small for some rays) contributes exact zeros -- the gradient has the
    bits of the batch without those rays;
(4) one pass (N_importance = 0);
(5) the table and its moments move by the Adam rule (tests/train_ref.py: float64 step, rounding-count bounds), three steps;
(6) a checkpoint round trip restores table and moments exactly; a resolution mismatch is refused;
(7) render_rays(envmap=) and render(envmap=) equal the bkgd= render bit for bit, in one chunk and in many, with march= and ert=;
(8) every ValueError, before any launch: the trainer's state is untouched; (9) run_nerf.train(args.envmap) steps the map."""
import os

import numpy as np
import pytest
import torch

import env_ref as E
import test_gpu_aux_maps as AM
import test_gpu_pose_train as PT
import train_ref as T
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

R_MAP = 8
N_RAYS = PT.N_RAYS
AB = torch.tensor([[0.8, 0.05], [-1.2, -0.1], [-0.4, 0.08]])
LAM = 0.3
ROUTES = ['fused', 'fused-plain', 'grid', 'tighten', 'march', 'call', 'pose', 'expo']
DENSE = ['fused', 'fused-plain', 'grid', 'tighten', 'call', 'pose', 'expo']


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

    def go(route, march_cap=32):
        G = fn.occupancy.OccupancyGrid
        if route in ('call', 'pose'):
            monkeypatch.setenv('FASTNERF_FUSED_STEP', '0')
            fn.render.set_compact('0')
        elif route == 'fused-plain':
            fn.render.set_compact('0')
        elif route == 'grid':
            return dict(occupancy=G.for_training(N=16, bound=1.5, device='cuda'), occupancy_warmup=10 ** 9)
        elif route == 'tighten':
            return dict(occupancy=G.for_training(N=16, bound=1.5, outside_occupied=False, device='cuda'), occupancy_warmup=10 ** 9, tighten=True)
        elif route == 'march':
            return dict(occupancy=G.for_training(N=16, bound=1.5, outside_occupied=False, device='cuda'), occupancy_warmup=10 ** 9,
                        march=24, march_cap=march_cap)
        elif route == 'expo':
            t = fn.exposure.ExposureTable(3).cuda()
            t.ab.data.copy_(AB)
            return dict(exposure=t, lambda_autoexpo=LAM)
        return {}
    yield go
    fn.render.set_compact(old)


def bits(t):
    t = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return t.view(np.uint32)


def rays(fn):
    images, base, K = PT.data(fn)
    pix, target = PT.batch(fn)
    ro, rd = fn.ops.gen_rays_pixels(pix, base, K)
    return pix, pix[:, 0].contiguous(), target, ro, rd


def env_map(fn, seed=0, R=R_MAP):
    m = fn.envmap.EnvMap(res=R).cuda()
    m.table.data.copy_(torch.rand(R, R, 3, generator=torch.Generator().manual_seed(40 + seed)))
    return m


_HEADS = {}


def new_trainer(fn, Ni=PT.N_I, poses=None, **kw):
    """PT.new_trainer with white_bkgd off and N_importance free: two networks (one with Ni = 0) from seed 0, their density heads loosened
    on the batch's rays (AM.loosen, through the float64 oracle once; later trainers get the same heads copied)."""
    images, base, K = PT.data(fn)
    args = fn.run_nerf.make_args(N_importance=Ni, N_samples=PT.N_S, perturb=0., white_bkgd=False, no_reload=True)
    torch.manual_seed(0)
    ktr = fn.run_nerf.create_nerf(args, device='cuda')[0]
    for k in ('network_fn', 'network_fine'):
        if ktr[k] is None:
            continue
        if k not in _HEADS:
            _, _, _, ro, rd = rays(fn)
            AM.loosen(ktr[k], O.make_ray_batch(ro.cpu(), rd.cpu(), 2.0, 6.0), PT.N_S)
            _HEADS[k] = (ktr[k].alpha_linear.weight.detach().clone(), ktr[k].alpha_linear.bias.detach().clone())
        with torch.no_grad():
            ktr[k].alpha_linear.weight.copy_(_HEADS[k][0])
            ktr[k].alpha_linear.bias.copy_(_HEADS[k][1])
    table = None if poses is None else fn.poses.PoseTable(poses).cuda()
    return fn.run_nerf.Trainer(ktr, PT.H, PT.W, K, 2.0, 6.0, poses=table, **kw), ktr


def step_grads(fn, out, target, img=None, ab=None):
    """The step's colour gradients, by hand on its own maps: (g1, acc1, g0, acc0) as numpy (g0, acc0 None with one pass)."""
    two = 'rgb0' in out
    e1, e0 = out['rgb_map'].contiguous(), out['rgb0'].contiguous() if two else None
    if img is not None:
        e1, e0 = fn.ops.expo_apply(e1, img, ab, rgb0=e0)
    _, g1, g0 = fn.ops.mse_leafmax(e1, e0, target)
    if img is not None:
        fn.ops.expo_grad(img, ab, LAM, 1.0, e1, g1, e0=e0, g0=g0)
    if 'march_overflow' in out:
        g1 = torch.where(out['march_overflow'][:, None], torch.zeros_like(g1), g1)
    c = lambda t: None if t is None else t.detach().cpu().numpy()      # noqa: E731
    return c(g1), c(out['acc_map']), c(g0), c(out['acc0']) if two else None


def same(x, y):
    """Bit for bit (a ray without a live sample has disp = 0 / 0: NaN on both sides)."""
    if x.dtype.is_floating_point:
        return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
    return torch.equal(x, y)


def same_outputs(out_a, out_b):
    both = [k for k in out_b if k in out_a and torch.is_tensor(out_b[k])]
    assert {'rgb_map', 'disp_map', 'acc_map', 'bkgd'} <= set(both)
    for k in both:
        assert same(out_a[k], out_b[k]), k


def same_state(a, b):
    assert torch.equal(a.grad, b.grad) and float(a.grad.abs().max()) > 0
    assert torch.equal(a.flat, b.flat) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)


def run_pair(fn, on_route, route, Ni=PT.N_I, march_cap=32):
    """One step of a trainer with the map and of its twin without, the map's colours injected -> (a, b, out_a, table before the step,
    the step's (g1, acc1, g0, acc0), directions)."""
    images, base, K = PT.data(fn)
    pix, img, target, ro, rd = rays(fn)
    env = env_map(fn)
    table0 = env.table.data.clone()
    colours = fn.ops.env_lookup(table0, rd.contiguous())
    kw_a, kw_b = on_route(route, march_cap), on_route(route, march_cap)
    a, _ = new_trainer(fn, Ni=Ni, envmap=env, poses=base if route == 'pose' else None, **kw_a)
    b, _ = new_trainer(fn, Ni=Ni, **kw_b)
    assert a.fused == (route not in ('call', 'pose')) and torch.equal(a.flat, b.flat) and b.env_grad is None
    step_kw = dict(img=img) if route == 'expo' else {}
    if route == 'pose':
        loss_a, out_a = a.step(None, None, target, pix=pix)
    else:
        loss_a, out_a = a.step(ro, rd, target, **step_kw)
    loss_b, out_b = b.step(ro, rd, target, bkgd=colours, **step_kw)
    assert torch.equal(loss_a, loss_b) and torch.isfinite(loss_a).all()
    same_outputs(out_a, out_b)
    same_state(a, b)
    assert torch.equal(out_a['bkgd'], colours)
    if route not in ('march', 'tighten'):      # the background shows: rays with an opacity well inside (0, 1) in every pass
        inside = [int(((out_a[k] > 0.02) & (out_a[k] < 0.98)).sum()) for k in ('acc_map', 'acc0') if k in out_a]
        assert min(inside) >= 16, inside
    if route == 'expo':
        assert torch.equal(a.expo_grad, b.expo_grad) and torch.equal(a.exposure.ab.data, b.exposure.ab.data)
    grads = step_grads(fn, out_a, target, img if route == 'expo' else None, AB.cuda() if route == 'expo' else None)
    if a.fused:      # the hand-made gradients are the step's own regions
        view = lambda name: fn.run_nerf._region(*a._last, name)      # noqa: E731
        assert np.array_equal(bits(view('g_rgb')), bits(grads[0]))
        if grads[2] is not None:
            assert np.array_equal(bits(view('g_rgb0')), bits(grads[2]))
    return a, b, out_a, table0, grads, rd.cpu().numpy()


@pytest.mark.parametrize('route', ROUTES)
def test_step_is_the_injected_colour_step(fn, mode, on_route, route):
    """(1)"""
    a, b, out, table0, (g1, a1, g0, a0), d = run_pair(fn, on_route, route)
    assert (g0 is None) == (route == 'march')
    if route == 'march':
        assert not out['march_overflow'].any() and int(a.march_counts[0]) > 0
    got = a.env_grad.cpu().numpy()
    v, e = E.grad64(d, R_MAP, g1, a1, g0, a0)
    err = np.abs(got.astype(np.float64) - v)
    print('\nenv step %-6s %-11s largest fraction of the bound reached %.3f; |grad| max %.3e' % (
        mode, route, float((err / np.maximum(e, 1e-300)).max()), float(np.abs(got).max())))
    assert (err <= e).all() and np.abs(got).max() > 0
    assert np.array_equal(bits(got), bits(E.grad32(d, R_MAP, g1, a1, g0, a0)))
    # Adam by hand from the fresh moments, bit for bit; the map moved
    tab, m, v2 = table0.clone(), torch.zeros_like(table0), torch.zeros_like(table0)
    fn.ops.adam_step(tab, a.env_grad, m, v2, a.envmap_lrate, 1, a.beta1, a.beta2, a.eps)
    assert torch.equal(a.envmap.table.data, tab) and torch.equal(a.env_m, m) and torch.equal(a.env_v, v2)
    assert not torch.equal(tab, table0)


@pytest.mark.parametrize('route', DENSE + ['march', 'march-overflow'])
def test_table_gradient_against_torch_autograd(fn, mode, on_route, route):
    """(2)"""
    march_cap = 12 if route == 'march-overflow' else 32
    marched, route = route.startswith('march'), route.split('-')[0] if route.startswith('march') else route
    a, b, out, table0, (g1, a1, g0, a0), d = run_pair(fn, on_route, route, march_cap=march_cap)
    pix, img, target, ro, rd = rays(fn)
    env = fn.envmap.EnvMap(res=R_MAP).cuda()
    env.table.data.copy_(table0)
    _, ktr = new_trainer(fn)      # (the pair's networks were stepped: fresh ones from the same seed)
    rb = fn.ops.pack_rays(ro, rd, 2.0, 6.0)
    kw = dict(N_importance=PT.N_I, network_fine=ktr['network_fine'], perturb=0.)
    if marched:
        with torch.no_grad():
            ret = fn.render.render_rays(rb, ktr['network_fn'], None, PT.N_S, network_fine=ktr['network_fine'], perturb=0., occupancy=a.occupancy,
                                        march=24, march_cap=march_cap)
        over = ret['march_overflow']
        assert torch.equal(over, out['march_overflow']) and bool(over.any()) == (march_cap == 12)
        rgb = ret['rgb_map'] + (1. - ret['acc_map'])[:, None] * env(rb[:, 3:6])
        assert torch.equal(rgb.detach(), out['rgb_map'])
        rgb = torch.where(over[:, None], rgb.detach(), rgb)      # the step zeroes an overflowed row's colour gradient; the loss stays the mean over all rays
        loss = torch.mean((rgb - target) ** 2)
    else:
        if route in ('grid', 'tighten'):
            with torch.no_grad():
                ret = fn.render.render_rays(rb, ktr['network_fn'], None, PT.N_S, occupancy=a.occupancy, tighten=route == 'tighten', **kw)
        else:
            ret = fn.render.render_rays(rb, ktr['network_fn'], None, PT.N_S, **kw)
        colours = env(rb[:, 3:6])
        rgb = ret['rgb_map'] + (1. - ret['acc_map'])[:, None] * colours
        rgb0 = ret['rgb0'] + (1. - ret['acc0'])[:, None] * colours
        assert torch.equal(rgb.detach(), out['rgb_map']) and torch.equal(rgb0.detach(), out['rgb0'])
        if route == 'expo':
            rgb, rgb0 = fn.exposure.apply(rgb, img, AB.cuda()), fn.exposure.apply(rgb0, img, AB.cuda())
        loss = torch.mean((rgb - target) ** 2) + torch.mean((rgb0 - target) ** 2)
    loss.backward()
    v, e = E.grad64(d, R_MAP, g1, a1, g0, a0)
    diff = np.abs(a.env_grad.cpu().numpy().astype(np.float64) - env.table.grad.cpu().numpy().astype(np.float64))
    print('\nenv autograd %-6s %-11s largest |trainer - autograd| %.3e, / e %.3f (tolerance 4)' % (
        mode, route, float(diff.max()), float((diff / np.maximum(e, 1e-300)).max())))
    assert (diff <= 4 * e).all()
    assert float(env.table.grad.abs().max()) > 0


def test_overflowed_rows_give_exact_zeros(fn, mode, on_route):
    """(3)"""
    a, b, out, table0, (g1, a1, g0, a0), d = run_pair(fn, on_route, 'march', march_cap=12)
    over = out['march_overflow'].cpu().numpy()
    print('\nenv march %-6s overflowed rows: %d of %d' % (mode, int(over.sum()), N_RAYS))
    assert 0 < over.sum() < N_RAYS
    assert not g1[over].any()
    keep = ~over
    assert np.array_equal(bits(a.env_grad), bits(E.grad32(d[keep], R_MAP, g1[keep], a1[keep])))
    # with their own colour gradient the overflowed rays would have been seen
    pix, img, target, ro, rd = rays(fn)
    _, g_all, _ = fn.ops.mse_leafmax(out['rgb_map'].contiguous(), None, target)
    assert not np.array_equal(bits(a.env_grad), bits(E.grad32(d, R_MAP, g_all.cpu().numpy(), a1)))


@pytest.mark.parametrize('route', ['fused', 'call'])
def test_one_pass(fn, mode, on_route, route):
    """(4)"""
    a, b, out, table0, (g1, a1, g0, a0), d = run_pair(fn, on_route, route, Ni=0)
    assert g0 is None and 'rgb0' not in out and a.net_f is None
    got = a.env_grad.cpu().numpy()
    v, e = E.grad64(d, R_MAP, g1, a1)
    assert (np.abs(got.astype(np.float64) - v) <= e).all() and np.abs(got).max() > 0
    assert np.array_equal(bits(got), bits(E.grad32(d, R_MAP, g1, a1)))


def test_adam_rule(fn, mode):
    """(5)"""
    pix, img, target, ro, rd = rays(fn)
    env = env_map(fn)
    a, _ = new_trainer(fn, envmap=env, envmap_lrate=3e-2, lrate_decay=1)
    colours_of = lambda: fn.ops.env_lookup(env.table.data, rd.contiguous())      # noqa: E731
    b, _ = new_trainer(fn, lrate_decay=1)
    for it in range(3):
        prev = [x.cpu().numpy().copy() for x in (env.table.data, a.env_m, a.env_v)]
        lr, t = a.env_lr, a.adam_t + 1
        assert abs(lr - 3e-2 * 0.1 ** (max(it - 1, 0) / 1000.)) <= 1e-12
        col = colours_of()
        a.step(ro, rd, target)
        b.step(ro, rd, target, bkgd=col)
        same_state(a, b)      # the networks' update is the injected-colour step's, step after step
        g = a.env_grad.cpu().numpy()
        got = [x.cpu().numpy() for x in (env.table.data, a.env_m, a.env_v)]
        p64, m64, v64, bp, bm, bv = T.adam_bounds(prev[0], g, prev[1], prev[2], lr, a.beta1, a.beta2, a.eps, t)
        assert (np.abs(got[0].astype(np.float64) - p64) <= bp).all(), it
        assert (np.abs(got[1].astype(np.float64) - m64) <= bm).all(), it
        assert (np.abs(got[2].astype(np.float64) - v64) <= bv).all(), it
        assert np.abs(got[0] - prev[0]).max() > 0 and np.abs(got[1]).max() > 0
    assert a.adam_t == 3 and a.env_lr < 3e-2


def test_checkpoint_round_trip(fn, tmp_path):
    """(6)"""
    pix, img, target, ro, rd = rays(fn)
    a, ktr = new_trainer(fn, envmap=env_map(fn))
    for _ in range(2):
        a.step(ro, rd, target)
    args = fn.run_nerf.make_args(basedir=str(tmp_path), expname='env')
    path = fn.run_nerf.save_checkpoint(args, 1, a, ktr, PT._NoTrees())
    ckpt = torch.load(path, map_location='cuda', weights_only=False)
    assert torch.equal(ckpt['env_table'], a.envmap.table.data) and torch.equal(ckpt['env_m'], a.env_m) and torch.equal(ckpt['env_v'], a.env_v)
    assert float(a.env_m.abs().max()) > 0
    c, _ = new_trainer(fn, envmap=env_map(fn, seed=1))
    assert c.load_env_checkpoint(path)
    assert torch.equal(c.envmap.table.data, a.envmap.table.data) and torch.equal(c.env_m, a.env_m) and torch.equal(c.env_v, a.env_v)
    d, _ = new_trainer(fn, envmap=env_map(fn, seed=2))
    sd = a.state_dict()
    assert 'env_m' in sd and 'env_v' in sd
    d.load_state_dict(sd)
    assert torch.equal(d.env_m, a.env_m) and torch.equal(d.env_v, a.env_v) and d.env_lr == a.env_lr
    b, kb = new_trainer(fn)
    assert 'env_m' not in b.state_dict()
    plain = fn.run_nerf.save_checkpoint(fn.run_nerf.make_args(basedir=str(tmp_path), expname='plain'), 1, b, kb, PT._NoTrees())
    assert 'env_table' not in torch.load(plain, map_location='cuda', weights_only=False)
    tab = c.envmap.table.data.clone()
    assert not c.load_env_checkpoint(plain) and torch.equal(c.envmap.table.data, tab) and not b.load_env_checkpoint(path)
    e, _ = new_trainer(fn, envmap=env_map(fn, R=4))
    with pytest.raises(ValueError, match='resolution'):
        e.load_env_checkpoint(path)
    # EnvMap.save / load, and a map loaded from the checkpoint itself
    p2 = os.path.join(str(tmp_path), 'map.pt')
    a.envmap.save(p2)
    for src in (p2, path):
        m = fn.envmap.EnvMap.load(src)
        assert m.res == R_MAP and torch.equal(m.table.data, a.envmap.table.data) and m.table.is_cuda


def test_rendering(fn, mode):
    """(7)"""
    images, base, K = PT.data(fn)
    pix, img, target, ro, rd = rays(fn)
    env = env_map(fn)
    _, ktr = new_trainer(fn)
    net_c, net_f = ktr['network_fn'], ktr['network_fine']
    G = fn.occupancy.OccupancyGrid
    grid = G.for_training(N=16, bound=1.5, outside_occupied=False, device='cuda')
    with torch.no_grad():
        rb = fn.ops.pack_rays(ro, rd, 2.0, 6.0)
        for kw in (dict(N_importance=PT.N_I, network_fine=net_f), dict(N_importance=PT.N_I, network_fine=net_f, ert=1e-3),
                   dict(network_fine=net_f, occupancy=grid, march=24, march_cap=32),
                   dict(network_fine=net_f, occupancy=grid, march=24, march_cap=32, ert=1e-3),
                   dict(N_importance=PT.N_I, network_fine=net_f, occupancy=grid, tighten=True)):
            x = fn.render.render_rays(rb, net_c, None, PT.N_S, envmap=env, **kw)
            y = fn.render.render_rays(rb, net_c, None, PT.N_S, bkgd=env(rb[:, 3:6]), **kw)
            assert set(x) == set(y)
            for k in x:
                assert same(x[k], y[k]), (sorted(kw), k)
            plain = fn.render.render_rays(rb, net_c, None, PT.N_S, **kw)
            assert not torch.equal(x['rgb_map'], plain['rgb_map'])
        # (these networks take view directions; an [N,8] batch is looked up with the same bits)
        assert torch.equal(env(rb[:, :8].contiguous()[:, 3:6]), env(rb[:, 3:6]))
        # render: whole images, in one chunk and in many; chunk by chunk the lookup sees the chunk's own directions
        kw = dict(network_fn=net_c, network_query_fn=None, N_samples=PT.N_S, N_importance=PT.N_I, network_fine=net_f, use_viewdirs=True,
                  ndc=False, near=2.0, far=6.0)
        one = fn.render.render(PT.H, PT.W, K, chunk=PT.H * PT.W, c2w=base[0], envmap=env, **kw)
        many = fn.render.render(PT.H, PT.W, K, chunk=100, c2w=base[0], envmap=env, **kw)
        ro_i, rd_i = fn.render.get_rays(PT.H, PT.W, K, base[0])
        ref = fn.render.render(PT.H, PT.W, K, chunk=100, c2w=base[0], bkgd=env(rd_i.reshape(-1, 3)).reshape(PT.H, PT.W, 3), **kw)
        for x, y, z in zip(one[:3], many[:3], ref[:3]):
            assert same(x, y) and same(x, z)
        rgbs, _ = fn.render.render_path([base[0].cpu().numpy()], (PT.H, PT.W, float(K[0][0])), K, 100,
                                        dict(kw, envmap=env))
        assert np.array_equal(rgbs[0], one[0].cpu().numpy())
    with pytest.raises(ValueError, match='envmap'):
        fn.render.render_rays(rb, net_c, None, PT.N_S, envmap=env, bkgd=torch.ones(3, device='cuda'))
    with pytest.raises(ValueError, match='envmap'):
        fn.render.render_rays(rb, net_c, None, PT.N_S, envmap=env, white_bkgd=True)
    with pytest.raises(ValueError, match='ndc'):
        fn.render.render(PT.H, PT.W, K, c2w=base[0], envmap=env, **dict(kw, ndc=True))


def test_refusals(fn, monkeypatch):
    """(8)"""
    pix, img, target, ro, rd = rays(fn)
    env = env_map(fn)
    a, _ = new_trainer(fn, envmap=env)
    flat, tab = a.flat.clone(), env.table.data.clone()
    colours = torch.rand(N_RAYS, 3, device='cuda')
    with pytest.raises(ValueError, match='bkgd='):
        a.step(ro, rd, target, bkgd=colours)
    with pytest.raises(ValueError, match='alpha='):
        a.step(ro, rd, target, alpha=torch.rand(N_RAYS, device='cuda'))
    with pytest.raises(ValueError, match='bkgd='):
        a.forward_backward(ro, rd, target, bkgd=colours)
    for kw, match in ((dict(bkgd='random'), 'bkgd='), (dict(bkgd=(0., 0., 0.)), 'bkgd=')):
        with pytest.raises(ValueError, match=match):
            new_trainer(fn, envmap=env, **kw)
    for name, value, match in (('white_bkgd', True, 'white_bkgd'), ('ndc', True, 'ndc')):
        setattr(a, name, value)
        with pytest.raises(ValueError, match=match):
            a.step(ro, rd, target)
        setattr(a, name, False)
    with pytest.raises(ValueError, match='is on'):
        new_trainer(fn, envmap=fn.envmap.EnvMap(res=4))      # a table on the host
    monkeypatch.setattr(fn.parallel, 'world_size', lambda: 2)
    with pytest.raises(ValueError, match='data parallel'):
        new_trainer(fn, envmap=env)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert a.adam_t == 0 and torch.equal(a.flat, flat) and torch.equal(env.table.data, tab) and not a.env_grad.any()
    # an empty batch: a zero gradient, and the update Adam makes of it
    a.step(ro[:0], rd[:0], target[:0])
    assert not a.env_grad.any() and torch.equal(env.table.data, tab) and a.adam_t == 1


def test_train_driver_fits_the_map(fn, tmp_path):
    """(9): run_nerf.train(args.envmap): the map is trainer.envmap, the test-time kwargs render over it, the checkpoint carries it."""
    imgs, poses, focal = fn.synthetic.make_dataset(n_images=3, H=32, W=32)
    torch.manual_seed(0)
    np.random.seed(0)
    args = fn.run_nerf.make_args(N_importance=16, N_samples=16, perturb=1.0, white_bkgd=False, no_reload=True, N_rand=256, n_epoch=2,
                                 init_level=2, subdivide_every=1, subdivide_thres=0.05, lrate=5e-4, lrate_decay=500, envmap=True,
                                 envmap_res=8, envmap_lrate=5e-3, save_ckpt=True, basedir=str(tmp_path), expname='env')
    ret = fn.run_nerf.train(imgs, poses, 32, 32, focal, args, log=lambda s: None, max_iters_per_epoch=3)
    torch.cuda.synchronize()
    kw_test, trainer, hist = ret[1], ret[2], ret[4]
    env = trainer.envmap
    assert isinstance(env, fn.envmap.EnvMap) and env.res == 8 and trainer.envmap_lrate == 5e-3 and kw_test['envmap'] is env
    assert len(hist) == 2 and all(np.isfinite(h[2]) for h in hist)
    assert torch.isfinite(env.table).all() and not torch.equal(env.table.data, torch.full_like(env.table.data, 0.5))
    ckpt = torch.load(os.path.join(str(tmp_path), 'env', '002.tar'), map_location='cuda', weights_only=False)
    assert torch.equal(ckpt['env_table'], env.table.data) and torch.equal(ckpt['env_m'], trainer.env_m)
