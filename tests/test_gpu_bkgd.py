"""Per-ray background colours on the GPU (include/fastnerf.h, "per-ray background colours"): the two kernels of csrc/bkgd.hip bit for
bit against tests/bkgd_ref.py, white as a special case, the fused / phased / call-by-call / marched steps of run_nerf.Trainer(bkgd=),
their gradient against float64 autograd of the oracle, and render_rays(bkgd=) / render(bkgd=).

Bounds.  Against float64: relative L2 per parameter tensor (per column group for rays) <= 16 x E32, E32 being the same metric for torch's
float32 CPU autograd of the same oracle -- the project's rule (FACTOR of tests/test_gpu_aux_maps.py / tests/test_gpu_ray_grad.py), for
the math modes of fp32 width.  What the reference must give for that check to notice a dropped, negated or pass-swapped g_acc is
asserted first, on the reference alone: `share`, the part of a tensor's float64 gradient that travels through the blend's acc, exceeds
16 x E32 on each of the 36 tensors of the density path.  Compacted against saving: the 3e-6 of the largest gradient of
tests/test_gpu_compact.py.  Everything else is bit for bit.  Every figure is printed before it is asserted (pytest -s; recorded in
profiles/bkgd.md)."""
import os

import numpy as np
import pytest
import torch

import bkgd_ref as B
import march_numpy as M
import test_gpu_aux_maps as AM
import test_gpu_march_train as MTG
import test_gpu_ray_grad as RG
import test_ray_grad_cpu as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

FACTOR = AM.FACTOR
F32 = np.float32
SEED_NETS = 3      # torch seed of the networks of sections 3 to 5 (create_nerf's init)


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


@pytest.fixture
def math3(fn):
    old = fn.ops.get_math()
    yield fn.ops.set_math
    fn.ops.set_math(old)


@pytest.fixture
def compact(fn):
    old = fn.render.get_compact()
    yield fn.render.set_compact
    fn.render.set_compact(old)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------------------
def kernel_inputs(n, seed):
    rs = np.random.RandomState(seed)
    d = dict(rgb1=rs.rand(n, 3), acc1=rs.rand(n), rgb0=rs.rand(n, 3), acc0=rs.rand(n), target=rs.rand(n, 3), bkgd=rs.rand(n, 3),
             alpha=rs.rand(n), g1=rs.randn(n, 3), g0=rs.randn(n, 3), add1=rs.randn(n), add0=rs.randn(n))
    d = {k: v.astype(F32) for k, v in d.items()}
    d['alpha'][::3] = 0.
    d['alpha'][1::5] = 1.
    d['acc1'][::4] = 0.
    d['acc0'][::7] = 1.
    return d


@pytest.mark.parametrize('n', [1, 255, 257, 1025])
@pytest.mark.parametrize('two', [False, True], ids=['one_pass', 'two_passes'])
@pytest.mark.parametrize('with_alpha', [False, True], ids=['no_alpha', 'alpha'])
def test_kernels_bit_for_bit(fn, n, two, with_alpha):
    d = kernel_inputs(n, 100 + n)
    cu = lambda k: torch.from_numpy(d[k]).cuda()      # noqa: E731
    alpha = d['alpha'] if with_alpha else None
    assert not with_alpha or ((alpha == 0).any() and (alpha == 1).any() and ((alpha > 0) & (alpha < 1)).any()) or n == 1
    seen = []
    for src in (dict(bkgd=d['bkgd']), dict(seed=7), dict(seed=2 ** 40 + 3)):
        want = B.blend(d['rgb1'], d['acc1'], d['target'], alpha=alpha, rgb0=d['rgb0'] if two else None, acc0=d['acc0'] if two else None, **src)

        def call():
            rgb1, rgb0 = cu('rgb1'), (cu('rgb0') if two else None)
            tout, used = fn.ops.bkgd_blend(rgb1, cu('acc1'), cu('target'), bkgd=None if 'bkgd' not in src else cu('bkgd'),
                                           seed=src.get('seed', 0), alpha=None if alpha is None else cu('alpha'), rgb0=rgb0,
                                           acc0=cu('acc0') if two else None)
            return rgb1, rgb0, tout, used
        got, again = call(), call()
        torch.cuda.synchronize()
        for name, g, g2, w in zip(('rgb1', 'rgb0', 'target_out', 'bkgd_used'), got, again, want):
            if w is None:
                assert g is None
                continue
            assert np.array_equal(g.cpu().numpy().view(np.int32), w.view(np.int32)), (list(src), name)
            assert same(g, g2), 'two calls, the same bits'
        if 'seed' in src:
            assert np.array_equal(want[3], B.draw(n, src['seed'])) and want[3].min() >= 0 and want[3].max() < 1
        seen.append(want[3])
        if not with_alpha:
            assert np.array_equal(got[2].cpu().numpy().view(np.int32), d['target'].view(np.int32)), 'no alpha: the target keeps its bits'
    assert not np.array_equal(seen[1], seen[2]), 'two seeds, two sets of colours'
    # the gradient rows, with and without the rows of another term
    for add in (False, True):
        a1, a0 = (d['add1'], d['add0']) if add else (None, None)
        want = B.grad(d['bkgd'], d['g1'], d['g0'] if two else None, a1, a0 if two else None)
        got = fn.ops.bkgd_grad(cu('bkgd'), cu('g1'), cu('g0') if two else None, add=cu('add1') if add else None,
                               add0=cu('add0') if (add and two) else None)
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if w is not None:
                assert np.array_equal(g.cpu().numpy().view(np.int32), w.view(np.int32)), add
    with pytest.raises(RuntimeError, match='exactly one'):
        fn.ops.bkgd_blend(cu('rgb1'), cu('acc1'), cu('target'))
    with pytest.raises(RuntimeError, match='exactly one'):
        fn.ops.bkgd_blend(cu('rgb1'), cu('acc1'), cu('target'), bkgd=cu('bkgd'), seed=3)


# ---- trainers of sections 2 to 5: tests/test_gpu_aux_maps.py's shapes (64 rays of the 32 x 32 camera, 16 + 32 samples) --------------------
def make_trainer(fn, loose_on=None, seed=SEED_NETS, white=False, Ni=32, **kw):
    """AM.trainer with the seed of the networks, white_bkgd and N_importance (0: one pass, one network) as parameters."""
    torch.manual_seed(seed)
    args = fn.run_nerf.make_args(N_importance=Ni, N_samples=16, perturb=1.0, white_bkgd=white, no_reload=True, lrate=5e-4, lrate_decay=500)
    ktr = fn.run_nerf.create_nerf(args)[0]
    with torch.no_grad():
        for net in (ktr['network_fn'], ktr['network_fine'])[:2 if Ni else 1]:
            if loose_on is None:
                net.alpha_linear.bias.add_(0.3)
            else:
                AM.loosen(net, loose_on, 16)
    K = np.array([[40.0, 0, 16.0], [0, 40.0, 16.0], [0, 0, 1]])
    return fn.run_nerf.Trainer(ktr, 32, 32, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500, **kw)


def step_extras(n, seed):
    """(alpha with exact 0 / 1 and values in between, colours) for a batch of n rays."""
    gen = torch.Generator().manual_seed(seed)
    alpha = torch.rand(n, generator=gen)
    alpha[::3] = 0.
    alpha[1::3] = 1.
    return alpha.cuda(), torch.rand(n, 3, generator=gen).cuda()


def injected(n=64):
    return (torch.rand(n, 16, generator=torch.Generator().manual_seed(1)).cuda(), torch.rand(n, 32, generator=torch.Generator().manual_seed(2)).cuda())


# ---- 2. white is a special case ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['fp32', 'bf16x6'])
def test_white_is_bkgd_ones(fn, math3, compact, mode):
    math3(mode)
    compact('0')
    (b, _), = AM.batches(fn, 1)
    t_rand, u = injected()
    res = {}
    for name, kw, white in (('ones', dict(bkgd=(1., 1., 1.)), False), ('white', {}, True)):
        tr = make_trainer(fn, white=white, **kw)
        loss2, out = tr.step(*b, t_rand=t_rand, u=u, decay=False)
        res[name] = (out['rgb_map'].clone(), out['rgb0'].clone(), loss2.clone(), tr.grad.clone(), out)
    torch.cuda.synchronize()
    for x, y, what in zip(res['ones'][:3], res['white'][:3], ('rgb_map', 'rgb0', 'loss2')):
        assert same(x, y), what
    assert same(res['ones'][4]['bkgd'], torch.ones(64, 3, device='cuda')) and 'bkgd' not in res['white'][4]
    # (the gradients come from two compositing backwards, the white branch and the g_acc row: a figure, not a contract)
    diff, scale = float((res['ones'][3] - res['white'][3]).abs().max()), float(res['white'][3].abs().max())
    print('\nwhite vs ones %-6s max |grad diff| %.3e of max %.3e' % (mode, diff, scale))
    assert scale > 0 and torch.isfinite(res['ones'][3]).all()
    with pytest.raises(ValueError, match='white_bkgd'):
        make_trainer(fn, white=True, bkgd='random').step(*b)
    with pytest.raises(ValueError, match='alpha'):
        make_trainer(fn).step(*b, alpha=torch.ones(64, device='cuda'))


def test_render_white_is_bkgd_ones_and_empty_rays_show_the_colour(fn, math3):
    math3('bf16x6')
    c = AM.loose(fn)
    kw = dict(network_fn=c['net_c'], network_fine=c['net_f'], network_query_fn=None, N_samples=AM.LNS, N_importance=AM.LNI, perturb=0.,
              use_viewdirs=True, near=2., far=6., ndc=False)
    pose = c['pose'].cuda()
    with torch.no_grad():
        white = fn.render.render(RG.H, RG.W, RG.K, c2w=pose, white_bkgd=True, **kw)
        ones = fn.render.render(RG.H, RG.W, RG.K, c2w=pose, bkgd=torch.ones(3, device='cuda'), **kw)
        assert same(white[0], ones[0]) and same(white[3]['rgb0'], ones[3]['rgb0']) and same(white[2], ones[2])
        # rays that look away from everything, through networks without density: acc == 0 exactly, the pixel is the colour
        rb = c['rb'].clone()
        bias = [net.alpha_linear.bias.clone() for net in (c['net_c'], c['net_f'])]
        try:
            for net in (c['net_c'], c['net_f']):
                net.alpha_linear.bias.sub_(1e4)
            colours = torch.rand(rb.shape[0], 3, device='cuda')
            out = fn.render.render_rays(rb, c['net_c'], None, AM.LNS, N_importance=AM.LNI, network_fine=c['net_f'], bkgd=colours)
        finally:
            for net, b0 in zip((c['net_c'], c['net_f']), bias):
                net.alpha_linear.bias.copy_(b0)
        assert (out['acc_map'] == 0).all() and (out['acc0'] == 0).all()
        assert same(out['rgb_map'], colours) and same(out['rgb0'], colours)
    with pytest.raises(ValueError, match='white_bkgd'):
        fn.render.render_rays(c['rb'], c['net_c'], None, AM.LNS, white_bkgd=True, bkgd=torch.ones(3, device='cuda'))


# ---- 3. the gradient against float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Ni', [32, 0], ids=['two_passes', 'one_pass'])
def test_trainer_gradient_against_float64(fn, math3, compact, Ni):
    """One pass (N_importance = 0, one network): the blend works on rgb0 / acc0 as the image pass, and the only g_acc row feeds the
    coarse buffers' backward; the conditions and the bound are the same, on that network's 18 density-path tensors."""
    compact('0')
    (b, _), = AM.batches(fn, 1)
    alpha, colours = step_extras(64, 17)
    on = O.make_ray_batch(b[0].cpu(), b[1].cpu(), 2.0, 6.0)
    t_rand, u = injected()
    if not Ni:
        u = None
    tr = make_trainer(fn, loose_on=on, Ni=Ni)
    nets = [tr.net_c, tr.net_f] if Ni else [tr.net_c]
    sds = {dt: [RG.state(net, dt) for net in nets] for dt in (torch.float64, torch.float32)}
    names = [p + '.' + k for p, sd in zip('cf', sds[torch.float64]) for k in sd]

    def oracle(dt, detach_acc=False):
        sd_c, sd_f = ([{k: v.clone().requires_grad_(True) for k, v in sd.items()} for sd in sds[dt]] + [None])[:2]
        loss2, _ = B.step_loss(O, on.to(dt), sd_c, sd_f, 16, Ni, b[2].cpu(), colours.cpu(), alpha.cpu(), t_rand.cpu(),
                               None if u is None else u.cpu(), detach_acc)
        leaves = list(sd_c.values()) + (list(sd_f.values()) if sd_f else [])
        g = torch.autograd.grad(loss2.sum(), leaves, allow_unused=True)
        return [torch.zeros_like(x) if y is None else y for x, y in zip(leaves, g)], loss2.detach()
    (g64, l64), (g32, _), (gdet, _) = oracle(torch.float64), oracle(torch.float32), oracle(torch.float64, True)
    e32 = [R.rel_l2(a, r) for a, r in zip(g32, g64)]
    share = [float((a - r).norm() / a.norm()) for a, r in zip(g64, gdet)]
    for name, s, e in zip(names, share, e32):
        print('\nbkgd reference %-26s share %.3e  E32 %.3e  16 x E32 %.3e' % (name, s, e, FACTOR * e))
    res = {}
    for mode in ('fp32', 'bf16x6'):
        math3(mode)
        tr = make_trainer(fn, loose_on=on, Ni=Ni)
        loss2, out = tr.step(*b, t_rand=t_rand, u=u, decay=False, alpha=alpha, bkgd=colours)
        torch.cuda.synchronize()
        assert ('acc0' in out) == bool(Ni)
        inside = [int(((a > 0.02) & (a < 0.98)).sum()) for a in ((out['acc_map'], out['acc0']) if Ni else (out['acc_map'],))]
        print('\nbkgd %-6s rays with acc in (0.02, 0.98): %s of 64; loss2 %s (float64 %s)' % (mode, inside, loss2.tolist(), l64.tolist()))
        # the conditions on the reference and on the forward's own outputs, first
        assert min(inside) >= 16, inside
        assert sum(s > 0 for s in share) == 18 * len(nets), 'eight trunk layers and the density head of every network; the colour branch has share 0'
        assert all(FACTOR * e < s for s, e in zip(share, e32) if s > 0), 'the reference resolves the background gradient on every tensor'
        assert same(out['bkgd'], colours)
        assert torch.allclose(loss2.cpu().double(), l64, rtol=1e-4)
        NP = fn.ops.NET_PARAMS
        assert tr.grad.numel() == NP * len(nets)
        res[mode] = [g for k, net in enumerate(nets) for g in net.param_grads_from(tr.grad[k * NP:(k + 1) * NP])]
    for mode, got in res.items():
        AM.check_tensors('bkgd trainer->params %s' % ('two passes' if Ni else 'one pass'), mode, got, names, g64, e32)


# ---- 4. routes ---------------------------------------------------------------------------------------------------------------------------
def loose_rays(fn):
    """The rays of the first batch, for `loosen` to centre the density heads on."""
    (b, _), = AM.batches(fn, 1)
    return O.make_ray_batch(b[0].cpu(), b[1].cpu(), 2.0, 6.0)


def run(fn, route='fused', steps=3, setting='random', use_alpha=True, inject=False, step_kw=None, **kw):
    """AM.run with a background -> (parameters, losses [steps, 2], aux losses [steps, 4], gradient of the last step, the Trainer, the
    colours of every step)."""
    step_kw = dict(step_kw or {})
    old = os.environ.get('FASTNERF_FUSED_STEP')
    if route == 'calls':
        os.environ['FASTNERF_FUSED_STEP'] = '0'      # read by the constructor
    try:
        tr = make_trainer(fn, **(dict(kw, bkgd=setting) if setting is not None else kw))
    finally:
        os.environ.pop('FASTNERF_FUSED_STEP', None)
        if old is not None:
            os.environ['FASTNERF_FUSED_STEP'] = old
    assert tr.fused == (route != 'calls') and tr.world == 1
    torch.manual_seed(5)
    losses, aux4, used = [], [], []
    for it, (b, aux) in enumerate(AM.batches(fn, steps)):
        extra = {k: aux[k] for k in ('acc', 'acc_weight')} if tr.lambda_acc else {}
        alpha, colours = step_extras(64, 30 + it)
        if use_alpha and (setting is not None or inject):
            extra['alpha'] = alpha
        if inject:
            extra['bkgd'] = colours
        if route == 'phased':
            loss2, out = AM.phased_step(fn, tr, b, extra, **step_kw)
        else:
            loss2, out = tr.step(*b, decay=False, **step_kw, **extra)
        losses.append(loss2.clone())
        aux4.append(tr.aux_losses.clone())
        used.append(out['bkgd'].clone() if 'bkgd' in out else None)
    torch.cuda.synchronize()
    return tr.flat.clone(), torch.stack(losses), torch.stack(aux4), tr.grad.clone(), tr, used


@pytest.mark.parametrize('mode', ['bf16x6', 'fp32', 'bf16x3'])
@pytest.mark.parametrize('route', ['0', '1'], ids=['saving', 'compacted'])
def test_routes_agree_bit_for_bit(fn, math3, compact, mode, route):
    math3(mode)
    compact(route)
    for kw in (dict(), dict(lambda_acc=AM.LAM_A)):
        res = {r: run(fn, route=r, **kw) for r in ('fused', 'phased', 'calls')}
        for r in ('phased', 'calls'):
            for x, y, what in zip(res['fused'][:4], res[r][:4], ('parameters', 'loss2', 'aux_losses', 'gradient')):
                assert same(x, y), (kw, r, what)
            assert all(same(x, y) for x, y in zip(res['fused'][5], res[r][5])), 'the same colours'
        f = res['fused']
        assert torch.isfinite(f[0]).all() and f[4].last_step_live == (route == '1') and float(f[3].abs().max()) > 0
        assert all(c is not None and c.shape == (64, 3) and float(c.min()) >= 0 and float(c.max()) < 1 for c in f[5])
        assert not same(f[5][0], f[5][1]), 'fresh colours every step'
        base = run(fn, setting=None, **kw)
        assert not same(f[0], base[0]), 'the background trains'
        if kw:      # the opacity term's own losses do not see the background: the first step's maps are the same
            assert (f[2][:, 2:] > 0).all() and same(f[2][0], base[2][0])
    # the drawn colours are the 'bkgd' stream of the step's seed
    seed = int(f[4]._bk.seed)
    assert seed != 0 and np.array_equal(f[5][2].cpu().numpy(), B.draw(64, seed))


@pytest.mark.parametrize('mode', ['bf16x6', 'fp32'])
@pytest.mark.parametrize('route', ['0', '1'], ids=['saving', 'compacted'])
def test_one_pass_routes_agree_bit_for_bit(fn, math3, compact, mode, route):
    """N_importance = 0: the fused step blends rgb0 / acc0 as the image pass, has no g_acc0, and its g_acc1 row goes to the backward
    of the coarse buffers.  Fused, phase by phase and call by call agree as with two passes."""
    math3(mode)
    compact(route)
    for kw in (dict(), dict(lambda_acc=AM.LAM_A)):
        res = {r: run(fn, route=r, Ni=0, **kw) for r in ('fused', 'phased', 'calls')}
        for r in ('phased', 'calls'):
            for x, y, what in zip(res['fused'][:4], res[r][:4], ('parameters', 'loss2', 'aux_losses', 'gradient')):
                assert same(x, y), (kw, r, what)
            assert all(same(x, y) for x, y in zip(res['fused'][5], res[r][5])), 'the same colours'
        f = res['fused']
        assert f[3].numel() == fn.ops.NET_PARAMS and f[4].net_f is None and (f[1][:, 1] == 0).all()
        assert torch.isfinite(f[0]).all() and f[4].last_step_live == (route == '1') and float(f[3].abs().max()) > 0
        assert not same(f[0], run(fn, setting=None, Ni=0, **kw)[0]), 'the background trains'


@pytest.mark.parametrize('mode', ['bf16x6', 'fp32'])
def test_compacted_against_saving_and_n_global(fn, math3, compact, mode):
    """On loosened networks: half of the coarse samples are dead and stay out of the compacted backward's lists."""
    math3(mode)
    on = loose_rays(fn)
    res = {}
    for route in ('0', '1'):
        compact(route)
        res[route] = run(fn, steps=1, inject=True, setting=None, lambda_acc=AM.LAM_A, loose_on=on)
        assert res[route][4].last_step_live == (route == '1')
    live = res['1'][4].live_counts.tolist()
    assert 0 < live[0] < live[1] and 0 < live[2] < live[3], live
    diff, scale = float((res['0'][3] - res['1'][3]).abs().max()), float(res['0'][3].abs().max())
    print('\nbkgd compacted vs saving %-6s max |diff| %.3e of max %.3e (bound %.3e)' % (mode, diff, scale, 3e-6 * scale))
    assert scale > 0 and diff < 3e-6 * scale
    for route in ('0', '1'):
        compact(route)
        half = run(fn, steps=1, inject=True, setting=None, lambda_acc=AM.LAM_A, loose_on=on, step_kw=dict(n_global=128))
        assert same(half[3] * 2, res[route][3]) and same(half[1], res[route][1]), route


@pytest.mark.parametrize('mode', ['bf16x6', 'fp32'])
def test_through_an_occupancy_grid(fn, math3, compact, mode):
    math3(mode)
    compact('1')
    G = fn.occupancy.OccupancyGrid
    plain = run(fn)
    full = run(fn, occupancy=G.for_training(N=16, bound=4.5), occupancy_warmup=10 ** 9)
    for x, y, what in zip(plain[:4], full[:4], ('parameters', 'loss2', 'aux_losses', 'gradient')):
        assert same(x, y), what
    mask = torch.ones(16, 16, 16, dtype=torch.bool, device='cuda')
    mask[:, :, 5:11] = False
    for tighten in (False, True):
        res = run(fn, occupancy=G.from_mask(mask, -4.5, 4.5, outside_occupied=False), tighten=tighten)
        live, occ = res[4].live_counts.tolist(), res[4].occupancy_counts.tolist()
        print('\nbkgd occupancy %-6s tighten %d live %s occupied %s' % (mode, tighten, live, occ))
        assert 0 < occ[0] <= occ[1] and 0 < occ[2] <= occ[3] and (tighten or (occ[0] < occ[1] and occ[2] < occ[3]))
        assert live[0] <= occ[2] and live[2] <= occ[0] and live[1] == occ[3] and live[3] == occ[1]
        assert torch.isfinite(res[0]).all() and torch.isfinite(res[1]).all() and torch.isfinite(res[3]).all()


def test_live_counts_with_and_without(fn, math3, compact):
    """A background makes every positive-density sample of a non-opaque ray live, as the opacity term does.  With random targets the
    colour loss alone already does that; it shows where the colour residual is exactly zero: the targets are the image pass's own
    colours of the same draws, so without a background the image pass has no live sample at all, and over a colour per ray with
    alpha = 1/2 (prediction rgb + (1 - acc) b against rgb / 2 + b / 2) it has."""
    math3('bf16x6')
    compact('1')
    on = loose_rays(fn)
    (b, _), = AM.batches(fn, 1)
    t_rand, u = injected()
    _, colours = step_extras(64, 41)
    half = torch.full((64,), 0.5, device='cuda')

    def step(target, **kw):
        tr = make_trainer(fn, loose_on=on, **({'bkgd': 'random'} if kw else {}))
        _, out = tr.step(b[0], b[1], target, t_rand=t_rand, u=u, decay=False, **kw)
        torch.cuda.synchronize()
        assert tr.last_step_live
        return out['rgb_map'].clone(), tr.live_counts.tolist()
    rgb, random_targets = step(b[2])
    same_rgb, without = step(rgb)
    _, with_bk = step(rgb, alpha=half, bkgd=colours)
    _, random_with = step(b[2], alpha=half, bkgd=colours)
    print('\nbkgd live_counts (live, total) fine, coarse: random targets %s, the same with a background %s; zero-residual targets without %s with %s'
          % (random_targets, random_with, without, with_bk))
    assert same(same_rgb, rgb), 'the same forward: the image pass has a residual of exactly zero'
    assert with_bk[1] == without[1] and with_bk[3] == without[3]
    assert without[0] == 0 and 0 < with_bk[0] <= with_bk[1], 'only the background reaches the image pass'
    assert 0 < without[2] <= with_bk[3] and 0 < with_bk[2] <= with_bk[3]


# ---- 5. nothing moved ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['fused', 'calls'])
def test_no_background_is_the_trainer_without_the_keyword(fn, math3, compact, route):
    math3('bf16x6')
    compact('auto')
    base = AM.run(fn, route=route, use_aux=False)
    for res in (run(fn, route=route, setting=None, white=True), run(fn, route=route, setting=None, white=True, bkgd=None)):
        for x, y, what in zip(base[:4], res[:4], ('parameters', 'loss2', 'aux_losses', 'gradient')):
            assert same(x, y), what
        assert all(c is None for c in res[5]) and res[4]._bk is None


def test_no_background_marched(fn, math3, compact):
    math3('bf16x6')
    compact('1')
    n, K, C = 96, 64, 32
    res = []
    for kw in (dict(), dict(bkgd=None)):
        tr, _, _ = MTG.new_trainer(fn, MTG.device_grid(fn, M.two_shells()), perturb=1.0, march=K, march_cap=C, **kw)
        torch.manual_seed(9)
        log = []
        for it in range(3):
            loss2, out = tr.step(*MTG.batch(n, 40 + it))
            log += [loss2.clone(), tr.grad.clone()]
            assert 'bkgd' not in out
        res.append(log + [tr.flat.clone()])
    assert all(same(x, y) for x, y in zip(*res))


def test_random_is_reproducible_and_the_empty_shard_burns_the_seed(fn, math3, compact):
    math3('bf16x6')
    compact('auto')
    a, b = run(fn), run(fn)
    for x, y in zip(a[:4], b[:4]):
        assert same(x, y)
    assert all(same(x, y) for x, y in zip(a[5], b[5]))
    e3, e1 = torch.empty(0, 3, device='cuda'), torch.empty(0, device='cuda')
    (batch, _), = AM.batches(fn, 1)
    alpha, _ = step_extras(64, 1)
    states = {}
    for setting in (None, 'random', (0.2, 0.4, 0.6)):
        for empty in (True, False):
            tr = make_trainer(fn, **({} if setting is None else dict(bkgd=setting)))
            before = tr.flat.clone()
            torch.manual_seed(77)
            if empty:
                loss2, out = tr.step(e3, e3, e3, n_global=64, **({} if setting is None else dict(alpha=e1)))
                assert (loss2 == 0).all() and out == {} and same(tr.flat, before) and int(tr.grad.count_nonzero()) == 0
            else:
                tr.step(*batch, n_global=64, **({} if setting is None else dict(alpha=alpha)))
            states[(setting, empty)] = torch.get_rng_state()
        assert torch.equal(states[(setting, True)], states[(setting, False)]), setting
    assert not torch.equal(states[('random', True)], states[(None, True)]), "'random' draws one seed more"
    assert torch.equal(states[((0.2, 0.4, 0.6), True)], states[(None, True)]), 'a constant colour draws none'


# ---- 6. the marched step -------------------------------------------------------------------------------------------------------------------
def march_by_hand(fn, tr, grid, ro, rd, tgt, u, K, C, which, colours, alpha, grad_scale=1.0):
    """MTG.by_hand with a background: the launches of fastnerf_train_step_march_bkgd through ops."""
    ops = fn.ops
    Nn = ops.NET_PARAMS
    n = ro.shape[0]
    sl = slice(which * Nn, (which + 1) * Nn)
    params, m, v = tr.flat[sl].clone(), tr.m[sl].clone(), tr.v[sl].clone()
    pf, pb = ops.mlp_pack(params)
    rays11 = ops.pack_rays(ro, rd, 2.0, 6.0)
    z, kidx, overflow, _ = ops.occ_march_jitter(grid._c, rays11, K, C, u=u)
    raw = torch.empty(n, C, 4, device='cuda')
    counts = torch.zeros(2, device='cuda', dtype=torch.int32)
    idx, cnt = ops.march_list(kidx, 0, C, raw=raw, total=counts, lattice=n * K)
    ops.mlp_fwd_list(rays11, z, params, pf, raw, idx, cnt, flags=1 if tr.skip_dead_rgb else 0)
    rgb, disp, acc, w, depth = ops.raw2outputs_fwd(raw, z, rays11, None, False)
    bare = rgb.clone()
    target, used = ops.bkgd_blend(rgb, acc, tgt, bkgd=colours, alpha=alpha)
    loss2, g, _ = ops.mse_leafmax(rgb, None, target, grad_scale=grad_scale)
    ops.march_mask(overflow, g)
    g_acc, _ = ops.bkgd_grad(used, g)
    draw = ops.raw2outputs_bwd_full(raw, z, rays11, acc, depth, g_rgb=g, g_acc=g_acc, white_bkgd=False)
    P = n * C
    ws = torch.empty(ops.dact_floats(P), device='cuda')
    draw_ws = torch.empty(P * 4, device='cuda')
    act = torch.empty(ops.act_floats(P), device='cuda')
    partial = torch.empty(ops.mlp_bwd_partial_floats(), device='cuda')
    live_ws = torch.empty(ops.live_ws_ints(P), device='cuda', dtype=torch.int32)
    grad = torch.full((Nn,), float('nan'), device='cuda')
    ops.render_rays_bwd_live(rays11, False, g, None, None, None, z, raw, None, None, params, (pf, pb), None, None, draw_ws, act, ws, partial,
                             live_ws, grad, None, C, 0, map_grads=dict(g_acc1=g_acc, acc0=acc, depth0=depth))
    res = dict(grad=grad.clone(), z=z, kidx=kidx, overflow=overflow, rgb=rgb, bare=bare, acc=acc, loss2=loss2, g=g, g_acc=g_acc, draw=draw,
               target=target, used=used, rays11=rays11)
    ops.adam_step(params, grad, m, v, tr.lr, tr.adam_t + 1, tr.beta1, tr.beta2, tr.eps)
    ops.mlp_pack(params, pf, pb)
    res.update(flat=params, m=m, v=v)
    return res


@pytest.mark.parametrize('n,K,C', [(193, 64, 32), (96, 13, 5)], ids=['fits', 'overflows'])
def test_marched_step_is_its_parts(fn, math_mode, compact, n, K, C):
    compact('1')
    grid = MTG.device_grid(fn, M.two_shells())
    Nn = fn.ops.NET_PARAMS
    ro, rd, tgt = MTG.batch(n, 3)
    u = torch.from_numpy(np.random.RandomState(9).rand(n).astype(F32)).cuda()
    alpha, colours = step_extras(n, 23)
    tr, _, _ = MTG.new_trainer(fn, grid, white_bkgd=False, march=K, march_cap=C)
    hand = march_by_hand(fn, tr, grid, ro, rd, tgt, u, K, C, 1, colours, alpha)
    loss2, out = tr.step(ro, rd, tgt, march_u=u, decay=False, alpha=alpha, bkgd=colours)
    torch.cuda.synchronize()
    ov = out['march_overflow']
    assert torch.equal(out['march_k'], hand['kidx']) and same(out['z_vals'], hand['z']) and torch.equal(ov, hand['overflow'].bool())
    assert same(out['rgb_map'], hand['rgb']) and same(loss2[:1], hand['loss2'][:1]) and same(out['bkgd'], colours)
    assert same(tr._bk_views['target'], hand['target']) and same(tr._bk_views['g_acc1'], hand['g_acc'])
    sl = slice(Nn, 2 * Nn)
    assert same(tr.grad[sl], hand['grad']) and float(hand['grad'].abs().max()) > 0
    for name, mine in (('flat', tr.flat[sl]), ('m', tr.m[sl]), ('v', tr.v[sl])):
        assert same(mine, hand[name]), name
    # a ray without live samples shows its colour, bit for bit
    empty = ~(out['march_k'] >= 0).any(1)
    assert int(empty.sum()) >= 4 and same(out['rgb_map'][empty], colours[empty]) and (out['acc_map'][empty] == 0).all()
    assert not same(out['rgb_map'][~empty], hand['bare'][~empty]) or bool((hand['acc'][~empty] == 1).all())
    if C == 5:
        assert 4 <= int(ov.sum()) <= n - 4
        g = MTG.block_view(tr, 'g_rgb')
        assert bool((g[ov] == 0).all()) and bool((tr._bk_views['g_acc1'][ov] == 0).all()), 'zero g_rgb, +-0 g_acc'
        assert bool((hand['draw'][ov] == 0).all()) and bool((hand['draw'][~ov] != 0).any()), 'the draw rows of an overflowed ray'
    else:
        assert not bool(ov.any())


_MARCH64 = {}


def march_f64(sd, rays11, z, live, target, colours, overflow, dtype, detach=False):
    """MTG.f64_grad with a background, per parameter tensor and in `dtype`: the network at o + d * z of the live slots, zero logits
    elsewhere, the reference's raw2outputs over the row, the blend, the mean squared error over all rays with the overflowed rays'
    gradient cut (their term is detached)."""
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    rb, z, lv = torch.from_numpy(rays11).to(dtype), torch.from_numpy(z).to(dtype), torch.from_numpy(live)
    pts = (rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None])[lv]
    dirs = rb[:, None, 8:11].expand(z.shape[0], z.shape[1], 3)[lv]
    raw = torch.zeros(z.shape[0], z.shape[1], 4, dtype=dtype)
    raw[lv] = O.nerf_forward(sd, torch.cat([O.posenc(pts, 10), O.posenc(dirs, 4)], -1))
    rgb, _, acc, _, _ = O.raw2outputs(raw, z, rb[:, 3:6], None, False)
    rgb = B.blend_torch(rgb, acc, torch.from_numpy(colours).to(dtype))
    keep = torch.from_numpy(~overflow)[:, None].to(dtype)
    rgb = rgb * keep + rgb.detach() * (1 - keep)
    loss = ((rgb - torch.from_numpy(target).to(dtype)) ** 2).mean()
    leaves = [sd[nm] for nm, _ in O.nerf_param_shapes()]
    g = torch.autograd.grad(loss, leaves, allow_unused=True)
    return [torch.zeros_like(x) if y is None else y for x, y in zip(leaves, g)]


@pytest.mark.parametrize('mode', ['fp32', 'bf16x6'])
def test_marched_gradient_against_float64(fn, math3, compact, mode):
    math3(mode)
    compact('1')
    n, K, C = 193, 64, 32
    grid = MTG.device_grid(fn, M.two_shells())
    ro, rd, tgt = MTG.batch(n, 3)
    u = torch.from_numpy(np.random.RandomState(9).rand(n).astype(F32)).cuda()
    alpha, colours = step_extras(n, 23)
    tr, _, (_, sdf) = MTG.new_trainer(fn, grid, white_bkgd=False, march=K, march_cap=C)
    loss2, out = tr.step(ro, rd, tgt, march_u=u, decay=False, alpha=alpha, bkgd=colours)
    torch.cuda.synchronize()
    z, k, ov = out['z_vals'].cpu().numpy(), out['march_k'].cpu().numpy(), out['march_overflow'].cpu().numpy()
    if 'ref' not in _MARCH64:      # (depths and live sets do not depend on the math mode: asserted below)
        r11 = fn.ops.pack_rays(ro, rd, 2.0, 6.0).cpu().numpy()
        target = tr._bk_views['target'].cpu().numpy()
        g64, g32 = [march_f64(sdf, r11, z, k >= 0, target, colours.cpu().numpy(), ov, dt) for dt in (torch.float64, torch.float32)]
        _MARCH64['ref'] = (z, k, g64, [R.rel_l2(a, r) if float(r.norm()) > 0 else 0.0 for a, r in zip(g32, g64)])
    z0, k0, g64, e32 = _MARCH64['ref']
    assert np.array_equal(z, z0) and np.array_equal(k, k0)
    Nn = fn.ops.NET_PARAMS
    got = tr.net_f.param_grads_from(tr.grad[Nn:])
    AM.check_tensors('bkgd marched->params', mode, got, [nm for nm, _ in O.nerf_param_shapes()], g64, e32)


# ---- 7. the render surface -------------------------------------------------------------------------------------------------------------------
_RENDER64 = {}


def render_oracle(c, colours, dtype, wrt_rays):
    sd_c = {k: v.clone().requires_grad_(True) for k, v in RG.state(c['net_c'], dtype).items()}
    sd_f = {k: v.clone().requires_grad_(True) for k, v in RG.state(c['net_f'], dtype).items()}
    rb = c['rb'].cpu().to(dtype).clone().requires_grad_(wrt_rays)
    ret = O.render_rays(rb, sd_c, sd_f, AM.LNS, AM.LNI)
    bb = colours.cpu().to(dtype)
    loss = (B.blend_torch(ret['rgb_map'], ret['acc_map'], bb) * c['cot']['rgb_map'].cpu().to(dtype)).sum() \
        + (B.blend_torch(ret['rgb0'], ret['acc0'], bb) * c['cot']['rgb0'].cpu().to(dtype)).sum()
    leaves = [rb] if wrt_rays else list(sd_c.values()) + list(sd_f.values())
    return [torch.zeros_like(x) if g is None else g for x, g in zip(leaves, torch.autograd.grad(loss, leaves, allow_unused=True))]


@pytest.mark.parametrize('mode', ['fp32', 'bf16x6'])
def test_render_rays_gradients_against_float64(fn, math3, compact, mode):
    math3(mode)
    compact('0')
    c = AM.loose(fn)
    colours = torch.rand(AM.LNR, 3, generator=torch.Generator().manual_seed(4)).cuda()
    if 'p' not in _RENDER64:
        p64, p32 = [render_oracle(c, colours, dt, False) for dt in (torch.float64, torch.float32)]
        r64, r32 = [render_oracle(c, colours, dt, True)[0] for dt in (torch.float64, torch.float32)]
        _RENDER64.update(p=(p64, [R.rel_l2(a, r) if float(r.norm()) > 0 else 0.0 for a, r in zip(p32, p64)]), r=(r64, RG.group_errors(r32, r64)))
    p64, pe32 = _RENDER64['p']
    r64, re32 = _RENDER64['r']
    rb = c['rb'].clone().requires_grad_()
    cot = {k: c['cot'][k] for k in ('rgb_map', 'rgb0')}
    nets = [c['net_c'], c['net_f']]
    for net in nets:
        for p in net.parameters():
            p.grad = None
    out = fn.render.render_rays(rb, c['net_c'], None, AM.LNS, N_importance=AM.LNI, network_fine=c['net_f'], perturb=0., bkgd=colours)
    sum((out[k] * v).sum() for k, v in cot.items()).backward()
    torch.cuda.synchronize()
    grads = [[p.grad.clone() for p in net.parameters()] for net in nets]
    inside = [int(((out[k] > 0.02) & (out[k] < 0.98)).sum()) for k in ('acc_map', 'acc0')]
    print('\nbkgd render %-6s rays with acc in (0.02, 0.98): %s of %d' % (mode, inside, AM.LNR))
    assert min(inside) >= 3, inside
    AM.check_tensors('bkgd render->params', mode, grads[0] + grads[1], c['names'], p64, pe32)
    assert rb.grad is not None and torch.isfinite(rb.grad).all() and (rb.grad[:, 6:8] == 0).all()
    for name, err in RG.group_errors(rb.grad.cpu(), r64).items():
        print('\nbkgd render->rays %-6s %-7s err %.3e  E32 %.3e  bound %.3e' % (mode, name, err, re32[name], FACTOR * re32[name]))
        assert err <= FACTOR * re32[name], (name, err, re32[name])
    # the maps are the call without bkgd plus (1 - acc) b
    with torch.no_grad():
        kw = dict(N_importance=AM.LNI, network_fine=c['net_f'], perturb=0.)
        bare = fn.render.render_rays(c['rb'], c['net_c'], None, AM.LNS, **kw)
        got = fn.render.render_rays(c['rb'], c['net_c'], None, AM.LNS, bkgd=colours, **kw)
        for k, a in (('rgb_map', 'acc_map'), ('rgb0', 'acc0')):
            assert same(got[k], bare[k] + (1. - bare[a])[:, None] * colours) and same(got[a], bare[a])


def test_closure_route_against_plain_torch_autograd(fn):
    import test_gpu_custom_network as CN
    n = 64
    net_c, net_f = CN.make_nets(True, True)
    net_c.cuda()
    net_f.cuda()
    rb = CN.ray_batch(True, n=n).cuda()
    colours = torch.rand(n, 3, generator=torch.Generator().manual_seed(6)).cuda()
    cot = torch.randn(2, n, 3, generator=torch.Generator().manual_seed(7)).cuda()
    params = list(net_c.parameters()) + list(net_f.parameters())
    kw = dict(N_importance=32, network_fine=net_f, perturb=1.0, pytest=True)

    def grads(with_kw):
        for p in params:
            p.grad = None
        if with_kw:
            out = fn.render.render_rays(rb, net_c, CN.query_fn(fn), 16, bkgd=colours, **kw)
            rgb, rgb0 = out['rgb_map'], out['rgb0']
        else:      # plain torch on the maps of the call without the keyword
            out = fn.render.render_rays(rb, net_c, CN.query_fn(fn), 16, **kw)
            rgb = out['rgb_map'] + (1. - out['acc_map'])[:, None] * colours
            rgb0 = out['rgb0'] + (1. - out['acc0'])[:, None] * colours
        ((rgb * cot[0]).sum() + (rgb0 * cot[1]).sum()).backward()
        return rgb.detach(), rgb0.detach(), [p.grad.clone() for p in params], out
    a, b = grads(True), grads(False)
    assert same(a[0], b[0]) and same(a[1], b[1])
    inside = int(((a[3]['acc_map'] > 0.02) & (a[3]['acc_map'] < 0.98)).sum())
    assert inside >= 4, inside
    # the same torch graph on the same kernels: equal up to the order of torch's own reductions
    for x, y in zip(a[2], b[2]):
        assert torch.isfinite(x).all() and float((x - y).abs().max()) <= 1e-5 * float(y.abs().max()) + 1e-12
    assert any(float(x.abs().max()) > 0 for x in a[2])


def test_inference_routes_add_the_colour(fn, math3):
    math3('bf16x6')
    import ert_numpy as E
    sdc, sdf = E.scene_networks(O)
    args = fn.run_nerf.make_args(N_importance=16, N_samples=16, perturb=0., use_viewdirs=True, no_reload=True)
    torch.manual_seed(0)
    ktr = fn.run_nerf.create_nerf(args)[0]
    ktr['network_fn'].load_state_dict(sdc)
    ktr['network_fine'].load_state_dict(sdf)
    grid = MTG.device_grid(fn, M.two_shells())
    ro, rd, _ = MTG.batch(96, 3)
    rb = fn.ops.pack_rays(ro, rd, 2.0, 6.0)
    colours = torch.rand(96, 3, generator=torch.Generator().manual_seed(8)).cuda()
    base = dict(N_importance=16, network_fine=ktr['network_fine'], perturb=0.)
    with torch.no_grad():
        for name, kw in (('march', dict(occupancy=grid, march=64, march_cap=32)), ('occupancy', dict(occupancy=grid)),
                         ('ert', dict(ert=1e-2, ert_block=8)), ('occupancy+ert+tighten', dict(occupancy=grid, ert=1e-2, ert_block=8, tighten=True))):
            bare = fn.render.render_rays(rb, ktr['network_fn'], None, 16, **base, **kw)
            for bk in (colours, torch.tensor([0.25, 0.5, 0.75], device='cuda')):
                got = fn.render.render_rays(rb, ktr['network_fn'], None, 16, bkgd=bk, **base, **kw)
                assert set(got) == set(bare), name
                assert same(got['rgb_map'], bare['rgb_map'] + (1. - bare['acc_map'])[:, None] * bk), name
                assert same(got['acc_map'], bare['acc_map']) and same(got['disp_map'], bare['disp_map']), name
                if 'rgb0' in bare:
                    assert same(got['rgb0'], bare['rgb0'] + (1. - bare['acc0'])[:, None] * bk), name
            assert bool((bare['acc_map'] < 1).any()), 'some ray shows its background'


def test_chunked_render_slices_per_ray_colours(fn, math3):
    math3('bf16x6')
    c = AM.loose(fn)
    H, W = RG.H, RG.W
    colours = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(10)).cuda()
    kw = dict(c2w=c['pose'].cuda(), ndc=False, network_fn=c['net_c'], network_fine=c['net_f'], network_query_fn=None, N_samples=AM.LNS,
              N_importance=AM.LNI, perturb=0., use_viewdirs=True, near=2., far=6.)
    with torch.no_grad():
        one = fn.render.render(H, W, RG.K, chunk=H * W, bkgd=colours, **kw)
        for chunk in (100, 257):
            many = fn.render.render(H, W, RG.K, chunk=chunk, bkgd=colours, **kw)
            assert same(one[0], many[0]) and same(one[3]['rgb0'], many[3]['rgb0']) and one[0].shape == (H, W, 3)
        flat = fn.render.render(H, W, RG.K, chunk=100, bkgd=colours.reshape(-1, 3), **kw)
        assert same(one[0], flat[0])
        bare = fn.render.render(H, W, RG.K, chunk=H * W, **kw)
        assert same(one[0], bare[0] + (1. - bare[2])[..., None] * colours) and bool((bare[2] < 0.98).any())
        rgbs, _ = fn.render.render_path([c['pose'].cuda()], [H, W, float(RG.K[0][0])], RG.K, 100, dict({k: v for k, v in kw.items() if k != 'c2w'},
                                                                                                  bkgd=colours))
        assert np.array_equal(rgbs[0], one[0].cpu().numpy())


# ---- 8. the data path ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compat_rng', [True, False], ids=['host_picks', 'device_picks'])
def test_train_loop_takes_alpha_at_the_rays_own_pixels(fn, monkeypatch, compat_rng):
    """run_nerf.train with args.random_bkgd: every step of the warm-up and of the epochs gets the alpha of its rays' pixels.  The images
    carry their red channel as alpha, so a row's alpha must equal its target's red, whatever route picked the pixel."""
    imgs, poses, focal = fn.synthetic.make_dataset(n_images=4, H=32, W=32)
    imgs = torch.as_tensor(imgs, dtype=torch.float32)
    rgba = torch.cat([imgs, imgs[..., :1]], -1)
    seen = []
    step = fn.run_nerf.Trainer.step

    def spy(self, rays_o, rays_d, target, *a, **kw):
        loss2, out = step(self, rays_o, rays_d, target, *a, **kw)
        seen.append((self.bkgd, target.clone(), kw.get('alpha'), out['bkgd'].clone(), loss2.clone()))
        return loss2, out
    monkeypatch.setattr(fn.run_nerf.Trainer, 'step', spy)
    torch.manual_seed(0)
    np.random.seed(0)
    args = fn.run_nerf.make_args(N_importance=16, N_samples=16, perturb=1.0, white_bkgd=False, random_bkgd=True, no_reload=True, N_rand=256,
                                 n_epoch=2, init_level=2, subdivide_every=1, subdivide_thres=0.05, lrate=5e-4, lrate_decay=500)
    _, _, trainer, mgr, hist = fn.run_nerf.train(rgba, poses, 32, 32, focal, args, log=lambda s: None, compat_rng=compat_rng,
                                                 max_iters_per_epoch=3)
    torch.cuda.synchronize()
    assert trainer.bkgd == 'random' and len(hist) == 2 and all(np.isfinite(h[2]) for h in hist) and len(seen) >= 6
    assert mgr.images.shape[-1] == 3 and mgr.result_pix is not None and mgr.result_pix.shape[1] == 3
    for setting, target, alpha, used, loss2 in seen:
        assert setting == 'random' and alpha is not None and alpha.shape == (target.shape[0],)
        assert same(alpha, target[:, 0].contiguous()), 'alpha of the row\'s own pixel'
        assert float(used.min()) >= 0 and float(used.max()) < 1 and torch.isfinite(loss2).all()
    assert not same(seen[0][3], seen[1][3])
    with pytest.raises(ValueError, match='RGBA'):
        fn.run_nerf.train(imgs, poses, 32, 32, focal, args, log=lambda s: None, max_iters_per_epoch=1)
