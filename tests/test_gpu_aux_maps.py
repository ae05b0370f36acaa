"""Depth / opacity supervision and every rendered map differentiable on the fused route: ops.aux_loss (csrc/train.hip
aux_loss_kernel), map gradients through render_rays (fastnerf_render_rays_bwd_maps / _bwd_live_maps), rays and poses, and
Trainer(lambda_depth=, lambda_acc=).step(depth=, acc=) (fastnerf_train_step_aux).

Networks: make_net of tests/test_gpu_ray_grad.py (density bias lifted by 0.3): every ray has acc > 0, so no disparity is NaN --
asserted on the forward's own acc output wherever a disparity cotangent is used.  With that lift the last sample of every ray is live
and its dist is 1e10, so acc = 1 to 1e-10 and d(acc)/d(raw) is below an fp32 ulp of the other terms: sections 2 to 6 pin the depth,
disparity and colour terms and would not notice a wrong opacity gradient.  Section 7 is the opacity's own: networks whose density head
is steepened and centred (`loosen`), so that half of the samples are dead, most rays end on a dead sample and acc lies well inside
(0, 1) -- asserted on the forward's own outputs -- with cotangents on acc_map / acc0 alone (no disparity cotangent: a ray may have
acc = 0).  The same networks put dead samples into the compacted backward's lists, and section 7 runs the shared-network route.

Bounds.  ops.aux_loss against the float64 restatement (tests/aux_loss_ref.py) on the same fp32 inputs: a gradient is at most three
fp32 roundings from exact -> 4 * 2^-24 relative; a loss stays within n * 2^-24 * sum |term|, the worst case of ANY fp32 summation
order.  Against the float64 oracle: relative L2 per parameter tensor (per column group for rays, R / t for a pose) <= 16 x E32, E32
being the same metric for torch's float32 CPU autograd of the same oracle -- the project's rule (tests/test_gpu_ray_grad.py,
tests/test_gpu_sigma_grad.py), for the two math modes of fp32 width, 'fp32' and 'bf16x6' ('bf16x3' multiplies with 16 significand
bits: the rule does not describe it; its composition is pinned bit for bit in section 2 instead).  Compacted against saving route:
the 3e-6 of the largest gradient that tests/test_gpu_compact.py documents for the regrouped partial sums.  Every figure is printed
before it is asserted (pytest -s; recorded in profiles/aux_maps.md)."""
import os

import numpy as np
import pytest
import torch

import aux_loss_ref as A
import test_gpu_ray_grad as RG
import test_ray_grad_cpu as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

FACTOR = 16.0
U = 2.0 ** -24
MAPS2 = ('rgb_map', 'disp_map', 'acc_map', 'depth_map', 'rgb0', 'disp0', 'acc0', 'depth0')
MAPS1 = MAPS2[:4]


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


@pytest.fixture
def math3(request, fn):
    old = fn.ops.get_math()
    yield lambda m: fn.ops.set_math(m)
    fn.ops.set_math(old)


@pytest.fixture
def compact(fn):
    old = fn.render.get_compact()
    yield fn.render.set_compact
    fn.render.set_compact(old)


# ---- 1. ops.aux_loss ----------------------------------------------------------------------------------------------------------
def aux_inputs(n, seed, weights, sparse):
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(n, generator=gen)      # noqa: E731
    maps = dict(depth1=2 + 4 * r(), acc1=r(), depth0=2 + 4 * r(), acc0=r())
    tg = dict(depth_target=2 + 4 * r(), acc_target=(r() > 0.5).float())
    if weights or sparse:
        tg.update(depth_weight=0.5 + r(), acc_weight=0.25 + 2 * r())
    if sparse:      # 30 % of the rays carry no target: weight 0, target NaN
        for k in ('depth', 'acc'):
            off = r() < 0.3
            off[0] = True
            tg[k + '_weight'][off] = 0.
            tg[k + '_target'][off] = float('nan')
    return maps, tg


@pytest.mark.parametrize('n', [1, 1023, 1025, 4097])
@pytest.mark.parametrize('kind', ['plain', 'weights', 'sparse'])
def test_aux_loss_against_float64(fn, n, kind):
    lam_d, lam_a, scale = 0.7, 0.3, 0.5
    maps, tg = aux_inputs(n, 7 * n + len(kind), kind == 'weights', kind == 'sparse')
    cu = lambda d: {k: v.cuda() for k, v in d.items()}      # noqa: E731
    m, t = cu(maps), cu(tg)
    call = lambda: fn.ops.aux_loss(m['depth1'], m['acc1'], m['depth0'], m['acc0'], lambda_depth=lam_d, lambda_acc=lam_a,      # noqa: E731
                                   grad_scale=scale, **t)
    loss4, g = call()
    loss4b, gb = call()
    torch.cuda.synchronize()
    ref4, gref = A.aux_loss(**maps, **tg, lambda_depth=lam_d, lambda_acc=lam_a, grad_scale=scale)
    assert loss4.shape == (4,) and torch.equal(loss4, loss4b) and all(torch.equal(g[k], gb[k]) for k in g), 'two calls, same bits'
    for slot, (name, x, w, tgt) in enumerate((('g_depth1', 'depth1', 'depth_weight', 'depth_target'), ('g_depth0', 'depth0', 'depth_weight', 'depth_target'),
                                              ('g_acc1', 'acc1', 'acc_weight', 'acc_target'), ('g_acc0', 'acc0', 'acc_weight', 'acc_target'))):
        got, want = g[name].cpu().double(), gref[name]
        err = float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())
        wv = tg.get(w)
        on = torch.ones(n, dtype=torch.bool) if wv is None else wv != 0
        terms = torch.where(on, (1.0 if wv is None else wv.double()) * (maps[x].double() - torch.where(on, tg[tgt], torch.zeros(())).double()) ** 2,
                            torch.zeros((), dtype=torch.float64)) / n
        lerr, lbound = abs(float(loss4[slot]) - float(ref4[slot])), n * U * float(terms.abs().sum())
        print('\naux_loss n=%d %-7s %-8s grad rel err %.3e (bound %.3e)  loss err %.3e (bound %.3e)' % (n, kind, name, err, 4 * U, lerr, lbound))
        assert torch.isfinite(got).all() and bool(((got - want).abs() <= 4 * U * want.abs()).all()), (name, err)
        assert lerr <= lbound, (name, lerr, lbound)
        if kind == 'sparse':
            bits = g[name].cpu().view(torch.int32)[~on]
            assert bits.numel() > 0 and (bits == 0).all(), 'a zero-weight ray gets +0, bit for bit'
    # a NULL target: its losses are 0 and it has no gradient; the coarse maps may be absent (one pass)
    l4, g1 = fn.ops.aux_loss(m['depth1'], m['acc1'], acc_target=t['acc_target'], acc_weight=t.get('acc_weight'), lambda_acc=lam_a, grad_scale=scale)
    assert l4[0] == 0 and l4[1] == 0 and l4[3] == 0 and g1['g_depth1'] is None and g1['g_acc0'] is None and g1['g_depth0'] is None
    assert torch.equal(g1['g_acc1'], g['g_acc1']) and l4[2] == loss4[2], 'a term does not depend on the other one'


# ---- 2. composition -----------------------------------------------------------------------------------------------------------
def ray_batch(n, seed):
    gen = torch.Generator().manual_seed(seed)
    ro = torch.randn(n, 3, generator=gen) * 0.4
    rd = torch.randn(n, 3, generator=gen)
    return O.make_ray_batch(ro, rd, 2.0, 6.0)


def cotangents(n, names, seed):
    gen = torch.Generator().manual_seed(seed)
    return {k: torch.randn(n, 3, generator=gen) if k.startswith('rgb') else torch.randn(n, generator=gen) for k in names}


def nets_of(fn, Ni, seed):
    return RG.make_net(fn, seed), (RG.make_net(fn, seed + 1) if Ni > 0 else None)


def fused(fn, net_c, net_f, rb, Ns, Ni, cot, **kw):
    """render_rays on the fused route with a loss sum_k <map_k, cot_k> -> (outputs, saved tensors, parameter gradients per net)."""
    nets = [net_c] + ([net_f] if net_f is not None else [])
    for net in nets:
        for p in net.parameters():
            p.grad = None
    out = fn.render.render_rays(rb, net_c, None, Ns, N_importance=Ni, network_fine=net_f, perturb=0., retdepth=True, **kw)
    sum((out[k] * c).sum() for k, c in cot.items()).backward()
    torch.cuda.synchronize()
    return out, out['rgb_map'].grad_fn.saved, [[p.grad.clone() for p in net.parameters()] for net in nets]


def hand_pass(fn, saved, k, net, packed, c, names):
    """raw2outputs_bwd_full -> mlp_bwd of one pass on the saved tensors: the pinned parts, called by hand."""
    z, raw = saved['z' + k], saved['raw' + k]
    draw = fn.ops.raw2outputs_bwd_full(raw, z, saved['rays11'], saved['acc' + k], saved['depth' + k], g_rgb=c[names[0]], g_disp=c[names[1]],
                                       g_acc=c[names[2]], g_depth=c[names[3]], noise=saved['noise' + k], white_bkgd=saved['white'])
    dact = torch.empty(fn.ops.dact_floats(z.numel()), device='cuda')
    partial = torch.empty(fn.ops.mlp_bwd_partial_floats(), device='cuda')
    flat = torch.full_like(net.flat, float('nan'))
    fn.ops.mlp_bwd(draw, saved['act' + k], net.flat, packed[1], dact, partial, flat)
    return draw, net.param_grads_from(flat)


@pytest.mark.parametrize('mode', ['fp32', 'bf16x3', 'bf16x6'])
@pytest.mark.parametrize('n,Ns,Ni', [(1, 2, 0), (3, 21, 46), (5, 64, 128)])
def test_composition_is_the_pinned_parts_bit_for_bit(fn, math3, compact, mode, n, Ns, Ni):
    math3(mode)
    compact('0')
    net_c, net_f = nets_of(fn, Ni, 400 + Ns)
    names = MAPS2 if Ni > 0 else MAPS1
    cot = {k: v.cuda() for k, v in cotangents(n, names, 50 + n).items()}
    before = RG_pair_launches(fn)
    out, saved, grads = fused(fn, net_c, net_f, ray_batch(n, 60 + n).cuda(), Ns, Ni, cot, white_bkgd=Ns % 2 == 0)
    paired = RG_pair_launches(fn) - before
    assert (out['acc_map'] > 0).all() and (Ni == 0 or (out['acc0'] > 0).all()), 'no NaN disparity: every ray has acc > 0'
    assert all(out[k].requires_grad for k in names) and set(out) == set(names) | ({'z_std'} if Ni > 0 else set())
    if Ni > 0:
        _, hand_f = hand_pass(fn, saved, '1', net_f, saved['pf'], cot, names[:4])
        _, hand_c = hand_pass(fn, saved, '0', net_c, saved['pc'], cot, names[4:])
        hand = [hand_c, hand_f]
    else:
        hand = [hand_pass(fn, saved, '0', net_c, saved['pc'], cot, names)[1]]
    for got, want in zip(grads, hand):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert torch.isfinite(a).all() and torch.equal(a, b), int((a != b).sum())
    assert float(max(g.abs().max() for g in grads[0])) > 0
    if mode == 'bf16x6' and Ni > 0:
        assert paired == 1, 'the one-call backward of two nets pairs the trunk launches, map gradients or not'
    else:
        assert paired == 0


def RG_pair_launches(fn):
    return int(fn._lib.lib().fastnerf_x6_pair_launches())


# ---- 3. against float64 autograd of the oracle ---------------------------------------------------------------------------------
NS, NI, NR = RG.N_SAMPLES, RG.N_IMP, RG.N_RAYS
_E2E = {}


def oracle_maps(sd_c, sd_f, rb, dtype):
    ret = O.render_rays(rb, sd_c, sd_f, NS, NI)
    ret['depth0'] = torch.sum(ret['weights0'] * ret['z0'], -1)      # raw2outputs' depth_map of the coarse pass (render.py:186)
    return ret


def oracle_grads(net_c, net_f, rb, cot, dtype, wrt_rays=False):
    sd_c = {k: v.clone().requires_grad_(True) for k, v in RG.state(net_c, dtype).items()}
    sd_f = {k: v.clone().requires_grad_(True) for k, v in RG.state(net_f, dtype).items()}
    rb = rb.to(dtype).clone().requires_grad_(wrt_rays)
    ret = oracle_maps(sd_c, sd_f, rb, dtype)
    loss = sum((ret[k] * c.to(dtype)).sum() for k, c in cot.items())
    leaves = [rb] if wrt_rays else list(sd_c.values()) + list(sd_f.values())
    return torch.autograd.grad(loss, leaves)


def e2e(fn):
    if not _E2E:
        net_c, net_f = RG.make_net(fn, 31), RG.make_net(fn, 32)
        rb = RG.e2e_batch()[0]
        cot = cotangents(NR, MAPS2, 77)
        p64, p32 = [oracle_grads(net_c, net_f, rb, cot, dt) for dt in (torch.float64, torch.float32)]
        r64, r32 = [oracle_grads(net_c, net_f, rb, cot, dt, wrt_rays=True)[0] for dt in (torch.float64, torch.float32)]
        names = ['c.' + k for k in net_c.state_dict()] + ['f.' + k for k in net_f.state_dict()]
        _E2E.update(net_c=net_c, net_f=net_f, rb=rb.cuda(), cot={k: v.cuda() for k, v in cot.items()}, names=names, p64=p64,
                    pe32=[R.rel_l2(a, b) for a, b in zip(p32, p64)], ref64=r64, e32=RG.group_errors(r32, r64), viewdirs=True)
    return _E2E


@pytest.mark.parametrize('mode', ['fp32', 'bf16x6'])
def test_parameter_gradients_against_float64(fn, math3, compact, mode):
    math3(mode)
    compact('0')
    c = e2e(fn)
    out, _, grads = fused(fn, c['net_c'], c['net_f'], c['rb'], NS, NI, c['cot'])
    assert (out['acc_map'] > 0).all() and (out['acc0'] > 0).all()
    got = grads[0] + grads[1]
    assert len(got) == len(c['p64']) == len(c['names'])      # parameters() order = state_dict order
    errs = [R.rel_l2(a.cpu(), b) for a, b in zip(got, c['p64'])]
    for name, err, e32 in zip(c['names'], errs, c['pe32']):
        print('\nmaps->params %-6s %-26s err %.3e  E32 %.3e  bound %.3e' % (mode, name, err, e32, FACTOR * e32))
    for name, err, e32 in zip(c['names'], errs, c['pe32']):
        assert err <= FACTOR * e32, (mode, name, err, e32)


@pytest.mark.parametrize('mode', ['fp32', 'bf16x6'])
def test_ray_gradients_with_map_cotangents(fn, math3, mode):
    math3(mode)
    c = e2e(fn)
    rb = c['rb'].clone().requires_grad_()
    out, _, grads = fused(fn, c['net_c'], c['net_f'], rb, NS, NI, c['cot'])
    assert rb.grad is not None and rb.grad.shape == (NR, 11) and (rb.grad[:, 6:8] == 0).all()
    RG.check_groups('maps->rays', mode, rb.grad, c)
    # the parameter gradients of this (pass by pass) route are those of the one call, bit for bit
    old = fn.render.get_compact()
    fn.render.set_compact('0')
    try:
        _, _, grads0 = fused(fn, c['net_c'], c['net_f'], c['rb'], NS, NI, c['cot'])
    finally:
        fn.render.set_compact(old)
    assert all(torch.equal(a, b) for x, y in zip(grads, grads0) for a, b in zip(x, y))


def oracle_pose_grad(net_c, net_f, pose, G, dtype):
    pose = pose.clone().requires_grad_(True)
    ro, rd = O.get_rays(RG.H, RG.W, RG.K, pose)
    rb = O.make_ray_batch(ro, rd, 2.0, 6.0).to(dtype)
    ret = O.render_rays(rb, RG.state(net_c, dtype), RG.state(net_f, dtype), NS, NI)
    return torch.autograd.grad((ret['acc_map'] * G.to(dtype)).sum(), pose)[0]


@pytest.mark.parametrize('mode', ['fp32', 'bf16x6'])
def test_pose_gradient_of_an_opacity_loss(fn, math3, mode):
    """The case as the feature's specification sets it.  With these networks every last sample has sigma > 0 and dist = 1e10, so
    acc = 1 - T_end with T_end of order 1e-10 times the transmittance before it: d(acc)/d(pose) is of that order, and float32 autograd
    of the oracle loses it altogether (E32 = 44 for R, 67 for t on MI355X), so this bound cannot fail; the closed form of
    raw2outputs_bwd_full keeps the gradient to 5e-3 / 6e-3 of the float64 value.  test_pose_gradient_of_an_opacity_loss_unsaturated is
    the same check on networks where the bound bites."""
    math3(mode)
    c = e2e(fn)
    pose0 = fn.synthetic.pose_spherical(30.0, -30.0, 4.0)[:3, :4].float().cpu()
    G = torch.randn(RG.H * RG.W, generator=torch.Generator().manual_seed(9))
    if 'pose64' not in c:
        c['pose64'], c['pose32'] = [oracle_pose_grad(c['net_c'], c['net_f'], pose0, G, dt) for dt in (torch.float64, torch.float32)]
    e32 = {'R': R.rel_l2(c['pose32'][:, :3], c['pose64'][:, :3]), 't': R.rel_l2(c['pose32'][:, 3], c['pose64'][:, 3])}
    pose = pose0.clone().requires_grad_()
    _, _, acc, _ = fn.render.render(RG.H, RG.W, RG.K, c2w=pose, ndc=False, network_fn=c['net_c'], network_fine=c['net_f'],
                                    network_query_fn=None, N_samples=NS, N_importance=NI, perturb=0., use_viewdirs=True, near=2., far=6.)
    (acc.reshape(-1) * G.cuda()).sum().backward()
    assert pose.grad is not None and pose.grad.shape == (3, 4) and torch.isfinite(pose.grad).all()
    errs = {'R': R.rel_l2(pose.grad[:, :3], c['pose64'][:, :3]), 't': R.rel_l2(pose.grad[:, 3], c['pose64'][:, 3])}
    for name in errs:
        print('\nacc->pose %-6s %s err %.3e  E32 %.3e  bound %.3e' % (mode, name, errs[name], e32[name], FACTOR * e32[name]))
    for name in errs:
        assert errs[name] <= FACTOR * e32[name], (name, errs[name], e32[name])


# ---- 4. nothing moved ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['fp32', 'bf16x3', 'bf16x6'])
def test_a_colour_loss_makes_the_calls_it_made(fn, math3, compact, mode):
    math3(mode)
    compact('0')
    c = e2e(fn)
    cot = {k: c['cot'][k] for k in ('rgb_map', 'rgb0')}
    _, saved, grads = fused(fn, c['net_c'], c['net_f'], c['rb'], NS, NI, cot)
    n, P1 = NR, NR * (NS + NI)
    ws = torch.empty(fn.ops.dact_floats(P1) + 4 * P1, device='cuda')
    gc, gf = torch.full_like(c['net_c'].flat, float('nan')), torch.full_like(c['net_f'].flat, float('nan'))
    fn.ops.render_rays_bwd(saved['rays11'], saved['white'], cot['rgb_map'], cot['rgb0'], None, None, saved['z0'], saved['raw0'],
                           saved['act0'], saved['z1'], saved['raw1'], saved['act1'], c['net_c'].flat, saved['pc'][1], c['net_f'].flat,
                           saved['pf'][1], ws[fn.ops.dact_floats(P1):], ws, torch.empty(fn.ops.mlp_bwd_partial_floats(), device='cuda'),
                           gc, gf, NS, NI)
    want = [c['net_c'].param_grads_from(gc), c['net_f'].param_grads_from(gf)]
    assert all(torch.equal(a, b) for x, y in zip(grads, want) for a, b in zip(x, y))
    assert n == saved['rays11'].shape[0]


def test_keys_without_retdepth(fn):
    c = e2e(fn)
    kw = dict(N_importance=NI, network_fine=c['net_f'], perturb=0.)
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            assert set(fn.render.render_rays(c['rb'], c['net_c'], None, NS, **kw)) == {'rgb_map', 'disp_map', 'acc_map', 'rgb0', 'disp0', 'acc0', 'z_std'}
            assert set(fn.render.render_rays(c['rb'], c['net_c'], None, NS)) == {'rgb_map', 'disp_map', 'acc_map'}
            full = fn.render.render_rays(c['rb'], c['net_c'], None, NS, retdepth=True, retraw=True, **kw)
            assert set(full) == {'rgb_map', 'disp_map', 'acc_map', 'rgb0', 'disp0', 'acc0', 'z_std', 'depth_map', 'depth0', 'raw'}
            assert full['depth_map'].requires_grad == grad and not full['raw'].requires_grad and not full['z_std'].requires_grad


# ---- 5. the compacted route ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['fp32', 'bf16x3', 'bf16x6'])
def test_compacted_route_with_map_cotangents(fn, math3, compact, mode):
    math3(mode)
    c = e2e(fn)
    res = {}
    for route in ('0', '1'):
        compact(route)
        _, saved, grads = fused(fn, c['net_c'], c['net_f'], c['rb'], NS, NI, c['cot'])
        assert bool(saved['live']) == (route == '1')
        res[route] = torch.cat([g.reshape(-1) for net in grads for g in net])
    diff, scale = float((res['0'] - res['1']).abs().max()), float(res['0'].abs().max())
    print('\ncompacted vs saving %-6s max |diff| %.3e of max %.3e (bound %.3e)' % (mode, diff, scale, 3e-6 * scale))
    assert scale > 0 and diff < 3e-6 * scale
    # dead samples are dead: with every map cotangent set, draw is +-0 in all four components wherever sigma' <= 0
    for k, names in (('1', MAPS2[:4]), ('0', MAPS2[4:])):
        raw = saved['raw' + k].clone()
        kill = (torch.rand(raw.shape[:2], generator=torch.Generator().manual_seed(3 + int(k))) < 0.4).cuda()
        raw[..., 3] = torch.where(kill, -raw[..., 3].abs(), raw[..., 3])                                # 40 % dead, the last sample maybe
        raw[0, :, 3] = -1.0                                                                              # and one ray with no density at all
        rgb, disp, acc, w, depth = fn.ops.raw2outputs_fwd(raw, saved['z' + k], saved['rays11'], None, saved['white'])
        cot = {n_: c['cot'][n_].clone() for n_ in names}
        cot[names[1]][0] = 0.      # (acc == 0 there: a disparity cotangent would rightly give NaN, as the reference's autograd does)
        draw = fn.ops.raw2outputs_bwd_full(raw, saved['z' + k], saved['rays11'], acc, depth, g_rgb=cot[names[0]], g_disp=cot[names[1]],
                                           g_acc=cot[names[2]], g_depth=cot[names[3]], white_bkgd=saved['white'])
        dead = raw[..., 3] <= 0
        assert int(dead.sum()) > 0 and (draw[dead] == 0).all() and torch.isfinite(draw).all()
        assert (draw[~dead][:, 3] != 0).any()


# ---- 6. Trainer ---------------------------------------------------------------------------------------------------------------
LAM_D, LAM_A = 0.25, 0.5


def trainer(fn, loose_on=None, **kw):
    torch.manual_seed(3)
    args = fn.run_nerf.make_args(N_importance=32, N_samples=16, perturb=1.0, white_bkgd=True, no_reload=True, lrate=5e-4, lrate_decay=500)
    ktr = fn.run_nerf.create_nerf(args)[0]
    with torch.no_grad():      # (the lift of make_net: most samples live, every ray with acc > 0)
        for net in (ktr['network_fn'], ktr['network_fine']):
            if loose_on is None:
                net.alpha_linear.bias.add_(0.3)
            else:              # (section 7: half of the coarse samples of the rays `loose_on` dead)
                loosen(net, loose_on, 16)
    K = np.array([[40.0, 0, 16.0], [0, 40.0, 16.0], [0, 0, 1]])
    return fn.run_nerf.Trainer(ktr, 32, 32, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500, **kw)


def batches(fn, steps=3, n=64):
    g = torch.Generator().manual_seed(11)
    c2w = fn.synthetic.pose_spherical(20.0, -30.0, 4.0)[:3, :4]
    K = np.array([[40.0, 0, 16.0], [0, 40.0, 16.0], [0, 0, 1]])
    ro, rd = fn.run_nerf_helpers.get_rays(32, 32, K, c2w)
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    out = []
    for _ in range(steps):
        sel = torch.randint(0, 1024, (n,), generator=g).cuda()
        depth = 2 + 4 * torch.rand(n, generator=g)
        dw = (torch.rand(n, generator=g) > 0.3).float()
        depth[dw == 0] = float('nan')                      # sparse depth: NaN where unknown, weight 0
        aux = dict(depth=depth.cuda(), depth_weight=dw.cuda(), acc=(torch.rand(n, generator=g) > 0.4).float().cuda(),
                   acc_weight=(0.5 + torch.rand(n, generator=g)).cuda())
        out.append(((ro[sel].contiguous(), rd[sel].contiguous(), torch.rand(n, 3, generator=g).cuda()), aux))
    return out


def phased_step(fn, tr, b, aux, **kw):
    """Trainer.step's fused route with every phase in a call of its own (_phased_step of tests/test_gpu_trunk_pair.py, with the keywords)."""
    L = fn._lib
    tr.adam_t += 1
    a, out, loss2, live = tr._fused_prepare(*b, None, None, 0, None, None, kw.get('n_global'), **aux)
    a.lr, a.adam_t = float(tr.lr), int(tr.adam_t)
    for phase in (L.STEP_FORWARD, L.STEP_BWD_FINE, L.STEP_BWD_COARSE, L.STEP_UPDATE):
        tr._fused_call(a, phase)
    tr._after_backward(live)
    return loss2, out


def run(fn, route='fused', use_aux=True, steps=3, keep_grad=False, **kw):
    """-> (parameters, losses [steps, 2], aux losses [steps, 4], gradient of the last step, the Trainer) after `steps` steps."""
    step_kw = {k: kw.pop(k) for k in ('n_global',) if k in kw}
    old = os.environ.get('FASTNERF_FUSED_STEP')
    if route == 'calls':
        os.environ['FASTNERF_FUSED_STEP'] = '0'      # read by the constructor
    try:
        tr = trainer(fn, **kw)
    finally:
        os.environ.pop('FASTNERF_FUSED_STEP', None)
        if old is not None:
            os.environ['FASTNERF_FUSED_STEP'] = old
    assert tr.fused == (route != 'calls') and tr.world == 1
    torch.manual_seed(5)
    losses, aux4 = [], []
    for b, aux in batches(fn, steps):
        aux = aux if use_aux else {}
        loss2, _ = phased_step(fn, tr, b, aux, **step_kw) if route == 'phased' else tr.step(*b, decay=False, **step_kw, **aux)
        losses.append(loss2.clone())
        aux4.append(tr.aux_losses.clone())
    torch.cuda.synchronize()
    return tr.flat.clone(), torch.stack(losses), torch.stack(aux4), tr.grad.clone(), tr


@pytest.mark.parametrize('mode', ['bf16x6', 'fp32'])
@pytest.mark.parametrize('route', ['0', '1'], ids=['saving', 'compacted'])
def test_trainer_unchanged_without_terms(fn, math3, compact, mode, route):
    """(a) targets with lambda = 0, or lambdas without targets: the step of a Trainer built without the keywords, bit for bit."""
    math3(mode)
    compact(route)
    base = run(fn, use_aux=False)
    for what, res in (('lambda = 0', run(fn, use_aux=True)), ('no targets', run(fn, use_aux=False, lambda_depth=LAM_D, lambda_acc=LAM_A))):
        assert torch.equal(res[0], base[0]) and torch.equal(res[1], base[1]) and torch.equal(res[3], base[3]), what
        assert (res[2] == 0).all(), what


@pytest.mark.parametrize('mode', ['bf16x6', 'fp32', 'bf16x3'])
@pytest.mark.parametrize('route', ['0', '1'], ids=['saving', 'compacted'])
def test_trainer_routes_agree_bit_for_bit(fn, math3, compact, mode, route):
    """(b) both terms on: the fused step, the phase-by-phase step and the call-by-call step; (e) n_global = 2 n halves the gradient."""
    math3(mode)
    compact(route)
    kw = dict(lambda_depth=LAM_D, lambda_acc=LAM_A)
    base = run(fn, use_aux=False)
    res = {r: run(fn, route=r, **kw) for r in ('fused', 'phased', 'calls')}
    for r in ('phased', 'calls'):
        for x, y, what in zip(res['fused'][:4], res[r][:4], ('parameters', 'loss2', 'aux_losses', 'gradient')):
            assert torch.equal(x, y), (r, what)
    f = res['fused']
    assert torch.isfinite(f[0]).all() and torch.isfinite(f[2]).all() and (f[2] > 0).all() and f[4].last_step_live == (route == '1')
    assert not torch.equal(f[0], base[0]) and torch.equal(f[1][0], base[1][0]), 'the terms train; the first forward is the same'
    one = run(fn, steps=1, **kw)
    half = run(fn, steps=1, n_global=128, **kw)
    assert torch.equal(half[3] * 2, one[3]) and torch.equal(half[2], one[2]) and float(one[3].abs().max()) > 0


def test_trainer_gradient_against_float64(fn, math3, compact):
    """(c) one step's gradient of the total loss against float64 autograd of the oracle, per parameter tensor, 16 x E32."""
    compact('0')
    (b, aux), = batches(fn, 1)
    t_rand, u = torch.rand(64, 16, generator=torch.Generator().manual_seed(1)), torch.rand(64, 32, generator=torch.Generator().manual_seed(2))
    tr = trainer(fn, lambda_depth=LAM_D, lambda_acc=LAM_A)
    sds = {dt: [RG.state(tr.net_c, dt), RG.state(tr.net_f, dt)] for dt in (torch.float64, torch.float32)}
    names = ['c.' + k for k in sds[torch.float64][0]] + ['f.' + k for k in sds[torch.float64][1]]

    def oracle(dt):
        sd_c, sd_f = [{k: v.clone().requires_grad_(True) for k, v in sd.items()} for sd in sds[dt]]
        rb = O.make_ray_batch(b[0].cpu(), b[1].cpu(), 2.0, 6.0).to(dt)
        ret = O.render_rays(rb, sd_c, sd_f, 16, 32, white_bkgd=True, t_rand=t_rand.to(dt), u=u.to(dt))
        ret['depth0'] = torch.sum(ret['weights0'] * ret['z0'], -1)
        cpu = {k: v.cpu() for k, v in aux.items()}
        loss4, _ = A.aux_loss(ret['depth_map'], ret['acc_map'], ret['depth0'], ret['acc0'], cpu['depth'], cpu['depth_weight'], cpu['acc'],
                              cpu['acc_weight'], dtype=dt)
        loss2 = torch.stack([O.img2mse(ret['rgb_map'], b[2].cpu().to(dt)), O.img2mse(ret['rgb0'], b[2].cpu().to(dt))])
        return torch.autograd.grad(A.total(loss2, loss4, LAM_D, LAM_A), list(sd_c.values()) + list(sd_f.values())), loss2, loss4
    (g64, l2, l4), (g32, _, _) = oracle(torch.float64), oracle(torch.float32)
    res = {}
    for mode in ('fp32', 'bf16x6'):
        math3(mode)
        tr = trainer(fn, lambda_depth=LAM_D, lambda_acc=LAM_A)
        loss2, _ = tr.step(*b, t_rand=t_rand.cuda(), u=u.cuda(), decay=False, **aux)
        got = tr.net_c.param_grads_from(tr.grad[:fn.ops.NET_PARAMS]) + tr.net_f.param_grads_from(tr.grad[fn.ops.NET_PARAMS:])
        res[mode] = [R.rel_l2(a.cpu(), r) for a, r in zip(got, g64)]
        print('\ntrainer %-6s loss2 %s (float64 %s)  aux_losses %s (float64 %s)' % (mode, loss2.tolist(), l2.tolist(), tr.aux_losses.tolist(), l4.tolist()))
        assert torch.allclose(tr.aux_losses.cpu().double(), l4.detach(), rtol=1e-4, atol=1e-7) and torch.allclose(loss2.cpu().double(), l2.detach(), rtol=1e-4)
    e32 = [R.rel_l2(a, r) for a, r in zip(g32, g64)]
    for mode, errs in res.items():
        for name, err, e in zip(names, errs, e32):
            print('\ntrainer->params %-6s %-26s err %.3e  E32 %.3e  bound %.3e' % (mode, name, err, e, FACTOR * e))
    for mode, errs in res.items():
        for name, err, e in zip(names, errs, e32):
            assert err <= FACTOR * e, (mode, name, err, e)


@pytest.mark.parametrize('mode', ['bf16x6', 'fp32'])
def test_trainer_through_an_occupancy_grid(fn, math3, compact, mode):
    """(d) both terms on: live <= occupied on both passes with a slab of cells cleared by hand; a full grid is the compacted step."""
    math3(mode)
    compact('1')
    kw = dict(lambda_depth=LAM_D, lambda_acc=LAM_A)
    G = fn.occupancy.OccupancyGrid
    plain = run(fn, **kw)
    full = run(fn, occupancy=G.for_training(N=16, bound=4.5), occupancy_warmup=10 ** 9, **kw)
    for x, y, what in zip(plain[:4], full[:4], ('parameters', 'loss2', 'aux_losses', 'gradient')):
        assert torch.equal(x, y), what
    assert torch.equal(plain[4].live_counts, full[4].live_counts)
    mask = torch.ones(16, 16, 16, dtype=torch.bool, device='cuda')
    mask[:, :, 5:11] = False
    res = run(fn, occupancy=G.from_mask(mask, -4.5, 4.5, outside_occupied=False), **kw)
    live, occ = res[4].live_counts.tolist(), res[4].occupancy_counts.tolist()      # (live, total) fine, coarse; (occupied, total) coarse, fine
    print('\noccupancy %-6s live %s occupied %s' % (mode, live, occ))
    assert 0 < occ[0] < occ[1] and 0 < occ[2] < occ[3], 'the slab removes samples, and leaves some'
    assert live[0] <= occ[2] and live[2] <= occ[0] and live[1] == occ[3] and live[3] == occ[1]
    assert torch.isfinite(res[0]).all() and torch.isfinite(res[2]).all()


def test_empty_shard(fn):
    tr = trainer(fn, lambda_depth=LAM_D, lambda_acc=LAM_A)
    e3, e1 = torch.empty(0, 3, device='cuda'), torch.empty(0, device='cuda')
    before = tr.flat.clone()
    loss2, out = tr.step(e3, e3, e3, depth=e1, depth_weight=e1, acc=e1, acc_weight=e1, n_global=64)
    assert (loss2 == 0).all() and out == {} and tr.aux_losses.shape == (4,) and (tr.aux_losses == 0).all()
    assert torch.equal(tr.flat, before) and int(tr.grad.count_nonzero()) == 0


# ---- 7. the opacity gradient on its own: unsaturated rays, dead samples, one shared network -------------------------------------
GAIN = 4.0
# N_importance - 1 = 9 shares no factor with the N_samples - 2 = 14 bins of sample_pdf: a ray without coarse density has a uniform
# pdf, and with perturb = 0 a shared factor would put fine samples exactly on bin edges, where float32 and float64 choose differently
LNS, LNI, LNR = 16, 10, 8
ACC_ONLY = ('acc_map', 'acc0')
NO_DISP = ('rgb_map', 'acc_map', 'depth_map', 'rgb0', 'acc0', 'depth0')
_LOOSE = {}


def loosen(net, rb, S, gain=GAIN):
    """Steepen the density head of `net` by `gain` and centre it on the rays `rb`: the bias is moved to the midpoint of the two
    middle density logits (float64 oracle) of the S unperturbed coarse samples of every ray, so half of them are dead and none sits
    on the kink of the relu."""
    with torch.no_grad():
        net.alpha_linear.weight.mul_(gain)
        rb = rb.detach().cpu().double()
        z = O.coarse_z(rb[:, 6:7], rb[:, 7:8], S)
        pts = rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]
        v = O.run_network(RG.state(net, torch.float64), pts, rb[:, 8:11])[..., 3].reshape(-1).sort().values
        k = v.numel() // 2
        net.alpha_linear.bias.sub_(float(0.5 * (v[k - 1] + v[k])))
    return net


def new_net(fn, seed):
    torch.manual_seed(seed)
    return fn.model.NeRF(use_viewdirs=True, input_ch_views=27)


def pose_rays(pose):
    ro, rd = O.get_rays(RG.H, RG.W, RG.K, pose)
    return O.make_ray_batch(ro, rd, 2.0, 6.0)


def loose_grads(c, names, dtype, wrt_rays=False, shared=False):
    """Float64 / float32 autograd of the oracle for the loss sum_k <map_k, cot_k> over `names`, w.r.t. the parameters or the rays."""
    sd_c = {k: v.clone().requires_grad_(True) for k, v in RG.state(c['net_c'], dtype).items()}
    sd_f = None if shared else {k: v.clone().requires_grad_(True) for k, v in RG.state(c['net_f'], dtype).items()}
    rb = c['rb'].cpu().to(dtype).clone().requires_grad_(wrt_rays)
    ret = O.render_rays(rb, sd_c, sd_f, LNS, LNI)
    ret['depth0'] = torch.sum(ret['weights0'] * ret['z0'], -1)
    loss = sum((ret[k] * c['cot'][k].cpu().to(dtype)).sum() for k in names)
    leaves = [rb] if wrt_rays else list(sd_c.values()) + ([] if shared else list(sd_f.values()))
    return [torch.zeros_like(x) if g is None else g for x, g in zip(leaves, torch.autograd.grad(loss, leaves, allow_unused=True))]


def loose(fn):
    """Two loosened networks, eight rays, cotangents for every map; the oracle's gradients are added by the tests that need them."""
    if not _LOOSE:
        gen = torch.Generator().manual_seed(121)
        rb = O.make_ray_batch(torch.randn(LNR, 3, generator=gen) * 0.4, torch.randn(LNR, 3, generator=gen), 2.0, 6.0)
        pose = O.pose_spherical(30.0, -30.0, 4.0)[:3, :4].float()
        on = torch.cat([rb, pose_rays(pose).detach()])      # (centred on the rays of both uses)
        net_c, net_f = loosen(new_net(fn, 31), on, LNS), loosen(new_net(fn, 32), on, LNS)
        names = ['c.' + k for k in net_c.state_dict()] + ['f.' + k for k in net_f.state_dict()]
        _LOOSE.update(net_c=net_c, net_f=net_f, rb=rb.cuda(), pose=pose, names=names, cot={k: v.cuda() for k, v in cotangents(LNR, MAPS2, 78).items()})
    return _LOOSE


def oracle_of(c, key, names, **kw):
    """(float64 gradients, E32 per tensor) of loose_grads, computed once."""
    if key not in c:
        g64, g32 = [loose_grads(c, names, dt, **kw) for dt in (torch.float64, torch.float32)]
        c[key] = (g64, [R.rel_l2(a, b) if float(b.norm()) > 0 else 0.0 for a, b in zip(g32, g64)])
    return c[key]


def assert_unsaturated(acc_maps, raws, least=3):
    """On the forward's own outputs: rays with acc well inside (0, 1), dead and live samples, rays that end on a dead sample."""
    for acc, raw in zip(acc_maps, raws):
        inside = int(((acc > 0.02) & (acc < 0.98)).sum())
        dead = raw[..., 3] <= 0
        assert inside >= least and bool(dead.any()) and bool((~dead).any()) and bool(dead[:, -1].any()), (inside, int(dead.sum()))


def check_tensors(what, mode, got, names, g64, e32):
    errs = [R.rel_l2(a.cpu(), r) if float(r.norm()) > 0 else float(a.abs().max()) for a, r in zip(got, g64)]
    for name, err, e in zip(names, errs, e32):
        print('\n%s %-6s %-26s err %.3e  E32 %.3e  bound %.3e' % (what, mode, name, err, e, FACTOR * e))
    for name, a, err, e in zip(names, got, errs, e32):
        assert torch.isfinite(a).all() and err <= FACTOR * e, (what, mode, name, err, e)      # (a zero reference: exactly zero)


@pytest.mark.parametrize('mode', ['fp32', 'bf16x6'])
def test_opacity_gradient_alone_against_float64(fn, math3, compact, mode):
    """Cotangents on acc_map and acc0 alone, rays that are not saturated.  What the reference must give for the check to bite is
    asserted first: on every tensor of the density path the opacity gradient is at least a tenth of the colour gradient and 16 x E32 is
    below 0.5, so a gradient that is dropped (error 1), negated (2) or given to the other pass fails; the colour branch gets exactly 0."""
    math3(mode)
    compact('0')
    c = loose(fn)
    g64, e32 = oracle_of(c, 'acc64', ACC_ONLY)
    col64, _ = oracle_of(c, 'col64', ('rgb_map', 'rgb0'))
    path = [float(g.norm()) > 0 for g in g64]
    assert sum(path) == 36, 'eight trunk layers and the density head of both networks'
    for name, on, g, gc, e in zip(c['names'], path, g64, col64, e32):
        assert not on or (float(g.norm()) >= 0.1 * float(gc.norm()) and FACTOR * e < 0.5), (name, float(g.norm()), float(gc.norm()), e)
    out, saved, grads = fused(fn, c['net_c'], c['net_f'], c['rb'], LNS, LNI, {k: c['cot'][k] for k in ACC_ONLY})
    assert_unsaturated((out['acc_map'], out['acc0']), (saved['raw1'], saved['raw0']))
    check_tensors('acc->params', mode, grads[0] + grads[1], c['names'], g64, e32)


@pytest.mark.parametrize('mode', ['fp32', 'bf16x6'])
def test_opacity_gradient_alone_reaches_rays_and_pose(fn, math3, mode):
    """The same loss w.r.t. the rays (origins and directions: the opacity does not depend on the view direction, whose gradient is
    exactly 0) and, through render(c2w=pose) with one pass, w.r.t. a pose -- the pose check of section 3 on a network where its bound can fail."""
    math3(mode)
    c = loose(fn)
    r64, _ = oracle_of(c, 'acc_rays64', ACC_ONLY, wrt_rays=True)
    r32 = loose_grads(c, ACC_ONLY, torch.float32, wrt_rays=True)[0]
    rb = c['rb'].clone().requires_grad_()
    fused(fn, c['net_c'], c['net_f'], rb, LNS, LNI, {k: c['cot'][k] for k in ACC_ONLY})
    assert torch.isfinite(rb.grad).all() and (rb.grad[:, 6:] == 0).all() and (r64[0][:, 8:] == 0).all()
    for name, sl in RG.GROUPS[:2]:
        err, e = R.rel_l2(rb.grad[:, sl].cpu(), r64[0][:, sl]), R.rel_l2(r32[:, sl], r64[0][:, sl])
        print('\nacc->rays %-6s %-2s err %.3e  E32 %.3e  bound %.3e' % (mode, name, err, e, FACTOR * e))
        assert FACTOR * e < 0.5 and err <= FACTOR * e, (name, err, e)
    G = torch.randn(RG.H * RG.W, generator=torch.Generator().manual_seed(9))

    def oracle_pose(dt):      # (one pass: the float32 oracle places the fine samples of a ray without density too loosely for the rule to bite)
        pose = c['pose'].clone().requires_grad_(True)
        ret = O.render_rays(pose_rays(pose).to(dt), RG.state(c['net_c'], dt), None, LNS, 0)
        return torch.autograd.grad((ret['acc_map'] * G.to(dt)).sum(), pose)[0]
    if 'pose64' not in c:
        c['pose64'], c['pose32'] = oracle_pose(torch.float64), oracle_pose(torch.float32)
    pose = c['pose'].clone().requires_grad_()
    _, _, acc, extras = fn.render.render(RG.H, RG.W, RG.K, c2w=pose, ndc=False, network_fn=c['net_c'], network_fine=None, retraw=True,
                                         network_query_fn=None, N_samples=LNS, N_importance=0, perturb=0., use_viewdirs=True, near=2., far=6.)
    assert_unsaturated((acc.reshape(-1),), (extras['raw'].reshape(RG.H * RG.W, LNS, 4),))
    (acc.reshape(-1) * G.cuda()).sum().backward()
    assert pose.grad is not None and pose.grad.shape == (3, 4) and torch.isfinite(pose.grad).all()
    for name, sl in (('R', slice(0, 3)), ('t', 3)):
        err, e = R.rel_l2(pose.grad[:, sl], c['pose64'][:, sl]), R.rel_l2(c['pose32'][:, sl], c['pose64'][:, sl])
        print('\nacc->pose (unsaturated) %-6s %s err %.3e  E32 %.3e  bound %.3e' % (mode, name, err, e, FACTOR * e))
        assert FACTOR * e < 0.5 and err <= FACTOR * e, (name, err, e)


@pytest.mark.parametrize('mode', ['fp32', 'bf16x3', 'bf16x6'])
def test_compacted_route_over_dead_samples(fn, math3, compact, mode):
    """Section 5 on networks that leave dead samples out of the live lists: colour, opacity and depth cotangents on both passes."""
    math3(mode)
    c = loose(fn)
    cot = {k: c['cot'][k] for k in NO_DISP}
    res = {}
    for route in ('0', '1'):
        compact(route)
        out, saved, grads = fused(fn, c['net_c'], c['net_f'], c['rb'], LNS, LNI, cot)
        assert bool(saved['live']) == (route == '1')
        assert_unsaturated((out['acc_map'], out['acc0']), (saved['raw1'], saved['raw0']))
        res[route] = torch.cat([g.reshape(-1) for net in grads for g in net])
    diff, scale = float((res['0'] - res['1']).abs().max()), float(res['0'].abs().max())
    print('\ncompacted vs saving, dead samples %-6s max |diff| %.3e of max %.3e (bound %.3e)' % (mode, diff, scale, 3e-6 * scale))
    assert scale > 0 and torch.isfinite(res['1']).all() and diff < 3e-6 * scale


@pytest.mark.parametrize('mode', ['fp32', 'bf16x3', 'bf16x6'])
def test_shared_network_route_with_map_cotangents(fn, math3, compact, mode):
    """N_importance > 0 without network_fine: the fine pass's gradient is added to the coarse pass's.  Bit for bit the sum of the two
    hand passes of section 2, and within 16 x E32 of float64 autograd of the oracle run with one network."""
    math3(mode)
    compact('0')
    c = loose(fn)
    cot = {k: c['cot'][k] for k in NO_DISP}
    out, saved, grads = fused(fn, c['net_c'], None, c['rb'], LNS, LNI, cot)
    assert saved['net_f'] is c['net_c'] and all(out[k].requires_grad for k in MAPS2)
    assert_unsaturated((out['acc_map'], out['acc0']), (saved['raw1'], saved['raw0']))
    hand_cot = dict(cot, disp_map=None, disp0=None)
    _, hand_f = hand_pass(fn, saved, '1', c['net_c'], saved['pf'], hand_cot, MAPS2[:4])
    _, hand_c = hand_pass(fn, saved, '0', c['net_c'], saved['pc'], hand_cot, MAPS2[4:])
    assert len(grads) == 1 and len(grads[0]) == len(hand_c)
    for a, x, y in zip(grads[0], hand_c, hand_f):
        assert torch.isfinite(a).all() and torch.equal(a, x + y), int((a != x + y).sum())
    if mode != 'bf16x3':
        g64, e32 = oracle_of(c, 'shared64', NO_DISP, shared=True)
        check_tensors('shared net', mode, grads[0], c['names'][:len(g64)], g64, e32)


LAM_ALONE = 4.0


def test_trainer_opacity_term_alone_against_float64(fn, math3, compact):
    """One step with lambda_acc alone on loosened networks, against float64 autograd of the oracle.  `share` is the part of a
    tensor's float64 gradient that the opacity term contributes; the reference is asserted to give 16 x E32 < share on every tensor
    of the density path, so a step that drops the term, or hands a pass the other pass's gradient, fails."""
    compact('0')
    (b, aux), = batches(fn, 1)
    aux = {k: aux[k] for k in ('acc', 'acc_weight')}
    on = O.make_ray_batch(b[0].cpu(), b[1].cpu(), 2.0, 6.0)
    t_rand, u = torch.rand(64, 16, generator=torch.Generator().manual_seed(1)), torch.rand(64, 32, generator=torch.Generator().manual_seed(2))
    tr = trainer(fn, loose_on=on, lambda_acc=LAM_ALONE)
    sds = {dt: [RG.state(tr.net_c, dt), RG.state(tr.net_f, dt)] for dt in (torch.float64, torch.float32)}
    names = ['c.' + k for k in sds[torch.float64][0]] + ['f.' + k for k in sds[torch.float64][1]]

    def oracle(dt, lam):
        sd_c, sd_f = [{k: v.clone().requires_grad_(True) for k, v in sd.items()} for sd in sds[dt]]
        ret = O.render_rays(on.to(dt), sd_c, sd_f, 16, 32, white_bkgd=True, t_rand=t_rand.to(dt), u=u.to(dt))
        loss4, _ = A.aux_loss(None, ret['acc_map'], None, ret['acc0'], None, None, aux['acc'].cpu(), aux['acc_weight'].cpu(), dtype=dt)
        loss2 = torch.stack([O.img2mse(ret['rgb_map'], b[2].cpu().to(dt)), O.img2mse(ret['rgb0'], b[2].cpu().to(dt))])
        return torch.autograd.grad(A.total(loss2, loss4, 0., lam), list(sd_c.values()) + list(sd_f.values())), loss4
    (g64, l4), (col64, _), (g32, _) = oracle(torch.float64, LAM_ALONE), oracle(torch.float64, 0.), oracle(torch.float32, LAM_ALONE)
    e32 = [R.rel_l2(a, r) for a, r in zip(g32, g64)]
    share = [float((a - r).norm() / a.norm()) for a, r in zip(g64, col64)]
    for name, s, e in zip(names, share, e32):
        print('\ntrainer acc alone %-26s share %.3e  E32 %.3e' % (name, s, e))
    assert sum(s > 1e-6 for s in share) == 36 and all(FACTOR * e < s for s, e in zip(share, e32) if s > 1e-6)
    for mode in ('fp32', 'bf16x6'):
        math3(mode)
        tr = trainer(fn, loose_on=on, lambda_acc=LAM_ALONE)
        _, out = tr.step(*b, t_rand=t_rand.cuda(), u=u.cuda(), decay=False, **aux)
        assert_unsaturated((out['acc_map'], out['acc0']), (out['raw'], out['raw']), least=16)
        assert tr.aux_losses[0] == 0 and tr.aux_losses[1] == 0, 'no depth term'
        assert torch.allclose(tr.aux_losses.cpu().double(), l4.detach(), rtol=1e-4, atol=1e-7)
        got = tr.net_c.param_grads_from(tr.grad[:fn.ops.NET_PARAMS]) + tr.net_f.param_grads_from(tr.grad[fn.ops.NET_PARAMS:])
        check_tensors('trainer acc alone', mode, got, names, g64, e32)


# ---- 8. the saved tensors live no longer than the graph ------------------------------------------------------------------------
@pytest.mark.parametrize('rays', [False, True], ids=['params', 'rays'])
def test_saved_activations_are_freed_with_the_outputs(fn, compact, rays):
    """No output of the autograd node is kept among its saved tensors (acc / depth are saved as detached aliases), so the graph holds
    no reference cycle: with the cyclic collector off, the saved activations die with the last output."""
    import gc
    import weakref
    compact('0')
    c = e2e(fn)
    was = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        rb = c['rb'].clone().requires_grad_(rays)
        out = fn.render.render_rays(rb, c['net_c'], None, NS, N_importance=NI, network_fine=c['net_f'], perturb=0., retdepth=True)
        node = out['acc_map'].grad_fn
        assert type(node).__name__.startswith('_RenderRaysRayGradFn' if rays else '_RenderRaysFn')
        refs = [weakref.ref(node.saved[k]) for k in ('act0', 'act1', 'acc1', 'depth0')]
        assert all(r() is not None for r in refs)
        for k in MAPS2:
            assert node.saved.get(k) is not out[k]
        (out['acc_map'].sum() + out['depth0'].sum()).backward()
        del out, node
        assert all(r() is None for r in refs), 'the saved tensors outlived the outputs'
    finally:
        if was:
            gc.enable()
