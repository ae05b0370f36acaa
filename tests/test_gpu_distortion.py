"""The distortion loss on the GPU (include/fastnerf.h, "distortion loss"): fastnerf_distortion against the float64 definition
(tests/distortion_ref.py), through the compositing backward, through render_rays(retdist=True) on both routes, and through the fused,
grid, marched and call-by-call steps of Trainer(lambda_dist=).

Bounds.
  1. Kernel: with its fp32 inputs taken as exact, l and every dl/dw_i above 1e-30 within (2 S + 32) 2^-24 relative of float64 -- two
     nested sums of at most S non-negative terms plus the per-term products; derived, not tuned (tests/test_distortion_cpu.py shows the
     textbook prefix form missing it 26- to 58-fold on the clustered fixture).  With coef and g_up the reference is coef * g_up * dl/dw in
     float64 on the fp32 values of coef and g_up.  Two calls are bit-identical; the edge cases are exact.
  2. The batch mean: float64 mean of its own fp32 inputs to 2^-22 relative (one rounding on the store is 2^-24).
  3. Through the compositing: check() of tests/test_gpu_raw2outputs_grad.py, the bound of its `weights` cotangent.
  4. Through the networks: relative L2 per parameter tensor <= 16 x E32 for 'fp32' and 'bf16x6' (tests/test_gpu_aux_maps.py); all three
     modes are pinned bit for bit to their parts called by hand; compacted against saving route: its 3e-6 of the largest gradient;
     torch-network route against fused route: the 2e-3 per tensor of tests/test_gpu_custom_network.py.
  5. Steps: bit for bit.
Every figure is printed before it is asserted (pytest -s)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import distortion_ref as D
import test_gpu_aux_maps as AM
import test_gpu_custom_network as CN
import test_gpu_march_train as MT
import test_gpu_ray_grad as RG
import test_gpu_raw2outputs_grad as RO
import test_ray_grad_cpu as R
import march_numpy as M
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32


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


def rays11_of(near, far, seed=0):
    n = len(near)
    r = np.random.default_rng(seed).standard_normal((n, 11)).astype(F32)
    r[:, 6], r[:, 7] = near, far
    return torch.from_numpy(r).cuda()


def kernel(fn, w, z, near, far, **kw):
    kw = {k: (torch.from_numpy(np.asarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    ell, g = fn.ops.distortion(torch.from_numpy(w).cuda(), torch.from_numpy(z).cuda(), rays11_of(near, far), **kw)
    torch.cuda.synchronize()
    return (None if ell is None else ell.cpu().numpy()), (None if g is None else g.cpu().numpy())


def assert_bar(what, S, ell, g, ell64, g64):
    e_l, e_g = D.rel_err(ell, ell64), D.rel_err(g, g64)
    print('\n%s: l %.1f, g %.1f x 2^-24 (bar %d)' % (what, e_l * 2 ** 24, e_g * 2 ** 24, 2 * S + 32))
    assert np.isfinite(ell).all() and np.isfinite(g).all()
    assert e_l <= D.bar(S) and e_g <= D.bar(S), (what, e_l, e_g, D.bar(S))
    small = np.abs(g64) <= 1e-30      # (outside the relative bar: still tiny)
    assert (np.abs(g[small]) <= 1e-29).all()


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lindisp', [False, True])
@pytest.mark.parametrize('S', [2, 3, 63, 64, 65, 192, 512])
def test_kernel_against_float64(fn, S, lindisp):
    n = 257
    fixtures = [('uniform', D.uniform_fixture(n, S, 10 + S, lindisp))]
    if S == 192:
        fixtures.append(('clustered', D.clustered_fixture(n, 11, lindisp)))
    for name, (w, z, near, far) in fixtures:
        assert w.shape == (n, S)
        ell64, g64 = D.distortion_ref(w, z, near, far, lindisp)
        ell, g = kernel(fn, w, z, near, far, lindisp=lindisp)
        ell2, g2 = kernel(fn, w, z, near, far, lindisp=lindisp)
        assert np.array_equal(ell.view(np.int32), ell2.view(np.int32)) and np.array_equal(g.view(np.int32), g2.view(np.int32)), 'two calls, same bits'
        assert_bar('%s S=%d lindisp=%d' % (name, S, lindisp), S, ell, g, ell64, g64)
        assert (ell >= 0).all() and (ell > 0).any() and (g >= 0).all()
        # one output at a time: the same bits
        only_l, none = kernel(fn, w, z, near, far, lindisp=lindisp, want=('ell',))
        none2, only_g = kernel(fn, w, z, near, far, lindisp=lindisp, want=('g_w',))
        assert none is None and none2 is None and np.array_equal(only_l, ell) and np.array_equal(only_g, g)
        # coef and g_up: g_w = coef * g_up[r] * dl/dw (l itself is not scaled); skip: l = +0 and a row of +0, the other rows untouched
        rng = np.random.default_rng(S)
        g_up = rng.standard_normal(n).astype(F32)
        coef = float(F32(0.37 / n))
        skip = (rng.uniform(size=n) < 0.25).astype(np.uint8)
        skip[0], skip[1] = 1, 0
        ell_s, g_s = kernel(fn, w, z, near, far, lindisp=lindisp, coef=coef, g_up=g_up, skip=skip)
        want = coef * g_up.astype(np.float64)[:, None] * g64
        keep = skip == 0
        assert_bar('%s S=%d lindisp=%d coef, g_up, skip' % (name, S, lindisp), S, ell_s[keep], g_s[keep], ell64[keep], want[keep])
        assert np.array_equal(ell_s[keep].view(np.int32), ell[keep].view(np.int32))
        assert (ell_s[~keep].view(np.int32) == 0).all() and (g_s[~keep].view(np.int32) == 0).all(), 'a skipped ray: +0, bit for bit'


def test_kernel_past_one_grid_and_the_batch_mean(fn):
    """16389 rays: the launch is capped at 4096 blocks of 4 rays, so every wave takes a second ray and five a third.  The mean of l over
    the batch: one workgroup, fixed order, fp64."""
    n, S = 16389, 5
    w, z, near, far = D.uniform_fixture(n, S, 3)
    ell64, g64 = D.distortion_ref(w, z, near, far)
    ell, g = kernel(fn, w, z, near, far)
    assert_bar('n=%d S=%d' % (n, S), S, ell, g, ell64, g64)
    e1, e0 = torch.from_numpy(ell).cuda(), torch.from_numpy(ell[::-1].copy()).cuda() * 0.5
    a, b = fn.ops.distortion_mean(e1, e0), fn.ops.distortion_mean(e1, e0)
    one = fn.ops.distortion_mean(e1)
    torch.cuda.synchronize()
    assert a.shape == (2,) and torch.equal(bits(a), bits(b)), 'two runs, same bits'
    assert torch.equal(bits(one[:1]), bits(a[:1])) and int(bits(one)[1]) == 0, 'without the coarse pass: the same mean, and +0'
    want = [float(ell.astype(np.float64).mean()), float((ell.astype(np.float64) * 0.5).mean())]
    errs = [abs(float(a[i]) - want[i]) / want[i] for i in (0, 1)]
    print('\nbatch mean n=%d: rel err %.2e, %.2e (bar %.2e)' % (n, errs[0], errs[1], 2.0 ** -22))
    assert max(errs) <= 2.0 ** -22


def test_kernel_edge_cases_are_exact(fn):
    n, S = 12, 67
    w, z, near, far = D.uniform_fixture(n, S, 4)
    far[0] = near[0]                 # an empty span
    far[1] = near[1] - 1             # a negative one
    far[2] = np.inf
    near[3] = np.nan
    far[4] = np.nan
    w[5] = 0                         # all-zero weights
    z[6] = z[6, 0]                   # repeated depths
    z[7, 20:40] = z[7, 20]
    w[8, 1::2] = 0                   # every other sample dead
    dead = [0, 1, 2, 3, 4]
    for coef in (1.0, -2.0):
        ell, g = kernel(fn, w, z, near, far, coef=coef)
        ell64, g64 = D.distortion_ref(w, z, near, far)
        assert (ell[dead].view(np.int32) == 0).all() and (g[dead].view(np.int32) == 0).all(), 'no positive finite span: l = +0, a row of +0'
        assert ell[5].view(np.int32) == 0 and (g[5].view(np.int32) == 0).all(), 'zero weights: +0 throughout'
        live = [6, 7, 8, 9, 10, 11]
        assert_bar('edge cases coef=%g' % coef, S, ell[live], g[live], ell64[live], coef * g64[live])
    # lindisp: near = 0 has no finite disparity span
    wl, zl, nl, fl = D.uniform_fixture(4, S, 5, lindisp=True)
    nl[1] = 0
    ell, g = kernel(fn, wl, zl, nl, fl, lindisp=True)
    assert ell[1].view(np.int32) == 0 and (g[1].view(np.int32) == 0).all() and (ell[[0, 2, 3]] > 0).all()
    # S = 1: one interval [z_0, far], l = w^2 delta / 3
    ell, g = kernel(fn, w[:, :1].copy(), z[:, :1].copy(), near, far)
    ell64, g64 = D.distortion_ref(w[:, :1], z[:, :1], near, far)
    assert_bar('S=1', 1, ell[8:], g[8:], ell64[8:], g64[8:])


def test_kernel_on_a_marched_row(fn):
    """Packed rows of grid.march: runs of live lattice points, each closed by an entry that ends the last live interval, then padding;
    closing and padding slots carry no weight, an overflowed row is skipped.  With the rays' own bounds, and with bounds tightened to
    the grid (a denser lattice on the shells: longer runs, rows that overflow)."""
    n, K, C = 257, 64, 32
    grid = MT.device_grid(fn, M.two_shells())
    plain = torch.from_numpy(MT.kernel_rays(n)).cuda()
    u = torch.from_numpy(np.random.RandomState(2).rand(n).astype(F32)).cuda()
    scored = 0
    for name, rays in (('plain', plain), ('tightened', grid.tighten(plain)[0].contiguous())):
        z, kidx, overflow = grid.march(rays, K, C, u=u)
        live = kidx >= 0
        assert not bool(overflow.all()) and bool((~live[:, :-1] & live[:, 1:]).any()), 'rows of several runs: closing entries inside, padding behind'
        assert bool((~live[~overflow, -1]).all()) and bool((z[:, 1:] >= z[:, :-1]).all()), 'padding behind; z is non-decreasing along a row'
        w = torch.rand(n, C, generator=torch.Generator().manual_seed(1)).cuda() ** 3 * live
        ell, g = fn.ops.distortion(w, z, rays, skip=overflow)
        torch.cuda.synchronize()
        r, ov = rays.cpu().numpy(), overflow.cpu().numpy()
        ell, g = ell.cpu().numpy(), g.cpu().numpy()
        ell64, g64 = D.distortion_ref(w.cpu().numpy(), z.cpu().numpy(), r[:, 6], r[:, 7], skip=ov)
        assert_bar('marched row, %s bounds' % name, C, ell, g, ell64, g64)
        assert (ell[ov].view(np.int32) == 0).all() and (g[ov].view(np.int32) == 0).all()
        hit = (w.sum(1) > 0).cpu().numpy() & ~ov
        print('%d rows overflow, %d rows with weight are scored' % (ov.sum(), hit.sum()))
        assert (g[hit] > 0).any(axis=1).all()
        scored += int(hit.sum())
    assert scored > n // 4


# ---- 2. through the compositing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['random', 'last', 'saturate'])
@pytest.mark.parametrize('S', [65, 192])
def test_through_the_compositing_backward(fn, kind, S):
    """d(sum_r l_r)/d(raw): the kernel's g_w through fastnerf_raw2outputs_bwd_full, against float64 autograd of compositing -> weights ->
    l; the torch op's registered formula makes the same two calls."""
    n = 16
    raw, z, rd, _ = RO.make_case(kind, n, S, False, seed=7 * S + len(kind))
    near, far = torch.full((n,), 2.0), torch.full((n,), 6.0)
    raw64 = raw.double().requires_grad_(True)
    w64 = O.raw2outputs(raw64, z.double(), rd.double(), None, False)[3]
    ref = torch.autograd.grad(D.torch_expression(w64, z.double(), near.double(), far.double()).sum(), raw64)[0]
    r11 = torch.zeros(n, 11)
    r11[:, 3:6], r11[:, 6], r11[:, 7] = rd, near, far
    r11, rawc, zc = r11.cuda(), raw.cuda(), z.cuda()
    _, _, acc, w, depth = fn.ops.raw2outputs_fwd(rawc, zc, r11, None, False)
    ell, g_w = fn.ops.distortion(w, zc, r11)
    draw = fn.ops.raw2outputs_bwd_full(rawc, zc, r11, acc, depth, g_w=g_w)
    ok, msg = RO.check(draw, ref)
    print('\ncompositing %-8s S=%d: %s' % (kind, S, msg))
    assert ok, msg
    assert float(ref.abs().max()) > 0 and (draw[..., :3] == 0).all(), 'the colour logits do not reach the weights'
    rawg = rawc.clone().requires_grad_(True)
    w_op = torch.ops.fastnerf.raw2outputs_full(rawg, zc, r11, None, False)[3]
    ell_op = torch.ops.fastnerf.distortion(w_op, zc, r11, False, None)
    ell_op.sum().backward()
    assert torch.equal(bits(ell_op.detach()), bits(ell)) and torch.equal(bits(rawg.grad), bits(draw))


# ---- 3. through the networks --------------------------------------------------------------------------------------------------------
NRAYS = 64
DIST = ('dist_map', 'dist0')
_NETS = {}


def dist_case(fn, Ns, Ni):
    """Two loosened networks (tests/test_gpu_aux_maps.py: half of the coarse samples dead, rays that are not saturated), 64 rays, and the
    oracle's float64 / float32 parameter gradients of dist_map.sum() + dist0.sum()."""
    key = (Ns, Ni)
    if key not in _NETS:
        gen = torch.Generator().manual_seed(200 + Ns)
        rb = O.make_ray_batch(torch.randn(NRAYS, 3, generator=gen) * 0.4, torch.randn(NRAYS, 3, generator=gen), 2.0, 6.0)
        net_c = AM.loosen(AM.new_net(fn, 41), rb, Ns)
        net_f = AM.loosen(AM.new_net(fn, 42), rb, Ns) if Ni > 0 else None
        names = ['c.' + k for k in net_c.state_dict()] + (['f.' + k for k in net_f.state_dict()] if Ni > 0 else [])

        def grads(dt):
            sd_c = {k: v.clone().requires_grad_(True) for k, v in RG.state(net_c, dt).items()}
            sd_f = {k: v.clone().requires_grad_(True) for k, v in RG.state(net_f, dt).items()} if Ni > 0 else None
            r = rb.to(dt)
            ret = O.render_rays(r, sd_c, sd_f, Ns, Ni)
            loss = D.torch_expression(ret['weights'], ret['z_vals'].detach(), r[:, 6], r[:, 7]).sum()
            if Ni > 0:
                loss = loss + D.torch_expression(ret['weights0'], ret['z0'].detach(), r[:, 6], r[:, 7]).sum()
            leaves = list(sd_c.values()) + (list(sd_f.values()) if Ni > 0 else [])
            g = torch.autograd.grad(loss, leaves, allow_unused=True)
            return [torch.zeros_like(x) if t is None else t for x, t in zip(leaves, g)]
        g64, g32 = grads(torch.float64), grads(torch.float32)
        e32 = [R.rel_l2(a, b) if float(b.norm()) > 0 else 0.0 for a, b in zip(g32, g64)]
        _NETS[key] = dict(net_c=net_c, net_f=net_f, rb=rb.cuda(), names=names, g64=g64, e32=e32, cot={k: torch.ones(NRAYS, device='cuda') for k in (DIST if Ni > 0 else DIST[:1])})
    return _NETS[key]


def hand_dist_pass(fn, saved, k, net, packed, lindisp=False):
    """distortion -> raw2outputs_bwd_full(g_w) -> mlp_bwd of one pass on the saved tensors, with a cotangent of ones."""
    z, raw, r11 = saved['z' + k], saved['raw' + k], saved['rays11']
    g_w = fn.ops.distortion(saved['w' + k], z, r11, lindisp, g_up=torch.ones(z.shape[0], device='cuda'), want=('g_w',))[1]
    draw = fn.ops.raw2outputs_bwd_full(raw, z, r11, saved['acc' + k], saved['depth' + k], g_w=g_w, noise=saved['noise' + k],
                                       white_bkgd=saved['white'])
    dact = torch.empty(fn.ops.dact_floats(z.numel()), device='cuda')
    partial = torch.empty(fn.ops.mlp_bwd_partial_floats(), device='cuda')
    flat = torch.full_like(net.flat, float('nan'))
    fn.ops.mlp_bwd(draw, saved['act' + k], net.flat, packed[1], dact, partial, flat)
    return net.param_grads_from(flat)


@pytest.mark.parametrize('mode', ['fp32', 'bf16x6', 'bf16x3'])
@pytest.mark.parametrize('Ns,Ni', [(64, 128), (32, 0)])
def test_render_rays_retdist_parameter_gradients(fn, math3, compact, mode, Ns, Ni):
    math3(mode)
    compact('0')
    c = dist_case(fn, Ns, Ni)
    out, saved, grads = AM.fused(fn, c['net_c'], c['net_f'], c['rb'], Ns, Ni, c['cot'], retdist=True)
    assert set(DIST if Ni > 0 else DIST[:1]) <= set(out) and all(out[k].shape == (NRAYS,) and out[k].requires_grad for k in c['cot'])
    AM.assert_unsaturated((out['acc_map'],) + ((out['acc0'],) if Ni > 0 else ()), (saved['raw1' if Ni > 0 else 'raw0'],) + ((saved['raw0'],) if Ni > 0 else ()))
    assert (out['dist_map'] > 0).any() and torch.isfinite(out['dist_map']).all()
    # the values are the kernel's on the forward's own weights, and a no-grad call returns the same bits
    k1 = '1' if Ni > 0 else '0'
    assert torch.equal(bits(out['dist_map'].detach()), bits(fn.ops.distortion(saved['w' + k1], saved['z' + k1], saved['rays11'], want=('ell',))[0]))
    with torch.no_grad():
        plain = fn.render.render_rays(c['rb'], c['net_c'], None, Ns, N_importance=Ni, network_fine=c['net_f'], perturb=0., retdist=True)
    assert all(torch.equal(bits(plain[k]), bits(out[k].detach())) for k in c['cot']) and 'dist_map' not in fn.render.render_rays(
        c['rb'], c['net_c'], None, Ns, N_importance=Ni, network_fine=c['net_f'], perturb=0.)
    # bit for bit the parts called by hand, in every mode
    hand = [hand_dist_pass(fn, saved, '0', c['net_c'], saved['pc'])] + ([hand_dist_pass(fn, saved, '1', c['net_f'], saved['pf'])] if Ni > 0 else [])
    for got, want in zip(grads, hand):
        for a, b in zip(got, want):
            assert torch.isfinite(a).all() and torch.equal(bits(a), bits(b)), int((a != b).sum())
    assert float(max(g.abs().max() for g in grads[0])) > 0
    if mode == 'bf16x3':
        return      # (16 significand bits per product: the 16 x E32 rule does not describe it -- tests/test_gpu_aux_maps.py)
    on = [float(g.norm()) > 0 for g in c['g64']]
    assert sum(on) == (36 if Ni > 0 else 18), 'eight trunk layers and the density head of every network'
    for name, o_, e in zip(c['names'], on, c['e32']):
        assert not o_ or AM.FACTOR * e < 0.5, ('the reference leaves no room for the check to bite', name, e)
    AM.check_tensors('dist->params (%d,%d)' % (Ns, Ni), mode, [g for net in grads for g in net], c['names'], c['g64'], c['e32'])


@pytest.mark.parametrize('mode', ['fp32', 'bf16x6', 'bf16x3'])
def test_render_rays_retdist_compacted_against_saving_route(fn, math3, compact, mode):
    math3(mode)
    c = dist_case(fn, 64, 128)
    res = {}
    for route in ('0', '1'):
        compact(route)
        _, saved, grads = AM.fused(fn, c['net_c'], c['net_f'], c['rb'], 64, 128, c['cot'], retdist=True)
        assert bool(saved['live']) == (route == '1')
        res[route] = torch.cat([g.reshape(-1) for net in grads for g in net])
    diff, scale = float((res['0'] - res['1']).abs().max()), float(res['0'].abs().max())
    print('\ndist: compacted vs saving %-6s max |diff| %.3e of max %.3e (bound %.3e)' % (mode, diff, scale, 3e-6 * scale))
    assert scale > 0 and torch.isfinite(res['1']).all() and diff < 3e-6 * scale


@pytest.mark.parametrize('Ns,Ni', [(32, 0), (16, 16)])
def test_torch_network_route_agrees_with_the_fused_route(fn, math3, Ns, Ni):
    """render_rays with plain torch networks: torch.ops.fastnerf.distortion on the weights of raw2outputs_full."""
    math3('fp32')
    c = dist_case(fn, 32, 0) if Ni == 0 else None
    torch.manual_seed(4)
    nc = c['net_c'] if c else AM.new_net(fn, 51)
    nf = None if Ni == 0 else AM.new_net(fn, 52)
    rb = c['rb'] if c else AM.ray_batch(NRAYS, 8).cuda()
    wc, wf = CN.Wrapped(nc).cuda(), (None if nf is None else CN.Wrapped(nf).cuda())
    kw = dict(perturb=0., N_importance=Ni, retdist=True)
    for p in nc.parameters():
        p.grad = None
    fused = fn.render.render_rays(rb, nc, None, Ns, network_fine=nf, **kw)
    clos = fn.render.render_rays(rb, wc, CN.query_fn(fn), Ns, network_fine=wf, **kw)
    keys = DIST if Ni > 0 else DIST[:1]
    for k in keys:
        err = float((fused[k].detach() - clos[k].detach()).abs().max())
        print('\nclosure vs fused (%d,%d) %s max |diff| %.3e of max %.3e' % (Ns, Ni, k, err, float(fused[k].detach().abs().max())))
        assert clos[k].requires_grad and err <= 1e-4 * max(1.0, float(fused[k].detach().abs().max())), (k, err)
    if Ni == 0:
        ga = torch.autograd.grad(fused['dist_map'].sum(), list(nc.parameters()), allow_unused=True)
        gb = torch.autograd.grad(clos['dist_map'].sum(), list(wc.parameters()), allow_unused=True)
        seen = 0
        for name, a, b in zip(wc.names, ga, gb):
            if b is None or float(b.norm()) == 0:
                assert a is None or float(a.abs().max()) == 0, name      # (the colour branch)
                continue
            seen += 1
            assert CN.rel(b, a) <= 2e-3, (name, CN.rel(b, a))
        assert seen == 18


def test_render_passes_retdist_on(fn, math3):
    """render(..., retdist=True): dist_map / dist0 among the extras, in the shape of the rays, chunk by chunk the same bits."""
    math3('fp32')
    c = dist_case(fn, 64, 128)
    ro, rd = c['rb'][:, 0:3].contiguous(), c['rb'][:, 3:6].contiguous()
    kw = dict(rays=(ro.reshape(8, 8, 3), rd.reshape(8, 8, 3)), ndc=False, near=2., far=6., use_viewdirs=True, network_fn=c['net_c'],
              network_fine=c['net_f'], network_query_fn=None, N_samples=64, N_importance=128, perturb=0.)
    with torch.no_grad():
        whole = fn.render.render(8, 8, RG.K, chunk=64, retdist=True, **kw)[3]
        parts = fn.render.render(8, 8, RG.K, chunk=24, retdist=True, **kw)[3]
        assert 'dist_map' not in fn.render.render(8, 8, RG.K, chunk=64, **kw)[3]
    for k in DIST:
        assert whole[k].shape == (8, 8) and torch.isfinite(whole[k]).all() and (whole[k] > 0).any() and torch.equal(bits(whole[k]), bits(parts[k]))


# ---- 4. the steps ---------------------------------------------------------------------------------------------------------------------
LAM = 0.5
NSTEP = 256


def step_batches(fn, steps=2):
    g = torch.Generator().manual_seed(21)
    out = []
    for b, _ in AM.batches(fn, steps, NSTEP):
        out.append((b, torch.rand(NSTEP, 16, generator=g).cuda(), torch.rand(NSTEP, 32, generator=g).cuda()))
    return out


def step_trainer(fn, **kw):
    """Trainer of tests/test_gpu_aux_maps.py (16 + 32 samples, two networks) loosened on the first batch's rays."""
    (b, _, _), = step_batches(fn, 1)
    return AM.trainer(fn, loose_on=O.make_ray_batch(b[0].cpu(), b[1].cpu(), 2.0, 6.0), **kw)


def slab_grid(fn):
    mask = torch.ones(16, 16, 16, dtype=torch.bool, device='cuda')
    mask[:, :, 5:11] = False
    return fn.occupancy.OccupancyGrid.from_mask(mask, -4.5, 4.5, outside_occupied=False)


def hand_step(fn, tr, b, t_rand, u, lam, grid=None, grad_scale=1.0):
    """The launches of one fastnerf_train_step_dist call through ops, on the trainer's own parameters, moments and gradient buffer."""
    ops = fn.ops
    ro, rd, tgt = b
    n, Ns, Ni = ro.shape[0], tr.N_samples, tr.N_importance
    live = grid is not None or tr.live.use_live(tr.net_c, tr.net_f, Ni)
    Nn = ops.NET_PARAMS
    fc, ff = tr.flat[:Nn], tr.flat[Nn:]
    rays11 = ops.pack_rays(ro, rd, tr.near, tr.far, ndc=tr.ndc, H=tr.H, W=tr.W, focal=float(tr.K[0][0]))
    common = dict(lindisp=tr.lindisp, perturb=bool(tr.perturb), det=not tr.perturb, white_bkgd=tr.white_bkgd, t_rand=t_rand, u=u)
    if grid is not None:
        o = ops.render_rays_fwd_occ(rays11, fc, tr.pc[0], ff, tr.pf[0], Ns, Ni, grid._c, skip_dead_rgb=tr.skip_dead_rgb, **common)
    else:
        o = ops.render_rays_fwd(rays11, fc, tr.pc[0], ff, tr.pf[0], Ns, Ni, save=not live, skip_dead_rgb=live and tr.skip_dead_rgb, **common)
    loss2, g, g0 = ops.mse_leafmax(o['rgb1'], o['rgb0'], tgt, grad_scale=grad_scale)
    coef = ctypes.c_float(grad_scale).value * ctypes.c_float(lam).value / n
    ell1, gw1 = ops.distortion(o['w1'], o['z1'], rays11, tr.lindisp, coef=coef)
    ell0, gw0 = ops.distortion(o['w0'], o['z0'], rays11, tr.lindisp, coef=coef)
    loss2d = ops.distortion_mean(ell1, ell0)
    P = n * (Ns + Ni)
    ws = torch.empty(ops.dact_floats(P) + 4 * P, device='cuda')
    draw = ws[ops.dact_floats(P):]
    partial = torch.empty(ops.mlp_bwd_partial_floats(), device='cuda')
    wg = dict(g_w1=gw1, g_w0=gw0)
    if live:
        act = torch.empty(ops.act_floats(P), device='cuda')
        live_ws = torch.empty(ops.live_ws_ints(P), device='cuda', dtype=torch.int32)
        ops.render_rays_bwd_live(rays11, tr.white_bkgd, g, g0, None, None, o['z0'], o['raw0'], o['z1'], o['raw1'], fc, tr.pc, ff, tr.pf, draw, act,
                                 ws, partial, live_ws, tr.grad[:Nn], tr.grad[Nn:], Ns, Ni, weight_grads=wg)
    else:
        ops.render_rays_bwd(rays11, tr.white_bkgd, g, g0, None, None, o['z0'], o['raw0'], o['act0'], o['z1'], o['raw1'], o['act1'], fc, tr.pc[1], ff,
                            tr.pf[1], draw, ws, partial, tr.grad[:Nn], tr.grad[Nn:], Ns, Ni, weight_grads=wg)
    grad = tr.grad.clone()
    tr.adam_t += 1
    ops.adam_step(tr.flat, tr.grad, tr.m, tr.v, tr.lr, tr.adam_t, tr.beta1, tr.beta2, tr.eps)
    tr.repack()
    return dict(loss2=loss2, loss2d=loss2d, grad=grad, ell1=ell1, ell0=ell0, gw1=gw1, gw0=gw0)


def phased(fn, tr, b, t_rand, u, groups):
    """Trainer.step's fused route with the phases in the call groups given -> (loss2, out)."""
    tr.adam_t += 1
    a, out, loss2, live = tr._fused_prepare(*b, None, None, 0, t_rand, u, None)
    a.lr, a.adam_t = float(tr.lr), int(tr.adam_t)
    for phases in groups:
        tr._fused_call(a, phases)
    tr._after_backward(live)
    return loss2, out


def state_of(tr):
    torch.cuda.synchronize()
    return [t.clone() for t in (tr.flat, tr.m, tr.v, tr.grad, tr.pc[0], tr.pc[1], tr.pf[0], tr.pf[1])]


STATE = ('parameters', 'adam m', 'adam v', 'gradient', 'packed fwd c', 'packed bwd c', 'packed fwd f', 'packed bwd f')


@pytest.mark.parametrize('mode', ['bf16x6', 'fp32'])
@pytest.mark.parametrize('route', ['plain', 'compacted', 'grid'])
def test_step_is_its_parts_bit_for_bit(fn, math3, compact, mode, route):
    """Two steps of Trainer(lambda_dist=) -- the second reads the moments of the first -- against the same launches through ops, the
    call-by-call route (plain, compacted), and the data-parallel phase split."""
    math3(mode)
    compact('0' if route == 'plain' else '1')
    L = fn._lib
    split = [L.STEP_FORWARD | L.STEP_BWD_FINE, L.STEP_BWD_COARSE, L.STEP_UPDATE]
    mk = lambda: step_trainer(fn, lambda_dist=LAM, **(dict(occupancy=slab_grid(fn), occupancy_warmup=10 ** 9) if route == 'grid' else {}))      # noqa: E731
    tr, th, ts = mk(), mk(), mk()
    for b, t_rand, u in step_batches(fn):
        loss2, out = tr.step(*b, t_rand=t_rand, u=u, decay=False)
        assert tr.last_step_live == (route != 'plain')
        hand = hand_step(fn, th, b, t_rand, u, LAM, grid=th.occupancy)
        loss2s, outs = phased(fn, ts, b, t_rand, u, split)
        got, want, third = state_of(tr), state_of(th), state_of(ts)
        assert torch.equal(bits(loss2), bits(hand['loss2'])) and torch.equal(bits(tr.dist_losses), bits(hand['loss2d']))
        assert torch.equal(bits(out['dist_map']), bits(hand['ell1'])) and torch.equal(bits(out['dist0']), bits(hand['ell0']))
        for name, x, y, s in zip(STATE, got, want, third):
            assert torch.isfinite(x).all() and torch.equal(bits(x), bits(y)), (name, 'by hand')
            assert torch.equal(bits(x), bits(s)), (name, 'phase split')
        assert torch.equal(bits(loss2s), bits(loss2)) and torch.equal(bits(ts.dist_losses), bits(tr.dist_losses))
        assert (tr.dist_losses > 0).all() and float(hand['gw1'].abs().max()) > 0 and float(hand['gw0'].abs().max()) > 0
    if route == 'grid':
        occ = tr.occupancy_counts.tolist()
        assert 0 < occ[0] < occ[1] and 0 < occ[2] < occ[3], 'the slab removes samples, and leaves some'
        return
    old = os.environ.get('FASTNERF_FUSED_STEP')
    os.environ['FASTNERF_FUSED_STEP'] = '0'      # (read by the constructor: the call-by-call route)
    try:
        tc = mk()
    finally:
        os.environ.pop('FASTNERF_FUSED_STEP', None)
        if old is not None:
            os.environ['FASTNERF_FUSED_STEP'] = old
    assert not tc.fused
    for b, t_rand, u in step_batches(fn):
        loss2c, outc = tc.step(*b, t_rand=t_rand, u=u, decay=False)
    for name, x, y in zip(STATE, state_of(tr), state_of(tc)):
        assert torch.equal(bits(x), bits(y)), (name, 'call by call')
    assert torch.equal(bits(loss2c), bits(loss2)) and torch.equal(bits(tc.dist_losses), bits(tr.dist_losses))
    assert torch.equal(bits(outc['dist_map']), bits(out['dist_map'])) and torch.equal(bits(outc['dist0']), bits(out['dist0']))


@pytest.mark.parametrize('route', ['plain', 'compacted'])
def test_the_term_trains_and_scales_with_n_global(fn, compact, route):
    compact('0' if route == 'plain' else '1')
    (b, t_rand, u), = step_batches(fn, 1)
    base, on, half = step_trainer(fn), step_trainer(fn, lambda_dist=LAM), step_trainer(fn, lambda_dist=LAM)
    l0, _ = base.step(*b, t_rand=t_rand, u=u, decay=False)
    l1, _ = on.step(*b, t_rand=t_rand, u=u, decay=False)
    l2, _ = half.step(*b, t_rand=t_rand, u=u, decay=False, n_global=2 * NSTEP)
    torch.cuda.synchronize()
    assert torch.equal(bits(l0), bits(l1)) and torch.equal(bits(l1), bits(l2)), 'the forward is the same'
    assert not torch.equal(base.grad, on.grad) and (base.dist_losses == 0).all() and (on.dist_losses > 0).all()
    assert torch.equal(half.grad * 2, on.grad) and torch.equal(bits(half.dist_losses), bits(on.dist_losses))


@pytest.mark.parametrize('mode', ['bf16x6', 'fp32'])
@pytest.mark.parametrize('route', ['plain', 'compacted', 'grid', 'marched'])
def test_lambda_zero_is_the_step_without_the_term(fn, math3, compact, mode, route):
    """lambda_dist = 0: a trainer built without the argument, bit for bit; and fastnerf_train_step_dist / _march_dist with dist == NULL or
    lambda_dist == 0 in the struct are the entry points without _dist (the struct's pointers are not looked at)."""
    math3(mode)
    compact('0' if route == 'plain' else '1')
    L = fn._lib
    lib = L.lib()
    everything = L.STEP_FORWARD | L.STEP_BWD_FINE | L.STEP_BWD_COARSE | L.STEP_UPDATE
    zero = L.StepDist()
    zero.lambda_dist = 0.0
    if route == 'marched':
        n, K, C = NSTEP, 64, 32
        ro, rd, tgt = MT.batch(n, 3)
        um = torch.from_numpy(np.random.RandomState(9).rand(n).astype(F32)).cuda()
        res = []
        for kw, call in (({}, None), (dict(lambda_dist=0.), None), ({}, zero), ({}, 'null')):
            tr, _, _ = MT.new_trainer(fn, MT.device_grid(fn, M.two_shells()), march=K, march_cap=C, **kw)
            if call is None:
                loss2, out = tr.step(ro, rd, tgt, march_u=um, decay=False)
                assert 'dist_map' not in out and tr._dist is None
            else:
                tr.adam_t += 1
                a, x, out, loss2 = tr._march_prepare(K, C, ro, rd, tgt, None, None, 0, um, None)
                a.lr, a.adam_t = float(tr.lr), int(tr.adam_t)
                assert lib.fastnerf_train_step_march_dist(ctypes.byref(a), ctypes.byref(x), None, None if call == 'null' else ctypes.byref(call),
                                                          everything, L.stream()) == 0
            res.append(state_of(tr) + [loss2.clone()])
            assert (tr.dist_losses == 0).all()
    else:
        (b, t_rand, u), = step_batches(fn, 1)
        gkw = lambda: dict(occupancy=slab_grid(fn), occupancy_warmup=10 ** 9) if route == 'grid' else {}      # noqa: E731
        res = []
        for kw, call in (({}, None), (dict(lambda_dist=0.), None), ({}, zero), ({}, 'null')):
            tr = step_trainer(fn, **kw, **gkw())
            if call is None:
                loss2, out = tr.step(*b, t_rand=t_rand, u=u, decay=False)
                assert 'dist_map' not in out and tr._dist is None
            else:
                tr.adam_t += 1
                a, out, loss2, live = tr._fused_prepare(*b, None, None, 0, t_rand, u, None)
                a.lr, a.adam_t = float(tr.lr), int(tr.adam_t)
                assert lib.fastnerf_train_step_dist(ctypes.byref(a), None, None, None if call == 'null' else ctypes.byref(call), everything,
                                                    L.stream()) == 0
            res.append(state_of(tr) + [loss2.clone()])
            assert (tr.dist_losses == 0).all()
    for other in res[1:]:
        for name, x, y in zip(STATE + ('loss2',), res[0], other):
            assert torch.equal(bits(x), bits(y)), name


def hand_march_step(fn, tr, grid, ro, rd, tgt, u, K, C, lam, tighten):
    """by_hand of tests/test_gpu_march_train.py with the distortion launches: the launches of fastnerf_train_step_march_dist through ops."""
    ops = fn.ops
    Nn = ops.NET_PARAMS
    n = ro.shape[0]
    which = tr._marched()[0]
    sl = slice(which * Nn, (which + 1) * Nn)
    params, m, v = tr.flat[sl].clone(), tr.m[sl].clone(), tr.v[sl].clone()
    pf, pb = ops.mlp_pack(params)
    rays11 = ops.pack_rays(ro, rd, 2.0, 6.0)
    if tighten:
        ops.occ_ray_bounds(grid._c, rays11, write_back=True)
    z, kidx, overflow, _ = ops.occ_march_jitter(grid._c, rays11, K, C, u=u, seed=0)
    raw = torch.empty(n, C, 4, device='cuda')
    counts = torch.zeros(2, device='cuda', dtype=torch.int32)
    idx, cnt = ops.march_list(kidx, 0, C, raw=raw, total=counts, lattice=n * K)
    ops.mlp_fwd_list(rays11, z, params, pf, raw, idx, cnt, flags=1 if tr.skip_dead_rgb else 0)
    rgb, _, _, w, _ = ops.raw2outputs_fwd(raw, z, rays11, None, bool(tr.white_bkgd))
    loss2, g, _ = ops.mse_leafmax(rgb, None, tgt)
    ops.march_mask(overflow, g)
    ell, g_w = ops.distortion(w, z, rays11, tr.lindisp, skip=overflow, coef=ctypes.c_float(1.0).value * ctypes.c_float(lam).value / n)
    loss2d = ops.distortion_mean(ell)
    P = n * C
    ws, draw, act = torch.empty(ops.dact_floats(P), device='cuda'), torch.empty(P * 4, device='cuda'), torch.empty(ops.act_floats(P), device='cuda')
    partial = torch.empty(ops.mlp_bwd_partial_floats(), device='cuda')
    live_ws = torch.empty(ops.live_ws_ints(P), device='cuda', dtype=torch.int32)
    grad = torch.full((Nn,), float('nan'), device='cuda')
    ops.render_rays_bwd_live(rays11, bool(tr.white_bkgd), g, None, None, None, z, raw, None, None, params, (pf, pb), None, None, draw, act,
                             ws, partial, live_ws, grad, None, C, 0, weight_grads=dict(g_w1=g_w))
    res = dict(grad=grad.clone(), overflow=overflow, loss2=loss2, loss2d=loss2d, ell=ell, g_w=g_w, w=w, z=z, rays11=rays11)
    ops.adam_step(params, grad, m, v, tr.lr, tr.adam_t + 1, tr.beta1, tr.beta2, tr.eps)
    ops.mlp_pack(params, pf, pb)
    res.update(flat=params, m=m, v=v, pf=pf, pb=pb)
    return res


def test_marched_step_is_its_parts_and_skips_overflowed_rays(fn, math_mode, compact):
    compact('1')
    n, K, C = NSTEP, 64, 32
    grid = MT.device_grid(fn, M.two_shells())
    Nn = fn.ops.NET_PARAMS
    ro, rd, tgt = MT.batch(n, 3)
    u = torch.from_numpy(np.random.RandomState(9).rand(n).astype(F32)).cuda()
    tr, _, _ = MT.new_trainer(fn, grid, march=K, march_cap=C, tighten=True, lambda_dist=LAM)
    tr.m.uniform_(-1e-3, 1e-3)
    tr.v.uniform_(0, 1e-6)
    state0 = [t.clone() for t in (tr.flat, tr.m, tr.v)]
    hand = hand_march_step(fn, tr, grid, ro, rd, tgt, u, K, C, LAM, True)
    loss2, out = tr.step(ro, rd, tgt, march_u=u, decay=False)
    torch.cuda.synchronize()
    ov = hand['overflow'].bool()
    assert bool(ov.any()) and not bool(ov.all()), 'the tightened lattice overflows some rows of 32 slots'
    assert torch.equal(out['march_overflow'], ov) and torch.equal(bits(loss2[:1]), bits(hand['loss2'][:1]))
    assert torch.equal(bits(out['dist_map']), bits(hand['ell'])) and torch.equal(bits(tr.dist_losses), bits(hand['loss2d']))
    g_w = fn.run_nerf._region(tr._march_block, tr._march_dist_regions, 'g_w1')
    assert torch.equal(bits(g_w), bits(hand['g_w']))
    assert (bits(g_w[ov]) == 0).all() and (bits(out['dist_map'][ov]) == 0).all(), 'an overflowed ray: l = +0 and a zero g_w row'
    hit = (hand['w'].sum(1) > 0) & ~ov
    assert int(hit.sum()) > 0 and bool((g_w[hit] != 0).any(dim=1).all()) and float(tr.dist_losses[0]) > 0 and int(bits(tr.dist_losses)[1]) == 0
    # the kernel's row against the definition, with the row's own closing and padding slots
    r = hand['rays11'].cpu().numpy()
    ell64, g64 = D.distortion_ref(hand['w'].cpu().numpy(), hand['z'].cpu().numpy(), r[:, 6], r[:, 7], skip=ov.cpu().numpy())
    assert_bar('marched step row', C, hand['ell'].cpu().numpy(), hand['g_w'].cpu().numpy(), ell64, F32(LAM / n).astype(np.float64) * g64)
    sl = slice(Nn, 2 * Nn)
    assert torch.equal(bits(tr.grad[sl]), bits(hand['grad'])) and float(hand['grad'].abs().max()) > 0
    for name, mine in (('flat', tr.flat[sl]), ('m', tr.m[sl]), ('v', tr.v[sl]), ('pf', tr.pf[0]), ('pb', tr.pf[1])):
        assert torch.equal(bits(mine), bits(hand[name])), name
    # the term reaches the field: another gradient than without it
    tr0, _, _ = MT.new_trainer(fn, grid, march=K, march_cap=C, tighten=True)
    tr0.m.copy_(state0[1])
    tr0.v.copy_(state0[2])
    tr0.step(ro, rd, tgt, march_u=u, decay=False)
    assert not torch.equal(tr0.grad[sl], tr.grad[sl])
    # FORWARD | BWD, then UPDATE, as two calls: the same bits
    tr2, _, _ = MT.new_trainer(fn, grid, march=K, march_cap=C, tighten=True, lambda_dist=LAM)
    tr2.m.copy_(state0[1])
    tr2.v.copy_(state0[2])
    tr2.adam_t += 1
    a, x, _, _ = tr2._march_prepare(K, C, ro, rd, tgt, None, None, 0, u, None)
    a.lr, a.adam_t = float(tr2.lr), int(tr2.adam_t)
    L = fn._lib
    tr2._march_call(a, x, L.STEP_FORWARD | L.STEP_BWD_FINE | L.STEP_BWD_COARSE)
    tr2._march_call(a, x, L.STEP_UPDATE)
    torch.cuda.synchronize()
    for name, p, q in (('flat', tr2.flat, tr.flat), ('m', tr2.m, tr.m), ('v', tr2.v, tr.v), ('pf', tr2.pf[0], tr.pf[0]), ('grad', tr2.grad[sl], tr.grad[sl])):
        assert torch.equal(bits(p), bits(q)), name


def test_refusals_enqueue_nothing(fn, compact):
    """-1 before the first launch: the step's block (rays11, the maps, loss2) keeps the sentinel it was filled with."""
    compact('1')
    L = fn._lib
    lib = L.lib()
    everything = L.STEP_FORWARD | L.STEP_BWD_FINE | L.STEP_BWD_COARSE | L.STEP_UPDATE
    (b, t_rand, u), = step_batches(fn, 1)
    tr = step_trainer(fn, lambda_dist=LAM)
    tr.adam_t += 1
    a, out, loss2, live = tr._fused_prepare(*b, None, None, 0, t_rand, u, None)
    a.lr, a.adam_t = float(tr.lr), int(tr.adam_t)
    good = tr._dist
    before = state_of(tr)

    def variant(**kw):
        d = L.StepDist()
        for k, _ in L.StepDist._fields_:
            setattr(d, k, getattr(good, k))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(call, prefix, block):
        block.fill_(-7.0)
        assert call() == -1
        msg = lib.fastnerf_last_error().decode()
        assert msg.startswith(prefix), msg
        torch.cuda.synchronize()
        assert bool((block == -7.0).all()), 'something was enqueued'

    for kw, phases in ((dict(lambda_dist=-1.0), everything), (dict(lambda_dist=float('nan')), everything), (dict(lambda_dist=float('inf')), everything),
                       (dict(g_w1=None), everything), (dict(g_w0=None), everything), (dict(ell1=None), everything), (dict(ell0=None), everything),
                       (dict(loss2d=None), everything), (dict(g_w0=None), L.STEP_BWD_COARSE), (dict(g_w1=None), L.STEP_BWD_FINE)):
        d = variant(**kw)
        refused(lambda: lib.fastnerf_train_step_dist(ctypes.byref(a), None, None, ctypes.byref(d), phases, L.stream()), 'fastnerf_train_step_dist:',
                out._block)
    w1 = a.w1
    a.w1 = None
    refused(lambda: lib.fastnerf_train_step_dist(ctypes.byref(a), None, None, ctypes.byref(good), everything, L.stream()), 'fastnerf_train_step_dist:',
            out._block)
    a.w1 = w1
    # a backward phase alone does not need ell / loss2d
    for name, x, y in zip(STATE, before, state_of(tr)):
        assert torch.equal(bits(x), bits(y)), name
    # the marched step
    n, K, C = NSTEP, 64, 32
    ro, rd, tgt = MT.batch(n, 3)
    trm, _, _ = MT.new_trainer(fn, MT.device_grid(fn, M.two_shells()), march=K, march_cap=C, lambda_dist=LAM)
    trm.adam_t += 1
    am, xm, _, _ = trm._march_prepare(K, C, ro, rd, tgt, None, None, 0, None, None)
    am.lr, am.adam_t = float(trm.lr), int(trm.adam_t)
    good = trm._dist
    for kw in (dict(lambda_dist=-1.0), dict(g_w1=None), dict(ell1=None), dict(loss2d=None)):
        d = variant(**kw)
        refused(lambda: lib.fastnerf_train_step_march_dist(ctypes.byref(am), ctypes.byref(xm), None, ctypes.byref(d), everything, L.stream()),
                'fastnerf_train_step_march_dist:', trm._march_block)
    # Python: a weight that is no weight
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            step_trainer(fn, lambda_dist=bad)
    tr.lambda_dist = -0.5      # (read on every step)
    with pytest.raises(ValueError):
        tr.step(*b, t_rand=t_rand, u=u)


def test_empty_shard(fn):
    tr = step_trainer(fn, lambda_dist=LAM)
    e3 = torch.empty(0, 3, device='cuda')
    before = tr.flat.clone()
    loss2, out = tr.step(e3, e3, e3, n_global=64)
    assert (loss2 == 0).all() and out == {} and tr.dist_losses.shape == (2,) and (tr.dist_losses == 0).all()
    assert torch.equal(tr.flat, before)
