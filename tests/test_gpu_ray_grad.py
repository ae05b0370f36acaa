"""Ray and camera-pose gradients through the fused renderer: ops.ray_grad (csrc/ray_grad.hip) per pass, render_rays with a ray
batch that requires grad, render(c2w=pose) with a pose that requires grad.

Reference: float64 autograd of the oracle (oracle.nerf_oracle) with respect to the rays.  Per pass it is run_network + raw2outputs
at the kernels' own fp32 z and fp32 points (the float64 points are snapped onto them, the derivative with respect to o and d
stays); end to end it is the oracle's render_rays (its fine samples detached, as render.py:281), for the pose with the oracle's
get_rays + make_ray_batch in front.
Metric: relative L2 error per column group -- o (0:3), d (3:6), viewdir (8:11) -- over the whole batch; no ray is excluded.
Bound: not chosen in advance.  E32 is the same metric for torch's float32 CPU autograd of the same oracle against the same float64
result; fp32 and bf16x6 stay within 16 E32, the spread the README documents for this project's first-layer gradients against
fp64, which is what ops.ray_grad consumes (the rule of tests/test_gpu_sigma_grad.py).  Every figure is printed before it is asserted
(pytest -s shows them; recorded in profiles/ray_grad.md).

Per-pass shapes (n, S): (1, 1) one sample (its compositing reference: raw2outputs_one_sample below), (3, 67) a ragged tile tail with sigma noise and a white background, (5, 64) exact
64-point tiles, (2, 129) one point past a tile, and a network without view directions at (3, 67).  Points as in the sigma-grad
test: a ray runs between two uniform draws of [-1.5, 1.5]^3, z ascending in [0, 1]; from two rays on, the ray before the last has
o_y = d_y = 0 (a zero coordinate in d, and in its view direction)."""
import ctypes

import pytest
import torch

import test_gpu_custom_network as C
import test_ray_grad_cpu as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 67), (5, 64), (2, 129)]
FACTOR = 16.0
GROUPS = (('o', slice(0, 3)), ('d', slice(3, 6)), ('viewdir', slice(8, 11)))


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


@pytest.fixture(params=['fp32', 'bf16x6'])
def mode(request, fn):
    """The two math modes that have ray gradients."""
    old = fn.ops.get_math()
    fn.ops.set_math(request.param)
    yield request.param
    fn.ops.set_math(old)


def make_net(fn, seed, viewdirs=True):
    """A freshly initialised network whose density head is lifted by 0.3, so that most samples are live (sigma > 0)."""
    torch.manual_seed(seed)
    net = fn.model.NeRF(use_viewdirs=viewdirs, input_ch_views=27 if viewdirs else 0)
    with torch.no_grad():
        if viewdirs:
            net.alpha_linear.bias.add_(0.3)
        else:
            net.output_linear.bias[3] += 0.3
    return net


def state(net, dtype):
    return {k: v.detach().cpu().to(dtype) for k, v in net.state_dict().items()}


def group_errors(d_rays, ref, viewdirs=True):
    """{group: relative L2} of a [n,11] gradient against a [n,11] reference."""
    return {name: R.rel_l2(d_rays[:, sl], ref[:, sl]) for name, sl in GROUPS if viewdirs or name != 'viewdir'}


def check_groups(what, mode, d_rays, c):
    errs = group_errors(d_rays.cpu(), c['ref64'], c['viewdirs'])
    for name, err in errs.items():
        e32 = c['e32'][name]
        print('\n%s %-6s %-7s err %.3e  E32 %.3e  bound %.3e' % (what, mode, name, err, e32, FACTOR * e32))
    assert torch.isfinite(d_rays).all()
    for name, err in errs.items():
        assert err <= FACTOR * c['e32'][name], (what, mode, name, err, c['e32'][name])


# ---- one pass ------------------------------------------------------------------------------------------------------------------
def make_pass(n, S, seed, viewdirs, with_noise):
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand(n, 3, generator=gen) * 3 - 1.5
    b = torch.rand(n, 3, generator=gen) * 3 - 1.5
    z = torch.sort(torch.rand(n, S, generator=gen), -1).values
    o, d = a.clone(), b - a
    if n >= 2:
        o[n - 2, 1] = 0
        d[n - 2, 1] = 0
    rays = torch.zeros(n, 11)
    rays[:, 0:3], rays[:, 3:6] = o, d
    if viewdirs:
        rays[:, 8:11] = d / d.norm(dim=-1, keepdim=True)
    pts = o[:, None, :] + d[:, None, :] * z[..., None]                       # separate roundings, as the kernels
    g_rgb = torch.randn(n, 3, generator=gen)
    noise = torch.randn(n, S, generator=gen) * 0.1 if with_noise else None
    return rays, z, pts, g_rgb, noise


def raw2outputs_one_sample(raw, z, rays_d, noise, white):
    """render.py:149-192 for S = 1, where the oracle's raw2outputs (like the reference's) cannot serve: it sizes the 1e10 of the last
    sample by dists[..., :1], which is EMPTY when there is no other sample, so its sample axis comes out empty, every map constant
    and every gradient exactly zero (the metric would be 0 / 0).  The one sample is the last one: dist = 1e10 |d|, transmittance 1."""
    dists = 1e10 * torch.norm(rays_d[..., None, :], dim=-1)
    sigma = raw[..., 3] if noise is None else raw[..., 3] + noise
    weights = 1.0 - torch.exp(-torch.relu(sigma) * dists)
    rgb_map = torch.sum(weights[..., None] * torch.sigmoid(raw[..., :3]), -2)
    if white:
        rgb_map = rgb_map + (1.0 - torch.sum(weights, -1)[..., None])
    return (rgb_map,)


def oracle_pass_grads(sd, rays, z, pts, g_rgb, noise, white, viewdirs, dtype):
    """[n,11] autograd gradient of sum(rgb_map * g_rgb) of one pass in `dtype`, at the fp32 points `pts`."""
    t = lambda x: None if x is None else x.to(dtype)      # noqa: E731
    leaves = [t(rays[:, 0:3]).clone().requires_grad_(True), t(rays[:, 3:6]).clone().requires_grad_(True)]
    v = t(rays[:, 8:11]).clone().requires_grad_(True) if viewdirs else None
    o, d = leaves
    p = o[:, None, :] + d[:, None, :] * t(z)[..., None]
    p = p + (t(pts) - p.detach())                                            # the kernels' points, the derivative of o + d z
    raw = O.run_network(sd, p, v)
    rgb = (O.raw2outputs if z.shape[1] > 1 else raw2outputs_one_sample)(raw, t(z), d, t(noise), white)[0]
    grads = torch.autograd.grad((rgb * t(g_rgb)).sum(), leaves + ([v] if viewdirs else []))
    out = torch.zeros(rays.shape[0], 11, dtype=dtype)
    out[:, 0:3], out[:, 3:6] = grads[0], grads[1]
    if viewdirs:
        out[:, 8:11] = grads[2]
    return out


_CASES = {}


def case(fn, n, S, viewdirs=True):
    """One network, one pass and its references per (shape, kind of network), computed once and shared by every test and mode."""
    key = (n, S, viewdirs)
    if key not in _CASES:
        net = make_net(fn, 2000 + 10 * n + S + (0 if viewdirs else 5), viewdirs)
        white, with_noise = S % 2 == 1, n == 3
        rays, z, pts, g_rgb, noise = make_pass(n, S, 91 + n * S, viewdirs, with_noise)
        ref64 = oracle_pass_grads(state(net, torch.float64), rays, z, pts, g_rgb, noise, white, viewdirs, torch.float64)
        ref32 = oracle_pass_grads(state(net, torch.float32), rays, z, pts, g_rgb, noise, white, viewdirs, torch.float32)
        cu = lambda x: None if x is None else x.cuda()      # noqa: E731
        _CASES[key] = dict(net=net, rays=cu(rays), z=cu(z), g_rgb=cu(g_rgb), noise=cu(noise), white=white, viewdirs=viewdirs,
                           ref64=ref64, e32=group_errors(ref32, ref64, viewdirs))
    return _CASES[key]


def run_pass(fn, net, rays, z, g_rgb, noise, white, **kw):
    """Saving forward -> raw2outputs_bwd -> mlp_bwd -> ray_grad of one pass.  -> (d_rays, parameter gradient)."""
    n, S = z.shape
    P = n * S
    pf, pb = net.packed()
    act = torch.empty(fn.ops.act_floats(P), device='cuda')
    raw = fn.ops.mlp_fwd(rays, z, net.flat, pf, act=act)
    draw = fn.ops.raw2outputs_bwd(raw, z, rays, g_rgb, noise, white)
    dact = torch.empty(fn.ops.dact_floats(P), device='cuda')
    partial = torch.empty(fn.ops.mlp_bwd_partial_floats(), device='cuda')
    grads = torch.empty(fn.ops.NET_PARAMS, device='cuda')
    fn.ops.mlp_bwd(draw, act, net.flat, pb, dact, partial, grads)
    return fn.ops.ray_grad(rays, z, raw, noise, draw, act, dact, net.flat, **kw), grads


def run_case(fn, c, **kw):
    return run_pass(fn, c['net'], c['rays'], c['z'], c['g_rgb'], c['noise'], c['white'], **kw)[0]


@pytest.mark.parametrize('n,S', SHAPES)
def test_pass_parity_with_float64_autograd(fn, mode, n, S):
    c = case(fn, n, S)
    d_rays = run_case(fn, c)
    torch.cuda.synchronize()
    assert d_rays.shape == (n, 11)
    assert (d_rays[:, 6:8] == 0).all(), 'near / far are constants: exact zeros'
    check_groups('(%d,%d)' % (n, S), mode, d_rays, c)


def test_pass_without_view_directions(fn, mode):
    n, S = 3, 67
    c = case(fn, n, S, viewdirs=False)
    d_rays = run_case(fn, c)
    assert (d_rays[:, 6:11] == 0).all(), 'no view directions: their columns (and near / far) are exact zeros'
    check_groups('noview (%d,%d)' % (n, S), mode, d_rays, c)


def test_canaries_accumulate_determinism_and_placement(fn, mode):
    n, S = 3, 67
    c = case(fn, n, S)
    d1 = run_case(fn, c)
    assert torch.equal(run_case(fn, c), d1), 'two calls must agree bit for bit'
    buf = torch.full((n + 4, 11), float('nan'), device='cuda')
    d2 = run_case(fn, c, d_rays=buf)
    torch.cuda.synchronize()
    assert d2.data_ptr() == buf.data_ptr() and torch.equal(buf[:n], d1)
    assert torch.isnan(buf[n:]).all(), 'rows behind the batch were written'
    base = torch.randn(n + 4, 11, generator=torch.Generator().manual_seed(1)).cuda()
    acc = base.clone()
    run_case(fn, c, d_rays=acc, accumulate=True)
    assert torch.equal(acc[:n], base[:n] + d1) and torch.equal(acc[n:], base[n:])
    # the same rays at other positions of a larger batch
    perm = torch.tensor([2, 0, 1, 2, 0], device='cuda')
    d5, _ = run_pass(fn, c['net'], c['rays'][perm].contiguous(), c['z'][perm].contiguous(), c['g_rgb'][perm].contiguous(),
                     c['noise'][perm].contiguous(), c['white'])
    assert torch.equal(d5, d1[perm])


def test_errors(fn):
    old = fn.ops.get_math()
    try:
        fn.ops.set_math('fp32')
        c = case(fn, 3, 67)
        with pytest.raises(RuntimeError, match='kind'):
            run_case(fn, c, kind=1)
        lib = fn._lib.lib()
        null = ctypes.c_void_p(None)
        rc = lib.fastnerf_ray_grad(1, 0, 3, 67, *([null] * 9), 0, null, null)      # scalar checks come before any pointer
        assert rc == -1 and b'bf16x3' in lib.fastnerf_last_error()
        assert lib.fastnerf_ray_grad(0, 0, 0, 67, *([null] * 9), 0, null, null) == 0, 'n == 0 returns before any pointer is touched'
        assert lib.fastnerf_ray_grad(0, 0, 3, 67, *([null] * 9), 0, null, null) == -1
        fn.ops.set_math('bf16x3')
        with pytest.raises(NotImplementedError, match='bf16x3'):
            run_case(fn, c)
        rb = torch.zeros(4, 11, device='cuda')
        rb[:, 5], rb[:, 6], rb[:, 7], rb[:, 10] = -1.0, 2.0, 6.0, -1.0
        with pytest.raises(NotImplementedError, match='bf16x3'):
            fn.render.render_rays(rb.requires_grad_(), c['net'], None, 16)
    finally:
        fn.ops.set_math(old)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
N_RAYS, N_SAMPLES, N_IMP = 5, 16, 8


def e2e_batch():
    gen = torch.Generator().manual_seed(21)
    ro = torch.randn(N_RAYS, 3, generator=gen) * 0.4
    rd = torch.randn(N_RAYS, 3, generator=gen)
    rb = O.make_ray_batch(ro, rd, 2.0, 6.0)
    return rb, torch.randn(N_RAYS, 3, generator=gen), torch.randn(N_RAYS, 3, generator=gen)


def oracle_render_grads(sd_c, sd_f, rb, G1, G0, dtype):
    rb = rb.to(dtype).clone().requires_grad_(True)
    ret = O.render_rays(rb, sd_c, sd_f, N_SAMPLES, N_IMP)
    loss = (ret['rgb_map'] * G1.to(dtype)).sum() + (ret['rgb0'] * G0.to(dtype)).sum()
    return torch.autograd.grad(loss, rb)[0]


_E2E = {}


def e2e(fn, shared):
    if shared not in _E2E:
        net_c = make_net(fn, 31)
        net_f = None if shared else make_net(fn, 32)
        rb, G1, G0 = e2e_batch()
        refs = [oracle_render_grads(state(net_c, dt), None if shared else state(net_f, dt), rb, G1, G0, dt)
                for dt in (torch.float64, torch.float32)]
        _E2E[shared] = dict(net_c=net_c, net_f=net_f, rb=rb.cuda(), G1=G1.cuda(), G0=G0.cuda(), ref64=refs[0], viewdirs=True,
                            e32=group_errors(refs[1], refs[0]))
    return _E2E[shared]


def fused_backward(fn, c, rb):
    nets = [c['net_c']] + ([c['net_f']] if c['net_f'] is not None else [])
    for net in nets:
        for p in net.parameters():
            p.grad = None
    out = fn.render.render_rays(rb, c['net_c'], None, N_SAMPLES, N_importance=N_IMP, network_fine=c['net_f'], perturb=0.)
    ((out['rgb_map'] * c['G1']).sum() + (out['rgb0'] * c['G0']).sum()).backward()
    return out, [p.grad.clone() for net in nets for p in net.parameters()]


@pytest.mark.parametrize('shared', [False, True], ids=['two_nets', 'shared_net'])
def test_render_rays_ray_gradients(fn, mode, shared):
    """ray_batch.grad against the oracle, and the parameter gradients bit-identical to those of the same call with rays that do not
    require grad.  That call runs with FASTNERF_COMPACT=0: rays that require grad force the saving backward, whose kernels, inputs and
    order this route repeats; the compacted backward groups its partial sums differently (tests/test_gpu_compact.py: 3e-6 relative)."""
    c = e2e(fn, shared)
    old = fn.render.get_compact()
    try:
        fn.render.set_compact('0')
        out0, grads0 = fused_backward(fn, c, c['rb'])
        rb = c['rb'].clone().requires_grad_()
        out1, grads1 = fused_backward(fn, c, rb)
    finally:
        fn.render.set_compact(old)
    assert rb.grad is not None and rb.grad.shape == (N_RAYS, 11)
    assert (rb.grad[:, 6:8] == 0).all()
    for k in out0:
        assert torch.equal(out0[k], out1[k]), k
    assert len(grads0) == len(grads1) and all(torch.equal(a, b) for a, b in zip(grads0, grads1))
    # (E32 is about 3e-4 for o and d here: the float32 and the float64 oracle draw their fine samples from their own coarse weights.
    # A bound of 16 E32 would not notice a small error in one term; the per-pass tests above carry the tight bounds, this one the plumbing.)
    check_groups('render_rays %s' % ('shared' if shared else 'two nets'), mode, rb.grad, c)
    if not shared:      # under the default policy the rays' gradient is the same (the saving route is forced)
        rb2 = c['rb'].clone().requires_grad_()
        fused_backward(fn, c, rb2)
        assert torch.equal(rb2.grad, rb.grad)


def test_render_rays_unchanged_without_ray_gradients(fn, mode):
    """A detached batch: the recorded forward gives the values of the torch.no_grad() forward, bit for bit, and no ray gradient."""
    c = e2e(fn, False)
    kw = dict(N_importance=N_IMP, network_fine=c['net_f'], perturb=0., retraw=True)
    with torch.no_grad():
        ref = fn.render.render_rays(c['rb'], c['net_c'], None, N_SAMPLES, **kw)
    rec = fn.render.render_rays(c['rb'].detach(), c['net_c'], None, N_SAMPLES, **kw)
    assert rec['rgb_map'].requires_grad and not ref['rgb_map'].requires_grad
    assert set(rec) == set(ref)
    for k in ref:
        assert torch.equal(rec[k].detach(), ref[k]), k
    rb = c['rb'].clone().requires_grad_()
    with torch.no_grad():
        off = fn.render.render_rays(rb, c['net_c'], None, N_SAMPLES, **kw)
    assert all(torch.equal(off[k], ref[k]) for k in ref) and not off['rgb_map'].requires_grad


def test_render_rays_without_view_directions(fn, mode):
    """An [N, 8] batch gets an [N, 8] gradient."""
    net = case(fn, 3, 67, viewdirs=False)['net']
    rb = e2e_batch()[0][:, :8].cuda().requires_grad_()
    out = fn.render.render_rays(rb, net, None, N_SAMPLES)
    out['rgb_map'].sum().backward()
    assert rb.grad.shape == (N_RAYS, 8) and torch.isfinite(rb.grad).all() and (rb.grad[:, 6:8] == 0).all()
    assert float(rb.grad[:, 0:6].abs().max()) > 0


def test_occupancy_grid_refuses_ray_gradients(fn):
    net = case(fn, 3, 67)['net']
    for p in net.parameters():
        p.requires_grad_(False)
    try:
        grid = fn.occupancy.OccupancyGrid.from_mask(torch.ones(2, 2, 2, dtype=torch.bool, device='cuda'), (-8., -8., -8.), (8., 8., 8.))
        rb = e2e_batch()[0].cuda().requires_grad_()
        with pytest.raises(ValueError, match='occupancy'):
            fn.render.render_rays(rb, net, None, N_SAMPLES, occupancy=grid)
    finally:
        for p in net.parameters():
            p.requires_grad_(True)


def test_closure_route_ray_gradients(fn):
    """Any torch network behind a query function written in torch (C.cpu_query: the oracle's posenc; a closure that encodes with the
    HIP posenc op cuts the graph itself): the points and view directions are differentiated by torch, dists * |d| through the
    compositing's logit."""
    c = e2e(fn, False)
    wc, wf = C.Wrapped(c['net_c']).cuda(), C.Wrapped(c['net_f']).cuda()
    rb = c['rb'].clone().requires_grad_()
    out = fn.render.render_rays(rb, wc, C.cpu_query, N_SAMPLES, N_importance=N_IMP, network_fine=wf, perturb=0.)
    ((out['rgb_map'] * c['G1']).sum() + (out['rgb0'] * c['G0']).sum()).backward()
    check_groups('closure route', 'torch', rb.grad, c)


H, W = 4, 6
K = [[7.0, 0.0, 3.0], [0.0, 7.0, 2.0], [0.0, 0.0, 1.0]]


def oracle_pose_grad(sd_c, sd_f, pose, G1, G0, dtype):
    """get_rays and make_ray_batch of the oracle work in float32 whatever they are given (the rays the kernels see); the
    rendering behind them runs in `dtype`."""
    pose = pose.clone().requires_grad_(True)
    ro, rd = O.get_rays(H, W, K, pose)
    rb = O.make_ray_batch(ro, rd, 2.0, 6.0).to(dtype)
    ret = O.render_rays(rb, sd_c, sd_f, N_SAMPLES, N_IMP)
    loss = (ret['rgb_map'] * G1.to(dtype)).sum() + (ret['rgb0'] * G0.to(dtype)).sum()
    return torch.autograd.grad(loss, pose)[0]


def test_render_pose_gradient(fn, mode):
    c = e2e(fn, False)
    pose0 = fn.synthetic.pose_spherical(30.0, -30.0, 4.0)[:3, :4].float().cpu()
    gen = torch.Generator().manual_seed(8)
    G1, G0 = torch.randn(H * W, 3, generator=gen), torch.randn(H * W, 3, generator=gen)
    if 'pose64' not in c:
        c['pose64'], c['pose32'] = [oracle_pose_grad(state(c['net_c'], dt), state(c['net_f'], dt), pose0, G1, G0, dt)
                                    for dt in (torch.float64, torch.float32)]
    e32 = {'R': R.rel_l2(c['pose32'][:, :3], c['pose64'][:, :3]), 't': R.rel_l2(c['pose32'][:, 3], c['pose64'][:, 3])}
    kw = dict(network_fn=c['net_c'], network_fine=c['net_f'], network_query_fn=None, N_samples=N_SAMPLES, N_importance=N_IMP,
              perturb=0., use_viewdirs=True, near=2., far=6.)
    pose = pose0.clone().requires_grad_()
    rgb, _, _, extras = fn.render.render(H, W, K, c2w=pose, ndc=False, **kw)
    assert rgb.shape == (H, W, 3)
    ((rgb.reshape(-1, 3) * G1.cuda()).sum() + (extras['rgb0'].reshape(-1, 3) * G0.cuda()).sum()).backward()
    assert pose.grad is not None and pose.grad.shape == (3, 4)
    errs = {'R': R.rel_l2(pose.grad[:, :3], c['pose64'][:, :3]), 't': R.rel_l2(pose.grad[:, 3], c['pose64'][:, 3])}
    for name in errs:
        print('\npose %-6s %s err %.3e  E32 %.3e  bound %.3e' % (mode, name, errs[name], e32[name], FACTOR * e32[name]))
    for name in errs:
        assert errs[name] <= FACTOR * e32[name], (name, errs[name], e32[name])
    with pytest.raises(NotImplementedError, match='ndc'):
        fn.render.render(H, W, K, c2w=pose0.clone().requires_grad_(), ndc=True, **kw)
