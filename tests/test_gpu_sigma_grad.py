"""d(sigma)/d(x) through the fused MLP (csrc/sigma_grad.hip, ops.mlp_sigma_grad, NeRF.density_gradient, mesh.vertex_normals)
against float64 autograd of the module's own torch forward, in every math mode.

Reference: NeRF.forward of a .double() copy of the network on a float64 positional encoding written out below, differentiated by
torch.autograd with respect to the points -- the kernels' own fp32 points o + d*z (one rounded product, one rounded sum).
Metric: relative L2 error over the whole batch, of grad and separately of sigma; no point is excluded.
Bound: not chosen in advance.  E32 is the same metric for torch's float32 autograd of the same forward (CPU) at the same points
against the same float64 result: it holds the ReLU decisions that flip within rounding and the conditioning of the 2^9 frequency
that any fp32 evaluation has.  fp32 and bf16x6 stay within 16 E32 (the spread the README documents for this project's
first-layer gradients against fp64, and dY0 is what the kernel consumes); bf16x3 within 32 times that (the ratio of the RMS
logit errors in the header of tests/test_gpu_mlp_fp64.py, 2.2e-7 against 7e-9).

Shapes (n, S): (1, 1) one point, (3, 67) a ragged tail, (5, 64) exact 64-point tiles, (2, 129) one point past a tile.  Points: a ray
runs between two uniform draws a, b of [-1.5, 1.5]^3 (o = a, d = b - a, z uniform in [0, 1]), so every sample lies in the box; from
two rays on, the last ray starts at the origin with z = 0 for its first sample (the origin itself) and the ray before it has
o_y = d_y = 0 (a coordinate of exactly 0).  Every figure is printed before it is asserted (pytest -s shows them)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 67), (5, 64), (2, 129)]
FACTOR = {'fp32': 16.0, 'bf16x6': 16.0, 'bf16x3': 16.0 * 32.0}


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


def posenc(x):
    """Embedder (run_nerf_helpers.py): [x, sin(2^0 x), cos(2^0 x), ..., sin(2^9 x), cos(2^9 x)] in x's dtype."""
    out = [x]
    for k in range(10):
        out += [torch.sin(x * 2.0 ** k), torch.cos(x * 2.0 ** k)]
    return torch.cat(out, -1)


def make_net(fn, seed, viewdirs=True):
    torch.manual_seed(seed)
    return fn.model.NeRF(use_viewdirs=viewdirs, input_ch_views=27 if viewdirs else 0)


def host_copy(fn, net, dtype):
    m = fn.model.NeRF(use_viewdirs=net.use_viewdirs, input_ch_views=net.input_ch_views, output_ch=net.output_ch)
    m.load_state_dict(net.state_dict())
    return m.to(device='cpu', dtype=dtype)


def autograd_sigma_grad(net, pts):
    """(sigma [P], grad [P,3]) of net.forward on posenc(pts), by autograd, in pts' dtype."""
    x = pts.clone().requires_grad_(True)
    inp = torch.cat([posenc(x), torch.zeros(x.shape[0], net.input_ch_views, dtype=x.dtype)], -1)
    sigma = net(inp)[..., 3]
    grad, = torch.autograd.grad(sigma.sum(), x)
    return sigma.detach(), grad


def make_rays(n, S, seed):
    """rays11 [n,11], z [n,S] (CPU, fp32) and the fp32 points [n*S,3] the kernels compute from them."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand(n, 3, generator=gen) * 3 - 1.5
    b = torch.rand(n, 3, generator=gen) * 3 - 1.5
    z = torch.rand(n, S, generator=gen)
    o, d = a.clone(), b - a
    if n >= 2:
        o[n - 1] = 0
        z[n - 1, 0] = 0
        o[n - 2, 1] = 0
        d[n - 2, 1] = 0
    rays = torch.zeros(n, 11)
    rays[:, 0:3], rays[:, 3:6] = o, d
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3)     # separate roundings, as the kernels
    if n >= 2:
        assert (pts[(n - 1) * S] == 0).all() and (pts[(n - 2) * S:(n - 1) * S, 1] == 0).all()
    return rays, z, pts


_CASES = {}


def case(fn, n, S, viewdirs=True):
    """One network, one batch and its references per (shape, kind of network), computed once and shared by every test and mode."""
    key = (n, S, viewdirs)
    if key not in _CASES:
        net = make_net(fn, 1000 + 10 * n + S + (0 if viewdirs else 5), viewdirs)
        rays, z, pts = make_rays(n, S, 77 + n * S)
        s64, g64 = autograd_sigma_grad(host_copy(fn, net, torch.float64), pts.double())
        s32, g32 = autograd_sigma_grad(host_copy(fn, net, torch.float32), pts)
        e32 = (rel_l2(s32, s64), rel_l2(g32, g64))
        _CASES[key] = dict(net=net, rays=rays.cuda(), z=z.cuda(), pts=pts, s64=s64, g64=g64, e32=e32)
    return _CASES[key]


def rel_l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def run(fn, c, **kw):
    pf, pb = c['net'].packed()
    return fn.ops.mlp_sigma_grad(c['rays'], c['z'], c['net'].flat, pf, pb, **kw)


def check_parity(fn, c, mode, what):
    sigma, grad = run(fn, c)
    torch.cuda.synchronize()
    es, eg = rel_l2(sigma.reshape(-1).cpu(), c['s64']), rel_l2(grad.reshape(-1, 3).cpu(), c['g64'])
    e32s, e32g = c['e32']
    print('\n%s %-7s sigma: err %.3e  E32 %.3e  bound %.3e | grad: err %.3e  E32 %.3e  bound %.3e'
          % (what, mode, es, e32s, FACTOR[mode] * e32s, eg, e32g, FACTOR[mode] * e32g))
    assert torch.isfinite(grad).all() and torch.isfinite(sigma).all()
    assert eg <= FACTOR[mode] * e32g, (what, mode, 'grad', eg, e32g)
    assert es <= FACTOR[mode] * e32s, (what, mode, 'sigma', es, e32s)
    return sigma, grad


@pytest.mark.parametrize('n,S', SHAPES)
def test_parity_with_float64_autograd(fn, math_mode, n, S):
    c = case(fn, n, S)
    sigma, grad = check_parity(fn, c, math_mode, '(%d,%d)' % (n, S))
    assert sigma.shape == (n, S) and grad.shape == (n, S, 3)
    # forward agreement: the logit is the plain forward's, bit for bit
    raw = fn.ops.mlp_fwd(c['rays'], c['z'], c['net'].flat, c['net'].packed()[0])
    assert torch.equal(sigma, raw[..., 3])


def test_no_view_directions(fn, math_mode):
    """A use_viewdirs=False network runs on its equivalent kernel network; same bound, against the autograd of ITS forward."""
    n, S = 3, 67
    c = case(fn, n, S, viewdirs=False)
    check_parity(fn, c, math_mode, 'noview (%d,%d)' % (n, S))
    sigma, grad = c['net'].density_gradient(c['pts'].cuda().reshape(n, S, 3), chunk=100)    # three chunks, the last ragged
    s2, g2 = run(fn, c)
    assert sigma.shape == (n, S) and grad.shape == (n, S, 3)
    assert rel_l2(grad.reshape(-1, 3).cpu(), c['g64']) <= FACTOR[math_mode] * c['e32'][1]
    assert rel_l2(sigma.reshape(-1).cpu(), c['s64']) <= FACTOR[math_mode] * c['e32'][0]


def test_canaries_and_optional_sigma(fn, math_mode):
    n, S = 3, 67
    c = case(fn, n, S)
    P = n * S
    buf = torch.full((P + 64, 3), float('nan'), device='cuda')
    sigma, grad = run(fn, c, grad=buf, want_sigma=False)
    torch.cuda.synchronize()
    assert sigma is None
    assert grad.data_ptr() == buf.data_ptr() and torch.isfinite(buf[:P]).all()
    assert torch.isnan(buf[P:]).all(), 'rows of the partial last tile were written'
    _, g2 = run(fn, c)
    assert torch.equal(g2.reshape(-1, 3), buf[:P])


def test_determinism_and_tile_placement(fn, math_mode):
    """Two calls agree bit for bit, and so do the 201 points as 3 rays of 67 samples and as 201 rays of one sample (the rows land
    in the same 64-point tiles, but every ray / sample index differs; all three modes' forwards and dX chains work row by row)."""
    n, S = 3, 67
    c = case(fn, n, S)
    s1, g1 = run(fn, c)
    s2, g2 = run(fn, c)
    assert torch.equal(g1, g2) and torch.equal(s1, s2)
    P = n * S
    rays = torch.zeros(P, 11, device='cuda')
    rays[:, 0:3] = c['pts'].cuda()            # d = 0, z = 0: the point is o itself
    pf, pb = c['net'].packed()
    s3, g3 = fn.ops.mlp_sigma_grad(rays, torch.zeros(P, 1, device='cuda'), c['net'].flat, pf, pb)
    assert torch.equal(g3.reshape(-1, 3), g1.reshape(-1, 3)) and torch.equal(s3.reshape(-1), s1.reshape(-1))
    # and through the module, in chunks that cut the tiles elsewhere
    s4, g4 = c['net'].density_gradient(c['pts'].cuda(), chunk=70)
    assert torch.equal(g4, g1.reshape(-1, 3)) and torch.equal(s4, s1.reshape(-1))


def read_ply(path):
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    lines = raw[:end].decode('ascii').split('\n')
    V = int([l for l in lines if l.startswith('element vertex')][0].split()[-1])
    T = int([l for l in lines if l.startswith('element face')][0].split()[-1])
    nprop = sum(1 for l in lines if l.startswith('property float'))
    vb = np.frombuffer(raw, '<f4', V * nprop, end).reshape(V, nprop)
    fb = np.frombuffer(raw, np.dtype([('n', 'u1'), ('i', '<i4', (3,))]), T, end + V * nprop * 4)
    return vb, fb['i']


def test_mesh_with_normals(fn, math_mode, tmp_path):
    torch.manual_seed(5)
    args = fn.run_nerf.make_args(N_importance=16, use_viewdirs=True, no_reload=True)
    _, kw, _, _, _, _ = fn.run_nerf.create_nerf(args)
    N, bound = 16, 1.2
    t = torch.linspace(-bound, bound, N + 1, device='cuda')
    thr = float(fn.mesh.density_grid(kw['network_fine'], t, t, t).median())     # a level set the random network has
    v, tri, nrm = fn.mesh.extract_mesh(kw, N=N, bound=bound, threshold=thr, normals=True)
    assert v.shape[0] > 0 and tri.shape[0] > 0, 'the case must not pass on an empty mesh'
    assert nrm.shape == v.shape and nrm.is_cuda and torch.isfinite(nrm).all()
    length = nrm.double().norm(dim=-1)
    zero = (nrm == 0).all(-1)
    assert ((length - 1).abs() < 1e-6)[~zero].all() and int((~zero).sum()) > 0
    assert torch.equal(nrm, fn.mesh.vertex_normals(kw['network_fine'], v))
    v2, tri2 = fn.mesh.extract_mesh(kw, N=N, bound=bound, threshold=thr)
    assert torch.equal(v2, v) and torch.equal(tri2, tri)
    path = str(tmp_path / 'm.ply')
    fn.mesh.export_ply(path, v, tri, nrm)
    vb, faces = read_ply(path)
    assert vb.shape == (v.shape[0], 6)
    assert np.array_equal(vb[:, :3], v.cpu().numpy()) and np.array_equal(vb[:, 3:], nrm.cpu().numpy())
    assert np.array_equal(faces, tri.cpu().numpy())


def test_normals_of_a_flat_gradient_are_zero(fn):
    """Exactly (0, 0, 0), never NaN, where the gradient vanishes: a network whose trunk is switched off has sigma = the head's bias."""
    net = make_net(fn, 3)
    with torch.no_grad():
        net.alpha_linear.weight.zero_()
    pts = torch.rand(70, 3, device='cuda') * 2 - 1
    sigma, grad = net.density_gradient(pts)
    assert (grad == 0).all() and (sigma - net.alpha_linear.bias.detach()).abs().max() < 1e-6
    nrm = fn.mesh.vertex_normals(net, pts)
    assert (nrm == 0).all()


def test_errors(fn):
    net = make_net(fn, 4)
    with pytest.raises(RuntimeError):
        net.density_gradient(torch.zeros(5, 3))                      # a host tensor
    with pytest.raises(RuntimeError):
        net.density_gradient(np.zeros((5, 3), np.float32))           # a host array
    with pytest.raises(TypeError, match='fastnerf NeRF'):
        fn.mesh.vertex_normals(torch.nn.Linear(3, 4).cuda(), torch.zeros(5, 3, device='cuda'))
    assert net.density_gradient(torch.zeros(0, 3, device='cuda'))[1].shape == (0, 3)
    # packed weights of another math mode trip the guard of ops.mlp_fwd / ops.mlp_bwd
    old = fn.ops.get_math()
    try:
        fn.ops.set_math('fp32')
        pf, pb = fn.ops.mlp_pack(net.flat)
        fn.ops.set_math('bf16x6')
        rays, z = torch.zeros(4, 11, device='cuda'), torch.zeros(4, 1, device='cuda')
        with pytest.raises(AssertionError, match='math mode'):
            fn.ops.mlp_sigma_grad(rays, z, net.flat, pf, pb)
    finally:
        fn.ops.set_math(old)
