"""render_rays / run_network with a network that is not a fastnerf NeRF (the closure route): the reference's
`network_query_fn(pts, viewdirs, net)` is called on the points of both passes, sampling and compositing run on the HIP
kernels, and every map is differentiable to the network's parameters.  Checked against a CPU restatement built from the
oracle (posenc / coarse_z / raw2outputs / sample_pdf on a CPU copy of the same module), against the fused 8 x 256 route on
the same weights, in a short training run, and for the routing rules."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

N_RAYS, N_SAMPLES, N_IMP = 256, 64, 128


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return fastnerf


class SmallMLP(nn.Module):
    """D x W ReLU trunk -> sigma, + a view branch -> rgb; `out_ch` > 4 pads extra channels (the reference's output_ch = 5)."""

    def __init__(self, D=4, W=128, in_ch=63, in_views=27, out_ch=4):
        super().__init__()
        self.in_ch, self.in_views, self.out_ch = in_ch, in_views, out_ch
        self.trunk = nn.ModuleList([nn.Linear(in_ch, W)] + [nn.Linear(W, W) for _ in range(D - 1)])
        self.sigma = nn.Linear(W, 1)
        self.head = nn.Linear(W + in_views, W // 2)
        self.rgb = nn.Linear(W // 2, 3 + out_ch - 4)
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, nn.Linear):
                    nn.init.normal_(m.weight, std=1.2 / m.in_features ** 0.5)
                    nn.init.uniform_(m.bias, -0.1, 0.1)

    def forward(self, x):
        h = x[..., :self.in_ch]
        for lin in self.trunk:
            h = torch.relu(lin(h))
        c = torch.relu(self.head(torch.cat([h, x[..., self.in_ch:]], -1)))
        rgbx = self.rgb(c)
        return torch.cat([rgbx[..., :3], self.sigma(h), rgbx[..., 3:]], -1)


def make_nets(viewdirs, two, out_ch=4, seed=0):
    torch.manual_seed(seed)
    nv = 27 if viewdirs else 0
    c = SmallMLP(in_views=nv, out_ch=out_ch)
    f = SmallMLP(in_views=nv, out_ch=out_ch) if two else None
    return c, f


def query_fn(fn, netchunk=1024 * 64):
    embed, _ = fn.run_nerf_helpers.get_embedder(10)
    embed_d, _ = fn.run_nerf_helpers.get_embedder(4)
    return lambda pts, vd, net: fn.run_nerf.run_network(pts, vd, net, embed_fn=embed, embeddirs_fn=embed_d, netchunk=netchunk)


def cpu_query(pts, viewdirs, net):
    flat = pts.reshape(-1, 3)
    emb = O.posenc(flat, 10)
    if viewdirs is not None:
        emb = torch.cat([emb, O.posenc(viewdirs[:, None].expand(pts.shape).reshape(-1, 3), 4)], -1)
    out = net(emb)
    return out.reshape(list(pts.shape[:-1]) + [out.shape[-1]])


def pytest_rand(shape):
    np.random.seed(0)
    return torch.Tensor(np.random.rand(*shape))


def cpu_render(rb, net_c, net_f, Ni, white):
    """CPU restatement of render_rays(perturb=1, raw_noise_std=1, pytest=True) with the closure."""
    n, S = rb.shape[0], N_SAMPLES
    ro, rd = rb[:, 0:3], rb[:, 3:6]
    vd = rb[:, -3:] if rb.shape[-1] > 8 else None
    z = O.coarse_z(rb[:, 6:7], rb[:, 7:8], S, False, pytest_rand((n, S)))
    raw = cpu_query(ro[..., None, :] + rd[..., None, :] * z[..., :, None], vd, net_c)[..., :4]
    rgb, disp, acc, w, depth = O.raw2outputs(raw, z, rd, pytest_rand((n, S)), white)
    out = {'rgb_map': rgb, 'disp_map': disp, 'acc_map': acc, 'depth_map': depth}
    if Ni > 0:
        out.update(rgb0=rgb, disp0=disp, acc0=acc, depth0=depth)
        zs = O.sample_pdf(0.5 * (z[..., 1:] + z[..., :-1]), w[..., 1:-1], Ni, pytest_rand((n, Ni))).detach()
        z1 = torch.sort(torch.cat([z, zs], -1), -1)[0]
        raw = cpu_query(ro[..., None, :] + rd[..., None, :] * z1[..., :, None], vd, net_f if net_f is not None else net_c)[..., :4]
        rgb, disp, acc, w, depth = O.raw2outputs(raw, z1, rd, pytest_rand((n, S + Ni)), white)
        out.update(rgb_map=rgb, disp_map=disp, acc_map=acc, depth_map=depth, z_vals=z1)
    return out


def ray_batch(viewdirs, n=N_RAYS, seed=3):
    g = torch.Generator().manual_seed(seed)
    ro = torch.randn(n, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, 4.0])
    rd = -ro / ro.norm(dim=-1, keepdim=True) + 0.3 * torch.randn(n, 3, generator=g)
    return O.make_ray_batch(ro, rd, 2.0, 6.0, use_viewdirs=viewdirs)


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def loss_of(out, tgt, Ni):
    # (render_rays does not return the depth map: its term enters through the disparity, which is a function of it)
    l = O.img2mse(out['rgb_map'], tgt) + 0.1 * out['disp_map'].mean() + 0.1 * out['acc_map'].mean()
    if Ni > 0:
        l = l + O.img2mse(out['rgb0'], tgt) + 0.1 * out['disp0'].mean() + 0.1 * out['acc0'].mean()
    return l


@pytest.mark.parametrize('viewdirs', [False, True])
@pytest.mark.parametrize('Ni', [0, N_IMP])
@pytest.mark.parametrize('white', [False, True])
def test_closure_route_against_the_cpu_oracle(fn, viewdirs, Ni, white):
    net_c, net_f = make_nets(viewdirs, Ni > 0)
    cpu_c, cpu_f = copy.deepcopy(net_c), copy.deepcopy(net_f)
    net_c.cuda()
    if net_f is not None:
        net_f.cuda()
    rb = ray_batch(viewdirs)
    tgt = torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(9))
    out = fn.render.render_rays(rb.cuda(), net_c, query_fn(fn), N_SAMPLES, retraw=True, perturb=1.0, N_importance=Ni,
                                network_fine=net_f, white_bkgd=white, raw_noise_std=1.0, pytest=True)
    ref = cpu_render(rb, cpu_c, cpu_f, Ni, white)
    keys = ['rgb_map', 'disp_map', 'acc_map'] + (['rgb0', 'disp0', 'acc0', 'z_std'] if Ni > 0 else [])
    assert set(out) == set(keys) | {'raw'}
    for k in [k for k in keys if k != 'z_std']:
        err = (out[k].detach().cpu() - ref[k].detach()).abs().max()
        assert err <= 1e-4, (k, float(err))
    assert out['raw'].shape == (N_RAYS, N_SAMPLES + Ni, 4)
    # coarse-net gradients straight from the route
    gl = torch.autograd.grad(loss_of(out, tgt.cuda(), Ni), list(net_c.parameters()))
    gr = torch.autograd.grad(loss_of(ref, tgt, Ni), list(cpu_c.parameters()))
    for (name, _), a, b in zip(net_c.named_parameters(), gl, gr):
        assert rel(a.cpu(), b) <= 2e-3, ('coarse', name, rel(a.cpu(), b))
    if Ni > 0:
        # fine net: replayed at the CPU's fine depths (inverse-CDF conditioning moves a few fine depths, as in the fused route)
        zf = ref['z_vals']
        rd = rb[:, 3:6]
        pts = (rb[:, None, 0:3] + rd[:, None, :] * zf[..., None]).cuda()
        vd = rb[:, -3:].cuda() if viewdirs else None
        raw = query_fn(fn)(pts, vd, net_f)
        rgb, disp, acc, _, _ = fn.render.raw2outputs(raw, zf.cuda(), rd.cuda(), 1.0, white, pytest=True)
        lg = O.img2mse(rgb, tgt.cuda()) + 0.1 * disp.mean() + 0.1 * acc.mean()
        lc = O.img2mse(ref['rgb_map'], tgt) + 0.1 * ref['disp_map'].mean() + 0.1 * ref['acc_map'].mean()
        gl = torch.autograd.grad(lg, list(net_f.parameters()))
        gr = torch.autograd.grad(lc, list(cpu_f.parameters()))
        for (name, _), a, b in zip(net_f.named_parameters(), gl, gr):
            assert rel(a.cpu(), b) <= 2e-3, ('fine', name, rel(a.cpu(), b))


class Wrapped(nn.Module):
    """A fastnerf 8 x 256 NeRF's weights as leaf parameters of a plain torch module (oracle.nerf_forward)."""

    def __init__(self, net):
        super().__init__()
        self.names = list(net.state_dict().keys())
        self.p = nn.ParameterList([nn.Parameter(v.detach().clone()) for v in net.state_dict().values()])

    def forward(self, x):
        return O.nerf_forward(dict(zip(self.names, self.p)), x)


@pytest.mark.parametrize('mode', ['fp32', None])
@pytest.mark.parametrize('Ni', [0, N_IMP])
def test_closure_route_matches_the_fused_route(fn, mode, Ni):
    old = fn.ops.get_math()
    try:
        if mode is not None:
            fn.ops.set_math(mode)
        torch.manual_seed(1)
        args = fn.run_nerf.make_args(N_importance=Ni, N_samples=N_SAMPLES, perturb=1.0, white_bkgd=True, no_reload=True)
        ktr, _, _, _, _, _ = fn.run_nerf.create_nerf(args)
        nc, nf = ktr['network_fn'], ktr['network_fine']
        wc, wf = Wrapped(nc), (Wrapped(nf) if nf is not None else None)
        rb = ray_batch(True).cuda()
        tgt = torch.rand(N_RAYS, 3, generator=torch.Generator().manual_seed(9)).cuda()
        kw = dict(retraw=False, perturb=1.0, N_importance=Ni, white_bkgd=True, raw_noise_std=1.0, pytest=True)
        fused = fn.render.render_rays(rb, nc, ktr['network_query_fn'], N_SAMPLES, network_fine=nf, **kw)
        clos = fn.render.render_rays(rb, wc, query_fn(fn), N_SAMPLES, network_fine=wf, **kw)
        for k in fused:
            err = (fused[k].detach() - clos[k].detach()).abs().max()
            assert err <= 1e-4, (k, float(err))
        if Ni == 0:
            ga = torch.autograd.grad(O.img2mse(fused['rgb_map'], tgt), list(nc.parameters()))
            gb = torch.autograd.grad(O.img2mse(clos['rgb_map'], tgt), list(wc.parameters()))
            for name, a, b in zip(wc.names, ga, gb):
                assert rel(b, a) <= 2e-3, (name, rel(b, a))
    finally:
        fn.ops.set_math(old)


def train_losses(fn, iters=30, seed=0):
    H = W = 32
    images, poses, focal = fn.synthetic.make_dataset(n_images=4, H=H, W=W)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    torch.manual_seed(seed)
    net_c, net_f = make_nets(True, True, out_ch=5, seed=seed)
    net_c.cuda(); net_f.cuda()
    opt = torch.optim.Adam(list(net_c.parameters()) + list(net_f.parameters()), lr=5e-4, betas=(0.9, 0.999))
    kw = dict(network_fn=net_c, network_fine=net_f, network_query_fn=query_fn(fn), N_samples=32, N_importance=32, perturb=1.0,
              white_bkgd=True, raw_noise_std=0.0, near=2.0, far=6.0, use_viewdirs=True, ndc=False)
    rays = [fn.run_nerf_helpers.get_rays(H, W, K, poses[i]) for i in range(images.shape[0])]
    imgs = torch.as_tensor(images).float().cuda()
    losses = []
    for it in range(iters):
        i = int(torch.randint(0, len(rays), (1,)))
        sel = torch.randint(0, H * W, (256,)).cuda()
        ro, rd = rays[i][0].reshape(-1, 3)[sel], rays[i][1].reshape(-1, 3)[sel]
        tgt = imgs[i].reshape(-1, 3)[sel]
        rgb, _, _, extras = fn.render.render(H, W, K, chunk=1024, rays=torch.stack([ro, rd], 0), retraw=True, **kw)
        assert extras['raw'].shape[-1] == 5
        loss = fn.run_nerf_helpers.img2mse(rgb, tgt) + fn.run_nerf_helpers.img2mse(extras['rgb0'], tgt)
        opt.zero_grad()
        loss.backward()
        opt.step()
        for group in opt.param_groups:
            group['lr'] = 5e-4 * 0.1 ** (it / (500 * 1000))
        losses.append(float(loss))
    return losses


def test_short_training_run_with_a_custom_network(fn):
    a = train_losses(fn)
    b = train_losses(fn)
    assert a == b, 'two identically seeded runs give bit-identical losses'
    assert np.mean(a[-5:]) < 0.9 * np.mean(a[:5]), (a[:5], a[-5:])


def test_routing(fn):
    torch.manual_seed(0)
    args = fn.run_nerf.make_args(N_importance=16, N_samples=16, perturb=0.0, white_bkgd=True, no_reload=True)
    ktr, _, _, _, _, _ = fn.run_nerf.create_nerf(args)
    rb = ray_batch(True, n=64).cuda()

    def refuse(*a):
        raise AssertionError('the fused route must not call network_query_fn')
    with torch.no_grad():
        out = fn.render.render_rays(rb, ktr['network_fn'], refuse, 16, N_importance=16, network_fine=ktr['network_fine'])
        ref = fn.render.render_rays(rb, ktr['network_fn'], ktr['network_query_fn'], 16, N_importance=16,
                                    network_fine=ktr['network_fine'])
    assert torch.equal(out['rgb_map'], ref['rgb_map'])
    small, _ = make_nets(True, False)
    small.cuda()
    with pytest.raises(TypeError):
        fn.render.render_rays(rb, ktr['network_fn'], query_fn(fn), 16, N_importance=16, network_fine=small)
    with pytest.raises(TypeError):
        fn.render.render_rays(rb, small, query_fn(fn), 16, N_importance=16, network_fine=ktr['network_fine'])
    # run_network with a custom network: the reference's flatten / embed / batchify / reshape, differentiable
    pts = torch.rand(8, 5, 3).cuda()
    vd = torch.nn.functional.normalize(torch.randn(8, 3), dim=-1).cuda()
    out = query_fn(fn, netchunk=7)(pts, vd, small)
    assert out.shape == (8, 5, 4) and out.requires_grad
    ref = cpu_query(pts.cpu(), vd.cpu(), copy.deepcopy(small).cpu())
    assert (out.detach().cpu() - ref.detach()).abs().max() < 1e-4
    # render() builds [N,8] / [N,11] batches for a custom network from use_viewdirs alone
    K = np.array([[40.0, 0, 8.0], [0, 40.0, 8.0], [0, 0, 1]])
    c2w = fn.synthetic.pose_spherical(30.0, -30.0, 4.0)[:3, :4]
    noview, _ = make_nets(False, False)
    noview.cuda()
    for net, uv in ((small, True), (noview, False)):
        rgb, disp, acc, _ = fn.render.render(16, 16, K, c2w=c2w, near=2.0, far=6.0, ndc=False, use_viewdirs=uv, network_fn=net,
                                             network_query_fn=query_fn(fn), N_samples=16)
        assert rgb.shape == (16, 16, 3) and torch.isfinite(rgb).all()
