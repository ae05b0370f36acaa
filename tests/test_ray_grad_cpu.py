"""The per-ray formulas of csrc/ray_grad.hip, restated in torch float64 on the host, against float64 autograd of the oracle
(oracle.nerf_oracle.run_network + raw2outputs) with respect to a pass's rays: origin o, direction d and view direction v.

The restatement consumes what the kernels consume -- draw = d(loss)/d(raw) of the compositing alone (what raw2outputs_bwd yields),
g = d(loss)/d(point) (what sigma_grad_kernel yields from dY0 / dY5), dYv = the view layer's pre-activation gradient -- and applies
    d_o = sum_s g,   d_d = sum_s z g + c d / |d|^2,  c = sum_s draw[..., 3] (raw[..., 3] + noise),
    d_v = PE(4) chain rule on (sum_s dYv) Wv[:, 256:283],
so the |d| identity (dists = dz |d|  =>  dL/d|d| = sum_s dL/dsigma'_s sigma'_s / |d|, no division by dist), the linearity of the view
branch over a ray's samples and the two chain rules are pinned before any kernel runs.  Sizes n = 3, S = 5, with and without sigma
noise and white background; sample 2 of every ray duplicates sample 1 (dz = 0) and one sample has sigma' < 0 by construction.
Agreement is asked at float64 rounding: relative L2 <= 1e-12 per column group (sums of ~1e3 terms of double rounding 1.1e-16)."""
import pytest
import torch

from oracle import nerf_oracle as O

F64 = torch.float64


def rel_l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


def make_sd(seed, dtype=F64):
    gen = torch.Generator().manual_seed(seed)
    return {k: v.to(dtype) for k, v in O.init_nerf_params(gen).items()}


def pass_loss(sd, o, d, v, z, noise, white, g_rgb):
    """sum(rgb_map * g_rgb) of one pass (render.py:268-272 for given z), and its raw [n,S,4]."""
    pts = o[:, None, :] + d[:, None, :] * z[..., None]
    raw = O.run_network(sd, pts, v)
    rgb = O.raw2outputs(raw, z, d, noise, white)[0]
    return (rgb * g_rgb).sum(), raw


def autograd_ray_grads(sd, o, d, v, z, noise, white, g_rgb):
    """(d_o, d_d, d_v) [n,3] each, by autograd of the oracle, in the dtype of the inputs (v None: no view directions, d_v None)."""
    leaves = [t.clone().requires_grad_(True) for t in (o, d)] + ([v.clone().requires_grad_(True)] if v is not None else [])
    loss, _ = pass_loss(sd, leaves[0], leaves[1], leaves[2] if v is not None else None, z, noise, white, g_rgb)
    grads = torch.autograd.grad(loss, leaves)
    return grads[0], grads[1], (grads[2] if v is not None else None)


def restated_ray_grads(sd, o, d, v, z, noise, white, g_rgb):
    """The kernel's route: draw from the compositing alone, g and dYv from the network alone, then the per-ray formulas."""
    n, S = z.shape
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).clone().requires_grad_(True)
    # the network, written out so that the view layer's pre-activation is at hand (oracle nerf_forward, model.py:38-63)
    lin = torch.nn.functional.linear
    pe = O.posenc(pts.reshape(-1, 3), 10)
    vpe = O.posenc(v[:, None].expand(n, S, 3).reshape(-1, 3), 4)
    h = pe
    for i in range(8):
        h = torch.relu(lin(h, sd[f'pts_linears.{i}.weight'], sd[f'pts_linears.{i}.bias']))
        if i == 4:
            h = torch.cat([pe, h], -1)
    alpha = lin(h, sd['alpha_linear.weight'], sd['alpha_linear.bias'])
    feat = lin(h, sd['feature_linear.weight'], sd['feature_linear.bias'])
    yv = lin(torch.cat([feat, vpe], -1), sd['views_linears.0.weight'], sd['views_linears.0.bias'])
    yv.retain_grad()
    raw = torch.cat([lin(torch.relu(yv), sd['rgb_linear.weight'], sd['rgb_linear.bias']), alpha], -1).reshape(n, S, 4)
    # draw: the compositing with raw as the leaf (rays_d detached: what raw2outputs_bwd differentiates)
    raw_leaf = raw.detach().clone().requires_grad_(True)
    rgb = O.raw2outputs(raw_leaf, z, d, noise, white)[0]
    draw, = torch.autograd.grad((rgb * g_rgb).sum(), raw_leaf)
    raw.backward(draw)
    g = pts.grad                                   # [n,S,3]
    dyv = yv.grad.reshape(n, S, 128)
    sig = raw.detach()[..., 3] if noise is None else raw.detach()[..., 3] + noise
    c = (draw[..., 3] * sig).sum(-1)
    d_o = g.sum(1)
    d_d = (z[..., None] * g).sum(1) + c[:, None] * d / (d * d).sum(-1, keepdim=True)
    dvpe = dyv.sum(1) @ sd['views_linears.0.weight'][:, 256:283]          # [n,27]
    e = O.posenc(v, 4)
    d_v = dvpe[:, 0:3].clone()
    for k in range(4):
        s0, c0 = 3 + 6 * k, 6 + 6 * k
        d_v = d_v + 2.0 ** k * (dvpe[:, s0:s0 + 3] * e[:, c0:c0 + 3] - dvpe[:, c0:c0 + 3] * e[:, s0:s0 + 3])
    return d_o, d_d, d_v, draw, sig


@pytest.mark.parametrize('white', [False, True])
@pytest.mark.parametrize('with_noise', [False, True])
def test_per_ray_formulas_match_float64_autograd(with_noise, white):
    n, S = 3, 5
    sd = make_sd(11)
    gen = torch.Generator().manual_seed(5)
    o = (torch.rand(n, 3, generator=gen, dtype=F64) - 0.5)
    d = (torch.rand(n, 3, generator=gen, dtype=F64) - 0.5) * 1.5
    d[1, 2] = 0.0                                   # a zero coordinate in d
    v = d / d.norm(dim=-1, keepdim=True)
    z = torch.sort(torch.rand(n, S, generator=gen, dtype=F64) * 2, -1).values
    z[:, 2] = z[:, 1]                               # an interior sample duplicated: dz = 0
    g_rgb = torch.randn(n, 3, generator=gen, dtype=F64)
    # sigma' = raw[..., 3] + noise: move the density head's bias to the middle of the two smallest, so that the smallest alone is negative
    with torch.no_grad():
        _, raw = pass_loss(sd, o, d, v, z, None, white, g_rgb)
    noise_used = (torch.rand(n, S, generator=gen, dtype=F64) * 0.5) if with_noise else None
    lo = torch.unique(raw[..., 3] if noise_used is None else raw[..., 3] + noise_used)      # sorted; the duplicated sample counts once
    sd['alpha_linear.bias'] = sd['alpha_linear.bias'] - 0.5 * (lo[0] + lo[1])
    do64, dd64, dv64 = autograd_ray_grads(sd, o, d, v, z, noise_used, white, g_rgb)
    d_o, d_d, d_v, draw, sig = restated_ray_grads(sd, o, d, v, z, noise_used, white, g_rgb)
    assert 1 <= int((sig < 0).sum()) <= 2, 'the case needs one sample with sigma < 0 (two when it is the duplicated one)'
    assert (draw[..., 3][sig < 0] == 0).all() and (draw[:, 1, 3] == 0).all(), 'sigma <= 0 and dz = 0 contribute exact zeros'
    assert (draw[:, -1, 3] == 0).all(), 'the last sample (dist 1e10 |d|) contributes an exact zero'
    assert float(draw[..., 3].abs().max()) > 0 and float(dd64.abs().min()) > 0
    for name, a, ref in (('o', d_o, do64), ('d', d_d, dd64), ('viewdir', d_v, dv64)):
        err = rel_l2(a, ref)
        print('%-7s noise=%d white=%d  rel L2 %.3e' % (name, with_noise, white, err))
        assert err <= 1e-12, (name, err)


def test_dists_term_matters():
    """Without c d / |d|^2 the direction gradient is wrong by far more than rounding: the identity is not vacuous."""
    n, S = 3, 5
    sd = make_sd(11)
    gen = torch.Generator().manual_seed(6)
    o = torch.rand(n, 3, generator=gen, dtype=F64) - 0.5
    d = (torch.rand(n, 3, generator=gen, dtype=F64) - 0.5) * 1.5
    v = d / d.norm(dim=-1, keepdim=True)
    z = torch.sort(torch.rand(n, S, generator=gen, dtype=F64) * 2, -1).values
    g_rgb = torch.randn(n, 3, generator=gen, dtype=F64)
    sd['alpha_linear.bias'] = sd['alpha_linear.bias'] + 1.0
    _, dd64, _ = autograd_ray_grads(sd, o, d, v, z, None, False, g_rgb)
    _, d_d, _, draw, sig = restated_ray_grads(sd, o, d, v, z, None, False, g_rgb)
    c = (draw[..., 3] * sig).sum(-1)
    without = d_d - c[:, None] * d / (d * d).sum(-1, keepdim=True)
    assert rel_l2(d_d, dd64) <= 1e-12 and rel_l2(without, dd64) > 1e-6
