"""Band weights on the GPU, below the trainer: the two kernels, the effective network against the truth, and the readers of `net.flat`.

(1) ops.band_apply / ops.band_grad against tests/bands_ref.py, bit for bit, kinds 0 and 2: random weights with exact 0 and 1 among them;
    every float outside the three regions is compared too; band_grad on a buffer that holds -0.0 and denormals (a float32 product of a
    denormal is the correctly rounded one in numpy; the kernels do not flush).
(2) truth: ops.mlp_fwd / mlp_bwd on a banded NeRF (NeRF.set_bands; its `flat`, `packed()` and `collect_grads`) with a random cotangent
    against float64 torch autograd of the reference MLP fed weight_encoding(gamma(x), w) -- the points are the float32 points the
    kernels make -- in all three math modes.  Bounds: those tests/test_gpu_mlp.py applies to the unweighted network in every mode: logits
    within 2e-5 (its forward test), every parameter tensor's gradient within 2e-5 max(1, |g|max) (its autograd test); and at 16 points
    every mode's gradients against the fp32 mode's within 2e-5 (bf16x6) / 2e-2 (bf16x3) of the tensor's maximum (its ragged test).  The
    scaled network is one more network with smaller columns, so they hold as they are.  Weights well away from 1 on every band of both
    encodings: leaving out the skip layer's columns, the view columns or the folded view packing moves logits by O(0.1).
(7) density_gradient and render_rays on the banded net, without grad and through autograd, equal the same calls on a plain net that
    holds the effective parameters, bit for bit; the parameters' .grad is the plain net's with the encoding columns times w.
(9) the ops' refusals, before any launch; NeRF.set_bands on a network without view directions."""
import os

import numpy as np
import pytest
import torch

import bands_ref as B
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


@pytest.fixture(scope='module')
def weights(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g7_weights.npz'))
    return {k[2:]: torch.from_numpy(g[k]).clone() for k in g.files if k.startswith('c.')}


def bits(t):
    t = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return t.view(np.uint32)


def ramp_weights():
    """Mid-ramp column weights with nothing at 1 but the identity columns and the lowest band, and a closed top band."""
    wp = B.columns_from_bands([1.0, 0.9, 0.75, 0.6, 0.5, 0.35, 0.25, 0.125, 0.05, 0.0])
    wv = B.columns_from_bands([1.0, 0.7, 0.3, 0.0])
    return torch.from_numpy(wp), torch.from_numpy(wv)


@pytest.mark.parametrize('kind', [0, 2])
def test_kernels_bit_for_bit(fn, kind):
    """(1)"""
    n = B.n_params(kind)
    assert n == fn.ops.net_floats(kind, 0) and n % 256 != 0
    rs = np.random.RandomState(10 + kind)
    master = rs.randn(n).astype(np.float32)
    master[rs.rand(n) < 0.01] = 0.0
    w_pos, w_view = B.random_weights(kind, 3 + kind)
    assert (w_pos == 0).any() and (w_pos == 1).any() and (w_view == 0).any() and (w_view == 1).any()
    wp, wv, m = torch.from_numpy(w_pos).cuda(), torch.from_numpy(w_view).cuda(), torch.from_numpy(master).cuda()
    eff = torch.full((n,), float('nan'), device='cuda')
    out = fn.ops.band_apply(wp, wv, m, eff, kind=kind)
    assert out is eff and np.array_equal(bits(m), bits(master))                      # the master is read only
    assert np.array_equal(bits(eff), bits(B.apply32(kind, w_pos, w_view, master)))     # every float, inside the regions and outside
    assert np.array_equal(bits(fn.ops.band_apply(wp, wv, m, kind=kind)), bits(eff))    # a buffer of its own making
    # the gradient, in place, on a buffer with -0.0, denormals, huge and tiny values
    g = rs.randn(n).astype(np.float32) * (10.0 ** rs.uniform(-30, 10, n)).astype(np.float32)
    g[rs.rand(n) < 0.05] = -0.0
    g[rs.rand(n) < 0.05] = np.float32(1e-42)
    g[rs.rand(n) < 0.05] = np.float32(-3e-39)
    index, which = B.column_map(kind)
    assert (bits(g[which > 0]) == 0x80000000).any() and (np.abs(g[which > 0]) < 1e-38).any()
    gd = torch.from_numpy(g).cuda()
    assert fn.ops.band_grad(wp, wv, gd, kind=kind) is gd
    want = B.grad32(kind, w_pos, w_view, g)
    assert np.array_equal(bits(gd), bits(want))
    assert np.array_equal(bits(gd)[which == 0], bits(g)[which == 0])
    assert (bits(want[which > 0]) == 0x80000000).any()                                # -0.0 * w and x * 0 with x < 0 keep their sign


def reference64(weights, rb, z, w_pos, w_view, cot):
    """float64: logits [n,S,4] of the reference MLP fed the weighted encodings of the kernels' float32 points, and the gradient of
    sum(logits * cot) with respect to every parameter tensor, parameters() order."""
    sd = {k: v.double().clone().requires_grad_(True) for k, v in weights.items()}
    pts = (rb[:, None, 0:3] + rb[:, None, 3:6] * z[..., None]).double()       # (float32 products and sums, as the kernels make them)
    from fastnerf import bands
    flat = pts.reshape(-1, 3)
    dirs = rb[:, 8:11].double()[:, None].expand(pts.shape).reshape(-1, 3)
    emb = torch.cat([bands.weight_encoding(O.posenc(flat, 10), w_pos), bands.weight_encoding(O.posenc(dirs, 4), w_view)], -1)
    out = O.nerf_forward(sd, emb, input_ch=63, input_ch_views=27).reshape(list(pts.shape[:-1]) + [4])
    grads = torch.autograd.grad((out * cot.double()).sum(), [sd[name] for name, _ in O.nerf_param_shapes()])
    return out.detach(), grads


def banded_net(fn, weights, w_pos, w_view):
    net = fn.model.NeRF()
    net.load_state_dict(weights)
    net.set_bands(w_pos, w_view)
    return net


def kernel_grads(fn, net, rb, z, cot):
    P = z.numel()
    pf, pb = net.packed()
    act = torch.empty(fn.ops.act_floats(P)).cuda()
    raw = fn.ops.mlp_fwd(rb, z, net.flat, pf, act=act)
    dact = torch.empty(fn.ops.dact_floats(P)).cuda()
    partial = torch.empty(fn.ops.mlp_bwd_partial_floats()).cuda()
    net.flat_grad.fill_(float('nan'))
    fn.ops.mlp_bwd(cot, act, net.flat, pb, dact, partial, net.flat_grad)
    net.collect_grads()
    return raw, net.param_grad.clone()


def test_truth_against_float64(fn, weights, math_mode):
    """(2)"""
    gen = torch.Generator().manual_seed(77)
    n, S = 9, 50          # P = 450: 3 full tiles + a tail
    ro = torch.randn(n, 3, generator=gen) * 0.5
    rd = torch.randn(n, 3, generator=gen)
    rb = O.make_ray_batch(ro, rd, 2.0, 6.0)
    z = torch.sort(torch.rand(n, S, generator=gen) * 4 + 2, -1).values
    cot = torch.randn(n, S, 4, generator=gen)
    w_pos, w_view = ramp_weights()
    ref, grads_ref = reference64(weights, rb, z, w_pos, w_view, cot)
    plain, _ = reference64(weights, rb, z, torch.ones(63), torch.ones(27), cot)
    assert float((ref - plain).abs().max()) > 0.05       # the weights matter: far above every bound below
    net = banded_net(fn, weights, w_pos, w_view)
    assert net.flat.data_ptr() != net.param_flat.data_ptr() and net.flat_grad.data_ptr() != net.param_grad.data_ptr()
    raw, grads = kernel_grads(fn, net, rb.cuda(), z.cuda(), cot.cuda())
    err = float((raw.cpu().double() - ref).abs().max())
    print('\nbands truth %-6s logits: max err %.3e (bound 2e-5)' % (math_mode, err))
    worst = []
    grads = grads.cpu().double()
    assert torch.isfinite(grads).all()
    off = 0
    for (name, shape), gr in zip(O.nerf_param_shapes(), grads_ref):
        k = gr.numel()
        got = grads[off:off + k].view(shape)
        scale = max(1.0, gr.abs().max().item())
        worst.append((float((got - gr).abs().max()) / scale, name))
        off += k
    print('bands truth %-6s gradients: worst err / max(1, |g|max) %.3e at %s (bound 2e-5)' % ((math_mode,) + max(worst)))
    assert err < 2e-5, err
    for e, name in worst:
        assert e < 2e-5, (name, e)
    # the closed band's columns: exact zeros in the parameters' gradient, zeros in the effective network
    g0 = grads[:256 * 63].view(256, 63)
    assert not g0[:, 57:].any() and g0[:, :57].abs().max() > 0
    assert not net.flat[:256 * 63].view(256, 63)[:, 57:].any()


@pytest.fixture(params=['bf16x3', 'bf16x6'])
def split_mode(request, fn):
    old = fn.ops.get_math()
    fn.ops.set_math(request.param)
    yield request.param
    fn.ops.set_math(old)


def test_small_batch_against_fp32_mode(fn, weights, split_mode):
    """(2), the third bound: 16 points, the two split modes against the fp32 mode."""
    math_mode = split_mode
    gen = torch.Generator().manual_seed(5)
    rb = fn.ops.pack_rays((torch.randn(1, 3, generator=gen) * 0.5).cuda(), torch.randn(1, 3, generator=gen).cuda(), 2.0, 6.0)
    z = torch.sort(torch.rand(1, 16, generator=gen) * 4 + 2, -1).values.cuda()
    cot = torch.randn(1, 16, 4, generator=gen).cuda()
    w_pos, w_view = ramp_weights()
    got = kernel_grads(fn, banded_net(fn, weights, w_pos, w_view), rb, z, cot)[1].double().cpu()
    fn.ops.set_math('fp32')
    try:
        ref = kernel_grads(fn, banded_net(fn, weights, w_pos, w_view), rb, z, cot)[1].double().cpu()
    finally:
        fn.ops.set_math(math_mode)
    tol = 2e-5 if math_mode == 'bf16x6' else 2e-2
    off = 0
    for name, shape in O.nerf_param_shapes():
        k = int(np.prod(shape))
        a, b = got[off:off + k], ref[off:off + k]
        scale = max(1e-6, b.abs().max().item())
        assert (a - b).abs().max().item() <= tol * scale, (name, (a - b).abs().max().item(), scale)
        off += k


def twin_nets(fn, weights):
    """(a banded net, a plain net that holds its effective parameters)."""
    w_pos, w_view = ramp_weights()
    a = banded_net(fn, weights, w_pos, w_view)
    b = fn.model.NeRF()
    b.flat.copy_(fn.ops.band_apply(w_pos.cuda(), w_view.cuda(), a.param_flat))
    assert torch.equal(a.flat, b.flat) and not torch.equal(a.param_flat, b.flat)
    return a, b, w_pos.cuda(), w_view.cuda()


def test_density_gradient_and_render_rays(fn, weights, math_mode):
    """(7)"""
    a, b, wp, wv = twin_nets(fn, weights)
    gen = torch.Generator().manual_seed(9)
    pts = (torch.rand(131, 3, generator=gen) * 2 - 1).cuda()
    if math_mode != 'bf16x3':      # (no density gradient in that mode)
        sa, ga = a.density_gradient(pts)
        sb, gb = b.density_gradient(pts)
        assert np.array_equal(bits(sa), bits(sb)) and np.array_equal(bits(ga), bits(gb)) and float(ga.abs().max()) > 0
    rb = fn.ops.pack_rays((torch.randn(37, 3, generator=gen) * 0.3).cuda(), torch.randn(37, 3, generator=gen).cuda(), 2.0, 6.0)
    target = torch.rand(37, 3, generator=gen).cuda()
    outs = []
    for net in (a, b):
        with torch.no_grad():
            ng = fn.render.render_rays(rb, net, None, 8, perturb=0., N_importance=0)
        ret = fn.render.render_rays(rb, net, None, 8, perturb=0., N_importance=0, retraw=True, retdepth=True)
        for k in ('rgb_map', 'acc_map', 'disp_map'):
            assert np.array_equal(bits(ng[k]), bits(ret[k])), k
        net.param_grad.zero_()
        (torch.mean((ret['rgb_map'] - target) ** 2) + 0.1 * torch.mean(ret['acc_map'])).backward()
        outs.append(ret)
    for k in ('rgb_map', 'disp_map', 'acc_map', 'depth_map', 'raw'):
        assert np.array_equal(bits(outs[0][k]), bits(outs[1][k])), k
    want = fn.ops.band_grad(wp, wv, b.param_grad.clone())
    assert torch.equal(a.param_grad, want) and float(want.abs().max()) > 0
    assert not torch.equal(a.param_grad, b.param_grad)                  # the factor w is there
    for p, (name, off, shape) in zip(a.parameters(), fn.model.param_slices()):
        assert p.grad.data_ptr() == a.param_grad[off:].data_ptr(), name       # .grad still views param_grad
    # clear_bands: the plain network on its own parameters again
    a.clear_bands()
    assert a.flat.data_ptr() == a.param_flat.data_ptr() and a.flat_grad.data_ptr() == a.param_grad.data_ptr()
    c = fn.model.NeRF()
    c.load_state_dict(weights)
    with torch.no_grad():
        ra, rc = (fn.render.render_rays(rb, net, None, 8, perturb=0., N_importance=0) for net in (a, c))
    assert np.array_equal(bits(ra['rgb_map']), bits(rc['rgb_map']))


def test_refusals(fn, weights):
    """(9)"""
    n = fn.ops.NET_PARAMS
    wp, wv, net = torch.ones(63).cuda(), torch.ones(27).cuda(), torch.zeros(n).cuda()
    eff = torch.full((n,), 7.0).cuda()
    bad = [
        (TypeError, lambda: fn.ops.band_apply(wp.double(), wv, net, eff)),
        (TypeError, lambda: fn.ops.band_apply(wp, wv.half(), net, eff)),
        (TypeError, lambda: fn.ops.band_apply(wp, wv, net.double(), eff)),
        (TypeError, lambda: fn.ops.band_grad(wp, wv, eff.double())),
        (ValueError, lambda: fn.ops.band_apply(torch.ones(126).cuda()[::2], wv, net, eff)),
        (ValueError, lambda: fn.ops.band_apply(wp, wv, torch.zeros(2 * n).cuda()[::2], eff)),
        (ValueError, lambda: fn.ops.band_grad(wp, wv, torch.full((2 * n,), 7.0).cuda()[::2])),
        (ValueError, lambda: fn.ops.band_apply(torch.ones(84).cuda(), wv, net, eff)),            # kind 0 has 63 columns
        (ValueError, lambda: fn.ops.band_apply(wp, wv, net, eff, kind=2)),                       # and kind 2 has 84
        (ValueError, lambda: fn.ops.band_apply(wp, torch.ones(26).cuda(), net, eff)),
        (ValueError, lambda: fn.ops.band_apply(wp, wv, net[:-1], eff)),
        (ValueError, lambda: fn.ops.band_apply(wp, wv, net, eff[:-1])),
        (ValueError, lambda: fn.ops.band_grad(wp, wv, eff[1:])),
        (ValueError, lambda: fn.ops.band_grad(torch.ones(84).cuda(), wv, torch.zeros(fn.ops.net_floats(2, 0)).cuda(), kind=1)),
        (ValueError, lambda: fn.ops.band_apply(wp, wv, net, net)),
        (ValueError, lambda: fn.ops.band_apply(wp, wv, net, eff, kind=3)),
        (RuntimeError, lambda: fn.ops.band_apply(wp.cpu(), wv, net, eff)),                       # weights on another device
        (RuntimeError, lambda: fn.ops.band_grad(wp, wv.cpu(), eff)),
        (RuntimeError, lambda: fn.ops.band_apply(wp, wv, net.cpu(), eff)),
    ]
    for exc, call in bad:
        with pytest.raises(exc):
            call()
    torch.cuda.synchronize()
    assert bool((eff == 7.0).all()) and not net.any()                  # nothing was launched
    noview = fn.model.NeRF(input_ch_views=0, use_viewdirs=False)
    before = noview.flat.clone()
    with pytest.raises(ValueError, match='view directions'):
        noview.set_bands(torch.ones(63), torch.ones(27))
    assert torch.equal(noview.flat, before) and noview._bands is None
    net = fn.model.NeRF()
    for w in (torch.full((63,), 2.0), torch.full((63,), float('nan')), torch.ones(62)):
        with pytest.raises(ValueError):
            net.set_bands(w, torch.ones(27))
    assert net._bands is None and net.flat.data_ptr() == net.param_flat.data_ptr()
