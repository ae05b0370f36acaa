"""Full-gradient compositing: torch.ops.fastnerf.raw2outputs_full / fastnerf_raw2outputs_bwd_full against float64 autograd
of the oracle's raw2outputs (render.py:149-192) on the same float32 inputs, one cotangent at a time and all five together,
over S in {2, 63, 64, 65, 192, 512}, sigma noise on / off, white background on / off, and rays that are hard for the
formula: nothing hit (acc == 0, NaN disparity), early saturation (T underflows), the 1e10 last interval carrying most of
the weight, and depths just above / below the disparity clamp."""
import os

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

KINDS = ('random', 'empty', 'saturate', 'last', 'clamp_above', 'clamp_below')
SIZES = (2, 63, 64, 65, 192, 512)
OUTS = ('rgb', 'disp', 'acc', 'w', 'depth')


def make_case(kind, n, S, with_noise, seed):
    """float32 (raw [n,S,4], z [n,S], rays_d [n,3], noise [n,S] or None) whose per-sample optical depth sigma * dist is set
    by `kind` (so that the alphas are well conditioned in float32 where the gradient lives)."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    ru = lambda *s: torch.rand(*s, generator=gen)
    rd = rn(n, 3)
    rd = rd / rd.norm(dim=-1, keepdim=True) * (0.5 + 1.5 * ru(n, 1))
    lo, hi = {'clamp_above': (1.2e-10, 2.5e-10), 'clamp_below': (0.3e-10, 0.8e-10)}.get(kind, (2.0, 6.0))
    z = O.coarse_z(torch.full((n, 1), lo), torch.full((n, 1), hi), S, False, ru(n, S)).contiguous()
    dist = (z[:, 1:] - z[:, :-1]) * rd.norm(dim=-1, keepdim=True)
    dist = torch.cat([dist, dist[:, -1:] if S > 1 else torch.ones(n, 1)], -1).clamp(min=1e-30)
    if kind == 'random' or kind.startswith('clamp'):
        x = 0.3 * (rn(n, S) + 0.5)
        # the last sample is hit: a ray whose weight sits on ONE sample has a disparity that does not depend on sigma at all
        # (exact gradient 0); float32 returns roundoff of the disparity's scale there, which no relative bar can measure
        x[:, -1] = x[:, -1].abs() + 0.1
    elif kind == 'empty':
        x = -(rn(n, S).abs() + 0.5)
    elif kind == 'saturate':
        x = 1.5 + ru(n, S)         # T underflows after ~50 samples; 1 - alpha stays >= 0.08 (its float32 rounding is the bar's enemy)
    else:   # 'last': small optical depth everywhere but the 1e10 interval
        x = (0.5 / S) * ru(n, S)
    noise = None
    if with_noise:
        noise = 0.1 * rn(n, S) * x.abs() / dist
        if kind == 'empty':
            x = x - noise.abs() * dist       # keeps sigma + noise < 0
    sigma = x / dist - (noise if noise is not None else 0.0)
    raw = torch.cat([2.0 * rn(n, S, 3), sigma[..., None]], -1).float().contiguous()
    return raw, z.float(), rd.float(), None if noise is None else noise.float().contiguous()


def cotangents(n, S, seed):
    """name -> {output: cotangent}: each output alone, then all five together."""
    gen = torch.Generator().manual_seed(seed + 1)
    full = {'rgb': torch.randn(n, 3, generator=gen), 'disp': torch.randn(n, generator=gen), 'acc': torch.randn(n, generator=gen),
            'w': torch.randn(n, S, generator=gen), 'depth': torch.randn(n, generator=gen)}
    out = {k: {k: v} for k, v in full.items()}
    out['all'] = full
    return out


def ref_grad(raw, z, rd, noise, white, cot):
    """float64 autograd of the oracle's raw2outputs w.r.t. raw, for the cotangents given (absent = not differentiated)."""
    raw64 = raw.double().requires_grad_(True)
    outs = dict(zip(OUTS, O.raw2outputs(raw64, z.double(), rd.double(), None if noise is None else noise.double(), white)))
    keys = [k for k in OUTS if k in cot]
    return torch.autograd.grad([outs[k] for k in keys], raw64, [cot[k].double() for k in keys])[0]


ATOL = 1e-12   # floor for gradients that are zero in exact arithmetic (S = 2, acc cotangent: float64 returns roundoff of 1e-17)


def check(got, ref):
    """(ok, message): same non-finite places; finite entries within relative L2 1e-5 and max-abs 1e-5 * max|ref| (+ ATOL)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    fin_g, fin_r = torch.isfinite(got), torch.isfinite(ref)
    if not torch.equal(fin_g, fin_r):
        return False, 'non-finite entries differ (%d vs %d)' % (int((~fin_g).sum()), int((~fin_r).sum()))
    g, r = got[fin_r], ref[fin_r]
    err = (g - r)
    scale = float(r.abs().max()) if r.numel() else 0.0
    rel = float(err.norm() / r.norm()) if float(r.norm()) > 0 else float(err.norm())
    mx = float(err.abs().max()) if r.numel() else 0.0
    ok = (rel <= 1e-5 or float(err.norm()) <= ATOL) and mx <= 1e-5 * scale + ATOL
    return ok, 'rel L2 %.3g, max %.3g of max|ref| %.3g' % (rel, mx, scale)


def _rays11(rd):
    r11 = torch.zeros(rd.shape[0], 11)
    r11[:, 3:6] = rd
    return r11.cuda()


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return fastnerf


def _full(fn, raw, z, rd, noise, white, cot):
    """d raw from the new op's registered autograd formula."""
    rawg = raw.cuda().requires_grad_(True)
    outs = dict(zip(OUTS, torch.ops.fastnerf.raw2outputs_full(rawg, z.cuda(), _rays11(rd), None if noise is None else noise.cuda(),
                                                              white)))
    keys = [k for k in OUTS if k in cot]
    return outs, torch.autograd.grad([outs[k] for k in keys], rawg, [cot[k].cuda() for k in keys])[0]


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('S', SIZES)
def test_against_float64_autograd(fn, kind, S):
    n = 16
    for with_noise in (False, True):
        for white in (False, True):
            raw, z, rd, noise = make_case(kind, n, S, with_noise, seed=1000 * S + 10 * KINDS.index(kind) + 2 * with_noise + white)
            ref_out = O.raw2outputs(raw.double(), z.double(), rd.double(), None if noise is None else noise.double(), white)
            for name, cot in cotangents(n, S, seed=S).items():
                outs, got = _full(fn, raw, z, rd, noise, white, cot)
                ok, msg = check(got, ref_grad(raw, z, rd, noise, white, cot))
                assert ok, (kind, S, with_noise, white, name, msg)
            for k, r in zip(OUTS, ref_out):      # the forward of the new op (NaN disparity where nothing is hit)
                assert torch.allclose(outs[k].detach().cpu().double(), r, rtol=1e-4, atol=1e-5, equal_nan=True), (kind, S, k)
            if kind == 'empty':
                assert torch.isnan(outs['disp']).all() and (outs['acc'] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('S', [64, 192])
@pytest.mark.parametrize('wb', [0, 1])
def test_rgb_only_matches_the_g5_golden(fn, golden_dir, S, wb):
    g = np.load(os.path.join(golden_dir, f'g5_raw2out_S{S}_wb{wb}.npz'))
    raw, z, rd, cot = (torch.from_numpy(g[k]).cuda() for k in ('raw', 'z', 'rd', 'cot'))
    r11 = _rays11(rd.cpu())
    _, _, acc, _, depth = fn.ops.raw2outputs_fwd(raw, z, r11, None, bool(wb))
    draw = fn.ops.raw2outputs_bwd_full(raw, z, r11, acc, depth, g_rgb=cot, white_bkgd=bool(wb))
    err = np.abs(draw.cpu().numpy() - g['graw'])
    assert np.all(err <= 2e-6 + 1e-4 * np.abs(g['graw'])), float(err.max())     # test_gpu_ops.py's bar for raw2outputs_bwd


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize('S', SIZES)
def test_bit_identical_to_the_rgb_only_backward(fn, S):
    n = 300
    for with_noise in (False, True):
        for white in (False, True):
            raw, z, rd, noise = (None if t is None else t.cuda() for t in make_case('random', n, S, with_noise, seed=S + 7))
            r11 = _rays11(rd.cpu())
            _, _, acc, _, depth = fn.ops.raw2outputs_fwd(raw, z, r11, noise, white)
            g_rgb = torch.randn(n, 3, device='cuda')
            base = fn.ops.raw2outputs_bwd(raw, z, r11, g_rgb, noise, white)
            absent = fn.ops.raw2outputs_bwd_full(raw, z, r11, acc, depth, g_rgb=g_rgb, noise=noise, white_bkgd=white)
            zeros = fn.ops.raw2outputs_bwd_full(raw, z, r11, acc, depth, g_rgb, torch.zeros(n, device='cuda'),
                                                torch.zeros(n, device='cuda'), torch.zeros(n, S, device='cuda'),
                                                torch.zeros(n, device='cuda'), noise=noise, white_bkgd=white)
            assert torch.equal(_bits(absent), _bits(base)), (S, with_noise, white)
            assert torch.equal(zeros, base), (S, with_noise, white)
            # all five gradients: two runs are bit-identical
            cot = cotangents(n, S, seed=S)['all']
            c = {k: v.cuda() for k, v in cot.items()}
            a = fn.ops.raw2outputs_bwd_full(raw, z, r11, acc, depth, c['rgb'], c['disp'], c['acc'], c['w'], c['depth'], noise, white)
            b = fn.ops.raw2outputs_bwd_full(raw, z, r11, acc, depth, c['rgb'], c['disp'], c['acc'], c['w'], c['depth'], noise, white)
            assert torch.equal(_bits(a), _bits(b))
            assert not torch.equal(a, base)


@pytest.mark.gpu
def test_render_raw2outputs_backward_and_refusals(fn):
    n, S = 64, 64
    raw, z, rd, _ = make_case('random', n, S, False, seed=5)
    rawg = raw.cuda().requires_grad_(True)
    rgb, disp, acc, w, depth = fn.render.raw2outputs(rawg, z.cuda(), rd.cuda(), 0, True)
    (rgb.sum() + depth.sum() + disp.nansum() + acc.sum()).backward()
    raw64 = raw.double().requires_grad_(True)
    r = O.raw2outputs(raw64, z.double(), rd.double(), None, True)
    (r[0].sum() + r[4].sum() + r[1].nansum() + r[2].sum()).backward()
    ok, msg = check(rawg.grad, raw64.grad)
    assert ok, msg
    # without requires_grad: the forward-only route of before, same values
    ref = fn.ops.raw2outputs_fwd(raw.cuda(), z.cuda(), _rays11(rd), None, True)
    got = fn.render.raw2outputs(raw.cuda(), z.cuda(), rd.cuda(), 0, True)
    assert all(torch.equal(a, b) for a, b in zip(got, ref)) and not got[0].requires_grad
    with pytest.raises(NotImplementedError):
        fn.render.raw2outputs(rawg, z.cuda().requires_grad_(True), rd.cuda(), 0, True)
    with pytest.raises(NotImplementedError):
        fn.render.raw2outputs(rawg, z.cuda(), rd.cuda().requires_grad_(True), 0, True)
