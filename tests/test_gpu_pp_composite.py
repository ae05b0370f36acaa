"""The NeRF++ branches of raw2outputs_fwd_kernel / raw2outputs_bwd_kernel (ops.pp_composite_fwd, ops.pp_composite_bwd under
pp_cfg(part): |sigma|, eps 1e-6, fg_far - z_last as the last interval, the flipped background order without |d|, bg_lambda and its
cotangent in the suffix term) against float64 autograd of tests/pp_composite_ref.py, called directly with hard rays and S from 2
to 512; and ops.pp_depth2pts_outside against the oracle's depth2pts_outside in float64.

Bars.  Forward: the project's rtol 1e-4, atol 1e-5.  Backward: check() of test_gpu_raw2outputs_grad.py (relative L2 and max / max|ref|
at most 1e-5).  Where float32 arithmetic itself, measured as the float32 CPU autograd of the same reference function against
float64, loses more than 2.5e-6 in one of the two figures, the bar of that figure is 4 x that loss; both numbers are printed."""
import pytest
import torch

import pp_composite_ref as C
from oracle import nerfpp_oracle as PP
from test_gpu_raw2outputs_grad import ATOL, check

pytestmark = pytest.mark.gpu

GRID_ROWS = 16384      # grid_waves: 4096 blocks of 4 waves; ray 16384 is the first a wave takes on its second trip


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return fastnerf


def figures(got, ref):
    """(same non-finite places, relative L2, max / max|ref|, absolute L2, absolute max, max|ref|) as check() measures them."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    fin = torch.isfinite(ref)
    same = torch.equal(torch.isfinite(got), fin)
    err, r = (got - ref)[fin], ref[fin]
    norm, scale = float(r.norm()), float(r.abs().max()) if r.numel() else 0.0
    l2, mx = float(err.norm()), float(err.abs().max()) if r.numel() else 0.0
    return same, (l2 / norm if norm > 0 else l2), (mx / scale if scale > 0 else mx), l2, mx, scale


def judge_grad(got, ref, ref32, what):
    """check() with its 1e-5 bars, each raised to 4 x the float32 CPU loss where that loss exceeds 2.5e-6.  -> report line."""
    _, rel32, max32, l2_32, _, _ = figures(ref32, ref)
    raised = l2_32 > ATOL          # (a gradient that is below check()'s absolute floor altogether has no relative loss to speak of)
    bar_rel = 4 * rel32 if raised and rel32 > 2.5e-6 else 1e-5
    bar_max = 4 * max32 if raised and max32 > 2.5e-6 else 1e-5
    same, rel, mxr, l2, mx, scale = figures(got, ref)
    line = '%s: rel L2 %.3g (float32 CPU %.3g, bar %.3g)  max/max|ref| %.3g (float32 CPU %.3g, bar %.3g)' % (
        what, rel, rel32, bar_rel, mxr, max32, bar_max)
    if bar_rel == 1e-5 and bar_max == 1e-5:
        ok, msg = check(got, ref)
        assert ok, (line, msg)
    else:
        assert same, (line, 'non-finite entries differ')
        assert (rel <= bar_rel or l2 <= ATOL) and mx <= bar_max * scale + ATOL, line
    return line


def device_case(fn, case):
    raw, z, ro, rd, far, g_rgb, g_lam = case
    rays11 = fn.ops.pack_rays(ro.cuda(), rd.cuda(), 0.0, 0.0)
    dnorm = rays11[:, 3:6].cpu().double().norm(dim=-1)          # the kernel's own |d|: the float32 direction it was given
    return rays11, dnorm, [None if t is None else t.cuda() for t in (raw, z, far, g_rgb, g_lam)]


def check_forward(fn, part, kind, S, case, rays11, dnorm, dev):
    raw, z, _, _, far, _, _ = case
    raw_d, z_d, far_d, _, _ = dev
    rgb, w, depth, lam = fn.ops.pp_composite_fwd(part, raw_d, z_d, rays11, far_d)
    r_rgb, r_w, r_depth, r_lam = C.composite(raw.double(), z, dnorm, far, part)
    for name, got, ref in (('rgb', rgb, r_rgb), ('weights', w, r_w), ('depth', depth, r_depth)):
        assert torch.allclose(got.cpu().double(), ref, rtol=1e-4, atol=1e-5), (part, kind, S, name, float((got.cpu().double() - ref).abs().max()))
    if part == 1:
        assert lam is None
        return
    err = (lam.cpu().double() - r_lam).abs()
    if kind in ('random', 'thin') or (kind == 'saturate' and S <= 3):
        rel = r_lam >= 1e-20            # 1 - alpha + 1e-6 is well conditioned in these kinds: the product is good to its last bits
        assert (err[rel] <= 1e-4 * r_lam[rel]).all(), (part, kind, S, 'lambda rel', float((err[rel] / r_lam[rel]).max()))
        assert (err[~rel] <= 1e-5).all(), (part, kind, S, 'lambda')
    else:
        assert (err <= 1e-5).all(), (part, kind, S, 'lambda', float(err.max()))


def backward_modes(part, g_rgb, g_lam):
    """name -> (g_rgb, g_lambda): part 0 without / with the bg_lambda cotangent and with it alone (isolates lam_term)."""
    if part == 1:
        return {'g_rgb': (g_rgb, None)}
    return {'g_rgb': (g_rgb, None), 'g_rgb+g_lambda': (g_rgb, g_lam), 'g_lambda alone': (torch.zeros_like(g_rgb), g_lam)}


def check_backward(fn, part, kind, S, case, rays11, dnorm, dev, sigma_column):
    raw, z, _, _, far, g_rgb, g_lam = case
    raw_d, z_d, far_d, _, _ = dev
    lines = []
    for name, (gr, gl) in backward_modes(part, g_rgb, g_lam).items():
        draw = fn.ops.pp_composite_bwd(part, raw_d, z_d, rays11, gr.cuda(), far_d, None if gl is None else gl.cuda()).cpu()
        ref = C.grad(raw, z, dnorm, far, part, gr, gl)
        ref32 = C.grad(raw, z, dnorm, far, part, gr, gl, torch.float32)
        what = 'PP_COMPOSITE part %d %-10s S=%3d %-15s' % (part, kind, S, name)
        lines.append(judge_grad(draw, ref, ref32, what + ' draw'))
        if sigma_column:
            lines.append(judge_grad(draw[..., 3], ref[..., 3], ref32[..., 3], what + ' sigma column'))
        zero = raw[..., 3] == 0
        if zero.any():                   # d|sigma| / d sigma at 0 is exactly 0, as torch.abs gives
            assert (ref[..., 3][zero] == 0).all() and (draw[..., 3][zero] == 0).all(), what
    return lines


@pytest.mark.parametrize('part', [0, 1])
@pytest.mark.parametrize('kind', C.KINDS)
@pytest.mark.parametrize('S', C.SIZES)
def test_against_float64(fn, part, kind, S):
    case = C.make_case(kind, 16, S, part, seed=1000 * S + 10 * C.KINDS.index(kind) + part)
    if kind == 'zero_sigma':
        assert (case[0][..., 3] == 0).any()
    rays11, dnorm, dev = device_case(fn, case)
    check_forward(fn, part, kind, S, case, rays11, dnorm, dev)
    # in `opaque` the exact sigma gradient is orders of magnitude below the colour columns: only the whole-tensor bar applies
    print('\n'.join(check_backward(fn, part, kind, S, case, rays11, dnorm, dev, sigma_column=kind in ('random', 'saturate', 'thin'))))


@pytest.mark.parametrize('part', [0, 1])
def test_second_trip_of_the_grid_stride_loop(fn, part):
    """n = 16384 + 3, S = 2: the last three rays are taken by waves on their second trip through the loop."""
    n = GRID_ROWS + 3
    case = C.make_case('random', n, 2, part, seed=77 + part)
    rays11, dnorm, dev = device_case(fn, case)
    check_forward(fn, part, 'random', 2, case, rays11, dnorm, dev)
    print('\n'.join(check_backward(fn, part, 'random', 2, case, rays11, dnorm, dev, sigma_column=True)))
    tail = tuple(None if t is None else t[GRID_ROWS:].contiguous() for t in case)
    raw, z, _, _, far, g_rgb, g_lam = case
    raw_d, z_d, far_d, g_rgb_d, g_lam_d = dev
    draw = fn.ops.pp_composite_bwd(part, raw_d, z_d, rays11, g_rgb_d, far_d, g_lam_d if part == 0 else None).cpu()
    ref = C.grad(tail[0], tail[1], dnorm[GRID_ROWS:], tail[4], part, tail[5], tail[6] if part == 0 else None)
    ok, msg = check(draw[GRID_ROWS:], ref)
    assert ok, ('rows >= %d' % GRID_ROWS, msg)
    rgb, w, depth, lam = fn.ops.pp_composite_fwd(part, raw_d, z_d, rays11, far_d)
    r_rgb, r_w, r_depth, r_lam = C.composite(tail[0].double(), tail[1], dnorm[GRID_ROWS:], tail[4], part)
    for got, r in ((rgb, r_rgb), (w, r_w), (depth, r_depth)) + (((lam, r_lam),) if part == 0 else ()):
        assert torch.allclose(got[GRID_ROWS:].cpu().double(), r, rtol=1e-4, atol=1e-5)


def test_refusals(fn):
    raw, z, ro, rd, far, g_rgb, _ = C.make_case('random', 4, 2, 0, seed=3)
    rays11, _, (raw_d, z_d, far_d, g_rgb_d, _) = device_case(fn, (raw, z, ro, rd, far, g_rgb, None))
    for args in ((0, raw_d[:, :1].contiguous(), z_d[:, :1].contiguous(), rays11), (2, raw_d, z_d, rays11)):      # S = 1, part = 2
        with pytest.raises(RuntimeError, match='fastnerf_pp_composite_fwd'):
            fn.ops.pp_composite_fwd(*args, far_d)
        with pytest.raises(RuntimeError, match='fastnerf_pp_composite_bwd'):
            fn.ops.pp_composite_bwd(*args, g_rgb_d, far_d)
    with pytest.raises(RuntimeError, match='fastnerf_pp_composite_fwd'):
        fn.ops.pp_composite_fwd(0, raw_d, z_d, rays11, None)
    with pytest.raises(RuntimeError, match='fastnerf_pp_composite_bwd'):
        fn.ops.pp_composite_bwd(0, raw_d, z_d, rays11, g_rgb_d, None)
    fn.ops.pp_composite_fwd(1, raw_d, z_d, rays11, None)          # the background needs no fg_far
    torch.cuda.synchronize()


@pytest.mark.parametrize('S', [1, 70])
def test_depth2pts_outside_against_float64(fn, S):
    """n = 33 rays from inside the unit sphere whose closest point to the origin has norm in [0.05, 0.95] (outside that range the
    asin and the axis normalisation are ill conditioned in the reference too), depths in [0.01, 1].  A bar that the float32 oracle
    on the CPU itself uses more than a third of is set to 3 x that oracle's own error (printed)."""
    n = 33
    gen = torch.Generator().manual_seed(40 + S)
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)       # noqa: E731
    p_mid = unit(torch.randn(n, 3, generator=gen).double()) * (0.05 + 0.9 * torch.rand(n, 1, generator=gen).double())
    d = torch.randn(n, 3, generator=gen).double()
    d = d - (d * p_mid).sum(-1, keepdim=True) * p_mid / (p_mid * p_mid).sum(-1, keepdim=True)       # perpendicular to p_mid
    d = unit(d) * (0.5 + 1.5 * torch.rand(n, 1, generator=gen).double())
    reach = torch.sqrt(1.0 - (p_mid * p_mid).sum(-1, keepdim=True))                                 # |o|^2 = |p_mid|^2 + t^2 < 1
    o = p_mid + unit(d) * reach * (1.8 * torch.rand(n, 1, generator=gen).double() - 0.9)
    o, d = o.float(), d.float()
    depth = (0.01 + 0.99 * torch.rand(n, S, generator=gen)).float()
    depth[0, 0] = 1.0
    expand = lambda t, dt: t.to(dt)[:, None, :].expand(n, S, 3)     # noqa: E731
    d1 = -(d.double() * o.double()).sum(-1) / (d.double() * d.double()).sum(-1)
    norm = (o.double() + d1[:, None] * d.double()).norm(dim=-1)
    assert (norm > 0.049).all() and (norm < 0.951).all() and (o.double().norm(dim=-1) < 1).all()
    r_pts, r_real = PP.depth2pts_outside(expand(o, torch.float64), expand(d, torch.float64), depth.double())
    c_pts, c_real = PP.depth2pts_outside(expand(o, torch.float32), expand(d, torch.float32), depth)
    pts, real = fn.ops.pp_depth2pts_outside(o.cuda(), d.cuda(), depth.cuda())
    pts, real = pts.cpu(), real.cpu()
    own_pts = float((c_pts[..., :3].double() - r_pts[..., :3]).abs().max())
    own_real = float(((c_real.double() - r_real).abs() / r_real.abs()).max())
    bar_pts = 3 * own_pts if own_pts > 1e-5 / 3 else 1e-5
    bar_real = 3 * own_real if own_real > 1e-5 / 3 else 1e-5
    e_pts = float((pts[..., :3].double() - r_pts[..., :3]).abs().max())
    e_real = float(((real.double() - r_real).abs() / r_real.abs()).max())
    e_norm = float((pts[..., :3].double().norm(dim=-1) - 1).abs().max())
    print('PP_DEPTH2PTS S=%d: pts %.3g (float32 oracle %.3g, bar %.3g)  depth_real rel %.3g (float32 oracle %.3g, bar %.3g)  |pts|-1 %.3g'
          % (S, e_pts, own_pts, bar_pts, e_real, own_real, bar_real, e_norm))
    assert e_norm <= 2e-6
    assert e_pts <= bar_pts
    assert torch.equal(pts[..., 3].view(torch.int32), depth.view(torch.int32))
    assert e_real <= bar_real
