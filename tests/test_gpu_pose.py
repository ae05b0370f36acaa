"""The pose-table kernels (csrc/pose.hip): ops.pose_exp / ops.pose_exp_bwd / ops.pose_grad, and fastnerf.poses on top of them.

pose_exp, pose_exp_bwd: float64 torch.matrix_exp and its autograd from the same fp32 inputs (tests/pose_ref.py), every theta of
pose_ref.THETAS in tables of 1, 5 and 300 images.  Bounds: every entry of R R0 within 32 * 2^-24, t the fp32 sum bit for bit, d_tau a
bit copy, every d_omega entry within 32 * 2^-24 * sum|G|.  The 32 is a cap, not a measurement: the float32 restatement of the formulas
peaks at 5.4 (rotation) and 2.9 (gradient) on these inputs (tests/test_pose_cpu.py); the margin is for the device's sin / sqrt /
division not being correctly rounded.
pose_grad: EXACT on integer inputs (pose_ref.exact_case: any order of fp32 sums gives the int64 sum, so a dropped, doubled or misrouted
ray shows at any count), up to three rays past one 2048 x 256 grid; and float64 at 800 x 800 cameras within (m_i + 32) 2^-24 B_i[j,k],
B the sum of the absolute values of the terms, which holds for any summation order.
Figures are printed before they are asserted (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

import pose_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@pytest.mark.parametrize('n_img', [1, 5, 300])
def test_pose_exp_and_its_backward_against_float64(fn, n_img):
    peak = [0.0, 0.0]
    for base, xi, g in P.exp_cases(n_img):
        got = fn.ops.pose_exp(base.cuda(), xi.cuda()).cpu()
        ref = P.exp_ref64(base, xi)
        assert torch.isfinite(got).all()
        peak[0] = max(peak[0], float((got.double() - ref)[:, :, :3].abs().max()) / 2.0 ** -24)
        assert np.array_equal(bits(got[:, :, 3]), bits(base[:, :, 3] + xi[:, 3:]))
        d_xi = fn.ops.pose_exp_bwd(base.cuda(), xi.cuda(), g.cuda()).cpu()
        dref = P.exp_bwd_ref64(base, xi, g)
        assert torch.isfinite(d_xi).all()
        scale = g[:, :, :3].double().abs().sum((1, 2))[:, None]
        peak[1] = max(peak[1], float(((d_xi.double() - dref)[:, :3].abs() / scale).max()) / 2.0 ** -24)
        assert np.array_equal(bits(d_xi[:, 3:]), bits(g[:, :, 3]))
    print('\npose_exp n_img %d: rotation %.1f x 2^-24, d_omega %.1f x 2^-24 sum|G| (cap 32)' % (n_img, *peak))
    assert peak[0] <= 32.0 and peak[1] <= 32.0


def test_pose_exp_at_zero_returns_the_base_bit_for_bit(fn):
    base, xi, g = P.exp_inputs(7, seed=5)
    base[2, 1, 3] = -0.0
    base[3, 0, 1] = -0.0
    b = base.cuda()
    for x in (None, torch.zeros(7, 6, device='cuda')):
        assert np.array_equal(bits(fn.ops.pose_exp(b, x)), bits(base))
        d_xi = fn.ops.pose_exp_bwd(b, x, g.cuda()).cpu()
        assert torch.isfinite(d_xi).all()
        assert (d_xi.double() - P.exp_bwd_ref64(base, torch.zeros(7, 6), g)).abs().max() <= P.BOUND * g.abs().sum((1, 2)).max()
    # one image turned, the others not: their rows are still the base's
    x = torch.zeros(7, 6)
    x[4, :3] = torch.tensor([0.3, -0.2, 0.1])
    got = fn.ops.pose_exp(b, x.cuda())
    keep = [i for i in range(7) if i != 4]
    assert np.array_equal(bits(got[keep]), bits(base[keep])) and not torch.equal(got[4].cpu(), base[4])


EXACT = [(1, 1, ()), (67, 3, (1,)), (257, 5, ()), (4099, 5, (3,)), (4099, 1, ()), (7, 300, ()), (2048 * 256 + 3, 5, ())]


@pytest.mark.parametrize('n,n_img,empty', EXACT, ids=['%dx%d' % c[:2] for c in EXACT])
def test_pose_grad_exact(fn, n, n_img, empty):
    pix, poses, K, d_rays, want = P.exact_case(n, n_img, empty)
    got = fn.ops.pose_grad(pix.cuda(), poses.cuda(), K, d_rays.cuda()).cpu()
    assert torch.equal(got.double(), want.double())
    for i in empty:
        assert (bits(got[i]) == 0).all()      # +0, written


FLOAT = [(67, 3, (1,)), (4099, 5, ()), (4099, 1, ())]


@pytest.mark.parametrize('n,n_img,empty', FLOAT, ids=['%dx%d' % c[:2] for c in FLOAT])
def test_pose_grad_against_float64(fn, n, n_img, empty):
    pix, poses, K, d_rays = P.float_case(n, n_img, empty)
    ref, B, counts = P.pose_grad_ref64(pix, poses, K, d_rays)
    got = fn.ops.pose_grad(pix.cuda(), poses.cuda(), K, d_rays.cuda()).cpu()
    bound = (counts.double()[:, None, None] + 32.0) * 2.0 ** -24 * B
    frac = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
    print('\npose_grad (%d, %d): %.4f of the bound (m + 32) 2^-24 B' % (n, n_img, frac))
    assert torch.isfinite(got).all() and frac <= 1.0
    for i in empty:
        assert (bits(got[i]) == 0).all()


def test_pose_grad_canaries_determinism_and_empty_batch(fn):
    pix, poses, K, d_rays = P.float_case(4099, 5, (3,))
    args = (pix.cuda(), poses.cuda(), K, d_rays.cuda())
    buf = torch.full((5 * 12 + 64,), float('nan'), device='cuda')
    got = fn.ops.pose_grad(*args, d_poses=buf[:60].view(5, 3, 4))
    assert torch.isnan(buf[60:]).all() and torch.isfinite(got).all()
    again = fn.ops.pose_grad(*args)
    assert np.array_equal(bits(got), bits(again))
    assert (bits(got[3]) == 0).all()
    # scratch handed in: nothing is written past its stated size
    need = fn.ops.pose_grad_ws_floats(4099, 5)
    assert need > 0
    ws = torch.full((need + 64,), float('nan'), device='cuda')
    third = fn.ops.pose_grad(*args, ws=ws)
    assert np.array_equal(bits(got), bits(third)) and torch.isnan(ws[need:]).all()
    # n == 0: zeros, written
    out = torch.full((5, 3, 4), float('nan'), device='cuda')
    fn.ops.pose_grad(torch.zeros(0, 3, dtype=torch.int32, device='cuda'), poses.cuda(), K, torch.zeros(0, 11, device='cuda'), d_poses=out)
    assert (bits(out) == 0).all()


def test_refusals(fn):
    lib, F = fn._lib.lib(), ctypes.c_float
    pix, poses, K, d_rays = [t.cuda() if torch.is_tensor(t) else t for t in P.float_case(67, 3)]
    out = torch.full((3, 3, 4), float('nan'), device='cuda')
    p = fn.ops.ptr

    def grad(n, n_img, pix_, poses_, d_rays_, out_):
        return lib.fastnerf_pose_grad(n, n_img, pix_, poses_, F(1), F(1), F(0), F(0), d_rays_, None, out_, None)
    for call, msg in (((-1, 3, p(pix), p(poses), p(d_rays), p(out)), 'n >= 0'), ((67, 0, p(pix), p(poses), p(d_rays), p(out)), 'n_img >= 1'),
                      ((67, 3, None, p(poses), p(d_rays), p(out)), 'null pointer'), ((67, 3, p(pix), None, p(d_rays), p(out)), 'null pointer'),
                      ((67, 3, p(pix), p(poses), None, p(out)), 'null pointer'), ((67, 3, p(pix), p(poses), p(d_rays), None), 'null pointer')):
        assert grad(*call) == -1
        err = lib.fastnerf_last_error().decode()
        assert 'fastnerf_pose_grad' in err and msg in err, err
    assert lib.fastnerf_pose_grad(4099, 5, p(pix), p(poses), F(1), F(1), F(0), F(0), p(d_rays), None, p(out), None) == -1      # scratch needed
    assert 'ws' in lib.fastnerf_last_error().decode()
    assert lib.fastnerf_pose_grad_ws_floats(-1, 3) == -1 and lib.fastnerf_pose_grad_ws_floats(5, 0) == -1
    assert lib.fastnerf_pose_exp(0, p(poses), None, p(out), None) == -1 and 'n_img >= 1' in lib.fastnerf_last_error().decode()
    assert lib.fastnerf_pose_exp(3, None, None, p(out), None) == -1 and 'null pointer' in lib.fastnerf_last_error().decode()
    assert lib.fastnerf_pose_exp_bwd(3, p(poses), None, None, p(out), None) == -1 and 'null pointer' in lib.fastnerf_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()      # nothing was enqueued
    # the wrappers: dtype, shape, device
    with pytest.raises(TypeError, match='float32'):
        fn.ops.pose_exp(poses.double())
    with pytest.raises(ValueError, match='shape'):
        fn.ops.pose_exp(poses, torch.zeros(3, 5, device='cuda'))
    with pytest.raises(TypeError, match='int32'):
        fn.ops.pose_grad(pix.long(), poses, K, d_rays)
    with pytest.raises(ValueError, match='shape'):
        fn.ops.pose_grad(pix, poses, K, d_rays[:, :8].contiguous())
    with pytest.raises(RuntimeError, match='GPU'):
        fn.ops.pose_grad(pix.cpu(), poses, K, d_rays)


def test_pose_rays_and_table(fn):
    pix, poses, K, d_rays = [t.cuda() if torch.is_tensor(t) else t for t in P.float_case(67, 3, (1,))]
    table = fn.poses.PoseTable(poses).cuda()
    assert table.xi.shape == (3, 6) and table.xi.requires_grad and np.array_equal(bits(table.poses()), bits(poses))
    rays = fn.poses.pose_rays(pix, table(), K, 2.0, 6.0)
    want = fn.ops.pack_rays(*fn.ops.gen_rays_pixels(pix, poses, K), 2.0, 6.0)
    assert np.array_equal(bits(rays), bits(want)) and rays.requires_grad
    # its backward is ops.pose_grad (to the poses) followed by ops.pose_exp_bwd (to xi)
    leaf = poses.clone().requires_grad_()
    (fn.poses.pose_rays(pix, leaf, K, 2.0, 6.0) * d_rays).sum().backward()
    d_poses = fn.ops.pose_grad(pix, poses, K, d_rays)
    assert np.array_equal(bits(leaf.grad), bits(d_poses))
    (rays * d_rays).sum().backward()
    assert np.array_equal(bits(table.xi.grad), bits(fn.ops.pose_exp_bwd(poses, table.xi.data, d_poses)))
    # a batch without view directions: the gradient of the first eight columns alone
    leaf8 = poses.clone().requires_grad_()
    (fn.poses.pose_rays(pix, leaf8, K, 2.0, 6.0)[:, :8] * d_rays[:, :8]).sum().backward()
    d8 = d_rays.clone()
    d8[:, 8:] = 0
    assert np.array_equal(bits(leaf8.grad), bits(fn.ops.pose_grad(pix, poses, K, d8)))
