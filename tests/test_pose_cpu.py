"""The formulas of csrc/pose.hip on the host (tests/pose_ref.py): the closed forms of include/fastnerf.h ("pose table") equal float64
autograd of torch.matrix_exp, and their float32 restatement stays inside the bounds the GPU tests (tests/test_gpu_pose.py) hold the
kernels to -- 32 * 2^-24 per rotation entry, 32 * 2^-24 * sum|G| per d_omega entry: a cap, with the restatement's own peaks printed
beside it (pytest -s).  The references of pose_grad agree with each other, and a sequential fp32 sum sits far inside its bound."""
import numpy as np
import pytest
import torch

import pose_ref as P

N_IMGS = [1, 5, 300]


@pytest.mark.parametrize('n_img', N_IMGS)
def test_closed_forms_equal_float64_autograd(n_img):
    worst = [0.0, 0.0]
    for base, xi, g in P.exp_cases(n_img):
        ref, got = P.exp_ref64(base, xi), P.closed_exp(base, xi)
        worst[0] = max(worst[0], float((got - ref).abs().max()))
        dref, dgot = P.exp_bwd_ref64(base, xi, g), P.closed_bwd(base, xi, g)
        assert torch.isfinite(dgot).all() and torch.isfinite(dref).all()
        scale = g[:, :, :3].double().abs().sum((1, 2))[:, None]
        worst[1] = max(worst[1], float(((dgot - dref).abs() / scale).max()))
    print('\nclosed forms vs float64 autograd, n_img %d: pose %.2e  d_xi / sum|G| %.2e' % (n_img, *worst))
    # 1e-12: six decades below the fp32 bounds these references serve, and above torch.matrix_exp's own error -- its Taylor approximant
    # of the degree it picks at theta = 0.01 is 8e-14 away from Rodrigues' formula with float64 sin / cos, which the closed form meets to 1e-16
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12


def test_closed_form_equals_plain_rodrigues_where_that_does_not_cancel():
    """theta >= 0.1: (1 - cos) / theta^2 loses at most 3 digits in float64; the half-angle form agrees to 1e-13."""
    for base, xi, _ in P.exp_cases(5):
        w = xi[:, :3].double()
        th = w.norm(dim=-1)
        keep = th >= 0.1
        if not keep.any():
            continue
        K = P.hat(w[keep])
        t = th[keep][:, None, None]
        R = torch.eye(3, dtype=torch.float64) + torch.sin(t) / t * K + (1 - torch.cos(t)) / t ** 2 * (K @ K)
        got = P.closed_exp(base[keep], xi[keep])[:, :, :3]
        assert (got - R @ base[keep].double()[:, :, :3]).abs().max() <= 1e-13


def test_closed_forms_at_theta_zero():
    base, xi, g = P.exp_inputs(4, seed=3)
    xi[:, :3] = 0
    assert torch.equal(P.closed_exp(base, xi)[:, :, :3], base.double()[:, :, :3])
    assert (P.closed_bwd(base, xi, g) - P.exp_bwd_ref64(base, xi, g)).abs().max() <= 1e-14


@pytest.mark.parametrize('n_img', N_IMGS)
def test_float32_restatement_stays_inside_the_bounds(n_img):
    peak = [0.0, 0.0]
    for base, xi, g in P.exp_cases(n_img):
        ref, got = P.exp_ref64(base, xi), P.exp_f32(base, xi)
        assert torch.isfinite(got).all()
        peak[0] = max(peak[0], float((got.double() - ref)[:, :, :3].abs().max()) / 2.0 ** -24)
        assert torch.equal(got[:, :, 3], base[:, :, 3] + xi[:, 3:])                      # t: the fp32 sum
        dref, dgot = P.exp_bwd_ref64(base, xi, g), P.exp_bwd_f32(base, xi, g)
        assert torch.isfinite(dgot).all()
        scale = g[:, :, :3].double().abs().sum((1, 2))[:, None]
        peak[1] = max(peak[1], float(((dgot.double() - dref)[:, :3].abs() / scale).max()) / 2.0 ** -24)
        assert torch.equal(dgot[:, 3:], g[:, :, 3])                                      # d_tau: a copy
    print('\nfloat32 restatement, n_img %d: rotation %.1f x 2^-24, d_omega %.1f x 2^-24 sum|G| (cap 32)' % (n_img, *peak))
    assert peak[0] <= 32.0 and peak[1] <= 32.0


def test_float32_restatement_returns_the_base_at_zero():
    base, xi, _ = P.exp_inputs(7, seed=5)
    got = P.exp_f32(base, torch.zeros_like(xi))
    assert np.array_equal(got.numpy().view(np.uint32), base.numpy().view(np.uint32))


@pytest.mark.parametrize('n,n_img,empty', [(1, 1, ()), (67, 3, (1,)), (257, 5, ()), (4099, 5, (3,))])
def test_pose_grad_references_agree(n, n_img, empty):
    """The int64 sums of the exact case equal the float64 reference's, entry for entry; images without rays are zero."""
    pix, poses, K, d_rays, want = P.exact_case(n, n_img, empty)
    ref, B, counts = P.pose_grad_ref64(pix, poses, K, d_rays)
    assert torch.equal(ref, want.double())
    for i in empty:
        assert counts[i] == 0 and (want[i] == 0).all()
    assert int(counts.sum()) == n and want.abs().max() < 2 ** 24


@pytest.mark.parametrize('n,n_img,empty', [(67, 3, (1,)), (4099, 5, ()), (4099, 1, ())])
def test_a_sequential_float32_sum_sits_inside_the_pose_grad_bound(n, n_img, empty):
    """|sum - ref| <= (m_i + 32) 2^-24 B_i[j,k] holds for any order of fp32 sums; the sequential one is printed as a fraction of it."""
    pix, poses, K, d_rays = P.float_case(n, n_img, empty)
    ref, B, counts = P.pose_grad_ref64(pix, poses, K, d_rays)
    F = np.float32
    dirs = P.dirs_of(pix, K, torch.float32).numpy()
    R = poses.numpy()[pix[:, 0].long().numpy()][:, :, :3]
    d = np.stack([(dirs[:, 0] * R[:, k, 0] + dirs[:, 1] * R[:, k, 1]) + dirs[:, 2] * R[:, k, 2] for k in range(3)], -1).astype(F)
    nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    v = d / nrm
    g = d_rays.numpy()
    vd = ((v[:, 0] * g[:, 8] + v[:, 1] * g[:, 9]) + v[:, 2] * g[:, 10])[:, None]
    g_d = g[:, 3:6] + (g[:, 8:11] - v * vd) / nrm
    rows = np.concatenate([g_d[:, :, None] * dirs[:, None, :], g[:, 0:3, None]], -1).astype(F)
    got = np.zeros((n_img, 3, 4), F)
    for r, i in zip(rows, pix[:, 0].numpy()):
        got[i] = got[i] + r
    bound = (counts.double()[:, None, None] + 32.0) * 2.0 ** -24 * B
    frac = float(((torch.from_numpy(got).double() - ref).abs() / bound.clamp_min(1e-300)).max())
    print('\nsequential fp32 pose_grad (%d, %d): %.4f of the bound' % (n, n_img, frac))
    assert frac <= 1.0
