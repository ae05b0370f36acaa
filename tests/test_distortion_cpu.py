"""The distortion loss without a GPU: the float64 reference (tests/distortion_ref.py) against torch float64 autograd of the same
expression, its edge cases, the accuracy bar on the cancellation-free order in float32 -- and the textbook prefix form missing it on
the clustered fixture: the mutant the bar exists to reject -- the new C-ABI symbols and the struct size."""
import ctypes as C

import numpy as np
import pytest
import torch

import distortion_ref as D
from fastnerf import _lib

NEW = ('fastnerf_distortion', 'fastnerf_distortion_mean', 'fastnerf_render_rays_bwd_w', 'fastnerf_render_rays_bwd_live_w',
       'fastnerf_step_dist_size', 'fastnerf_train_step_dist', 'fastnerf_train_step_march_dist')


@pytest.mark.parametrize('lindisp', [False, True])
@pytest.mark.parametrize('fixture', ['uniform', 'clustered'])
def test_reference_is_float64_autograd(fixture, lindisp):
    w, z, near, far = D.uniform_fixture(5, 33, 1, lindisp) if fixture == 'uniform' else D.clustered_fixture(3, 2, lindisp)
    ell, g = D.distortion_ref(w, z, near, far, lindisp)
    tw = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    tz, tn, tf = (torch.tensor(a, dtype=torch.float64) for a in (z, near, far))
    tl = D.torch_expression(tw, tz, tn, tf, lindisp)
    tl.sum().backward()
    np.testing.assert_allclose(ell, tl.detach().numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(g, tw.grad.numpy(), rtol=1e-11, atol=1e-300)
    assert (ell > 0).all() and (g >= 0).all()


def test_reference_edge_cases():
    w, z, near, far = D.uniform_fixture(8, 9, 3)
    far[0] = near[0]                 # empty span
    far[1] = near[1] - 1             # negative span
    far[2] = np.inf
    near[3] = np.nan
    skip = np.zeros(8, np.uint8)
    skip[4] = 1
    w[5] = 0                         # all-zero weights
    z[6] = z[6, 0]                   # repeated depths: every interval but the last is empty
    ell, g = D.distortion_ref(w, z, near, far, skip=skip)
    for r in range(6):
        assert ell[r] == 0 and not np.signbit(ell[r])
    for r in range(5):
        assert (g[r] == 0).all() and not np.signbit(g[r]).any()
    # zero weights: l = 0; the gradient of a zero-weight sample is 2 sum_j w_j |m_i - m_j| = 0 here as well
    assert (g[5] == 0).all()
    # repeated depths: all m but the last coincide, delta = 0 on those
    m_last = 0.5 * (1 + (z[6, 0] - near[6]) / (far[6] - near[6]))
    m0 = (z[6, 0] - near[6]) / (far[6] - near[6])
    want = 2 * w[6, :-1].sum() * w[6, -1] * (m_last - m0) + w[6, -1] ** 2 * (1 - m0) / 3
    assert ell[6] == pytest.approx(want, rel=1e-6)
    assert ell[7] > 0
    # lindisp: near = 0 has an infinite disparity span
    near0 = near.copy()
    near0[7] = 0
    assert D.distortion_ref(w, z, near0, far, lindisp=True)[0][7] == 0


@pytest.mark.parametrize('lindisp', [False, True])
@pytest.mark.parametrize('case', ['clustered', 'uniform2', 'uniform65', 'uniform512'])
def test_cancellation_free_order_meets_the_bar(case, lindisp):
    w, z, near, far = (D.clustered_fixture(64, 5, lindisp) if case == 'clustered'
                       else D.uniform_fixture(16, int(case[7:]), 6, lindisp))
    S = w.shape[1]
    ell, g = D.distortion_ref(w, z, near, far, lindisp)
    ell32, g32 = D.distortion_f32(w, z, near, far, lindisp)
    e_l, e_g = D.rel_err(ell32, ell), D.rel_err(g32, g)
    print(f'{case} lindisp={lindisp}: l {e_l * 2 ** 24:.1f}, g {e_g * 2 ** 24:.1f} (x 2^-24; bar {2 * S + 32})')
    assert e_l <= D.bar(S) and e_g <= D.bar(S)


@pytest.mark.parametrize('lindisp', [False, True])
def test_textbook_prefix_form_misses_the_bar(lindisp):
    """m_i W_{<i} - WM_{<i}: two numbers of order 1 subtracted for one of order |m_i - m_j| ~ 1e-3."""
    w, z, near, far = D.clustered_fixture(64, 5, lindisp)
    ell, g = D.distortion_ref(w, z, near, far, lindisp)
    _, g32 = D.textbook_f32(w, z, near, far, lindisp)
    e_g = D.rel_err(g32, g)
    print(f'textbook lindisp={lindisp}: g {e_g:.2e} against the bar {D.bar(192):.2e}')
    assert e_g > 10 * D.bar(192)


def test_symbols_and_struct():
    lib = _lib.lib()
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert lib.fastnerf_step_dist_size() == C.sizeof(_lib.StepDist) == 48
    assert C.sizeof(_lib.WeightGrads) == 16


def test_refusals_need_no_gpu():
    """The argument checks come before anything touches a pointer or the GPU."""
    lib = _lib.lib()
    one = C.c_void_p(8)         # (never dereferenced)
    assert lib.fastnerf_distortion(4, 0, one, one, one, 0, None, 1.0, None, one, one, None) == -1
    assert lib.fastnerf_last_error().decode().startswith('fastnerf_distortion:')
    assert lib.fastnerf_distortion(4, 513, one, one, one, 0, None, 1.0, None, one, one, None) == -1
    assert lib.fastnerf_distortion(-1, 8, one, one, one, 0, None, 1.0, None, one, one, None) == -1
    assert lib.fastnerf_distortion(4, 8, one, one, one, 0, None, 1.0, None, None, None, None) == -1      # neither ell nor g_w
    assert lib.fastnerf_distortion(4, 8, None, one, one, 0, None, 1.0, None, one, one, None) == -1
    assert lib.fastnerf_distortion(0, 8, None, None, None, 0, None, 1.0, None, None, None, None) == 0
    assert lib.fastnerf_distortion_mean(0, one, None, one, None) == -1
    assert lib.fastnerf_distortion_mean(4, None, None, one, None) == -1
