"""tests/train_ref.py validated on the CPU before the GPU tests rely on it: the rounding-count bounds of adam_step64 hold for an fp32
emulation of adam_kernel's exact operation order and for torch.optim.Adam (fp32, CPU) over every regime the GPU test runs, and
loss_chain restates the launch geometry of fastnerf_mse_leafmax (hand-computed values)."""
import numpy as np
import pytest
import torch

import train_ref as T

B1, B2, EPS = 0.9, 0.999, 1e-8
N = 200000


@pytest.fixture(scope='module')
def states():
    return {seed: T.adam_state(N, seed) for seed in (1, 2)}


def check(got, state, lr, t):
    p, g, m, v, zero = state
    p1, m1, v1 = got
    p64, m64, v64, bp, bm, bv = T.adam_bounds(p, g, m, v, lr, B1, B2, EPS, t)
    r = T.adam_ratios(p1, m1, v1, p, g, m, v, lr, B1, B2, EPS, t)
    assert (np.abs(m1.astype(np.float64) - m64) <= bm).all(), ('m', r)
    assert (np.abs(v1.astype(np.float64) - v64) <= bv).all(), ('v', r)
    assert (np.abs(p1.astype(np.float64) - p64) <= bp).all(), ('p', r)
    # the block with g = m = v = 0: nothing moves
    assert np.array_equal(p1[zero], p[zero]) and not m1[zero].any() and not v1[zero].any() and zero.any()
    return r


@pytest.mark.parametrize('lr', T.ADAM_LR)
@pytest.mark.parametrize('t', T.ADAM_T)
def test_bounds_hold_for_the_fp32_emulation_of_the_kernel(states, t, lr, capsys):
    worst = np.zeros(3)
    for seed, st in states.items():
        p, g, m, v, _ = st
        worst = np.maximum(worst, check(T.adam_step32(p, g, m, v, lr, B1, B2, EPS, t), st, lr, t))
    with capsys.disabled():
        print('\nADAM_EMULATION t=%d lr=%g: worst ratios p %.2f (bound %d)  m %.2f (%d)  v %.2f (%d)' % (
            t, lr, worst[0], T.P_ROUNDINGS, worst[1], T.M_ROUNDINGS, worst[2], T.V_ROUNDINGS))
    assert worst[0] > 1.0 and worst[1] > 1.0 and worst[2] > 1.0, 'the emulation rounds: the bounds are not vacuous'


@pytest.mark.parametrize('lr', T.ADAM_LR)
@pytest.mark.parametrize('t', T.ADAM_T)
def test_bounds_hold_for_torch_adam(states, t, lr):
    """torch.optim.Adam from the same state at step t: its fp32 arithmetic (lerp for m, addcmul for v, addcdiv for p) rounds no more
    often than the kernel's, so the same bounds hold; a restatement that were not Adam would miss them by orders of magnitude."""
    p, g, m, v, _ = st = states[1]
    prm = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([prm], lr=lr, betas=(B1, B2), eps=EPS)
    opt.state[prm] = {'step': torch.tensor(float(t - 1)), 'exp_avg': torch.from_numpy(m.copy()), 'exp_avg_sq': torch.from_numpy(v.copy())}
    prm.grad = torch.from_numpy(g.copy())
    opt.step()
    s = opt.state[prm]
    assert int(s['step']) == t
    check((prm.detach().numpy(), s['exp_avg'].numpy(), s['exp_avg_sq'].numpy()), st, lr, t)


def test_wrong_kernels_miss_the_bounds(states):
    """The three slips the parameter bar of the old test (1e-7 + 1e-6 |p|) lets through, restated in the emulation: each one leaves
    the bound on p'."""
    p, g, m, v, _ = states[1]
    F = np.float32

    def variant(t, lr, eps_inside=False, fp32_bc=False, t_step=None):
        bc1 = 1.0 - B1 ** (t if t_step is None else t_step)
        bc2_sqrt = F(np.sqrt(F(1.0) - F(np.power(F(B2), F(t))))) if fp32_bc else F(np.sqrt(1.0 - B2 ** t))
        step_size = F(lr / bc1)
        m1 = (m * F(B1)) + (F(1.0 - B1) * g)
        v1 = (v * F(B2)) + (F(1.0 - B2) * (g * g))
        denom = np.sqrt(v1 + F(EPS)) / bc2_sqrt if eps_inside else np.sqrt(v1) / bc2_sqrt + F(EPS)
        return p - step_size * (m1 / denom)

    def misses(p1, t, lr):
        p64, _, _, bp, _, _ = T.adam_bounds(p, g, m, v, lr, B1, B2, EPS, t)
        return bool((np.abs(p1.astype(np.float64) - p64) > bp).any())
    assert not misses(variant(3, 5e-4), 3, 5e-4)
    assert misses(variant(3, 5e-4, eps_inside=True), 3, 5e-4)
    assert misses(variant(1, 5e-4, fp32_bc=True), 1, 5e-4)
    assert misses(variant(10, 5e-4, t_step=9), 10, 5e-4)


@pytest.mark.parametrize('n,want', [(1000, (1, 1, 17)), (65536, (1, 64, 206)), (65537, (65, 1, 82)), (1048576, (1024, 1, 1041)),
                                    (1049601, (1024, 2, 1044))])
def test_loss_chain_by_hand(n, want):
    """n = 1000: one workgroup, one ray per thread: 3 + 2 + 10 + 2 = 17.  65536: 64 rays per thread: 3 + 191 + 10 + 2 = 206.
    65537: ceil(65537 / 1024) = 65 workgroups of one round, 17 + 65 atomics = 82.  2^20: 1024 workgroups, 17 + 1024 = 1041.
    2^20 + 1025: 1026 workgroups wanted, capped at 1024, so the first threads take a second ray: 3 + 5 + 10 + 2 + 1024 = 1044."""
    assert T.loss_chain(n) == want


def test_mse64_is_the_mean_squared_error():
    rs = np.random.RandomState(0)
    a, b, t = (rs.rand(777, 3).astype(np.float32) for _ in range(3))
    l1, l0, g1, g0 = T.mse64(a, b, t, 0.25)
    ta, tb, tt = (torch.from_numpy(x).double().requires_grad_(True) for x in (a, b, t))
    L1, L0 = ((ta - tt) ** 2).mean(), ((tb - tt) ** 2).mean()
    ga, gb = torch.autograd.grad(0.25 * (L1 + L0), [ta, tb])
    assert abs(l1 - L1.item()) < 1e-15 and abs(l0 - L0.item()) < 1e-15
    assert np.abs(g1 - ga.numpy()).max() < 1e-18 and np.abs(g0 - gb.numpy()).max() < 1e-18
    one = T.mse64(a, None, t, 1.0)
    assert one[0] == l1 and one[1] == 0.0 and one[3] is None
