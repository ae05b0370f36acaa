"""float64 restatements of the small kernels of csrc/train.hip (adam_kernel, mse_leafmax_kernel) and the rounding-count bounds their
outputs are held to.  numpy only; imported by tests/test_train_ref_cpu.py (which validates it against an fp32 emulation of the
kernel's operation order and against torch.optim.Adam) and by tests/test_gpu_loss_adam_fp64.py.

u = 2^-24 is the unit roundoff of fp32 (round to nearest): fl(x) = x (1 + d), |d| <= u.

adam_kernel, per element (fastnerf_adam_step forms the constants in double and rounds each to fp32 once):
    M  = fadd(fmul(m, b1), fmul(omb1, g))                  b1, omb1 = fl(beta1), fl(1 - beta1)
    V  = fadd(fmul(v, b2), fmul(omb2, fmul(g, g)))         b2, omb2 = fl(beta2), fl(1 - beta2)
    dn = fadd(sqrtf(V) / bc2_sqrt, eps)                    bc2_sqrt = fl(sqrt(1 - beta2^t)), eps = fl(eps)
    P  = fsub(p, fmul(step_size, M / dn))                  step_size = fl(lr / (1 - beta1^t))
Counting every rounding once (the constants count one each; sqrtf and `/` are correctly rounded):
    M:  each product carries its constant and its own rounding (2), the sum one more: 3 on every term, and the terms may cancel, so
        |M - M64| <= 3u (|b1 m| + |(1 - b1) g|).
    V:  the longer term is omb2 (1), g g (1), their product (1), the sum (1) = 4; the terms are non-negative:
        |V - V64| <= 4u V64.
    dn: sqrt halves V's 4 to 2, sqrtf (1), bc2_sqrt (1), the division (1) = 5 on the first term; eps (1) on the second; the sum (1):
        6, both terms non-negative, so relative to dn64.
    update = step_size M / dn: 3 (M, relative to A below) + 6 (dn) + the division (1) + step_size (1) + the product (1) = 12, all
        relative to A = (lr / bc1) (|b1 m| + |(1 - b1) g|) / dn64 >= |update64|, the update's magnitude before the two terms of M
        cancel.  The subtraction adds one rounding of the result:
        |P - P64| <= u |P64| + 12u A.
These are the first-order counts; the second-order terms are below 80 u^2."""
import numpy as np

U = 2.0 ** -24
F32 = np.float32

M_ROUNDINGS = 3
V_ROUNDINGS = 4
P_ROUNDINGS = 12


def _f64(x):
    return np.asarray(x, F32).astype(np.float64)


def adam_step64(p, g, m, v, lr, b1, b2, eps, t):
    """One Adam step (torch.optim.Adam without weight decay or amsgrad) in float64 from fp32 state -> (p', m', v', A); A is the
    magnitude the update's error is relative to (module docstring)."""
    p, g, m, v = (_f64(x) for x in (p, g, m, v))
    lr, b1, b2, eps, t = float(lr), float(b1), float(b2), float(eps), int(t)
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v1) / np.sqrt(bc2) + eps
    p1 = p - (lr / bc1) * (m1 / denom)
    A = (lr / bc1) * (np.abs(b1 * m) + np.abs((1.0 - b1) * g)) / denom
    return p1, m1, v1, A


def adam_bounds(p, g, m, v, lr, b1, b2, eps, t):
    """(p64, m64, v64, bound_p, bound_m, bound_v): the float64 step and the absolute error each fp32 output may have."""
    p1, m1, v1, A = adam_step64(p, g, m, v, lr, b1, b2, eps, t)
    bm = M_ROUNDINGS * U * (np.abs(float(b1) * _f64(m)) + np.abs((1.0 - float(b1)) * _f64(g)))
    bv = V_ROUNDINGS * U * v1
    bp = U * np.abs(p1) + P_ROUNDINGS * U * A
    return p1, m1, v1, bp, bm, bv


def adam_ratios(got_p, got_m, got_v, p, g, m, v, lr, b1, b2, eps, t):
    """Worst |fp32 output - float64| in units of u times the quantity its bound is relative to: (r_p, r_m, r_v), to be compared with
    P_ROUNDINGS (after taking u |p'| off), M_ROUNDINGS and V_ROUNDINGS.  An output that differs where its bound is 0 gives inf."""
    p1, m1, v1, A = adam_step64(p, g, m, v, lr, b1, b2, eps, t)
    sm = np.abs(float(b1) * _f64(m)) + np.abs((1.0 - float(b1)) * _f64(g))

    def ratio(err, scale):
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.where(err == 0, 0.0, err / (U * scale))
        return float(r.max()) if r.size else 0.0
    ep = np.maximum(np.abs(_f64(got_p) - p1) - U * np.abs(p1), 0.0)
    return ratio(ep, A), ratio(np.abs(_f64(got_m) - m1), sm), ratio(np.abs(_f64(got_v) - v1), v1)


def adam_step32(p, g, m, v, lr, b1, b2, eps, t):
    """fp32 emulation of fastnerf_adam_step + adam_kernel in the kernel's operation order (numpy float32 arithmetic rounds every
    operation once, like fadd / fmul / fsub, sqrtf and `/` under -ffp-contract=off) -> (p', m', v') float32."""
    p, g, m, v = (np.asarray(x, F32) for x in (p, g, m, v))
    bc1 = 1.0 - float(b1) ** int(t)
    bc2 = 1.0 - float(b2) ** int(t)
    step_size, bc2_sqrt = F32(float(lr) / bc1), F32(np.sqrt(bc2))
    fb1, fb2, omb1, omb2, feps = F32(b1), F32(b2), F32(1.0 - float(b1)), F32(1.0 - float(b2)), F32(eps)
    m1 = (m * fb1) + (omb1 * g)
    v1 = (v * fb2) + (omb2 * (g * g))
    denom = np.sqrt(v1) / bc2_sqrt + feps
    p1 = p - step_size * (m1 / denom)
    assert p1.dtype == F32 and m1.dtype == F32 and v1.dtype == F32
    return p1, m1, v1


def adam_state(n, seed, zero_block=True):
    """The state the one-step Adam tests start from -> float32 (p, g, m, v) and the bool mask of the block with g = m = v = 0:
    scale = 10^U(-12, 1) per element; g = N(0,1) scale with 10 % exact zeros; m = N(0,1) scale c, c in {0.01, 1, 10};
    v = (U(0,1) + 1e-3) scale^2 c', c' in {0.01, 1, 100} (>= ~1e-29: no subnormals); p = N(0,1) with half of the entries exactly 0
    (there p' is the rounded update itself)."""
    rs = np.random.RandomState(seed)
    scale = 10.0 ** rs.uniform(-12.0, 1.0, n)
    g = rs.randn(n) * scale
    g[rs.rand(n) < 0.1] = 0.0
    m = rs.randn(n) * scale * rs.choice([0.01, 1.0, 10.0], n)
    v = (rs.rand(n) + 1e-3) * scale * scale * rs.choice([0.01, 1.0, 100.0], n)
    p = rs.randn(n)
    p[rs.rand(n) < 0.5] = 0.0
    zero = np.zeros(n, bool)
    if zero_block and n >= 8:
        zero[n // 3:n // 3 + max(1, n // 8)] = True
        g[zero] = m[zero] = v[zero] = 0.0
        p[zero] = rs.randn(int(zero.sum())) + 3.0        # (non-zero parameters that must come back bit for bit)
    return p.astype(F32), g.astype(F32), m.astype(F32), v.astype(F32), zero


ADAM_T = (1, 2, 3, 10, 1000, 200000)
ADAM_LR = (5e-4, 5e-5)


# ---- the loss ---------------------------------------------------------------------------------------------------------------------
MSE_THREADS = 1024


def mse64(rgb, rgb0, target, grad_scale):
    """(loss, loss0, g, g0) in float64 from fp32 inputs: mean((x - t)^2) over rays and channels and grad_scale * 2 (x - t) / (3 n);
    loss0 = 0.0 and g0 = None without rgb0."""
    t = _f64(target)
    n = t.shape[0]

    def one(x):
        d = _f64(x) - t
        return float((d * d).sum() / (3.0 * n)), float(grad_scale) * 2.0 * d / (3.0 * n)
    l1, g1 = one(rgb)
    l0, g0 = (0.0, None) if rgb0 is None else one(rgb0)
    return l1, l0, g1, g0


def loss_chain(n):
    """(g, rounds, k) of fastnerf_mse_leafmax at n rays: g workgroups of 1024 threads (1 up to 65536 rays, else ceil(n / 1024) capped
    at 1024), `rounds` rays per thread at the most, and k = the roundings on the longest path from an input to a loss:
        3              a term: the difference (1), squared: twice that and the product's own (2 + 1)
        3 rounds - 1   the thread's running sum: three channels per ray, the first addition is to 0 and exact
        10             block_sum: 6 butterfly steps over a wave, 4 over the 16 wave sums
        2              inv_count = fl(1 / 3n) and the product with it
        g              for g > 1: the atomic additions of the block results
    All terms are non-negative, so every rounding is relative to a partial sum below the total: |loss - loss64| <= k u loss64."""
    n = int(n)
    g = 1 if n <= 65536 else min(1024, (n + MSE_THREADS - 1) // MSE_THREADS)
    rounds = (n + g * MSE_THREADS - 1) // (g * MSE_THREADS)
    k = 3 + (3 * rounds - 1) + 10 + 2 + (g if g > 1 else 0)
    return g, rounds, k


GRAD_ROUNDINGS = 3      # gscale = fl(2 grad_scale / 3n) (1), the difference (1), their product (1)
