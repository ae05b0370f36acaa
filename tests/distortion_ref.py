"""The distortion loss on the ray weights (include/fastnerf.h, "distortion loss"), restated on the host.

  distortion_ref      the float64 O(S^2) definition, loss and gradient: the reference of every test
  distortion_f32      the kernel's cancellation-free order (csrc/distortion.hip) in numpy float32
  textbook_f32        the O(S) prefix form m_i W_{<i} - WM_{<i} in numpy float32: the mutant the accuracy bar rejects
  fixtures            uniform depths, and the clustered fine pass (64 linspace + 128 samples within 1e-3 of the span of a surface)

Per ray: edges e_i = z_i (i < S), e_S = max(far, z_{S-1}); t(x) = (x - near) / (far - near), or with lindisp
(1/near - 1/x) / (1/near - 1/far); delta_i = t(e_{i+1}) - t(e_i), m_i = (t(e_i) + t(e_{i+1})) / 2;
l = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i.  A ray whose span is not a positive finite number, or whose `skip` byte is
set, has l = 0 and a zero gradient."""
import numpy as np


def bar(S):
    """Relative error allowed for l and for every dl/dw_i against float64 on the same fp32 inputs: two nested sums of at most S
    non-negative terms plus the per-term products."""
    return (2 * S + 32) * 2.0 ** -24


def _edges(z, far):
    return np.concatenate([z, np.maximum(far, z[:, -1])[:, None]], axis=1)


def _span(near, far, lindisp):
    with np.errstate(all='ignore'):
        return 1.0 / near - 1.0 / far if lindisp else far - near


def _valid(span, skip):
    ok = np.isfinite(span) & (span > 0)
    if skip is not None:
        ok &= np.asarray(skip) == 0
    return ok


def distortion_ref(w, z, near, far, lindisp=False, skip=None):
    """float64, straight from the definition -> (l [n], dl/dw [n,S])."""
    w, z, near, far = (np.asarray(a, np.float64) for a in (w, z, near, far))
    n, S = w.shape
    span = _span(near, far, lindisp)
    ok = _valid(span, skip)
    e = _edges(z, far)
    with np.errstate(all='ignore'):
        if lindisp:
            t = (1.0 / near[:, None] - 1.0 / e) / span[:, None]
        else:
            t = (e - near[:, None]) / span[:, None]
        delta = t[:, 1:] - t[:, :-1]
        m = 0.5 * (t[:, 1:] + t[:, :-1])
    ell = np.zeros(n)
    g = np.zeros((n, S))
    for r in np.nonzero(ok)[0]:
        D = np.abs(m[r][:, None] - m[r][None, :])
        ell[r] = w[r] @ D @ w[r] + (w[r] ** 2 * delta[r]).sum() / 3.0
        g[r] = 2.0 * (D @ w[r]) + 2.0 / 3.0 * w[r] * delta[r]
    return ell, g


def torch_expression(w, z, near, far, lindisp=False):
    """The same expression on torch tensors (any dtype, differentiable in w) -> l [n].  Valid spans only."""
    import torch
    e = torch.cat([z, torch.maximum(far, z[:, -1])[:, None]], 1)
    if lindisp:
        t = (1.0 / near[:, None] - 1.0 / e) / (1.0 / near - 1.0 / far)[:, None]
    else:
        t = (e - near[:, None]) / (far - near)[:, None]
    delta = t[:, 1:] - t[:, :-1]
    m = 0.5 * (t[:, 1:] + t[:, :-1])
    D = (m[:, :, None] - m[:, None, :]).abs()
    return (w[:, :, None] * w[:, None, :] * D).sum((1, 2)) + (w * w * delta).sum(1) / 3.0


def _gamma_delta_f32(z, near, far, lindisp):
    f = np.float32
    z, near, far = (np.asarray(a, f) for a in (z, near, far))
    e = _edges(z, far)
    inv = (f(1) / _span(near, far, lindisp).astype(f))[:, None]
    d1 = e[:, 1:] - e[:, :-1]
    d2 = e[:, 2:] - e[:, :-2]
    if lindisp:
        delta = d1 / (e[:, :-1] * e[:, 1:]) * inv
        gam = f(0.5) * d2 / (e[:, :-2] * e[:, 2:]) * inv
    else:
        delta = d1 * inv
        gam = f(0.5) * d2 * inv
    return np.concatenate([gam, np.zeros((len(z), 1), f)], 1).astype(f), delta.astype(f)


def distortion_f32(w, z, near, far, lindisp=False):
    """The cancellation-free order in float32 (sequential sums): gamma from depth differences, P from the near end, Q from the far end,
    A_i = sum_{k<i} gamma_k P_k, B_i = sum_{k>=i} gamma_k Q_k.  Valid spans only -> (l, dl/dw) float32."""
    f = np.float32
    w = np.asarray(w, f)
    gam, delta = _gamma_delta_f32(z, near, far, lindisp)
    P = np.cumsum(w, axis=1, dtype=f)
    Qincl = np.cumsum(w[:, ::-1], axis=1, dtype=f)[:, ::-1]
    Q = np.concatenate([Qincl[:, 1:], np.zeros((len(w), 1), f)], 1)
    gp, gq = gam * P, gam * Q
    A = np.concatenate([np.zeros((len(w), 1), f), np.cumsum(gp, axis=1, dtype=f)[:, :-1]], 1)
    B = np.cumsum(gq[:, ::-1], axis=1, dtype=f)[:, ::-1]
    g = f(2) * (A + B) + f(2.0 / 3.0) * (w * delta)
    ell = np.sum(f(2) * (w * A) + f(1.0 / 3.0) * (w * (w * delta)), axis=1, dtype=f)
    return ell, g


def textbook_f32(w, z, near, far, lindisp=False):
    """The O(S) form from two prefix sums of w and w m, in float32: sum_j w_j |m_i - m_j| = (m_i W_{<i} - WM_{<i}) + (WM_{>i} - m_i W_{>i}).
    Valid spans only -> (l, dl/dw) float32."""
    f = np.float32
    w, z, near, far = (np.asarray(a, f) for a in (w, z, near, far))
    e = _edges(z, far)
    span = _span(near, far, lindisp).astype(f)[:, None]
    t = ((f(1) / near[:, None] - f(1) / e) / span if lindisp else (e - near[:, None]) / span).astype(f)
    delta = t[:, 1:] - t[:, :-1]
    m = f(0.5) * (t[:, 1:] + t[:, :-1])
    zero = np.zeros((len(w), 1), f)
    W = np.cumsum(w, axis=1, dtype=f)
    WM = np.cumsum(w * m, axis=1, dtype=f)
    Wlt, WMlt = np.concatenate([zero, W[:, :-1]], 1), np.concatenate([zero, WM[:, :-1]], 1)
    Wgt, WMgt = W[:, -1:] - W, WM[:, -1:] - WM
    inner = (m * Wlt - WMlt) + (WMgt - m * Wgt)
    g = f(2) * inner + f(2.0 / 3.0) * (w * delta)
    ell = np.sum(w * inner + f(1.0 / 3.0) * (w * (w * delta)), axis=1, dtype=f)
    return ell, g


def rel_err(got, ref, floor=1e-30):
    """max over the elements with |ref| > floor of |got - ref| / |ref| (0 when there is none)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    sel = np.abs(ref) > floor
    return float(np.max(np.abs(got[sel] - ref[sel]) / np.abs(ref[sel]))) if sel.any() else 0.0


# ---- fixtures: float32 arrays (w [n,S], z [n,S], near [n], far [n]) -------------------------------------------------------------------
def _bounds(n, rng):
    near = rng.uniform(1.5, 2.5, n).astype(np.float32)
    far = (near + rng.uniform(3.0, 5.0, n)).astype(np.float32)
    return near, far


def _lin(near, far, S, lindisp):
    u = np.linspace(0.0, 1.0, S)[None, :]
    nr, fr = near[:, None].astype(np.float64), far[:, None].astype(np.float64)
    return 1.0 / (1.0 / nr * (1 - u) + 1.0 / fr * u) if lindisp else nr * (1 - u) + fr * u


def uniform_fixture(n, S, seed=0, lindisp=False):
    """Evenly placed depths, jittered inside their bins, with weights of a random compositing (some exact zeros)."""
    rng = np.random.default_rng(seed)
    near, far = _bounds(n, rng)
    z = _lin(near, far, S + 1, lindisp)
    z = np.sort(z[:, :-1] + rng.uniform(0, 1, (n, S)) * (z[:, 1:] - z[:, :-1]), axis=1).astype(np.float32)
    alpha = rng.uniform(0, 1, (n, S)) ** 4 * (rng.uniform(0, 1, (n, S)) > 0.3)
    T = np.cumprod(np.concatenate([np.ones((n, 1)), 1 - alpha[:, :-1]], 1), axis=1)
    return (alpha * T).astype(np.float32), z, near, far


def clustered_fixture(n, seed=0, lindisp=False, coarse=64, fine=128):
    """A fine pass: `coarse` linspace depths plus `fine` importance samples from N(c, 1e-3 of the span) around a surface at c, sorted;
    weights a bump of width 2e-3 of the span around c on a floor of 1e-6, the total scaled into [0.05, 1]."""
    rng = np.random.default_rng(seed)
    near, far = _bounds(n, rng)
    span = (far - near).astype(np.float64)[:, None]
    c = near[:, None] + span * rng.uniform(0.2, 0.8, (n, 1))
    z = np.concatenate([_lin(near, far, coarse, lindisp), c + 1e-3 * span * rng.standard_normal((n, fine))], 1)
    z = np.sort(np.clip(z, near[:, None], far[:, None]), axis=1).astype(np.float32)
    w = 1e-6 + np.exp(-0.5 * ((z - c) / (2e-3 * span)) ** 2)
    w = w / w.sum(1, keepdims=True) * rng.uniform(0.05, 1.0, (n, 1))
    return w.astype(np.float32), z, near, far
