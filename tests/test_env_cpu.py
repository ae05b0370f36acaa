"""The references of the environment map against each other (tests/env_ref.py), the octahedral map's geometry, and what of the binding
and the wrappers needs no GPU.

(i)   the numpy-float32 restatement stays inside the bound of the float64 evaluation on the GPU tests' inputs, lookup and gradient;
(ii)  the mirror wrap: directions a hair either side of each border edge, and near each corner, get the same colour up to the bound;
(iii) the six axes and the eight diagonals land on the expected texel coordinates;
(iv)  the adjoint identity <lookup(T), G> = <T, scatter(G)> in float64;
(v)   header, library and binding agree on the new symbols; the C entry points' and the wrappers' refusals that come before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import env_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS = (2, 5, 8)
NS = (1, 257, E.N_BIG)
F32 = np.float32


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('R', RS)
def test_lookup_restatement_within_the_bound(R, n):
    T, d = E.table(R, R), E.directions(n, n + R)
    got = E.lookup32(T, d)
    v, e = E.lookup64(T, d)
    assert np.isfinite(e).all() and np.isfinite(got).all()
    assert (np.abs(got.astype(np.float64) - v) <= e).all(), np.max(np.abs(got - v) / e)
    assert np.median(e) < 1e-4      # the bound says something: colours are O(1)


@pytest.mark.parametrize('acc_kind', ['zero', 'one', 'random'])
@pytest.mark.parametrize('two', [False, True], ids=['one_pass', 'two_passes'])
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('R', RS)
def test_grad_restatement_within_the_bound(R, n, two, acc_kind):
    d = E.directions(n, n + R)
    g1, a1, g0, a0 = E.grad_inputs(n, n, two, acc_kind)
    got = E.grad32(d, R, g1, a1, g0, a0)
    v, e = E.grad64(d, R, g1, a1, g0, a0)
    assert (np.abs(got.astype(np.float64) - v) <= e).all()
    if acc_kind == 'one':
        assert not got.any()      # an opaque ray shows no background: exact zeros
    else:
        assert (e <= 1e-4 * np.abs(v).max() + 1e-9).all()


def test_a_wrong_formula_leaves_the_bound():
    """The bound is tight enough to tell the map from one without the fold or with the wrap's flip left out."""
    R, n = 8, 4096
    T, d = E.table(R, 3), E.directions(n, 5)
    v, e = E.lookup64(T, d)
    no_fold = E.lookup32(T, np.abs(d) * np.sign(d[:, :1] + 0.5) * [1, 1, 1])      # dz >= 0 everywhere
    assert (np.abs(no_fold - v) > e).any()
    idx, w, _ = E.taps32(d, R)
    c = E.coords32(d, R)
    i0, j0 = np.floor(c['x']).astype(int), np.floor(c['y']).astype(int)
    clamp = lambda i, j: np.clip(j, 0, R - 1) * R + np.clip(i, 0, R - 1)      # noqa: E731
    idx2 = np.stack([clamp(i0, j0), clamp(i0 + 1, j0), clamp(i0, j0 + 1), clamp(i0 + 1, j0 + 1)], 1)
    plain = (w[:, :, None].astype(np.float64) * T.reshape(-1, 3)[idx2]).sum(1)
    assert (np.abs(plain - v) > e).any()


def _dir_of(px, py, lower):
    """A float64 direction whose octahedral image is (px, py) on the upper (|px| + |py| <= 1) or, folded, the lower hemisphere."""
    if not lower:
        return np.array([px, py, 1 - abs(px) - abs(py)])
    sx, sy = (1.0 if px >= 0 else -1.0), (1.0 if py >= 0 else -1.0)
    ux, uy = (1 - abs(py)) * sx, (1 - abs(px)) * sy
    return np.array([ux, uy, -(1 - abs(ux) - abs(uy))])


@pytest.mark.parametrize('R', RS)
def test_mirror_wrap_has_no_seam(R):
    """On the border px = +-1 the points (+-1, t) and (+-1, -t) are one direction (and the same along py = +-1); the four corners are the
    -z pole.  Two directions a hair (1e-6 of the square) either side get colours that differ by what the interpolant's slope allows over
    that distance, plus the two bounds."""
    T = E.table(R, 7 + R)
    Dx, Dy = E.lipschitz(T)
    h = 1e-6
    pairs = []
    for t in (0.1, 0.37, 0.5, 0.93):
        for sgn in (1.0, -1.0):
            pairs.append((_dir_of(sgn * (1 - h), t, True), _dir_of(sgn * (1 - h), -t, True)))      # the edges px = +-1
            pairs.append((_dir_of(t, sgn * (1 - h), True), _dir_of(-t, sgn * (1 - h), True)))      # the edges py = +-1
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):                                                                      # the corners against each other
            pairs.append((_dir_of(sx * (1 - h), sy * (1 - h), True), _dir_of(-sx * (1 - h), -sy * (1 - h), True)))
            pairs.append((_dir_of(sx * (1 - h), sy * (1 - h), True), np.array([0.0, 0.0, -1.0])))
    a = np.array([p[0] for p in pairs], F32)
    b = np.array([p[1] for p in pairs], F32)
    ca, cb = E.lookup32(T, a), E.lookup32(T, b)
    _, ea = E.lookup64(T, a)
    _, eb = E.lookup64(T, b)
    # each direction is within 2 h (+ fp32 rounding of the direction) of the border in p, R/2 texels per unit of p, on both axes
    slack = (Dx + Dy)[None, :] * (2 * (2 * h + 8 * E.U) * R / 2)
    assert (np.abs(ca.astype(np.float64) - cb) <= slack + ea + eb).all()
    assert slack.max() < 1e-3      # colours are O(1): a seam would show
    # and the fold matters: the same directions mirrored to the upper hemisphere have other colours (R = 2 is too symmetric to tell)
    if R > 2:
        assert np.abs(ca - E.lookup32(T, a * np.array([1, 1, -1], F32))).max() > 1e-2


@pytest.mark.parametrize('R', RS)
def test_axes_and_diagonals_land_where_expected(R):
    third = 1.0 / 3.0
    cases = [((1, 0, 0), (1, 0)), ((-1, 0, 0), (-1, 0)), ((0, 1, 0), (0, 1)), ((0, -1, 0), (0, -1)), ((0, 0, 1), (0, 0)),
             ((0, 0, -1), (1, 1))]
    for sx in (1, -1):
        for sy in (1, -1):
            cases.append(((sx, sy, 1), (sx * third, sy * third)))
            cases.append(((sx, sy, -1), (sx * 2 * third, sy * 2 * third)))
    d = np.array([c[0] for c in cases], F32)
    for scale in (1.0, 7.5, 1e-20, 1e20):
        c = E.coords32(d * F32(scale), R)
        want = (np.array([k[1] for k in cases]) * 0.5 + 0.5) * R - 0.5
        tol = 4 * E.U * R
        assert (np.abs(c['x'] - want[:, 0]) <= tol).all() and (np.abs(c['y'] - want[:, 1]) <= tol).all()
    # the axes are exact, and +x / -x sit on the middle of the right / left border
    c = E.coords32(d[:6], R)
    assert np.array_equal(c['x'], np.array([R - 0.5, -0.5, R / 2 - 0.5, R / 2 - 0.5, R / 2 - 0.5, R - 0.5], F32))
    assert np.array_equal(c['y'], np.array([R / 2 - 0.5, R / 2 - 0.5, R - 0.5, -0.5, R / 2 - 0.5, R - 0.5], F32))


def test_centre_directions_have_unit_weights():
    R = 4
    idx, w, _ = E.taps32(E.centre_directions(R), R)
    assert np.array_equal(idx[:, 0], np.arange(R * R))
    assert np.array_equal(w, np.tile(np.array([[1, 0, 0, 0]], F32), (R * R, 1)))


@pytest.mark.parametrize('R', RS)
def test_adjoint_identity_in_float64(R):
    n = 2001
    d = E.directions(n, 11)
    rng = np.random.default_rng(R)
    T = rng.standard_normal((R, R, 3))
    G = rng.standard_normal((n, 3)).astype(F32)
    idx, _, (_, _, fx, fy) = E.taps32(d, R)
    fx, fy = fx.astype(np.float64), fy.astype(np.float64)
    w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], 1)
    look = (w[:, :, None] * T.reshape(-1, 3)[idx]).sum(1)
    lhs, rhs = (look * G).sum(), (T * E.scatter64(d, R, G)).sum()
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(look * G).sum() + 1)


def test_integer_sums_do_not_depend_on_order():
    R, n = 5, 3001
    d = E.directions(n, 4)
    g1, a1, g0, a0 = E.grad_inputs(n, 4, True, 'random')
    p = np.random.default_rng(0).permutation(n)
    a, b = E.grad32(d, R, g1, a1, g0, a0), E.grad32(d[p], R, g1[p], a1[p], g0[p], a0[p])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- header, library, binding ------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ('fastnerf_env_lookup', 'fastnerf_env_grad_ws_bytes', 'fastnerf_env_grad')


def test_symbols_declared_exported_and_bound():
    import fastnerf
    from fastnerf import _lib
    src = open(os.path.join(ROOT, 'include', 'fastnerf.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, src), name + ' is not declared in fastnerf.h'
        assert hasattr(lib, name), name + ' is not exported'
        assert name in _lib.SIGNATURES
    m = re.search(r'int fastnerf_env_lookup\((.*?)\);', src, re.S)
    assert len(m.group(1).split(',')) == len(_lib.SIGNATURES['fastnerf_env_lookup'][1]) == 7
    m = re.search(r'int fastnerf_env_grad\((.*?)\);', src, re.S)
    assert len(m.group(1).split(',')) == len(_lib.SIGNATURES['fastnerf_env_grad'][1]) == 11
    assert _lib.SIGNATURES['fastnerf_env_grad_ws_bytes'] == (ctypes.c_int64, [ctypes.c_int])
    for name in ('env_lookup', 'env_grad', 'env_grad_ws_bytes'):
        assert callable(getattr(fastnerf.ops, name))
    assert issubclass(fastnerf.envmap.EnvMap, torch.nn.Module)


def test_c_refusals_come_before_any_launch():
    """Every refusal returns -1 with a message; the pointers are not device memory, so a launch would not survive them."""
    from fastnerf import _lib
    lib = _lib.lib()
    p = 0x1000
    assert lib.fastnerf_env_grad_ws_bytes(4) == 4 * 4 * 3 * 8 and lib.fastnerf_env_grad_ws_bytes(2) == 96
    assert lib.fastnerf_env_grad_ws_bytes(1) == -1 and lib.fastnerf_env_grad_ws_bytes(-3) == -1
    bad_lookup = [(-1, p, 3, p, 4, p), (5, p, 3, p, 1, p), (5, p, 2, p, 4, p), (5, None, 3, p, 4, p), (5, p, 3, None, 4, p),
                  (5, p, 3, p, 4, None), (0, None, 3, None, 0, None)]
    for a in bad_lookup:
        assert lib.fastnerf_env_lookup(*a, None) == -1, a
        assert b'fastnerf_env_lookup' in lib.fastnerf_last_error()
    assert lib.fastnerf_env_lookup(0, None, 3, None, 4, None, None) == 0      # n == 0: nothing to do
    bad_grad = [(-1, p, 3, 4, p, p, None, None, p, p), (5, p, 3, 1, p, p, None, None, p, p), (5, p, 2, 4, p, p, None, None, p, p),
                (5, None, 3, 4, p, p, None, None, p, p), (5, p, 3, 4, None, p, None, None, p, p), (5, p, 3, 4, p, None, None, None, p, p),
                (5, p, 3, 4, p, p, None, None, None, p), (5, p, 3, 4, p, p, None, None, p, None), (5, p, 3, 4, p, p, p, None, p, p),
                (5, p, 3, 4, p, p, None, p, p, p), (0, None, 3, 4, None, None, None, None, None, None)]
    for a in bad_grad:
        assert lib.fastnerf_env_grad(*a, None) == -1, a
        assert b'fastnerf_env_grad' in lib.fastnerf_last_error()


def test_wrapper_refusals_need_no_gpu():
    from fastnerf import envmap, ops
    T, d = torch.zeros(4, 4, 3), torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.env_lookup(T, d)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.env_grad(4, d, torch.zeros(5, 3), torch.zeros(5))
    for bad in (torch.zeros(4, 4), torch.zeros(4, 5, 3), torch.zeros(1, 1, 3), torch.zeros(4, 4, 4)):
        with pytest.raises(ValueError, match='table'):
            ops._need_table(bad)
    with pytest.raises(TypeError, match='float32'):
        ops._need_table(torch.zeros(4, 4, 3, dtype=torch.float64))
    with pytest.raises(TypeError, match='float32'):
        ops._need_dirs(d.double())
    for bad in (torch.zeros(5), torch.zeros(5, 4), torch.zeros(3, 5).t(), torch.zeros(5, 6)[:, ::2]):
        with pytest.raises(ValueError, match='dirs'):
            ops._need_dirs(bad)
    rays = torch.zeros(7, 11)
    assert ops._need_dirs(rays[:, 3:6]) == (7, 11) and ops._need_dirs(d) == (5, 3) and ops._need_dirs(torch.zeros(7, 8)[:, 3:6]) == (7, 8)
    assert ops._need_dirs(torch.zeros(0, 3)) == (0, 3) and ops._need_dirs(rays[:1, 3:6]) == (1, 3)
    with pytest.raises(ValueError, match='R >= 2'):
        envmap.EnvMap(res=1)
    with pytest.raises(ValueError, match='colour'):
        envmap.EnvMap(res=4, colour=(0.5, 0.5))
    env = envmap.EnvMap(res=4, colour=(0.25, 0.5, 0.75))
    assert tuple(env.table.shape) == (4, 4, 3) and env.res == 4 and isinstance(env.table, torch.nn.Parameter)
    assert torch.equal(env.table.detach()[2, 3], torch.tensor([0.25, 0.5, 0.75]))
    with pytest.raises(RuntimeError, match='GPU only'):
        env(d)
