"""The environment-map kernels (csrc/envmap.hip: ops.env_lookup, ops.env_grad) against tests/env_ref.py.

Shapes: R in {2, 5, 8} x n in {1, 257, 70 001} (the last past one grid of 65 536 threads).  Directions: Gaussian draws of mixed length,
and (env_ref.special_directions) the six axes and eight diagonals, dz = +-0, zero and -0 components, the zero vector, lengths 1e-20 and
1e20, points on the |x| + |y| = 1 diamond, on the border and at the corners, a non-finite 1-norm.
(1) lookup: bit for bit against the float32 restatement, and within the float64 bound; read in place from an [n,11] batch;
(2) env_grad within its float64 bound, one pass and two, acc in {0, 1, random}; and bit for bit the restatement's integer sums;
(3) exactness: unit weights, small integers times 2^-20, 10 000 rays over 16 texels: the exact sums;
(4) order freedom: a permutation, the two halves in either order, two calls: identical bits;
(5) the adjoint identity on the GPU's outputs, within the sum of the two bounds;
(6) EnvMap autograd = ops.env_grad with acc = 0; an Adam fit of a hidden table comes down monotonically;
(7) n = 0, canaries around the outputs, the wrappers' refusals."""
import numpy as np
import pytest
import torch

import env_ref as E

pytestmark = pytest.mark.gpu

RS = (2, 5, 8)
NS = (1, 257, E.N_BIG)
F32 = np.float32


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


def bits(t):
    t = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return t.view(np.uint32)


def cu(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('R', RS)
def test_lookup(fn, R, n):
    """(1)"""
    T, d = E.table(R, R), E.directions(n, n + R)
    got = fn.ops.env_lookup(cu(T), cu(d))
    want = E.lookup32(T, d)
    bad = np.nonzero((bits(got) != bits(want)).any(1))[0]
    assert bad.size == 0, (bad[:8], d[bad[:8]], got.cpu().numpy()[bad[:8]], want[bad[:8]])
    v, e = E.lookup64(T, d)
    err = np.abs(got.cpu().numpy().astype(np.float64) - v)
    print('lookup R=%d n=%d: largest fraction of the bound reached %.3f' % (R, n, float((err / np.maximum(e, 1e-300)).max())))
    assert (err <= e).all()
    # the same read in place from columns 3:6 of an [n,11] batch, and of an [n,8] one
    for width in (11, 8):
        rays = torch.full((n, width), 7.0, device='cuda')
        rays[:, 3:6] = cu(d)
        assert np.array_equal(bits(fn.ops.env_lookup(cu(T), rays[:, 3:6])), bits(want))


@pytest.mark.parametrize('acc_kind', ['zero', 'one', 'random'])
@pytest.mark.parametrize('two', [False, True], ids=['one_pass', 'two_passes'])
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('R', RS)
def test_grad(fn, R, n, two, acc_kind):
    """(2)"""
    d = E.directions(n, n + R)
    g1, a1, g0, a0 = E.grad_inputs(n, n, two, acc_kind)
    got = fn.ops.env_grad(R, cu(d), cu(g1), cu(a1), cu(g0), cu(a0))
    v, e = E.grad64(d, R, g1, a1, g0, a0)
    err = np.abs(got.cpu().numpy().astype(np.float64) - v)
    print('grad R=%d n=%d: largest fraction of the bound reached %.3f' % (R, n, float((err / np.maximum(e, 1e-300)).max())))
    assert (err <= e).all()
    assert np.array_equal(bits(got), bits(E.grad32(d, R, g1, a1, g0, a0)))
    if acc_kind == 'one':
        assert not got.any()


def test_exact_integer_sums(fn):
    """(3)"""
    R, n = 4, 10000
    rng = np.random.default_rng(5)
    tex = rng.integers(0, R * R, n)
    d = E.centre_directions(R)[tex]
    k = rng.integers(-8, 9, (n, 3))
    g = (k * 2.0 ** -20).astype(F32)
    want = np.zeros((R * R, 3), np.int64)
    np.add.at(want, tex, k)
    got = fn.ops.env_grad(R, cu(d), cu(g), torch.zeros(n, device='cuda'))
    assert np.array_equal(bits(got), bits((want * 2.0 ** -20).astype(F32).reshape(R, R, 3)))
    # and the lookup at the centres returns the texels' own bits
    T = E.table(R, 1)
    assert np.array_equal(bits(fn.ops.env_lookup(cu(T), cu(E.centre_directions(R)))), bits(T.reshape(-1, 3)))


@pytest.mark.parametrize('R', (5, 8))
def test_order_freedom(fn, R):
    """(4)"""
    n = 20001
    d = E.directions(n, 3 + R)
    g1, a1, g0, a0 = E.grad_inputs(n, R, True, 'random')
    args = [cu(x) for x in (d, g1, a1, g0, a0)]
    first = fn.ops.env_grad(R, *args)
    again = fn.ops.env_grad(R, *args)
    assert np.array_equal(bits(first), bits(again))
    perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).cuda()
    assert np.array_equal(bits(fn.ops.env_grad(R, *[x[perm].contiguous() for x in args])), bits(first))
    h = 7777      # two calls' worth of rows, concatenated in the other order
    swapped = [torch.cat([x[h:], x[:h]], 0).contiguous() for x in args]
    assert np.array_equal(bits(fn.ops.env_grad(R, *swapped)), bits(first))


@pytest.mark.parametrize('R', RS)
def test_adjoint_identity(fn, R):
    """(5): |<lookup(T), G> - <T, env_grad(G)>| <= sum |G| e_lookup + sum |T| e_grad."""
    n = 4099
    T, d = E.table(R, 20 + R), E.directions(n, 30 + R)
    G = np.random.default_rng(R).standard_normal((n, 3)).astype(F32)
    zero = np.zeros(n, F32)
    look = fn.ops.env_lookup(cu(T), cu(d)).cpu().numpy().astype(np.float64)
    dT = fn.ops.env_grad(R, cu(d), cu(G), cu(zero)).cpu().numpy().astype(np.float64)
    _, e_look = E.lookup64(T, d)
    _, e_grad = E.grad64(d, R, G, zero)
    lhs, rhs = (look * G).sum(), (T.astype(np.float64) * dT).sum()
    cap = (np.abs(G) * e_look).sum() + (np.abs(T) * e_grad).sum()
    print('adjoint R=%d: |lhs - rhs| = %.3e, cap %.3e' % (R, abs(lhs - rhs), cap))
    assert abs(lhs - rhs) <= cap


def test_envmap_autograd_and_fit(fn):
    """(6)"""
    R, n = 8, 4096
    d = cu(E.directions(n, 77))
    env = fn.envmap.EnvMap(res=R).cuda()
    G = cu(np.random.default_rng(2).standard_normal((n, 3)).astype(F32))
    rays = torch.zeros(n, 11, device='cuda')
    rays[:, 3:6] = d
    out = env(rays[:, 3:6])
    assert np.array_equal(bits(out), bits(fn.ops.env_lookup(env.table.data, d)))
    (out * G).sum().backward()
    assert np.array_equal(bits(env.table.grad), bits(fn.ops.env_grad(R, d, G, torch.zeros(n, device='cuda'))))
    d_req = d.clone().requires_grad_(True)
    env(d_req).sum().backward()
    assert d_req.grad is None      # the directions get no gradient
    # an Adam fit of a hidden table from its own lookups
    hidden = cu(E.table(R, 9))
    target = fn.ops.env_lookup(hidden, d)
    idx, w, _ = E.taps32(d.cpu().numpy(), R)
    hit = np.zeros(R * R, bool)
    hit[idx[w > 0]] = True
    hit = torch.from_numpy(hit).cuda()
    env = fn.envmap.EnvMap(res=R).cuda()
    opt = torch.optim.Adam(env.parameters(), lr=2e-2)
    errs = []
    for it in range(200):
        opt.zero_grad()
        loss = ((env(d) - target) ** 2).mean()
        loss.backward()
        opt.step()
        if (it + 1) % 25 == 0:
            errs.append(float((env.table.data - hidden).reshape(-1, 3)[hit].abs().mean()))
    print('EnvMap fit: mean |table - hidden| on the %d hit texels every 25 steps: %s' % (int(hit.sum()), ' '.join('%.4f' % x for x in errs)))
    assert all(b < a for a, b in zip(errs, errs[1:])), errs
    assert errs[-1] < 0.5 * errs[0]


def test_empty_batch_canaries_and_refusals(fn):
    """(7)"""
    R = 5
    T = cu(E.table(R, 0))
    assert tuple(fn.ops.env_lookup(T, torch.zeros(0, 3, device='cuda')).shape) == (0, 3)
    buf = torch.full((R * R * 3 + 64,), 3.0, device='cuda')
    d_table = buf[32:32 + R * R * 3].view(R, R, 3)
    fn.ops.env_grad(R, torch.zeros(0, 3, device='cuda'), torch.zeros(0, 3, device='cuda'), torch.zeros(0, device='cuda'), d_table=d_table)
    assert not d_table.any() and (buf[:32] == 3).all() and (buf[-32:] == 3).all()
    # canaries around out, d_table and ws of a full call
    n = 257
    d = cu(E.directions(n, 1))
    obuf = torch.full((n * 3 + 64,), 3.0, device='cuda')
    fn.ops.env_lookup(T, d, out=obuf[32:32 + n * 3].view(n, 3))
    assert (obuf[:32] == 3).all() and (obuf[-32:] == 3).all()
    ws = torch.full((R * R * 3 + 16,), 5, device='cuda', dtype=torch.int64)
    g1, a1, _, _ = E.grad_inputs(n, 1, False, 'random')
    buf.fill_(3.0)
    fn.ops.env_grad(R, d, cu(g1), cu(a1), d_table=d_table, ws=ws[8:8 + R * R * 3])
    assert (buf[:32] == 3).all() and (buf[-32:] == 3).all() and (ws[:8] == 5).all() and (ws[-8:] == 5).all()
    assert np.array_equal(bits(d_table), bits(E.grad32(d.cpu().numpy(), R, g1, a1)))
    with pytest.raises(ValueError, match='table'):
        fn.ops.env_lookup(torch.zeros(1, 1, 3, device='cuda'), d)
    with pytest.raises(TypeError, match='float32'):
        fn.ops.env_lookup(T.double(), d)
    with pytest.raises(ValueError, match='dirs'):
        fn.ops.env_lookup(T, torch.zeros(n, 4, device='cuda'))
    with pytest.raises(ValueError, match='go together'):
        fn.ops.env_grad(R, d, cu(g1), cu(a1), g_rgb0=cu(g1))
    with pytest.raises(ValueError, match='acc'):
        fn.ops.env_grad(R, d, cu(g1), cu(a1)[:-1].contiguous())
    with pytest.raises(ValueError, match='ws'):
        fn.ops.env_grad(R, d, cu(g1), cu(a1), ws=torch.zeros(3, device='cuda', dtype=torch.int64))
    with pytest.raises(ValueError, match='ws'):      # enough words, but strided: the kernel writes consecutive ones
        fn.ops.env_grad(R, d, cu(g1), cu(a1), ws=torch.zeros(2 * R * R * 3, device='cuda', dtype=torch.int64)[::2])
    frozen = fn.envmap.EnvMap(res=R).cuda().requires_grad_(False)
    assert not frozen(d).requires_grad      # a frozen map: no scatter is recorded
    with pytest.raises(RuntimeError, match='GPU only'):
        fn.ops.env_lookup(T, d.cpu())
