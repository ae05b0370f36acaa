"""The exposure kernels (csrc/exposure.hip: ops.expo_apply, ops.expo_grad) against tests/expo_ref.py.

Shapes: n in {0, 1, 67, 257, 4099} x n_img in {1, 3, 5 with image 3 empty, 100}, one and two passes: one block and several, one chunk
and several (4099 rays: 5 chunks of 820 with n_img <= 100), the finish launch alone (n = 0).
(i)    e and the in-place g: bit for bit against the float32 restatement, rays that name no image (-1, n_img) included: they keep
       their bits and are counted nowhere;
(ii)   d_ab and counts: exact on the integer case (any fp32 summation order gives the int64 sums);
(iii)  the float case: |d_ab - ref64| <= (6 m_i + 32) 2^-24 B_i (expo_ref: a derived cap); the largest fraction of it that is reached
       is printed (recorded in profiles/exposure.md); loss_reg within (n_img + 8) 2^-24 of the float64 sum of its non-negative terms;
(iv)   the identity table: e has rgb's bits, g has G's;
(v)    two calls give identical bits; canaries on both sides of d_ab, counts and ws survive;
(vi)   the refusals, at the C boundary and in ops."""
import ctypes

import numpy as np
import pytest
import torch

import expo_ref as E

pytestmark = pytest.mark.gpu

NS = [0, 1, 67, 257, 4099]
IMGS = [(1, None), (3, None), (5, 3), (100, None)]
LAM, GS = 0.7, 0.5


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def cu(x):
    return None if x is None else x.cuda().contiguous()


def run(fn, c, lam, gs):
    """apply, then grad on copies of G -> (e1, e0, g1, g0, d_ab, counts, loss_reg) on the device."""
    img, ab = cu(c['img']), cu(c['ab'])
    e1, e0 = fn.ops.expo_apply(cu(c['rgb1']), img, ab, rgb0=cu(c['rgb0']))
    g1, g0 = cu(c['G1']).clone(), None if c['G0'] is None else cu(c['G0']).clone()
    d_ab, counts, loss_reg = fn.ops.expo_grad(img, ab, lam, gs, e1, g1, e0=e0, g0=g0)
    return e1, e0, g1, g0, d_ab, counts, loss_reg


@pytest.mark.parametrize('two', [False, True], ids=['one_pass', 'two_passes'])
@pytest.mark.parametrize('n_img,empty', IMGS)
@pytest.mark.parametrize('n', NS)
def test_float_case(fn, n, n_img, empty, two):
    """(i), (iii)."""
    c = E.float_case(n, n_img, two, seed=100 * n_img + n, empty=empty)
    e1, e0, g1, g0, d_ab, counts, loss_reg = run(fn, c, LAM, GS)
    img, ab = c['img'].numpy(), c['ab'].numpy()
    for e, rgb in ((e1, c['rgb1']), (e0, c['rgb0'])):
        if rgb is not None:
            assert np.array_equal(bits(e), E.restate_apply(img, ab, rgb.numpy()).view(np.uint32))
    rs = E.restate_grad(img, ab, LAM, GS, e1.cpu().numpy(), c['G1'].numpy(), None if e0 is None else e0.cpu().numpy(),
                        None if not two else c['G0'].numpy())
    assert np.array_equal(bits(g1), rs['g1'].view(np.uint32))
    if two:
        assert np.array_equal(bits(g0), rs['g0'].view(np.uint32))
    ok = E.in_range(img, n_img)
    if n >= 67:
        assert (~ok).sum() >= 2
    assert np.array_equal(bits(e1)[~ok], bits(c['rgb1'])[~ok]) and np.array_equal(bits(g1)[~ok], bits(c['G1'])[~ok])
    ref = E.ref64(c['img'], c['ab'], LAM, GS, e1.cpu(), c['G1'], None if e0 is None else e0.cpu(), c['G0'])
    assert torch.equal(counts.cpu().long(), ref['counts']) and int(counts.sum()) == int(ok.sum())
    if empty is not None:
        assert int(counts[empty]) == 0 and np.array_equal(bits(d_ab[empty]), np.zeros(2, np.uint32))
    err = (d_ab.cpu().double() - ref['d_ab']).abs()
    cap = E.bound_factor(ref['counts'].double()[:, None]) * ref['B']
    frac = float((err / cap.clamp_min(1e-300)).max()) if n else 0.0
    print('\nexpo_grad n %5d n_img %3d passes %d: reached %.4f of the cap' % (n, n_img, 2 if two else 1, frac))
    assert torch.isfinite(d_ab).all() and (err <= cap).all(), frac
    want = float(ref['loss_reg'])
    assert abs(float(loss_reg) - want) <= (n_img + 8) * E.U * want
    if n == 0:
        assert not d_ab.any() and not counts.any() and float(loss_reg) == 0.0


@pytest.mark.parametrize('two', [False, True], ids=['one_pass', 'two_passes'])
@pytest.mark.parametrize('n_img,empty', IMGS)
@pytest.mark.parametrize('n', NS)
def test_exact_integer_case(fn, n, n_img, empty, two):
    """(ii)."""
    c, want, m = E.exact_case(n, n_img, two, seed=7 * n_img + n, empty=empty)
    e1, e0, g1, g0, d_ab, counts, loss_reg = run(fn, c, 0.0, 1.0)
    assert torch.equal(d_ab.cpu().double(), want), (d_ab.cpu().double() - want).abs().max()
    assert torch.equal(counts.cpu().long(), m)
    if n:
        assert np.array_equal(bits(e1), E.restate_apply(c['img'].numpy(), c['ab'].numpy(), c['rgb1'].numpy()).view(np.uint32))


def test_identity_table(fn):
    """(iv): a fresh ExposureTable."""
    c = E.float_case(4099, 5, True, seed=1, empty=3)
    table = fn.exposure.ExposureTable(5).cuda()
    assert torch.equal(table.ab.data.cpu(), torch.tensor([[0.5, 0.0]]).repeat(5, 1))
    c['ab'] = table.ab.data.cpu()
    c['rgb1'][0, 0], c['rgb1'][1, 1] = -0.0, 0.0
    e1, e0, g1, g0, d_ab, counts, loss_reg = run(fn, c, 3.0, 1.0)
    assert np.array_equal(bits(e1), bits(c['rgb1'])) and np.array_equal(bits(e0), bits(c['rgb0']))
    assert np.array_equal(bits(g1), bits(c['G1'])) and np.array_equal(bits(g0), bits(c['G0']))
    assert float(loss_reg) == 0.0
    ref = E.ref64(c['img'], c['ab'], 3.0, 1.0, c['rgb1'], c['G1'], c['rgb0'], c['G0'])
    assert ((d_ab.cpu().double() - ref['d_ab']).abs() <= E.bound_factor(ref['counts'].double()[:, None]) * ref['B']).all()
    scale, shift = table.table()
    assert torch.equal(scale.detach().cpu(), torch.ones(5)) and torch.equal(shift.detach().cpu(), torch.zeros(5))


def test_sign_points(fn):
    """The kinks of the absolute values: a = 0, scale = 1 from both sides of a, shift = 0 -- against float64 autograd with torch.abs."""
    ab = torch.tensor([[0.0, 0.3], [0.5, 0.0], [-0.5, -0.2], [1.0, 0.0], [-1.25, 0.1], [0.25, -0.1]])
    gen = torch.Generator().manual_seed(2)
    n = 600
    c = dict(img=(torch.arange(n) % 6).int(), ab=ab, rgb1=torch.rand(n, 3, generator=gen), G1=torch.randn(n, 3, generator=gen), rgb0=None, G0=None)
    e1, _, g1, _, d_ab, counts, loss_reg = run(fn, c, 2.0, 0.25)
    ref = E.ref64(c['img'], ab, 2.0, 0.25, e1.cpu(), c['G1'])
    assert ((d_ab.cpu().double() - ref['d_ab']).abs() <= E.bound_factor(100.0) * ref['B']).all()
    assert float(d_ab[0, 0]) == 0.0 and float(ref['d_ab'][0, 0]) == 0.0
    assert abs(float(loss_reg) - float(ref['loss_reg'])) <= 14 * E.U * float(ref['loss_reg'])


@pytest.mark.parametrize('n,n_img', [(67, 3), (4099, 5), (4099, 100)])
def test_same_bits_twice_and_canaries(fn, n, n_img):
    """(v)."""
    c = E.float_case(n, n_img, True, seed=5)
    img, ab = cu(c['img']), cu(c['ab'])
    e1, e0 = fn.ops.expo_apply(cu(c['rgb1']), img, ab, rgb0=cu(c['rgb0']))
    need = fn.ops.expo_grad_ws_floats(n, n_img)
    assert need == n_img * min(-(-n // 1024), 1024 // n_img) * 3
    pad = 64
    outs = []
    for _ in range(2):
        d_buf = torch.full((pad + 2 * n_img + pad,), 7.25, device='cuda')
        c_buf = torch.full((pad + n_img + pad,), -77, device='cuda', dtype=torch.int32)
        w_buf = torch.full((pad + need + pad,), 7.25, device='cuda')
        g1, g0 = cu(c['G1']).clone(), cu(c['G0']).clone()
        d_ab, counts, loss_reg = fn.ops.expo_grad(img, ab, LAM, GS, e1, g1, e0=e0, g0=g0, d_ab=d_buf[pad:pad + 2 * n_img].view(n_img, 2),
                                                  counts=c_buf[pad:pad + n_img], ws=w_buf[pad:pad + need])
        for buf, canary in ((d_buf, 7.25), (c_buf, -77), (w_buf, 7.25)):
            assert (buf[:pad] == canary).all() and (buf[-pad:] == canary).all()
        assert int(counts.sum()) == int(E.in_range(c['img'].numpy(), n_img).sum())
        outs.append((bits(g1), bits(g0), bits(d_ab), counts.cpu().numpy(), bits(loss_reg), bits(w_buf[pad:pad + need])))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_autograd_function(fn):
    """exposure.apply: e and the gradients with respect to rgb and the table are the two ops'."""
    c = E.float_case(257, 3, False, seed=8, outside=False)      # (penalty() indexes the table in torch: every ray names an image)
    table = fn.exposure.ExposureTable(3).cuda()
    table.ab.data.copy_(c['ab'])
    rgb = cu(c['rgb1']).requires_grad_(True)
    img = cu(c['img'])
    e = fn.exposure.apply(rgb, img.long(), table)
    G = cu(c['G1'])
    (e * G).sum().backward()
    e1, _, g1, _, d_ab, _, _ = run(fn, c, 0.0, 1.0)
    assert torch.equal(e, e1) and torch.equal(rgb.grad, g1) and torch.equal(table.ab.grad, d_ab)
    want = float(E.ref64(c['img'], c['ab'], 0.0, 1.0, e1.cpu(), c['G1'])['loss_reg'])
    assert abs(float(table.penalty(img).detach()) - want) <= 1e-5 * want


def test_refusals(fn):
    """(vi): -1 before any launch, by name."""
    lib = fn._lib.lib()
    n, n_img = 67, 3
    c = E.float_case(n, n_img, True, seed=3)
    img, ab = cu(c['img']), cu(c['ab'])
    t = {k: cu(c[k]) for k in ('rgb1', 'rgb0', 'G1', 'G0')}
    e1, e0 = torch.empty_like(t['rgb1']), torch.empty_like(t['rgb1'])
    d_ab, counts, loss_reg = torch.zeros(n_img, 2, device='cuda'), torch.zeros(n_img, device='cuda', dtype=torch.int32), torch.zeros(1, device='cuda')
    ws = torch.zeros(fn.ops.expo_grad_ws_floats(n, n_img), device='cuda')
    p = fn._lib.ptr
    s = fn._lib.stream()

    def apply(**kw):
        a = dict(n=n, n_img=n_img, img=p(img), ab=p(ab), rgb1=p(t['rgb1']), rgb0=p(t['rgb0']), e1=p(e1), e0=p(e0))
        a.update(kw)
        return lib.fastnerf_expo_apply(a['n'], a['n_img'], a['img'], a['ab'], a['rgb1'], a['rgb0'], a['e1'], a['e0'], s)

    def grad(**kw):
        a = dict(n=n, n_img=n_img, img=p(img), ab=p(ab), lam=1.0, gs=1.0, e1=p(e1), e0=p(e0), g1=p(t['G1']), g0=p(t['G0']), ws=p(ws),
                 d_ab=p(d_ab), counts=p(counts), loss_reg=p(loss_reg))
        a.update(kw)
        return lib.fastnerf_expo_grad(a['n'], a['n_img'], a['img'], a['ab'], a['lam'], a['gs'], a['e1'], a['e0'], a['g1'], a['g0'], a['ws'],
                                      a['d_ab'], a['counts'], a['loss_reg'], s)
    before = [x.clone() for x in (t['G1'], t['G0'], d_ab, counts, loss_reg)]
    bad_apply = [dict(n=-1), dict(n=2 ** 31), dict(n_img=0), dict(img=None), dict(ab=None), dict(rgb1=None), dict(e1=None), dict(rgb0=None),
                 dict(e0=None)]
    for kw in bad_apply:
        assert apply(**kw) == -1, kw
        assert b'fastnerf_expo_apply' in lib.fastnerf_last_error()
    bad_grad = [dict(n=-1), dict(n=2 ** 31), dict(n_img=0), dict(img=None), dict(ab=None), dict(e1=None), dict(g1=None), dict(e0=None),
                dict(g0=None), dict(ws=None), dict(d_ab=None), dict(counts=None), dict(loss_reg=None), dict(lam=-0.5), dict(lam=float('inf')),
                dict(lam=float('nan'))]
    for kw in bad_grad:
        assert grad(**kw) == -1, kw
        assert b'fastnerf_expo_grad' in lib.fastnerf_last_error()
    assert lib.fastnerf_expo_grad_ws_floats(-1, 3) == -1 and lib.fastnerf_expo_grad_ws_floats(2 ** 31, 3) == -1
    assert lib.fastnerf_expo_grad_ws_floats(5, 0) == -1 and lib.fastnerf_expo_grad_ws_floats(0, 3) == 0
    torch.cuda.synchronize()
    for x, y in zip(before, (t['G1'], t['G0'], d_ab, counts, loss_reg)):
        assert torch.equal(x, y)
    # ops: dtype and shape, before the library is called
    with pytest.raises(TypeError, match='int32'):
        fn.ops.expo_apply(t['rgb1'], img.long(), ab)
    with pytest.raises(ValueError, match='img'):
        fn.ops.expo_apply(t['rgb1'], img[:-1].contiguous(), ab)
    with pytest.raises(TypeError, match='float32'):
        fn.ops.expo_apply(t['rgb1'].double(), img, ab)
    with pytest.raises(ValueError, match='ab'):
        fn.ops.expo_apply(t['rgb1'], img, ab.reshape(-1))
    with pytest.raises(ValueError, match='go together'):
        fn.ops.expo_grad(img, ab, 1.0, 1.0, e1, t['G1'], e0=e0)
    with pytest.raises(ValueError, match='lam'):
        fn.ops.expo_grad(img, ab, -1.0, 1.0, e1, t['G1'])
    with pytest.raises(ValueError, match='integer'):
        fn.exposure.apply(t['rgb1'], img.float(), ab)
    with pytest.raises(ValueError, match='at least one'):
        fn.exposure.ExposureTable(0)
    assert ctypes.sizeof(fn._lib.StepExpo) == lib.fastnerf_step_expo_size()
