"""The references of the exposure table against each other (tests/expo_ref.py); no GPU.

(i)   the numpy-float32 restatement agrees with the float64 autograd reference within the bound the GPU test applies to the kernel,
      |d_ab - ref64| <= (6 m_i + 32) 2^-24 B_i, and its e and g within 2 and 1 roundings;
(ii)  the exact integer case: the restatement reproduces the int64 sums exactly, and float64 autograd agrees;
(iii) with the identity table e has the bits of rgb and g those of G;
(iv)  the sign conventions at a = 0, scale = 1 and shift = 0 are torch's (torch.abs differentiates to 0 at 0);
(v)   the keys of NerfNetWithAutoExpo's per-image parameters follow the reference's rule."""
import numpy as np
import pytest
import torch

import expo_ref as E

SHAPES = [(1, 1), (67, 3), (257, 5), (4099, 100)]


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


@pytest.mark.parametrize('two', [False, True], ids=['one_pass', 'two_passes'])
@pytest.mark.parametrize('n,n_img', SHAPES)
def test_restatement_within_the_bound(n, n_img, two):
    c = E.float_case(n, n_img, two, seed=n + n_img, empty=3 if n_img == 5 else None)
    e1 = E.restate_apply(c['img'].numpy(), c['ab'].numpy(), c['rgb1'].numpy())
    e0 = E.restate_apply(c['img'].numpy(), c['ab'].numpy(), c['rgb0'].numpy()) if two else None
    lam, gs = 0.7, 0.5
    got = E.restate_grad(c['img'].numpy(), c['ab'].numpy(), lam, gs, e1, c['G1'].numpy(), e0, c['G0'].numpy() if two else None)
    t = lambda x: None if x is None else torch.from_numpy(np.asarray(x))      # noqa: E731
    ref = E.ref64(c['img'], c['ab'], lam, gs, t(e1), c['G1'], t(e0), c['G0'])
    assert np.array_equal(got['counts'], ref['counts'].numpy())
    m = ref['counts'].double()[:, None]
    err = (torch.from_numpy(got['d_ab']).double() - ref['d_ab']).abs()
    cap = E.bound_factor(m) * ref['B']
    assert (err <= cap).all(), (err / cap.clamp_min(1e-300)).max()
    assert abs(float(got['loss_reg']) - float(ref['loss_reg'])) <= (n_img + 8) * E.U * float(ref['loss_reg']) + 1e-300
    assert (np.abs(got['g1'].astype(np.float64) - ref['g1'].numpy()) <= 2 * E.U * np.abs(ref['g1'].numpy())).all()
    # e against the formula in float64 on the same fp32 inputs: fsub and the division, on a difference of magnitudes <= |rgb| + |shift|
    ok = E.in_range(c['img'].numpy(), n_img)
    idx = np.clip(c['img'].numpy(), 0, n_img - 1)
    ab64 = c['ab'].double().numpy()
    sc, sh = np.abs(ab64[:, 0]) + 0.5, ab64[:, 1]
    rgb = c['rgb1'].double().numpy()
    want = np.where(ok[:, None], (rgb - sh[idx][:, None]) / sc[idx][:, None], rgb)
    cap_e = 3 * E.U * (np.abs(rgb) + np.abs(sh[idx][:, None])) / sc[idx][:, None]
    assert (np.abs(e1.astype(np.float64) - want) <= cap_e).all()
    assert np.array_equal(bits(e1[~ok]), bits(c['rgb1'].numpy()[~ok])) and np.array_equal(bits(got['g1'][~ok]), bits(c['G1'].numpy()[~ok]))


@pytest.mark.parametrize('two', [False, True], ids=['one_pass', 'two_passes'])
@pytest.mark.parametrize('n,n_img', SHAPES)
def test_exact_case_is_self_consistent(n, n_img, two):
    c, want, counts = E.exact_case(n, n_img, two, seed=3 * n + n_img, empty=3 if n_img == 5 else None)
    img, ab = c['img'].numpy(), c['ab'].numpy()
    e1 = E.restate_apply(img, ab, c['rgb1'].numpy())
    e0 = E.restate_apply(img, ab, c['rgb0'].numpy()) if two else None
    assert (e1 * 2 == np.round(e1 * 2)).all() and np.abs(e1).max() <= 12
    got = E.restate_grad(img, ab, 0.0, 1.0, e1, c['G1'].numpy(), e0, c['G0'].numpy() if two else None)
    assert np.array_equal(got['d_ab'].astype(np.float64), want.numpy())
    assert np.array_equal(got['counts'], counts.numpy())
    assert (got['g1'] == np.round(got['g1'])).all() and np.abs(got['g1']).max() <= 2
    t = lambda x: None if x is None else torch.from_numpy(x)      # noqa: E731
    ref = E.ref64(c['img'], c['ab'], 0.0, 1.0, t(e1), c['G1'], t(e0), c['G0'])
    assert torch.allclose(ref['d_ab'], want, rtol=0, atol=1e-9)
    if n_img == 5:
        assert counts[3] == 0 and (want[3] == 0).all()


def test_identity_table_keeps_the_bits():
    c = E.float_case(257, 3, True, seed=9)
    ab = np.tile(np.array([[0.5, 0.0]], np.float32), (3, 1))
    rgb = c['rgb1'].numpy().copy()
    rgb[0, 0], rgb[1, 1] = -0.0, 0.0
    e = E.restate_apply(c['img'].numpy(), ab, rgb)
    assert np.array_equal(bits(e), bits(rgb))
    got = E.restate_grad(c['img'].numpy(), ab, 1.0, 1.0, e, c['G1'].numpy())
    assert np.array_equal(bits(got['g1']), bits(c['G1'].numpy()))
    # scale = 1 and shift = 0: the penalty has no slope, d_ab[:, 1] = -sum g
    ok = E.in_range(c['img'].numpy(), 3)
    for i in range(3):
        rows = ok & (c['img'].numpy() == i)
        assert abs(float(got['d_ab'][i, 1]) + c['G1'].numpy()[rows].astype(np.float64).sum()) <= E.bound_factor(rows.sum()) * np.abs(c['G1'].numpy()[rows]).sum()
    assert float(got['loss_reg']) == 0.0


def test_sign_conventions_are_torchs():
    """Rows at the kinks: a = 0 (|a| has slope 0 there: the whole first column is 0), scale = 1 from both sides of a, shift = 0."""
    ab = torch.tensor([[0.0, 0.3], [0.5, 0.0], [-0.5, -0.2], [1.0, 0.0], [-1.25, 0.1], [0.25, -0.1]])
    n = 60
    gen = torch.Generator().manual_seed(2)
    img = (torch.arange(n) % 6).int()
    e, G = torch.rand(n, 3, generator=gen), torch.randn(n, 3, generator=gen)
    lam, gs = 2.0, 0.25
    ref = E.ref64(img, ab, lam, gs, e, G)
    got = E.restate_grad(img.numpy(), ab.numpy(), lam, gs, e.numpy(), G.numpy())
    err = (torch.from_numpy(got['d_ab']).double() - ref['d_ab']).abs()
    assert (err <= E.bound_factor(10.0) * ref['B']).all()
    pen = lam * gs * 10 / n
    sums = torch.zeros(6, 2, dtype=torch.float64)
    g = G.double() / (ab[:, 0].abs().double() + 0.5)[img.long()][:, None]
    sums[:, 1].index_add_(0, img.long(), -g.sum(-1))
    sums[:, 0].index_add_(0, img.long(), -(g * e.double()).sum(-1))
    d = ref['d_ab']
    assert d[0, 0] == 0                                              # a = 0
    assert abs(d[1, 0] - sums[1, 0]) < 1e-12 and abs(d[1, 1] - sums[1, 1]) < 1e-12      # scale = 1, shift = 0: no pull
    assert abs(d[2, 0] + sums[2, 0]) < 1e-12 and abs(d[2, 1] - (sums[2, 1] - pen)) < 1e-12      # a < 0 flips the scale's gradient
    assert abs(d[3, 0] - (sums[3, 0] + pen)) < 1e-12                 # scale > 1
    assert abs(d[4, 0] + (sums[4, 0] + pen)) < 1e-12                 # a < 0, scale > 1
    assert abs(d[5, 0] - (sums[5, 0] - pen)) < 1e-12 and abs(d[5, 1] - (sums[5, 1] - pen)) < 1e-12      # scale < 1, shift < 0


def test_autoexpo_parameter_names():
    """The key of an image in NerfNetWithAutoExpo.autoexpo_params, by the reference's rule (ddp_model.py:146-154): dots become '-' (a
    parameter's name may hold none), one trailing '/' goes, the last three components of the path stay."""
    import fastnerf
    key = fastnerf.nerfpp._short_name
    for path, want in (('/data/scene/train/rgb/0001.png', 'train/rgb/0001-png'), ('a.b/c.d', 'a-b/c-d'), ('x.png', 'x-png'),
                       ('/b/c.jpg', '/b/c-jpg'), ('a/b/c/d/', 'b/c/d'), ('./x/y/z/w.png', 'y/z/w-png'), ('a/b/', 'a/b')):
        assert key(path) == want, path
        torch.nn.ParameterDict({key(path): torch.nn.Parameter(torch.zeros(2))})      # a name torch accepts
