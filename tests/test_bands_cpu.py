"""Band weights without a GPU: the restatement (tests/bands_ref.py) against the layouts, the schedule (fastnerf/bands.py) against the
restatement, and the identity the design rests on.

(i)   the column map marks exactly LW[0][:, :in_pe], LW[5][:, :in_pe] and VW[:, 256:283] of model.SHAPES (kind 0) and has the library's
      size and the 84-column geometry for kind 2; apply32 multiplies there and nowhere else;
(ii)  BandSchedule: all-zero bands up to `start`, every weight exactly 1.0 from `end` on, monotone in the step and in the band, identity
      columns always 1, view=False, the bits of the restatement; constant() refuses weights that are none; done();
(iii) a tiny float64 network fed an explicitly weighted encoding: the autograd gradient of its master columns equals the gradient of the
      scaled network (columns times w as its own leaves) times w, to 1e-12 -- and a column at w = 0 has gradient exactly 0;
(iv)  the C entry points refuse a kind outside 0..2, NULL pointers and master == effective before any launch (no GPU is touched)."""
import numpy as np
import pytest
import torch

import bands_ref as B
import fastnerf
from fastnerf import _lib, bands, model, ops


def test_column_map_against_the_layouts():
    index, which = B.column_map(0)
    assert B.n_params(0) == ops.NET_PARAMS == which.size
    expect = np.zeros(ops.NET_PARAMS, np.int8)
    cols = np.zeros(ops.NET_PARAMS, np.int64)
    for name, off, shape in model.param_slices():
        if name in ('pts_linears.0.weight', 'pts_linears.5.weight'):
            v = expect[off:off + shape[0] * shape[1]].reshape(shape)
            v[:, :63] = 1
            cols[off:off + shape[0] * shape[1]].reshape(shape)[:, :63] = np.arange(63)
        elif name == 'views_linears.0.weight':
            assert shape == (128, 283)
            expect[off:off + 128 * 283].reshape(shape)[:, 256:] = 2
            cols[off:off + 128 * 283].reshape(shape)[:, 256:] = np.arange(27)
    assert np.array_equal(which, expect) and np.array_equal(index, cols)
    assert int((which == 1).sum()) == 2 * 256 * 63 and int((which == 2).sum()) == 128 * 27
    for kind in (1, 2):
        i2, w2 = B.column_map(kind)
        assert B.n_params(kind) == ops.net_floats(kind, 0)
        pe = B.in_pe(kind)
        assert int((w2 == 1).sum()) == 2 * 256 * pe and int((w2 == 2).sum()) == 128 * 27
        assert int(i2[w2 == 1].max()) == pe - 1 and int(i2[w2 == 2].max()) == 26
    # the 84 columns of kind 2: a 4-D point, 4 identity columns and 10 bands of 8
    assert B.in_pe(2) == 84 == bands.columns(2) == 4 + 8 * 10 and bands.columns(0) == 63 and bands.columns('view') == 27
    w = bands.column_weights(2, np.arange(10) / 10.).numpy()
    assert np.array_equal(w, B.columns_from_bands(np.arange(10) / 10., d=4)) and (w[:4] == 1).all() and (w[4:12] == 0).all()
    with pytest.raises(ValueError):
        bands.column_weights(0, [1.] * 4)
    with pytest.raises(ValueError):
        bands.column_weights(3, [1.] * 10)


@pytest.mark.parametrize('kind', [0, 2])
def test_apply_restatement(kind):
    rs = np.random.RandomState(kind)
    buf = rs.randn(B.n_params(kind)).astype(np.float32)
    w_pos, w_view = B.random_weights(kind, 5 + kind)
    out = B.apply32(kind, w_pos, w_view, buf)
    index, which = B.column_map(kind)
    assert np.array_equal(out[which == 0].view(np.uint32), buf[which == 0].view(np.uint32))
    ones = B.apply32(kind, np.ones_like(w_pos), np.ones_like(w_view), buf)
    assert np.array_equal(ones.view(np.uint32), buf.view(np.uint32))
    zeros = B.apply32(kind, np.zeros_like(w_pos), np.zeros_like(w_view), buf)
    assert not zeros[which > 0].any() and np.array_equal(zeros[which == 0], buf[which == 0])
    # a row of layer 0 is the row times w_pos, a row of the view layer's tail the tail times w_view
    pe = B.in_pe(kind)
    assert np.array_equal(out[:pe], buf[:pe] * w_pos) and np.array_equal(out[7 * pe:8 * pe], buf[7 * pe:8 * pe] * w_pos)


@pytest.mark.parametrize('name', ['cosine', 'linear'])
def test_schedule(name):
    s = bands.BandSchedule(name, start=10, end=50)
    prev = None
    for step in list(range(0, 60)) + [10 ** 6]:
        wp, wv = s.weights(step)
        assert wp.dtype == torch.float32 and wp.shape == (63,) and wv.shape == (27,) and not wp.is_cuda
        rp, rv = B.schedule(name, 10, 50, step)
        assert np.array_equal(wp.numpy().view(np.uint32), rp.view(np.uint32)) and np.array_equal(wv.numpy().view(np.uint32), rv.view(np.uint32))
        assert (wp[:3] == 1).all() and (wv[:3] == 1).all()
        assert (wp >= 0).all() and (wp <= 1).all()
        for w, L in ((wp, 10), (wv, 4)):
            b = w[3:].reshape(L, 6)
            assert (b == b[:, :1]).all()                       # one weight per band
            assert (b[1:, 0] <= b[:-1, 0]).all()               # monotone in k
        if step <= 10:
            assert not wp[3:].any() and not wv[3:].any() and not s.done(step)
        if step >= 50:
            assert (wp == 1).all() and (wv == 1).all() and s.done(step)
        else:
            assert not s.done(step)
        if prev is not None:
            assert (wp >= prev[0]).all() and (wv >= prev[1]).all()     # monotone in the step
        prev = (wp, wv)
    # mid-ramp: alpha = 10 * 0.25 = 2.5 for the points: bands 0, 1 open, band 2 at win(0.5), the rest closed
    wp, wv = s.weights(20)
    half = 0.5
    assert wp[3 + 6] == 1 and abs(float(wp[3 + 12]) - half) < 1e-7 and wp[3 + 18] == 0
    assert wv[3] == 1 and wv[3 + 6] == 0
    nv = bands.BandSchedule(name, 10, 50, view=False)
    assert (nv.weights(0)[1] == 1).all() and not nv.weights(0)[0][3:].any() and not nv.done(49) and nv.done(50)
    assert bands.BandSchedule(name, 5, 5).done(5) and not bands.BandSchedule(name, 5, 5).done(4)
    assert s.settings() == {'window': name, 'start': 10.0, 'end': 50.0, 'view': True}
    again = bands.BandSchedule.from_settings(s.settings())
    assert all(torch.equal(a, b) for a, b in zip(again.weights(33), s.weights(33)))


def test_schedule_refusals_and_constant():
    with pytest.raises(ValueError):
        bands.BandSchedule('gaussian', 0, 10)
    with pytest.raises(ValueError):
        bands.BandSchedule('cosine', 10, 0)
    wp, wv = torch.rand(63), torch.rand(27)
    c = bands.BandSchedule.constant(wp, wv)
    assert torch.equal(c.weights(0)[0], wp) and torch.equal(c.weights(10 ** 9)[1], wv) and not c.done(10 ** 9)
    assert bands.BandSchedule.constant(torch.ones(63), torch.ones(27)).done(0)
    again = bands.BandSchedule.from_settings(c.settings(), c.weights(0))
    assert torch.equal(again.weights(7)[0], wp)
    for bad in (torch.full((63,), float('nan')), torch.full((63,), 1.5), torch.full((63,), -0.1), torch.full((63,), float('inf')),
                torch.ones(62)):
        with pytest.raises(ValueError):
            bands.BandSchedule.constant(bad, wv)
    with pytest.raises(ValueError):
        bands.BandSchedule.constant(wp, torch.ones(28))
    x = torch.randn(5, 63, dtype=torch.float64)
    assert torch.equal(bands.weight_encoding(x, wp), x * wp.double())
    with pytest.raises(ValueError):
        bands.weight_encoding(x, wv)


def _tiny(seed, C=9, Cv=9, H=8):
    """A float64 network of the reference's structure in small: layer 0 on the encoding, a skip layer on [encoding, h], a feature layer,
    a view layer on [feature, direction encoding], heads."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) * 0.5      # noqa: E731
    return {'W0': r(H, C), 'W1': r(H, H), 'W5': r(H, C + H), 'Wf': r(H, H), 'Wa': r(1, H), 'Wv': r(H // 2, H + Cv), 'Wr': r(3, H // 2)}


def _tiny_forward(p, pe, vpe):
    h = torch.relu(pe @ p['W0'].T)
    h = torch.relu(h @ p['W1'].T)
    h = torch.relu(torch.cat([pe, h], -1) @ p['W5'].T)
    alpha = h @ p['Wa'].T
    hv = torch.relu(torch.cat([h @ p['Wf'].T, vpe], -1) @ p['Wv'].T)
    return torch.cat([hv @ p['Wr'].T, alpha], -1)


def test_scaled_network_identity_float64():
    """(iii)"""
    C = Cv = 9
    H = 8
    g = torch.Generator().manual_seed(1)
    pe, vpe = torch.randn(33, C, generator=g, dtype=torch.float64), torch.randn(33, Cv, generator=g, dtype=torch.float64)
    cot = torch.randn(33, 4, generator=g, dtype=torch.float64)
    w = torch.tensor([1, 1, 1, 0.7, 0.7, 0.7, 0, 0, 0], dtype=torch.float64)
    wv = torch.tensor([1, 1, 1, 0.25, 0.25, 0.25, 0, 0, 0], dtype=torch.float64)
    master = {k: v.clone().requires_grad_(True) for k, v in _tiny(0).items()}
    out_m = _tiny_forward(master, bands.weight_encoding(pe, w), bands.weight_encoding(vpe, wv))
    (out_m * cot).sum().backward()
    # the scaled network: its encoding columns are the master's times w, leaves of their own; fed the plain encoding
    scaled = {k: v.detach().clone() for k, v in master.items()}
    scaled['W0'] = scaled['W0'] * w
    scaled['W5'] = torch.cat([scaled['W5'][:, :C] * w, scaled['W5'][:, C:]], 1)
    scaled['Wv'] = torch.cat([scaled['Wv'][:, :H], scaled['Wv'][:, H:] * wv], 1)
    scaled = {k: v.requires_grad_(True) for k, v in scaled.items()}
    out_s = _tiny_forward(scaled, pe, vpe)
    (out_s * cot).sum().backward()
    assert (out_m - out_s).abs().max() <= 1e-12 * out_s.abs().max()
    for k in master:
        gs = scaled[k].grad.clone()
        if k == 'W0':
            gs = gs * w
        elif k == 'W5':
            gs[:, :C] = gs[:, :C] * w
        elif k == 'Wv':
            gs[:, H:] = gs[:, H:] * wv
        scale = max(float(gs.abs().max()), 1e-300)
        assert float((master[k].grad - gs).abs().max()) <= 1e-12 * scale, k
        assert float(gs.abs().max()) > 0
    assert not master['W0'].grad[:, 6:].any() and not master['W5'].grad[:, 6:C].any() and not master['Wv'].grad[:, H + 6:].any()
    assert scaled['W0'].grad[:, 6:].abs().max() > 0      # (the scaled network's own gradient there is not zero: the factor w makes it so)


def test_entry_points_refuse_before_any_launch():
    """(iv)"""
    lib = _lib.lib()
    buf = (np.zeros(8, np.float32), np.zeros(8, np.float32))
    p = [b.ctypes.data for b in buf]
    err = lambda: lib.fastnerf_last_error().decode()      # noqa: E731
    for kind in (-1, 3):
        assert lib.fastnerf_band_apply(kind, p[0], p[0], p[0], p[1], None) == -1 and 'kind' in err()
        assert lib.fastnerf_band_grad(kind, p[0], p[0], p[1], None) == -1 and 'kind' in err()
    for args in ((None, p[0], p[0], p[1]), (p[0], None, p[0], p[1]), (p[0], p[0], None, p[1]), (p[0], p[0], p[0], None)):
        assert lib.fastnerf_band_apply(0, *args, None) == -1 and 'non-null' in err()
    for args in ((None, p[0], p[1]), (p[0], None, p[1]), (p[0], p[0], None)):
        assert lib.fastnerf_band_grad(2, *args, None) == -1 and 'non-null' in err()
    assert lib.fastnerf_band_apply(0, p[0], p[0], p[1], p[1], None) == -1 and 'two buffers' in err()
    assert err().startswith('fastnerf_band_apply')


def test_ops_refuse_host_tensors():
    wp, wv, net = torch.ones(63), torch.ones(27), torch.zeros(ops.NET_PARAMS)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.band_apply(wp, wv, net)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.band_grad(wp, wv, net)
    with pytest.raises(ValueError, match='kind'):
        ops.band_grad(wp, wv, net, kind=3)
    assert fastnerf.bands is bands
