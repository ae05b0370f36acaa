"""A numpy restatement of the band weights (fastnerf/bands.py, csrc/bands.hip), written from the definitions alone:

  * the column map: which floats of a flat net of layout `kind` carry a column of the positional encodings -- rows of layer 0, the first
    in_pe columns of the rows of the skip layer, columns 256:283 of the rows of the view layer -- from the parameters() order itself
    (kind 0: model.SHAPES; kinds 1 / 2: trunk, sigma head, remap layer, view layer, rgb head, nerf_network.py:70-142; kind 2 has an
    84-column point encoding, a 4-D point);
  * apply and grad in float32: one multiply in the regions, nothing anywhere else;
  * the two windows and the schedule."""
import math

import numpy as np

F32 = np.float32
VIEW_COLS = 27


def in_pe(kind):
    return 84 if kind == 2 else 63


def net_shapes(kind):
    """[(out, in)] of the linear layers of a net of layout `kind` in parameters() order (weight then bias each)."""
    pe = in_pe(kind)
    trunk = [(256, pe if i == 0 else (256 + pe if i == 5 else 256)) for i in range(8)]
    view, feat, alpha, rgb = (128, 256 + VIEW_COLS), (256, 256), (1, 256), (3, 128)
    return trunk + ([view, feat, alpha, rgb] if kind == 0 else [alpha, feat, view, rgb])


def n_params(kind):
    return sum(o * i + o for o, i in net_shapes(kind))


def column_map(kind):
    """(index [n_params] int64, which [n_params] int8): which = 0 where a float carries no encoding column, 1 where it is column
    index[e] of the point encoding, 2 where it is column index[e] of the direction encoding."""
    pe = in_pe(kind)
    shapes = net_shapes(kind)
    view_layer = 8 if kind == 0 else 10
    index = np.zeros(n_params(kind), np.int64)
    which = np.zeros(n_params(kind), np.int8)
    off = 0
    for layer, (o, i) in enumerate(shapes):
        cols = np.tile(np.arange(i), o)
        w = np.zeros(o * i, np.int8)
        if layer in (0, 5):
            w[cols < pe] = 1
        elif layer == view_layer:
            w[cols >= 256] = 2
            cols = np.where(cols >= 256, cols - 256, cols)
        index[off:off + o * i] = np.where(w > 0, cols, 0)
        which[off:off + o * i] = w
        off += o * i + o
    assert off == n_params(kind)
    return index, which


def scale32(kind, w_pos, w_view, buf):
    """buf with the floats of the three regions times their column's weight (one float32 multiply), every other float as it is, bit for
    bit: what band_apply writes from a master and what band_grad leaves of a gradient."""
    buf = np.asarray(buf, F32)
    w_pos, w_view = np.asarray(w_pos, F32), np.asarray(w_view, F32)
    assert w_pos.shape == (in_pe(kind),) and w_view.shape == (VIEW_COLS,) and buf.shape == (n_params(kind),)
    index, which = column_map(kind)
    out = buf.copy()
    p, v = which == 1, which == 2
    out[p] = buf[p] * w_pos[index[p]]
    out[v] = buf[v] * w_view[index[v]]
    assert out.dtype == F32
    return out


apply32 = grad32 = scale32


def window(name, t):
    t = min(max(float(t), 0.0), 1.0)
    if name == 'linear':
        return t
    assert name == 'cosine'
    return 0.0 if t == 0.0 else (1.0 if t == 1.0 else (1.0 - math.cos(math.pi * t)) / 2.0)


def columns_from_bands(per_band, d=3):
    """[L] -> [d + 2 d L]: ones on the identity columns, per_band[k] on columns d + 2 d k .. d + 2 d k + 2 d - 1."""
    out = np.ones(d + 2 * d * len(per_band), F32)
    for k, w in enumerate(per_band):
        out[d + 2 * d * k:d + 2 * d * (k + 1)] = F32(w)
    return out


def schedule(name, start, end, step, view=True):
    """(w_pos [63], w_view [27]) float32 at `step`: band k of L weighs win(clamp(alpha - k, 0, 1)), alpha = L clamp((step - start) /
    (end - start), 0, 1)."""
    if step >= end:
        t = 1.0
    elif step <= start:
        t = 0.0
    else:
        t = (float(step) - float(start)) / (float(end) - float(start))
    out = []
    for L, on in ((10, True), (4, view)):
        out.append(columns_from_bands([window(name, L * t - k) if on else 1.0 for k in range(L)]))
    return out[0], out[1]


def random_weights(kind, seed):
    """Column weights in [0, 1] with exact zeros and ones among them (identity columns included: the kernels take any weights)."""
    rs = np.random.RandomState(seed)
    out = []
    for n in (in_pe(kind), VIEW_COLS):
        w = rs.rand(n).astype(F32)
        w[rs.rand(n) < 0.2] = 0.0
        w[rs.rand(n) < 0.2] = 1.0
        w[0], w[n - 1] = 0.0, 1.0
        out.append(w)
    return out[0], out[1]
