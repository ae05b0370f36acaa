"""Coarse-to-fine positional encoding: a weight per frequency band, ramped from low to high frequency while training (host code only;
the kernels are csrc/bands.hip; include/fastnerf.h, "band weights"; DESIGN.md, "Band weights").

With the full encoding the high-frequency bands hand a camera pose a gradient that is noise as soon as the misalignment exceeds their
period (BARF); Nerfies ramps the same weights for its deformation code, FreeNeRF to make a handful of views train.  The weighted encoding
gamma_w(x) = w (.) gamma(x) needs no kernel of its own: W (w (.) gamma) = (W diag(w)) gamma, so the networks' kernels run on an effective
network whose encoding columns are the parameters' times w (NeRF.set_bands), and the parameters' gradient is that network's times w.

    sched = BandSchedule('cosine', start=0, end=20000)
    trainer = Trainer(kw, H, W, K, near, far, bands=sched)      # every step route; from step `end` on the plain trainer, launch for launch

    w_pos, w_view = sched.weights(step)                        # or by hand, with any torch network on the closure route:
    x = weight_encoding(embed_fn(pts), w_pos)

The encodings are the reference's (run_nerf_helpers.py get_embedder): the identity columns first, then per band k = 0 .. L-1 the columns
sin(2^k x), cos(2^k x), d each, for a d-dimensional input: band k covers columns d + 2 d k .. d + 2 d k + 2 d - 1 (3 + 6 k .. 3 + 6 k + 5 for
points and directions).  Identity columns always weigh 1."""
import math

import torch

POS_BANDS, VIEW_BANDS = 10, 4      # multires, multires_views: the encodings the kernels implement
WINDOWS = ('cosine', 'linear')


def _geometry(kind):
    """(input dimension d, bands L) of an encoding: the point encoding of a net of layout `kind` (0 NeRF, 1 nerf++ foreground: 63 columns;
    2 nerf++ background, a 4-D point: 84 columns), or 'view': the direction encoding, 27 columns."""
    if kind == 'view':
        return 3, VIEW_BANDS
    if kind in (0, 1):
        return 3, POS_BANDS
    if kind == 2:
        return 4, POS_BANDS
    raise ValueError("bands: kind is 0, 1, 2 or 'view', not {!r}".format(kind))


def columns(kind):
    """Columns of the encoding `kind` (_geometry): 63, 84 or 27."""
    d, L = _geometry(kind)
    return d + 2 * d * L


def column_weights(kind, per_band):
    """A weight per band [L] -> a weight per column of the encoding `kind` (fp32 host tensor [63], [84] or [27]): 1 on the identity
    columns, per_band[k] on the 2 d columns of band k."""
    d, L = _geometry(kind)
    pb = torch.as_tensor(per_band, dtype=torch.float32).reshape(-1).cpu()
    if pb.numel() != L:
        raise ValueError('bands: the encoding {!r} has {} bands, got {} weights'.format(kind, L, pb.numel()))
    return torch.cat([torch.ones(d, dtype=torch.float32), pb.repeat_interleave(2 * d)])


def weight_encoding(embedded, w):
    """w (.) gamma: an embedded input [..., C] times the column weights w [C], in plain torch (any device, any dtype, differentiable)."""
    w = torch.as_tensor(w)
    if embedded.shape[-1] != w.shape[-1]:
        raise ValueError('bands: {} columns, {} weights'.format(embedded.shape[-1], w.shape[-1]))
    return embedded * w.to(device=embedded.device, dtype=embedded.dtype)


def window(name, t):
    """The ramp of one band over t in [0, 1]: 'cosine' (1 - cos(pi t)) / 2 (BARF, Nerfies), 'linear' t.  Exactly 0 at 0 and 1 at 1."""
    t = min(max(float(t), 0.), 1.)
    if t <= 0. or t >= 1. or name == 'linear':
        return t
    return (1. - math.cos(math.pi * t)) / 2.


def check_weights(w_pos, w_view, kind=0):
    """Fixed column weights as fp32 host tensors ([63] or [84], [27]); ValueError unless they have those lengths and are finite and in
    [0, 1]."""
    out = []
    for name, w, n in (('w_pos', w_pos, columns(kind)), ('w_view', w_view, columns('view'))):
        w = torch.as_tensor(w).detach().to(device='cpu', dtype=torch.float32).reshape(-1).contiguous()
        if w.numel() != n:
            raise ValueError('bands: {} holds {} weights, the encoding has {} columns'.format(name, w.numel(), n))
        if not bool(torch.isfinite(w).all()) or bool((w < 0).any()) or bool((w > 1).any()):
            raise ValueError('bands: {} must be finite and in [0, 1]'.format(name))
        out.append(w)
    return tuple(out)


class BandSchedule:
    """The band weights of every training step.  Band k of an encoding with L bands weighs win(clamp(alpha - k, 0, 1)) at `step`, with
    alpha = L clamp((step - start) / (end - start), 0, 1): every band at 0 up to `start`, the bands opening one after the other from the
    lowest frequency on, every weight exactly 1.0 from `end` on.  window: 'cosine' or 'linear' (window()).  view=False leaves the
    direction encoding at 1 throughout.  Both encodings of a net span the same steps.  BandSchedule.constant(w_pos, w_view): fixed column
    weights instead."""

    def __init__(self, window='cosine', start=0, end=0, view=True):
        if window not in WINDOWS:
            raise ValueError('BandSchedule: window is one of {}, not {!r}'.format(WINDOWS, window))
        start, end = float(start), float(end)
        if not (math.isfinite(start) and math.isfinite(end)) or end < start:
            raise ValueError('BandSchedule: start <= end, both finite, got {!r}, {!r}'.format(start, end))
        self.window, self.start, self.end, self.view = window, start, end, bool(view)
        self._fixed = None

    @classmethod
    def constant(cls, w_pos, w_view):
        s = cls()
        s.window, s._fixed = 'constant', check_weights(w_pos, w_view)
        return s

    def progress(self, step):
        """clamp((step - start) / (end - start), 0, 1); a ramp of no length is open from `end` on."""
        if step >= self.end:
            return 1.
        if step <= self.start:
            return 0.
        return (float(step) - self.start) / (self.end - self.start)

    def per_band(self, step, L):
        alpha = L * self.progress(step)
        return [window(self.window, alpha - k) for k in range(L)]

    def weights(self, step):
        """(w_pos [63], w_view [27]) at `step`, fp32 host tensors."""
        if self._fixed is not None:
            return self._fixed[0].clone(), self._fixed[1].clone()
        w_pos = column_weights(0, self.per_band(step, POS_BANDS))
        w_view = column_weights('view', self.per_band(step, VIEW_BANDS) if self.view else [1.] * VIEW_BANDS)
        return w_pos, w_view

    def done(self, step):
        """Whether every weight is exactly 1.0 at `step` (and, the ramp being monotone, from then on)."""
        return all(bool((w == 1.).all()) for w in self.weights(step))

    def settings(self):
        """What a checkpoint carries under 'band_schedule'."""
        return {'window': self.window, 'start': self.start, 'end': self.end, 'view': self.view}

    @classmethod
    def from_settings(cls, settings, weights=None):
        """The schedule of settings(); a constant one needs the weights a checkpoint carries beside them."""
        if settings['window'] == 'constant':
            if weights is None:
                raise ValueError('BandSchedule: a constant schedule is made from its weights')
            return cls.constant(*weights)
        return cls(settings['window'], settings['start'], settings['end'], settings['view'])
