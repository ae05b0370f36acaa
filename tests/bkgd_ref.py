"""Host restatement of the per-ray background colours (csrc/bkgd.hip), for tests: the two kernels in numpy float32, operation for
operation (every product and sum rounded on its own, as fmul / fadd / fsub do), the colour draw of the 'bkgd' stream through
tests/philox_numpy.py, and the float64 / float32 torch form of a step with a background on the oracle.  It never calls the library."""
import numpy as np
import torch

import philox_numpy as P

F32 = np.float32
BKGD = 0x626B6764      # 'bkgd'  background colours   counter = ray r (lo, hi)   words 0..2


def draw(n, seed):
    """float32 [n, 3]: (u01(w0), u01(w1), u01(w2)) of Philox block r of the 'bkgd' stream under `seed`."""
    w = P.stream_words(BKGD, np.arange(int(n), dtype=P.U64), seed)
    return np.stack([P.u01(w[0]), P.u01(w[1]), P.u01(w[2])], -1).astype(F32)


def _f(x):
    return None if x is None else np.ascontiguousarray(np.asarray(x, dtype=F32))


def blend(rgb1, acc1, target, bkgd=None, seed=0, alpha=None, rgb0=None, acc0=None):
    """fastnerf_bkgd_blend -> (rgb1', rgb0' or None, target_out, bkgd_used), float32; nothing is changed in place."""
    rgb1, acc1, target, bkgd, alpha, rgb0, acc0 = (_f(x) for x in (rgb1, acc1, target, bkgd, alpha, rgb0, acc0))
    assert (bkgd is not None) != (seed != 0), 'exactly one of bkgd and seed != 0'
    n = rgb1.shape[0]
    b = bkgd if bkgd is not None else draw(n, seed)
    one = F32(1)
    out1 = rgb1 + (one - acc1)[:, None] * b            # numpy float32: each ufunc rounds once
    out0 = None if rgb0 is None else rgb0 + (one - acc0)[:, None] * b
    if alpha is None:
        tout = target.copy()
    else:
        tout = target * alpha[:, None] + (one - alpha)[:, None] * b
    return out1.astype(F32), out0, tout.astype(F32), b.copy()


def grad(bkgd_used, g_rgb1, g_rgb0=None, add1=None, add0=None):
    """fastnerf_bkgd_grad -> (g_acc1, g_acc0 or None), float32."""
    b, g1, g0, add1, add0 = (_f(x) for x in (bkgd_used, g_rgb1, g_rgb0, add1, add0))

    def one(g, add):
        x = (g[:, 0] * b[:, 0] + g[:, 1] * b[:, 1]) + g[:, 2] * b[:, 2]
        return (-x if add is None else add - x).astype(F32)
    return one(g1, add1), (None if g0 is None else one(g0, add0))


def blend_torch(rgb, acc, b, detach_acc=False):
    """rgb + (1 - acc)[:, None] * b in the dtype of the maps; detach_acc: the blend without its way back to the opacity."""
    a = acc.detach() if detach_acc else acc
    return rgb + (1. - a)[:, None] * b.to(rgb.dtype)


def target_torch(target, alpha, b):
    if alpha is None:
        return target
    return target * alpha[:, None] + (1. - alpha)[:, None] * b


def step_loss(O, rb, sd_c, sd_f, Ns, Ni, target, b, alpha=None, t_rand=None, u=None, detach_acc=False):
    """The colour loss of one step with background colours on the oracle `O` (oracle.nerf_oracle), in the dtype of `rb`:
    O.render_rays(..., white_bkgd=False) maps plus (1 - acc)[:, None] * b, the target blended through alpha, O.img2mse of both
    passes.  -> (loss2 [2] = (image pass, coarse pass; the coarse slot is 0 with one pass), the oracle's maps with the blended rgb)."""
    dt = rb.dtype
    ret = O.render_rays(rb, sd_c, sd_f, Ns, Ni, white_bkgd=False, t_rand=None if t_rand is None else t_rand.to(dt),
                        u=None if u is None else u.to(dt))
    b = b.to(dt)
    tgt = target_torch(target.to(dt), None if alpha is None else alpha.to(dt), b)
    ret['rgb_map'] = blend_torch(ret['rgb_map'], ret['acc_map'], b, detach_acc)
    losses = [O.img2mse(ret['rgb_map'], tgt)]
    if Ni > 0:
        ret['rgb0'] = blend_torch(ret['rgb0'], ret['acc0'], b, detach_acc)
        losses.append(O.img2mse(ret['rgb0'], tgt))
    else:
        losses.append(torch.zeros((), dtype=dt))
    return torch.stack(losses), ret
