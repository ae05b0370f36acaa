"""The depth / opacity losses of fastnerf_aux_loss (include/fastnerf.h, csrc/train.hip) restated in torch, in any dtype:

    L    = 1/n sum_r w_r (map[r] - target[r])^2          (unscaled by lambda)
    g[r] = grad_scale lambda 2 w_r (map[r] - target[r]) / n

for the depth and the opacity map of the image pass (1) and of the coarse pass (0).  A ray whose weight is 0 is SELECTED out: it
contributes exactly 0 and gets a gradient of +0 whatever its target holds (NaN marks "unknown" in sparse depth).  Weights None =
ones; a target None switches its term off (losses 0, gradients None).  lambda and grad_scale are fp32 values at the C ABI: the
restatement rounds them to fp32 first, whatever dtype it then computes in."""
import numpy as np
import torch


def f32(x):
    return float(np.float32(x))


def term(x, target, weight, lam, grad_scale, dtype=torch.float64):
    """One map against its target -> (loss, gradient [n]) in `dtype`; differentiable w.r.t. x (for autograd checks)."""
    x = x.to(dtype)
    n = x.numel()
    w = torch.ones(n, dtype=dtype) if weight is None else weight.to(dtype).reshape(-1)
    on = w != 0
    d = torch.where(on, x.reshape(-1) - torch.where(on, target.to(dtype).reshape(-1), torch.zeros((), dtype=dtype)),
                    torch.zeros((), dtype=dtype))
    loss = (torch.where(on, w, torch.zeros((), dtype=dtype)) * d * d).sum() / n
    coef = f32(grad_scale) * f32(lam) * 2.0 / n
    grad = torch.where(on, coef * w * d.detach(), torch.zeros((), dtype=dtype))
    return loss, grad


def aux_loss(depth1, acc1, depth0=None, acc0=None, depth_target=None, depth_weight=None, acc_target=None, acc_weight=None,
             lambda_depth=0., lambda_acc=0., grad_scale=1., dtype=torch.float64):
    """-> (loss4 = (Ld_1, Ld_0, La_1, La_0), {g_depth1, g_acc1, g_depth0, g_acc0}) with the conventions of ops.aux_loss."""
    loss4 = [torch.zeros((), dtype=dtype) for _ in range(4)]
    g = {'g_depth1': None, 'g_acc1': None, 'g_depth0': None, 'g_acc0': None}
    for slot, name, x, tgt, w, lam in ((0, 'g_depth1', depth1, depth_target, depth_weight, lambda_depth),
                                        (1, 'g_depth0', depth0, depth_target, depth_weight, lambda_depth),
                                        (2, 'g_acc1', acc1, acc_target, acc_weight, lambda_acc),
                                        (3, 'g_acc0', acc0, acc_target, acc_weight, lambda_acc)):
        if tgt is not None and x is not None:
            loss4[slot], g[name] = term(x, tgt, w, lam, grad_scale, dtype)
    return torch.stack(loss4), g


def total(loss2, loss4, lambda_depth, lambda_acc):
    """The loss the step minimises: mse(fine) + mse(coarse) + lambda_depth (Ld_1 + Ld_0) + lambda_acc (La_1 + La_0)."""
    return loss2.sum() + f32(lambda_depth) * (loss4[0] + loss4[1]) + f32(lambda_acc) * (loss4[2] + loss4[3])
