"""Per-image exposures that training fits beside the field (csrc/exposure.hip; include/fastnerf.h, "exposure table").

Captures drift in exposure and white level from frame to frame; a field fitted to all frames as if they shared one exposure answers
with view-dependent fog.  The table holds a scale and a shift per training image, applied to the predicted colour before the loss, with
an L1 pull towards (1, 0) (the reference's autoexposure, nerf++-ours ddp_model.py:157-188, which its own loop never reaches):

    table = ExposureTable(n_images)                     # rows (0.5, 0): scale = |a| + 0.5 = 1, shift = 0
    out = render_rays(rays, **kw)
    e = apply(out['rgb_map'], img, table)               # (rgb - shift_i) / scale_i, i = img[r]
    loss = img2mse(e, target) + lam * table.penalty(img)
    loss.backward(); optimizer.step()                   # over the networks and table.ab

Trainer(exposure=table) is the same without autograd, on every step route."""
import torch

from . import ops


def check_img(img):
    """The refusals of an image list -> contiguous int32 [n]."""
    ops.require_gpu(img)
    if img.dim() != 1 or img.dtype not in (torch.int32, torch.int64):
        raise ValueError('img: an integer [n] list of image indices, got {} {}'.format(img.dtype, tuple(img.shape)))
    return img.int().contiguous()


class _ApplyFn(torch.autograd.Function):
    """e = ops.expo_apply(rgb, img, ab); backward: ops.expo_grad (no penalty: lam = 0) on a copy of the incoming gradient."""

    @staticmethod
    def forward(ctx, rgb, img, ab):
        e, _ = ops.expo_apply(rgb.detach().contiguous().float(), img, ab.detach().contiguous())
        ctx.save_for_backward(img, ab.detach(), e)
        return e

    @staticmethod
    def backward(ctx, g_e):
        img, ab, e = ctx.saved_tensors
        g = g_e.contiguous().float().clone()      # (expo_grad rescales its gradient in place)
        d_ab, _, _ = ops.expo_grad(img, ab.contiguous(), 0., 1., e, g)
        return g, None, d_ab


def apply(rgb, img, table):
    """The colours rgb [n,3] as image img[r] exposed them: (rgb - shift_i) / scale_i, an autograd function of rgb and of the table
    (an ExposureTable, or its `ab` [n_img,2]).  A ray whose img lies outside the table keeps its colour."""
    ab = table.ab if isinstance(table, ExposureTable) else table
    return _ApplyFn.apply(rgb, check_img(img), ab)


class ExposureTable(torch.nn.Module):
    """One exposure per image: parameter `ab` [n_images,2] = (a, shift), rows (0.5, 0) at first; scale = |a| + 0.5."""

    def __init__(self, n_images):
        super().__init__()
        if int(n_images) < 1:
            raise ValueError('ExposureTable: at least one image, got {}'.format(n_images))
        self.ab = torch.nn.Parameter(torch.tensor([0.5, 0.], dtype=torch.float32).repeat(int(n_images), 1))

    @property
    def n_images(self):
        return self.ab.shape[0]

    def table(self):
        """(scale [n_images], shift [n_images]), differentiable."""
        return torch.abs(self.ab[:, 0]) + 0.5, self.ab[:, 1]

    def penalty(self, img):
        """The batch mean of |scale - 1| + |shift| over the rays' images (the term Trainer weighs with lambda_autoexpo)."""
        scale, shift = self.table()
        return (torch.abs(scale - 1.) + torch.abs(shift))[img.long()].mean()
