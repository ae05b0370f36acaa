"""A learned environment map: a trained background behind every ray (csrc/envmap.hip; include/fastnerf.h, "environment map").

A capture with a sky or a wall behind the subject has a colour in every pixel that looks past the box; a field that can only explain it
with density answers with fog on the box faces and floaters.  The map is a small table of colours indexed by ray direction alone
(octahedral, bilinear, mirror-wrapped: no seam), composited behind the volume and trained beside the field:

    env = EnvMap(res=64)
    out = render_rays(rays, **kw)
    rgb = out['rgb_map'] + (1 - out['acc_map'])[:, None] * env(rays[:, 3:6])      # the same for rgb0 / acc0
    loss.backward(); optimizer.step()                                             # over the networks and env.table

The direction is always columns 3:6 of the ray batch, the unnormalised d: the lookup normalises by the 1-norm itself, so training and
rendering index the table with the same bits, and [N,8] batches work.  render_rays(..., envmap=env) is the loop's second line;
Trainer(envmap=env) is the same without autograd, on every step route."""
import torch

from . import ops


class _EnvFn(torch.autograd.Function):
    """colours = ops.env_lookup(table, dirs); backward: ops.env_grad with acc = 0.  The directions get no gradient."""

    @staticmethod
    def forward(ctx, table, dirs):
        t = table.detach().contiguous()
        ctx.save_for_backward(dirs)
        ctx.res = t.shape[0]
        return ops.env_lookup(t, dirs)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:      # a frozen map: nothing to scatter
            return None, None
        dirs, = ctx.saved_tensors
        g = g.contiguous().float()
        return ops.env_grad(ctx.res, dirs, g, torch.zeros(g.shape[0], device=g.device, dtype=torch.float32)), None


def _dirs(dirs):
    """Directions as the kernels read them: fp32 rows of three, a column view of a ray batch left in place."""
    ops.require_gpu(dirs)
    d = dirs.detach()
    if d.dtype != torch.float32:
        d = d.float()
    if d.dim() != 2 or d.shape[1] != 3:
        raise ValueError('env: directions [n,3] (columns 3:6 of a ray batch), got {}'.format(tuple(d.shape)))
    if d.shape[0] > 1 and (d.stride(1) != 1 or d.stride(0) < 3):
        d = d.contiguous()
    return d


def env(table, dirs):
    """The map's colours [n,3] for directions dirs [n,3] of any length: an autograd function of the table (an EnvMap, or its `table`
    [R,R,3]).  The gradient with respect to `dirs` is None: a direction's colour is a constant of the ray (a background that helps pose
    refinement is out of scope)."""
    t = table.table if isinstance(table, EnvMap) else table
    return _EnvFn.apply(t, _dirs(dirs))


class EnvMap(torch.nn.Module):
    """The table: parameter `table` [res,res,3] (row = y, column = x of the octahedral square), filled with `colour` at first.
    env(dirs [n,3]) -> colours [n,3], differentiable with respect to the table; the gradient with respect to dirs is None."""

    def __init__(self, res=64, colour=(0.5, 0.5, 0.5)):
        super().__init__()
        res = int(res)
        if res < 2:
            raise ValueError('EnvMap: a table of R >= 2 texels a side, got {}'.format(res))
        c = torch.as_tensor(colour, dtype=torch.float32).reshape(-1)
        if c.numel() != 3:
            raise ValueError('EnvMap: colour is 3 floats, got {!r}'.format(colour))
        self.table = torch.nn.Parameter(c.repeat(res, res, 1).contiguous())

    @property
    def res(self):
        return self.table.shape[0]

    def forward(self, dirs):
        return env(self, dirs)

    def save(self, path):
        """The table alone (a checkpoint of run_nerf.save_checkpoint holds it with its moments)."""
        torch.save({'env_table': self.table.data.cpu()}, path)

    @classmethod
    def load(cls, path, device='cuda'):
        """The map of `save` (or of a checkpoint that holds `env_table`)."""
        d = torch.load(path, map_location='cpu', weights_only=False)
        t = d['env_table']
        if t.dim() != 3 or t.shape[0] != t.shape[1] or t.shape[2] != 3:
            raise ValueError('EnvMap.load: no [R,R,3] table in {}: {}'.format(path, tuple(t.shape)))
        m = cls(res=t.shape[0])
        m.table.data.copy_(t)
        return m.to(device)
