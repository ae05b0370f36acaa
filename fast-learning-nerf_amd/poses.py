"""Camera poses that training refines (csrc/pose.hip; include/fastnerf.h, "pose table").

A ray batch drawn from many images, every ray belonging to the pose of its image:

    table = PoseTable(base_poses)                       # xi = 0: the poses the data set came with
    rays = pose_rays(pix, table(), K, near, far)        # [n,11], differentiable with respect to the poses
    out = render_rays(rays, **kw)                       # (rays[:, :8] for networks without view directions)
    loss.backward(); optimizer.step()                   # over the networks and table.xi

Parametrisation: per image a 6-vector xi = (omega, tau) beside its fixed base pose (R0 | t0), R = exp(hat(omega)) R0, t = t0 + tau:
the camera turns about its own centre, in world axes, and moves independently.  (tools/refine_pose.py registers ONE view and turns it
about the world origin: the other convention.)  `pose_rays` takes the poses themselves, so a caller may write any other
parametrisation in torch.  Pinhole rays only (ndc=False), as for render(c2w=pose).  Trainer(poses=table) is the same without autograd."""
import torch

from . import ops


class _PoseRaysFn(torch.autograd.Function):
    """rays11 [n,11] = pack_rays(*gen_rays_pixels(pix, poses, K), near, far); backward: ops.pose_grad."""

    @staticmethod
    def forward(ctx, poses, pix, K, near, far):
        ro, rd = ops.gen_rays_pixels(pix, poses.detach(), K)
        ctx.K = K
        ctx.save_for_backward(pix, poses.detach())
        return ops.pack_rays(ro, rd, near, far)

    @staticmethod
    def backward(ctx, d_rays):
        pix, poses = ctx.saved_tensors
        return ops.pose_grad(pix, poses, ctx.K, d_rays.contiguous().float()), None, None, None, None


def check_pix(pix):
    ops.require_gpu(pix)
    if pix.dim() != 2 or pix.shape[1] != 3 or pix.dtype not in (torch.int32, torch.int64):
        raise ValueError('pix: an integer [n, 3] list of (image, row, col), got {} {}'.format(pix.dtype, tuple(pix.shape)))
    return pix.int().contiguous()


def pose_rays(pix, poses, K, near, far):
    """The ray batch [n,11] (o, d, near, far, viewdir) of the pixels pix [n,3] = (image, row, col) under the poses [n_img,3,4]: the
    launches of ops.gen_rays_pixels + ops.pack_rays, bit for bit, as an autograd function of `poses`."""
    pix = check_pix(pix)
    ops.require_gpu(poses)
    ops._need_f32('poses', poses, poses.shape[0], 3, 4)
    return _PoseRaysFn.apply(poses.contiguous(), pix, K, float(near), float(far))


def perturbed(poses, degrees, shift, seed=0):
    """The poses [n,3,4] with every camera turned about its own centre by `degrees` about a random axis and moved by `shift` in a
    random direction (float64 on the host, rounded once): noisy poses with a known truth, for studies and tests."""
    gen = torch.Generator().manual_seed(seed)
    p = poses.detach().cpu().double()
    axis = torch.randn(p.shape[0], 3, generator=gen, dtype=torch.float64)
    axis = axis / axis.norm(dim=-1, keepdim=True) * (degrees * torch.pi / 180.0)
    z = torch.zeros_like(axis[:, 0])
    K = torch.stack([torch.stack([z, -axis[:, 2], axis[:, 1]], -1), torch.stack([axis[:, 2], z, -axis[:, 0]], -1),
                     torch.stack([-axis[:, 1], axis[:, 0], z], -1)], -2)
    move = torch.randn(p.shape[0], 3, generator=gen, dtype=torch.float64)
    move = move / move.norm(dim=-1, keepdim=True) * shift
    return torch.cat([torch.matrix_exp(K) @ p[:, :, :3], p[:, :, 3:] + move[..., None]], -1).float().to(poses.device)


def gauge_free_errors(poses, truth):
    """(rotation error in degrees, translation error) of poses [n,3,4] against the true ones that no rigid motion of the whole set
    changes: the mean over image pairs of the angle between the relative rotations R_i^T R_j and their true values, and of the
    difference between the pair distances |t_i - t_j| and theirs."""
    p, q = poses.detach().cpu().double(), truth.detach().cpu().double()
    n = p.shape[0]
    i, j = torch.triu_indices(n, n, 1)
    rel = lambda x: x[i, :, :3].transpose(1, 2) @ x[j, :, :3]      # noqa: E731
    d = rel(p).transpose(1, 2) @ rel(q)
    cos = ((torch.diagonal(d, dim1=-2, dim2=-1).sum(-1) - 1) / 2).clamp(-1, 1)
    # (the angle from the skew part: acos loses half the digits near 0)
    skew = torch.stack([d[:, 2, 1] - d[:, 1, 2], d[:, 0, 2] - d[:, 2, 0], d[:, 1, 0] - d[:, 0, 1]], -1).norm(dim=-1) / 2
    ang = torch.atan2(skew, cos)
    dist = lambda x: (x[i, :, 3] - x[j, :, 3]).norm(dim=-1)      # noqa: E731
    return float(ang.mean() * 180.0 / torch.pi), float((dist(p) - dist(q)).abs().mean())


class _PoseExpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xi, base):
        ctx.save_for_backward(xi.detach(), base)
        return ops.pose_exp(base, xi.detach().contiguous())

    @staticmethod
    def backward(ctx, d_poses):
        xi, base = ctx.saved_tensors
        return ops.pose_exp_bwd(base, xi.contiguous(), d_poses.contiguous().float()), None


class PoseTable(torch.nn.Module):
    """One pose per image: buffer `base` [n_img,3,4], parameter `xi` [n_img,6] = (omega, tau), zeros at first.  forward() -> the
    poses [n_img,3,4] with autograd through ops.pose_exp / ops.pose_exp_bwd; poses() the same without a graph."""

    def __init__(self, base_poses):
        super().__init__()
        base = torch.as_tensor(base_poses, dtype=torch.float32)
        if base.dim() != 3 or base.shape[0] < 1 or base.shape[1] < 3 or base.shape[2] != 4:
            raise ValueError('PoseTable: base poses [n_img, 3 (or 4), 4], got {}'.format(tuple(base.shape)))
        self.register_buffer('base', base[:, :3, :4].contiguous().clone())
        self.xi = torch.nn.Parameter(torch.zeros(base.shape[0], 6, dtype=torch.float32, device=base.device))

    @property
    def n_images(self):
        return self.base.shape[0]

    def forward(self):
        return _PoseExpFn.apply(self.xi, self.base)

    def poses(self):
        return ops.pose_exp(self.base, self.xi.detach())
