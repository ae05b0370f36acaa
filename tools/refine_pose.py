"""iNeRF-style pose refinement through the fused renderer: a tool, not a test.

A field is fitted to the analytic scene of synthetic.py for --train-iters steps, an image is rendered from a known pose, and a
perturbed pose is pulled back to it by Adam on a 6-vector (axis-angle rotation + translation, applied on the left of the start pose)
whose gradient comes through `render(H, W, K, c2w=pose)` -- get_rays / pack_rays, the fused render_rays and ops.ray_grad.
Prints the rotation error (degrees) and the translation error per iteration.
(The pose table that training refines, fastnerf.poses.PoseTable, uses the OTHER convention: there the camera turns about its own
centre, t = t0 + tau; here the rotation is about the world origin and moves the camera centre with it.)

usage: python tools/refine_pose.py [--iters 100] [--train-iters 300] [--size 24] [--rot-deg 4] [--trans 0.1] [--lr 0.01]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastnerf as fn   # noqa: E402


def hat(w):
    z = torch.zeros((), dtype=w.dtype)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def se3(xi, c2w):
    """(exp(hat(xi[:3])), xi[3:]) applied to the pose c2w [3,4]: rotation about the world origin, then translation."""
    R = torch.matrix_exp(hat(xi[:3]))
    return torch.cat([R @ c2w[:, :3], (R @ c2w[:, 3] + xi[3:])[:, None]], -1)


def pose_error(a, b):
    cos = ((a[:, :3].T @ b[:, :3]).diagonal().sum() - 1) / 2
    return float(torch.rad2deg(torch.acos(cos.clamp(-1, 1)))), float((a[:, 3] - b[:, 3]).norm())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--train-iters', type=int, default=300)
    ap.add_argument('--size', type=int, default=24, help='the refined view is size x size pixels')
    ap.add_argument('--rot-deg', type=float, default=4.0)
    ap.add_argument('--trans', type=float, default=0.1)
    ap.add_argument('--lr', type=float, default=0.01)
    a = ap.parse_args()
    torch.manual_seed(0)
    H = W = a.size
    imgs, poses, focal = fn.synthetic.make_dataset(n_images=8, H=H, W=W)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    args = fn.run_nerf.make_args(N_importance=32, N_samples=32, perturb=1.0, white_bkgd=True, no_reload=True)
    k_train, k_test, _, _, _, _ = fn.run_nerf.create_nerf(args)
    # fit the field (the fused Trainer: no ray gradients involved)
    rays = [fn.run_nerf_helpers.get_rays(H, W, K, p) for p in poses]
    ro = torch.cat([r[0].reshape(-1, 3) for r in rays], 0)
    rd = torch.cat([r[1].reshape(-1, 3) for r in rays], 0)
    tgt = imgs.reshape(-1, 3).float().cuda()
    tr = fn.run_nerf.Trainer(k_train, H, W, K, 2.0, 6.0)
    for it in range(a.train_iters):
        sel = torch.randint(0, ro.shape[0], (1024,)).cuda()
        loss2, _ = tr.step(ro[sel], rd[sel], tgt[sel])
    if a.train_iters:
        print('field fitted: loss %.5f after %d steps' % (float(loss2[0]), a.train_iters))
    # the view to register: a pose between two training cameras, rendered by the field itself
    kw = dict(k_test, ndc=False, near=2.0, far=6.0, perturb=0., raw_noise_std=0.)
    for p in list(kw['network_fn'].parameters()) + list(kw['network_fine'].parameters()):
        p.requires_grad_(False)
    true = fn.synthetic.pose_spherical(-150.0, -30.0, 4.0)[:3, :4]
    with torch.no_grad():
        target = fn.render.render(H, W, K, c2w=true, **kw)[0]
    gen = torch.Generator().manual_seed(1)
    axis = torch.randn(3, generator=gen)
    xi0 = torch.cat([axis / axis.norm() * np.deg2rad(a.rot_deg), torch.randn(3, generator=gen) * a.trans])
    start = se3(xi0, true)
    xi = torch.zeros(6, requires_grad=True)
    opt = torch.optim.Adam([xi], lr=a.lr)
    for it in range(a.iters + 1):
        pose = se3(xi, start)
        rot, trans = pose_error(pose.detach(), true)
        if it == a.iters:
            print('%4d  rotation %.4f deg  translation %.5f' % (it, rot, trans))
            break
        rgb = fn.render.render(H, W, K, c2w=pose, **kw)[0]
        loss = ((rgb - target) ** 2).mean()
        print('%4d  rotation %.4f deg  translation %.5f  loss %.3e' % (it, rot, trans, float(loss)))
        opt.zero_grad()
        loss.backward()
        opt.step()


if __name__ == '__main__':
    main()
