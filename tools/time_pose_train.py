#!/usr/bin/env python3
"""What refining poses costs, and what it buys on a set with noisy poses: one JSON line (recorded in profiles/pose_train.md).

a. `kernels_us`: ops.pose_exp and ops.pose_exp_bwd on a table of 100 images, ops.pose_grad at (n, n_img) = (4096, 8), (4096, 100) and
   (65536, 300) -- --reps launches back to back between two HIP events, outputs and scratch allocated before, so a figure is the
   launch-to-launch time on a busy stream -- and the two ops.ray_grad calls of a pose step at the bench shape (4096 rays x 64 and
   x 192 samples, bf16x6), HIP events around each call inside the steps.
   `step_ms`: the pose step, Trainer(poses=table).step(None, None, target, pix=pix), beside the call-by-call step of a trainer without
   a table (FASTNERF_FUSED_STEP=0, FASTNERF_COMPACT=0) on the same 4096 rays, alternated in slices of --slice steps; the ratio of the
   medians.  The call-by-call step is the yardstick: the pose step is that step plus ray_grad x 2, pose_grad, pose_exp_bwd and an Adam
   launch, with the saving backward run pass by pass.
b. `study`: synthetic.make_dataset (--images images of --size^2 pixels), all poses perturbed by --degrees / --shift, --steps steps of
   --rays rays from the same seeds with and without a pose table: per 100 steps the gauge-free pose error (poses.gauge_free_errors:
   relative rotations between image pairs in degrees, pair distances) and the training PSNR (mean over the 100 steps).

usage: python tools/time_pose_train.py [--part a|b|ab] [--reps 200] [--slice 10] [--rounds 8] [--warm 2]
                                       [--images 8] [--size 64] [--degrees 2] [--shift 0.05] [--steps 1000] [--rays 1024] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS, N_SAMPLES, N_IMPORTANCE = 4096, 64, 128
FOV = 0.6911112070083618


def stats(ms):
    return {'median': float(np.median(ms)), 'min': float(np.min(ms)), 'max': float(np.max(ms)), 'n': len(ms)}


def burst(f, reps):
    """us per call of `reps` calls between two events, after 10 warm calls."""
    for _ in range(10):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def pose_kernels(fastnerf, dev, reps):
    ops = fastnerf.ops
    gen = torch.Generator().manual_seed(3)
    K = [[1111.0, 0.0, 400.0], [0.0, 1111.0, 400.0], [0.0, 0.0, 1.0]]
    out = {}

    def table(n_img):
        base = torch.stack([fastnerf.synthetic.pose_spherical(-180.0 + 360.0 * k / n_img, -30.0, 4.0)[:3, :4] for k in range(n_img)], 0)
        return base.to(dev).contiguous(), (torch.randn(n_img, 6, generator=gen) * 0.01).to(dev)
    base, xi = table(100)
    poses, d_xi, g = torch.empty_like(base), torch.empty(100, 6, device=dev), torch.randn(100, 3, 4, generator=gen).to(dev)
    out['pose_exp n_img=100'] = burst(lambda: ops.pose_exp(base, xi, out=poses), reps)
    out['pose_exp_bwd n_img=100'] = burst(lambda: ops.pose_exp_bwd(base, xi, g, d_xi=d_xi), reps)
    for n, n_img in ((4096, 8), (4096, 100), (65536, 300)):
        base, xi = table(n_img)
        pix = torch.stack([torch.randint(0, n_img, (n,), generator=gen), torch.randint(0, 800, (n,), generator=gen),
                           torch.randint(0, 800, (n,), generator=gen)], 1).int().to(dev)
        d_rays = torch.randn(n, 11, generator=gen).to(dev)
        d_poses = torch.empty(n_img, 3, 4, device=dev)
        ws = torch.empty(max(1, ops.pose_grad_ws_floats(n, n_img)), device=dev)
        out['pose_grad n=%d n_img=%d' % (n, n_img)] = burst(lambda: ops.pose_grad(pix, base, K, d_rays, d_poses=d_poses, ws=ws), reps)
    return out


def steps(fastnerf, dev, a):
    ops, synthetic = fastnerf.ops, fastnerf.synthetic
    ops.set_math('bf16x6')
    fastnerf.render.set_compact('0')
    H = W = 800
    focal = 0.5 * W / np.tan(0.5 * FOV)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    base = torch.stack([synthetic.pose_spherical(-180.0 + 3.6 * k, -30.0, 4.0)[:3, :4] for k in range(100)], 0).to(dev)
    gen = torch.Generator().manual_seed(1000)
    batches = []
    for _ in range(16):
        pix = torch.stack([torch.randint(0, 100, (N_RAYS,), generator=gen), torch.randint(0, H, (N_RAYS,), generator=gen),
                           torch.randint(0, W, (N_RAYS,), generator=gen)], 1).int().to(dev)
        batches.append((pix, ops.gen_rays_pixels(pix, base, K), torch.rand(N_RAYS, 3, generator=gen).to(dev)))
    args = fastnerf.run_nerf.make_args(N_importance=N_IMPORTANCE, N_samples=N_SAMPLES, perturb=1.0, white_bkgd=False, no_reload=True)
    os.environ['FASTNERF_FUSED_STEP'] = '0'      # (read when a Trainer is built)
    arms = {}
    for name in ('call_by_call', 'pose'):
        torch.manual_seed(0)
        ktr = fastnerf.run_nerf.create_nerf(args, device=dev)[0]
        table = fastnerf.poses.PoseTable(base).to(dev) if name == 'pose' else None
        arms[name] = dict(tr=fastnerf.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, poses=table), ms=[], it=0)
    marks = []
    plain_ray_grad = ops.ray_grad

    def marked_ray_grad(*args_, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = plain_ray_grad(*args_, **kw)
        e1.record()
        marks.append((args_[1].shape[1], e0, e1))
        return r
    ops.ray_grad = marked_ray_grad      # (render._backward_passes looks it up on the module)
    try:
        for rnd in range(a.warm + a.rounds):
            for name, v in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.slice):
                    pix, (ro, rd), tgt = batches[v['it'] % 16]
                    if name == 'pose':
                        v['tr'].step(None, None, tgt, pix=pix)
                    else:
                        v['tr'].step(ro, rd, tgt)
                    v['it'] += 1
                e1.record()
                torch.cuda.synchronize()
                if rnd >= a.warm:
                    v['ms'].append(e0.elapsed_time(e1) / a.slice)
    finally:
        ops.ray_grad = plain_ray_grad
        os.environ.pop('FASTNERF_FUSED_STEP', None)
    skip = a.warm * a.slice * 2
    per_S = {}
    for S, e0, e1 in marks[skip:]:
        per_S.setdefault(S, []).append(1e3 * e0.elapsed_time(e1))
    res = {name: stats(v['ms']) for name, v in arms.items()}
    res['ratio'] = res['pose']['median'] / res['call_by_call']['median']
    return res, {'ray_grad S=%d (events around the call)' % S: float(np.median(t)) for S, t in sorted(per_S.items())}


def study(fastnerf, dev, a):
    ops, synthetic, poses_mod = fastnerf.ops, fastnerf.synthetic, fastnerf.poses
    ops.set_math('bf16x6')
    images, truth, focal = synthetic.make_dataset(n_images=a.images, H=a.size, W=a.size, device=dev)
    images, truth = images.float().to(dev), truth.float().to(dev)
    K = np.array([[focal, 0, 0.5 * a.size], [0, focal, 0.5 * a.size], [0, 0, 1]])
    noisy = poses_mod.perturbed(truth, a.degrees, a.shift, seed=3)
    args = fastnerf.run_nerf.make_args(N_importance=32, N_samples=32, perturb=1.0, white_bkgd=True, no_reload=True)
    res = {'images': a.images, 'size': a.size, 'degrees': a.degrees, 'shift': a.shift, 'rays': a.rays, 'samples': [32, 32],
           'start_error': poses_mod.gauge_free_errors(noisy, truth)}
    for name in ('fixed', 'refined'):
        torch.manual_seed(0)
        gen = torch.Generator().manual_seed(17)
        ktr = fastnerf.run_nerf.create_nerf(args, device=dev)[0]
        table = poses_mod.PoseTable(noisy).to(dev) if name == 'refined' else None
        tr = fastnerf.run_nerf.Trainer(ktr, a.size, a.size, K, 2.0, 6.0, poses=table, pose_lrate=a.pose_lrate)
        rows, mse = [], []
        for it in range(1, a.steps + 1):
            pix = torch.stack([torch.randint(0, a.images, (a.rays,), generator=gen), torch.randint(0, a.size, (a.rays,), generator=gen),
                               torch.randint(0, a.size, (a.rays,), generator=gen)], 1).int().to(dev)
            p = pix.long()
            tgt = images[p[:, 0], p[:, 1], p[:, 2]].contiguous()
            if table is not None:
                loss2, _ = tr.step(None, None, tgt, pix=pix)
            else:
                loss2, _ = tr.step(*ops.gen_rays_pixels(pix, noisy, K), tgt)
            mse.append(loss2[:1])
            if it % 100 == 0:
                err = poses_mod.gauge_free_errors(table.poses() if table is not None else noisy, truth)
                rows.append({'step': it, 'rotation_deg': err[0], 'translation': err[1],
                             'train_psnr': float(-10.0 * torch.log10(torch.cat(mse).mean()))})
                mse = []
        res[name] = rows
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='ab')
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--slice', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--warm', type=int, default=2)
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--degrees', type=float, default=2.0)
    ap.add_argument('--shift', type=float, default=0.05)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--rays', type=int, default=1024)
    ap.add_argument('--pose-lrate', type=float, default=1e-3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import fastnerf
    dev = torch.device('cuda')
    res = {'tool': 'time_pose_train'}
    if 'a' in a.part:
        res['kernels_us'] = pose_kernels(fastnerf, dev, a.reps)
        res['step_ms'], ray_grad_us = steps(fastnerf, dev, a)
        res['kernels_us'].update(ray_grad_us)
    if 'b' in a.part:
        res['study'] = study(fastnerf, dev, a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
