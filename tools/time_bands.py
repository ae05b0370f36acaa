#!/usr/bin/env python3
"""What band weights cost and what they do for pose refinement: prints markdown sections (profiles/pe_bands.md collects them).

a. kernels: ops.band_apply and ops.band_grad on one network -- --reps calls back to back between two HIP events into buffers allocated
   before, so a figure is the call-to-call time on a busy stream: the launch and what the host spends around it, not a kernel time.
b. steps: the bench-shape step (4096 rays, 64 + 128 samples, bf16x6) of a trainer without bands= -- the step of the parent commit, launch
   for launch -- beside Trainer(bands=BandSchedule.constant(mid-ramp weights)), whose step runs without the update phase and then
   band_grad x 2, Adam, band_apply x 2 and the two packings from the host; and beside a cosine ramp that is mid-ramp throughout (new weights
   every step: two small uploads more).  The trainers alternate in slices of --slice steps; medians over --rounds slices after --warm.
c. poses: in the manner of tools/time_pose_train.py -- a synthetic set, every pose perturbed by --degrees / --shift, field and poses
   trained together from scratch -- with the full encoding and with a cosine ramp over the first --ramp steps; gauge-free rotation and
   translation error every 100 steps.  There is no pass / fail bound on it.

usage: python tools/time_bands.py [--part a|b|c|abc] [--reps 200] [--slice 10] [--rounds 8] [--warm 2] [--degrees 5] [--shift 0.1]
                                  [--steps 1000] [--ramp 600] [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS, N_SAMPLES, N_IMPORTANCE = 4096, 64, 128
FOV = 0.6911112070083618


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


def mid_ramp(fn):
    return fn.bands.BandSchedule('cosine', 0, 1000).weights(450)


def kernels(fn, dev, reps):
    ops = fn.ops
    wp, wv = (w.to(dev) for w in mid_ramp(fn))
    master = torch.randn(ops.NET_PARAMS, device=dev)
    eff, grad = torch.empty_like(master), torch.randn(ops.NET_PARAMS, device=dev)
    return burst(lambda: ops.band_apply(wp, wv, master, eff), reps), burst(lambda: ops.band_grad(wp, wv, grad), reps)


def step_arms(fn, dev, a):
    ops = fn.ops
    ops.set_math('bf16x6')
    H = W = 800
    focal = 0.5 * W / np.tan(0.5 * FOV)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    base = torch.stack([fn.synthetic.pose_spherical(-180.0 + 3.6 * k, -30.0, 4.0)[:3, :4] for k in range(100)], 0).to(dev)
    gen = torch.Generator().manual_seed(1000)
    batches = []
    for _ in range(16):
        pix = torch.stack([torch.randint(0, 100, (N_RAYS,), generator=gen), torch.randint(0, H, (N_RAYS,), generator=gen),
                           torch.randint(0, W, (N_RAYS,), generator=gen)], 1).int().to(dev)
        batches.append((ops.gen_rays_pixels(pix, base, K), torch.rand(N_RAYS, 3, generator=gen).to(dev)))
    args = fn.run_nerf.make_args(N_importance=N_IMPORTANCE, N_samples=N_SAMPLES, perturb=1.0, white_bkgd=True, no_reload=True)
    n_steps = (a.warm + a.rounds) * a.slice
    scheds = {'plain': None, 'constant': fn.bands.BandSchedule.constant(*mid_ramp(fn)),
              'ramp': fn.bands.BandSchedule('cosine', -10 * n_steps, 10 * n_steps)}
    arms = {}
    for name, sched in scheds.items():
        torch.manual_seed(0)
        ktr = fn.run_nerf.create_nerf(args, device=dev)[0]
        arms[name] = dict(tr=fn.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, bands=sched), ms=[], it=0)
    for rnd in range(a.warm + a.rounds):
        for name, v in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.slice):
                (ro, rd), tgt = batches[v['it'] % len(batches)]
                v['tr'].step(ro, rd, tgt)
                v['it'] += 1
            e1.record()
            torch.cuda.synchronize()
            if rnd >= a.warm:
                v['ms'].append(e0.elapsed_time(e1) / a.slice)
    assert arms['constant']['tr']._banded() and arms['ramp']['tr']._banded() and not arms['plain']['tr']._banded()
    return {name: float(np.median(v['ms'])) for name, v in arms.items()}


def study(fn, dev, a):
    ops, P = fn.ops, fn.poses
    ops.set_math('bf16x6')
    images, truth, focal = fn.synthetic.make_dataset(n_images=a.images, H=a.size, W=a.size, device=dev)
    images, truth = images.float().to(dev), truth.float().to(dev)
    K = np.array([[focal, 0, 0.5 * a.size], [0, focal, 0.5 * a.size], [0, 0, 1]])
    noisy = P.perturbed(truth, a.degrees, a.shift, seed=3)
    args = fn.run_nerf.make_args(N_importance=32, N_samples=32, perturb=1.0, white_bkgd=True, no_reload=True)
    res = {'start': P.gauge_free_errors(noisy, truth)}
    for name in ('full encoding', 'cosine ramp'):
        torch.manual_seed(0)
        gen = torch.Generator().manual_seed(17)
        ktr = fn.run_nerf.create_nerf(args, device=dev)[0]
        table = P.PoseTable(noisy).to(dev)
        sched = fn.bands.BandSchedule('cosine', 0, a.ramp) if name == 'cosine ramp' else None
        tr = fn.run_nerf.Trainer(ktr, a.size, a.size, K, 2.0, 6.0, poses=table, pose_lrate=a.pose_lrate, bands=sched)
        rows, mse = [], []
        for it in range(1, a.steps + 1):
            pix = torch.stack([torch.randint(0, a.images, (a.rays,), generator=gen), torch.randint(0, a.size, (a.rays,), generator=gen),
                               torch.randint(0, a.size, (a.rays,), generator=gen)], 1).int().to(dev)
            p = pix.long()
            loss2, _ = tr.step(None, None, images[p[:, 0], p[:, 1], p[:, 2]].contiguous(), pix=pix)
            mse.append(loss2[:1])
            if it % 100 == 0:
                err = P.gauge_free_errors(table.poses(), truth)
                rows.append((it, err[0], err[1], float(-10.0 * torch.log10(torch.cat(mse).mean()))))
                mse = []
        res[name] = rows
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='abc')
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--slice', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--warm', type=int, default=2)
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--size', type=int, default=64)
    ap.add_argument('--degrees', type=float, default=5.0)
    ap.add_argument('--shift', type=float, default=0.1)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--ramp', type=int, default=600)
    ap.add_argument('--rays', type=int, default=1024)
    ap.add_argument('--pose-lrate', type=float, default=1e-3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import fastnerf as fn
    if not torch.cuda.is_available():
        raise SystemExit('time_bands.py measures on the GPU: none found')
    dev = torch.device('cuda')
    out = ['Written by `tools/time_bands.py` on %s.' % torch.cuda.get_device_name(0), '']
    if 'a' in a.part:
        t_apply, t_grad = kernels(fn, dev, a.reps)
        out += ['## The two ops (one network; us per call, %d calls back to back: call-to-call time on a busy stream, not kernel time)' % a.reps,
                '', '| band_apply (595 844 floats read and written) | band_grad (35 712 floats, in place) |', '|---|---|',
                '| %.1f | %.1f |' % (t_apply, t_grad), '']
    if 'b' in a.part:
        ms = step_arms(fn, dev, a)
        out += ['## The bench-shape step (4096 x (64 + 128), bf16x6; ms per step, medians of %d slices of %d steps)' % (a.rounds, a.slice), '',
                '| without bands= (one call) | constant mid-ramp weights | cosine ramp, new weights every step | ratios |', '|---|---|---|---|',
                '| %.3f | %.3f | %.3f | %.4f, %.4f |' % (ms['plain'], ms['constant'], ms['ramp'], ms['constant'] / ms['plain'],
                                                      ms['ramp'] / ms['plain']), '']
    if 'c' in a.part:
        res = study(fn, dev, a)
        out += ['## Poses %g degrees / %g off, field and poses trained together (%d images of %d x %d, %d rays, 32 + 32 samples, pose_lrate %g)'
                % (a.degrees, a.shift, a.images, a.size, a.size, a.rays, a.pose_lrate), '',
                'Start: rotation %.3f deg, translation %.4f (gauge-free).  The ramp spans the steps 0 .. %d.' % (res['start'] + (a.ramp,)), '',
                '| step | full encoding: rotation (deg) | translation | train PSNR | cosine ramp: rotation (deg) | translation | train PSNR |',
                '|---|---|---|---|---|---|---|']
        for r0, r1 in zip(res['full encoding'], res['cosine ramp']):
            out.append('| %d | %.3f | %.4f | %.2f | %.3f | %.4f | %.2f |' % (r0 + r1[1:]))
        out.append('')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(out))
    print('\n'.join(out))


if __name__ == '__main__':
    main()
