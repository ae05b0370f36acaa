#!/usr/bin/env python3
"""Kernel launches per training step, with every optional term of the step off or on (profiles/step_host.md).

  step_launches.py run off|on|expo <k>   k steps at the benchmark's shape (4096 rays, 64 + 128 samples, bf16x6, plain backward); `on`: depth /
                                     opacity supervision, random per-ray backgrounds with an alpha, the distortion loss; `expo`: the terms
                                     off and an exposure table of 100 images (profiles/exposure.md).  For
                                     rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o steps -- python tools/step_launches.py run on 4
  step_launches.py count DIR         launches per step from DIR's kernel trace: the dispatches from one pack_rays_kernel (the first launch of a
                                     step) to the next.  The first count includes what only a first step launches and the last one runs to the
                                     end of the trace: read the middle ones."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def run(terms, k):
    import numpy as np
    import torch
    import fastnerf as fn
    on = terms == 'on'
    fn.ops.set_math('bf16x6')
    fn.render.set_compact('0')
    N, H, W = 4096, 800, 800
    focal = 0.5 * W / np.tan(0.5 * 0.6911112070083618)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    args = fn.run_nerf.make_args(N_importance=128, N_samples=64, perturb=1.0, white_bkgd=not on, no_reload=True)
    torch.manual_seed(0)
    ktr = fn.run_nerf.create_nerf(args, device='cuda')[0]
    terms_kw = dict(lambda_depth=0.1, lambda_acc=0.1, lambda_dist=0.01, bkgd='random') if on else {}
    if terms == 'expo':
        terms_kw = dict(exposure=fn.exposure.ExposureTable(100).cuda())
    tr = fn.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, **terms_kw)
    g = torch.Generator().manual_seed(1)
    poses = torch.stack([fn.synthetic.pose_spherical(-180.0 + 3.6 * i, -30.0, 4.0)[:3, :4] for i in range(100)], 0).cuda()
    pix = torch.stack([torch.randint(0, 100, (N,), generator=g), torch.randint(0, H, (N,), generator=g), torch.randint(0, W, (N,), generator=g)], 1).int()
    ro, rd = fn.ops.gen_rays_pixels(pix.cuda(), poses, K)
    tgt = torch.rand(N, 3, generator=g).cuda()
    kw = {}
    if on:
        kw = dict(alpha=torch.rand(N, generator=g).cuda(), depth=(2 + 4 * torch.rand(N, generator=g)).cuda(), acc=torch.rand(N, generator=g).cuda())
    if terms == 'expo':
        kw = dict(img=pix[:, 0].contiguous().cuda())
    for _ in range(k):
        loss2, _ = tr.step(ro, rd, tgt, **kw)
    torch.cuda.synchronize()
    print('loss', loss2.tolist(), 'aux', tr.aux_losses.tolist(), 'dist', tr.dist_losses.tolist())


def count(d):
    f = glob.glob(d + '/**/*kernel_trace.csv', recursive=True)[0]
    names = [r['Kernel_Name'] for r in sorted(csv.DictReader(open(f)), key=lambda r: int(r['Start_Timestamp']))]
    first = [i for i, name in enumerate(names) if 'pack_rays_kernel' in name]
    print(d, 'dispatches', len(names), 'steps', len(first), 'launches per step', [b - a for a, b in zip(first, first[1:])] + [len(names) - first[-1]])


if __name__ == '__main__':
    if sys.argv[1] == 'run':
        run(sys.argv[2], int(sys.argv[3]))
    else:
        count(sys.argv[2])
