#!/usr/bin/env python3
"""What the exposure table costs and what it does: writes profiles/exposure.md (or --out).

a. kernels: ops.expo_apply and ops.expo_grad (its two launches) on two passes at (n, n_img) = (4096, 8), (4096, 100), (4096, 300) --
   --reps calls back to back between two HIP events, every output and the scratch allocated before (the ops' out-parameters), so a
   figure is the call-to-call time on a busy stream: the launches and what the host spends between them, not a kernel time.
b. steps: the bench-shape step (4096 rays, 64 + 128 samples, bf16x6) with and without Trainer(exposure=) on the fused route and on the
   marched route (96 lattice depths in rows of 128 slots through a 64^3 grid that is all occupied inside its box), the two trainers
   alternated in slices of --slice steps; medians over --rounds slices after --warm, and their ratio.
c. behaviour: the run of tests/test_gpu_expo_train.py::test_table_recovers_known_exposures (8 views of 24 x 24 re-exposed by known
   scales and shifts, 300 steps of 1024 rays), the mean error of log(scale_i / scale_j) every 50 steps, in both math modes.
--fractions LOG: the lines 'reached ... of the cap' / 'expo step ...' of a pytest -s log of the exposure tests are copied into the file.
--trace OFF_DIR EXPO_DIR: the output directories of
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o steps -- python tools/step_launches.py run off|expo 4
  give the kernel times of the three exposure kernels inside the bench-shape step (n = 4096, 100 images) and the launches per step with
  the table off and on -- the structural condition: a step without exposure= launches what it launched before.

usage: python tools/time_exposure.py [--part a|b|c|abc] [--reps 200] [--slice 10] [--rounds 8] [--warm 2] [--fractions LOG]
                                     [--trace OFF_DIR EXPO_DIR] [--out FILE]"""
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


def kernels(fn, dev, reps):
    ops = fn.ops
    gen = torch.Generator().manual_seed(3)
    rows = []
    for n, n_img in ((4096, 8), (4096, 100), (4096, 300)):
        ab = torch.stack([0.3 + torch.rand(n_img, generator=gen), (torch.rand(n_img, generator=gen) - 0.5) * 0.2], 1).to(dev)
        img = torch.randint(0, n_img, (n,), generator=gen).int().to(dev)
        rgb1, rgb0, g1, g0 = (torch.rand(n, 3, generator=gen).to(dev) for _ in range(4))
        e1, e0 = ops.expo_apply(rgb1, img, ab, rgb0=rgb0)
        d_ab, counts, reg = torch.empty(n_img, 2, device=dev), torch.empty(n_img, device=dev, dtype=torch.int32), torch.empty(1, device=dev)
        ws = torch.empty(ops.expo_grad_ws_floats(n, n_img), device=dev)
        t_apply = burst(lambda: ops.expo_apply(rgb1, img, ab, rgb0=rgb0, out=e1, out0=e0), reps)
        # (g is rescaled in place call after call: the values do not matter to the time)
        t_grad = burst(lambda: ops.expo_grad(img, ab, 1.0, 1.0, e1, g1, e0=e0, g0=g0, d_ab=d_ab, counts=counts, ws=ws, loss_reg=reg), reps)
        rows.append((n, n_img, ws.numel() // (3 * n_img), t_apply, t_grad))
    return rows


def step_arms(fn, dev, a, march):
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
        batches.append((ops.gen_rays_pixels(pix, base, K), torch.rand(N_RAYS, 3, generator=gen).to(dev), pix[:, 0].contiguous()))
    args = fn.run_nerf.make_args(N_importance=N_IMPORTANCE, N_samples=N_SAMPLES, perturb=1.0, white_bkgd=False, no_reload=True)
    arms = {}
    for name in ('plain', 'exposure'):
        torch.manual_seed(0)
        ktr = fn.run_nerf.create_nerf(args, device=dev)[0]
        kw = {}
        if march:
            kw = dict(occupancy=fn.occupancy.OccupancyGrid.for_training(N=64, bound=1.5, outside_occupied=False, device=dev),
                      occupancy_warmup=10 ** 9, march=96, march_cap=128)
        if name == 'exposure':
            kw['exposure'] = fn.exposure.ExposureTable(100).to(dev)
        arms[name] = dict(tr=fn.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, **kw), ms=[], it=0)
    for rnd in range(a.warm + a.rounds):
        for name, v in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.slice):
                (ro, rd), tgt, img = batches[v['it'] % len(batches)]
                v['tr'].step(ro, rd, tgt, **({'img': img} if name == 'exposure' else {}))
                v['it'] += 1
            e1.record()
            torch.cuda.synchronize()
            if rnd >= a.warm:
                v['ms'].append(e0.elapsed_time(e1) / a.slice)
    return {name: float(np.median(v['ms'])) for name, v in arms.items()}


def behaviour(fn, dev, mode):
    fn.ops.set_math(mode)
    n_img, n_steps, n_rays, H, W = 8, 300, 1024, 24, 24
    images, poses, focal = fn.synthetic.make_dataset(n_images=n_img, H=H, W=W)
    images, poses = images.float().to(dev), poses.float().to(dev)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    gen = torch.Generator().manual_seed(5)
    s = (0.7 + 0.6 * torch.rand(n_img, generator=gen)).to(dev)
    o = ((torch.rand(n_img, generator=gen) - 0.5) * 0.1).to(dev)
    seen = (images - o[:, None, None, None]) / s[:, None, None, None]
    args = fn.run_nerf.make_args(N_importance=16, N_samples=16, perturb=1., white_bkgd=True, no_reload=True)
    torch.manual_seed(0)
    ktr = fn.run_nerf.create_nerf(args, device=dev)[0]
    t = fn.exposure.ExposureTable(n_img).to(dev)
    tr = fn.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, lrate=1e-3, exposure=t, lambda_autoexpo=1e-3, exposure_lrate=2e-3)
    i, j = torch.triu_indices(n_img, n_img, 1)
    lt = torch.log(s.cpu().double())

    def pair_error():
        ls = torch.log(t.table()[0].detach().cpu().double())
        return float(((ls[i] - ls[j]) - (lt[i] - lt[j])).abs().mean())
    track = [(0, pair_error(), float('nan'))]
    for k in range(1, n_steps + 1):
        pix = torch.stack([torch.randint(0, n_img, (n_rays,), generator=gen), torch.randint(0, H, (n_rays,), generator=gen),
                           torch.randint(0, W, (n_rays,), generator=gen)], 1).int().to(dev)
        p = pix.long()
        loss2, _ = tr.step(*fn.ops.gen_rays_pixels(pix, poses, K), seen[p[:, 0], p[:, 1], p[:, 2]].contiguous(), img=pix[:, 0].contiguous())
        if k % 50 == 0:
            track.append((k, pair_error(), float(loss2[0])))
    return track


def trace_section(off_dir, expo_dir):
    """Kernel times and launches per step out of two rocprofv3 traces of tools/step_launches.py (the counting rule is that tool's)."""
    import csv
    import glob

    def find(d, tail):
        return glob.glob(d + '/**/*' + tail, recursive=True)[0]

    def per_step(d):
        names = [r['Kernel_Name'] for r in sorted(csv.DictReader(open(find(d, 'kernel_trace.csv'))), key=lambda r: int(r['Start_Timestamp']))]
        first = [i for i, name in enumerate(names) if 'pack_rays_kernel' in name]
        return len(names), [b - a for a, b in zip(first, first[1:])] + [len(names) - first[-1]]
    out = ['## Inside the bench-shape step under `rocprofv3 --kernel-trace --stats` (`tools/step_launches.py run off|expo 4`)', '',
           'Kernel times (us; n = 4096, two passes, 100 images):', '', '| kernel | calls | average | min | max |', '|---|---|---|---|---|']
    for r in csv.DictReader(open(find(expo_dir, 'kernel_stats.csv'))):
        if 'expo_' in r['Name']:
            short = r['Name'].split('(')[1 if r['Name'].startswith('(') else 0].split('::')[-1]
            out.append('| `%s` | %s | %.2f | %.2f | %.2f |' % (short, r['Calls'], float(r['AverageNs']) / 1e3, float(r['MinNs']) / 1e3, float(r['MaxNs']) / 1e3))
    out += ['', 'Launches per step (from one `pack_rays_kernel` to the next; the first count includes what only a first step launches, the last',
            'runs to the end of the trace: read the middle ones):', '', '| setting | dispatches | per step |', '|---|---|---|']
    for label, d in (('no `exposure=`', off_dir), ('`exposure=` a table of 100 images', expo_dir)):
        total, steps = per_step(d)
        out.append('| %s | %d | %s |' % (label, total, ', '.join(str(s) for s in steps)))
    return out + ['']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='abc')
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--slice', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--warm', type=int, default=2)
    ap.add_argument('--fractions', default=None)
    ap.add_argument('--trace', nargs=2, default=None, metavar=('OFF_DIR', 'EXPO_DIR'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'exposure.md'))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import fastnerf as fn
    if not torch.cuda.is_available():
        raise SystemExit('time_exposure.py measures on the GPU: none found')
    dev = torch.device('cuda')
    out = ['# Exposure table: kernel times, step times, bounds reached, behaviour', '',
           'Written by `tools/time_exposure.py` on %s.' % torch.cuda.get_device_name(0), '']
    if 'a' in a.part:
        out += ['## The two ops (two passes; us per call, %d calls back to back into buffers allocated before: call-to-call time on a busy '
                'stream, not kernel time)' % a.reps, '',
                '| n | n_img | chunks | expo_apply | expo_grad (walk + finish) |', '|---|---|---|---|---|']
        out += ['| %d | %d | %d | %.1f | %.1f |' % r for r in kernels(fn, dev, a.reps)] + ['']
    if 'b' in a.part:
        out += ['## The bench-shape step with and without the table (ms per step, medians of %d slices of %d steps, bf16x6)' % (a.rounds, a.slice), '',
                '| route | without | with exposure= | ratio |', '|---|---|---|---|']
        for route, march in (('fused', False), ('marched', True)):
            ms = step_arms(fn, dev, a, march)
            out.append('| %s | %.3f | %.3f | %.4f |' % (route, ms['plain'], ms['exposure'], ms['exposure'] / ms['plain']))
        out += ['', 'With the table a step makes four launches more: `expo_apply`, the two of `expo_grad`, and the table\'s Adam.', '']
    if a.trace:
        out += trace_section(*a.trace)
    if a.fractions:
        keep = [ln.rstrip() for ln in open(a.fractions) if 'of the cap' in ln or ln.startswith('expo step') or ln.startswith('exposure recovery')]
        out += ['## Bounds reached in the tests (`pytest -s`)', '', '`expo_grad`: the fraction of the cap (6 m_i + 32) 2^-24 B_i that the worst row reaches.', '',
                '```'] + keep + ['```', '']
    if 'c' in a.part:
        out += ['## Behaviour: known exposures come back', '',
                '8 views of 24 x 24 seen as (c - o_i) / s_i, s_i in [0.7, 1.3], o_i in +-0.05; 300 steps of 1024 rays, lambda_autoexpo = 1e-3, the',
                'table at 2e-3.  Mean over image pairs of |log(scale_i / scale_j) - log(s_i / s_j)|:', '',
                '| mode | ' + ' | '.join('step %d' % k for k in range(0, 301, 50)) + ' | fine mse at 300 |', '|---|' + '---|' * 8]
        for mode in ('fp32', 'bf16x6'):
            tk = behaviour(fn, dev, mode)
            out.append('| %s | ' % mode + ' | '.join('%.4f' % e for _, e, _ in tk) + ' | %.5f |' % tk[-1][2])
        out.append('')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(out))
    print('\n'.join(out))


if __name__ == '__main__':
    main()
