"""What clamping near / far to the occupancy grid (`tighten`) costs and buys on the synthetic scene: one JSON line.

The scene of tools/time_occupancy.py (three solid bodies, 4096 rays per step, 64 + 128 samples, a 128^3 training grid over
+-1.2) with `outside_occupied=False` -- the configuration tightening is for.  Everything that is compared alternates inside one
process, so drift of the machine spreads over all variants; the comparison base of every time is the same build with tighten=False.

  kernel    fastnerf_occ_ray_bounds alone, HIP events around the launch: 4096 training rays and one 400 x 400 image, on the trained
            grid; median / min / max of 50 launches after 5 warm-ups.
  training  three trainers from the same initial weights, one step each in turn: the grid, the grid with tighten, and the grid with
            tighten and N_samples reduced until its occupied coarse samples per step match the untightened run's (the reduction is
            read off a pilot of --pilot steps).  Per run: ms per step (mean / median over the steps after the warm-up of the grid),
            occupied and total samples per step of both passes (trainer.occupancy_counts, mean over those steps), and held-out PSNR
            after the same number of steps, rendered the way the run was trained.
  rendering the networks of the untightened run through its grid: plain, grid, grid + tighten at N_samples in {64, 32, 16}
            (N_importance = 128), ms per image and PSNR against the analytic ground truth.

Tightening raises the occupied share of a step's samples: a step may get slower while each sample does more.  Both sides are in
the output; profiles/ray_bounds.md is written from it.

usage: python tools/time_ray_bounds.py [--steps 600] [--pilot 400] [--views 4] [--rounds 2] [--size 400] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTOFF = 1.5
N_RAYS, N_SAMPLES, N_IMPORTANCE = 4096, 64, 128
FOV = 0.6911112070083618
WARMUP = 256      # steps before the grid's first refresh: the grid is full until then, and nothing can be tightened


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=600)
    ap.add_argument('--pilot', type=int, default=400)
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--size', type=int, default=400)
    ap.add_argument('--chunk', type=int, default=32768)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import fastnerf
    from fastnerf import _lib, ops, synthetic
    dev = torch.device('cuda')
    H = W = 800
    focal = 0.5 * W / np.tan(0.5 * FOV)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    poses = torch.stack([synthetic.pose_spherical(-180.0 + 3.6 * k, -30.0, 4.0)[:3, :4] for k in range(100)], 0).to(dev)

    def new_run(tighten, n_samples):
        args = fastnerf.run_nerf.make_args(N_importance=N_IMPORTANCE, N_samples=n_samples, perturb=1.0, white_bkgd=True, no_reload=True,
                                           lrate=5e-4, lrate_decay=500)
        torch.manual_seed(0)
        ktr, kte, _, _, _, _ = fastnerf.run_nerf.create_nerf(args, device=dev)
        grid = fastnerf.occupancy.OccupancyGrid.for_training(N=128, bound=1.2, outside_occupied=False, device=dev)
        tr = fastnerf.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500, occupancy=grid, occupancy_warmup=WARMUP,
                                       tighten=tighten)
        return dict(tr=tr, kte=kte, grid=grid, tighten=tighten, N_samples=n_samples, events=[], counts=torch.zeros(4, device=dev, dtype=torch.int64),
                    counted=0)

    def train(runs, steps, seed):
        """One step of every run in turn, on the same batch."""
        gen = torch.Generator().manual_seed(seed)
        for it in range(steps):
            pix = torch.stack([torch.randint(0, 100, (N_RAYS,), generator=gen), torch.randint(0, H, (N_RAYS,), generator=gen),
                               torch.randint(0, W, (N_RAYS,), generator=gen)], 1).int()
            ro, rd = ops.gen_rays_pixels(pix.to(dev), poses, K)
            tgt = synthetic.render_rays(ro, rd, cutoff=CUTOFF).contiguous()
            for r in runs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r['tr'].step(ro, rd, tgt)
                e1.record()
                if it > WARMUP:
                    r['events'].append((e0, e1))
                    r['counts'] += r['tr'].occupancy_counts.long()
                    r['counted'] += 1
        torch.cuda.synchronize()

    # the pilot: how far N_samples can come down before the tightened run has the untightened run's occupied coarse samples
    pilot = [new_run(False, N_SAMPLES), new_run(True, N_SAMPLES)]
    train(pilot, max(a.pilot, WARMUP + 32), 999)
    occ = [float(r['counts'][0]) / max(1, r['counted']) for r in pilot]
    n_reduced = int(min(N_SAMPLES, max(8, round(N_SAMPLES * occ[0] / max(1.0, occ[1])))))
    del pilot

    runs = [new_run(False, N_SAMPLES), new_run(True, N_SAMPLES), new_run(True, n_reduced)]
    names = ['grid', 'grid+tighten', 'grid+tighten N_samples=%d' % n_reduced]
    train(runs, a.steps, 1000)

    Hv = Wv = a.size
    fv = 0.5 * Wv / np.tan(0.5 * FOV)
    Kv = np.array([[fv, 0, 0.5 * Wv], [0, fv, 0.5 * Hv], [0, 0, 1]])
    views = [synthetic.pose_spherical(-180.0 + 360.0 * (k + 0.5) / a.views + 1.8, -20.0, 4.0)[:3, :4].to(dev) for k in range(a.views)]
    gts = []
    for c2w in views:
        ro, rd = fastnerf.run_nerf_helpers.get_rays(Hv, Wv, Kv, c2w)
        gts.append(torch.cat([synthetic.render_rays(ro.reshape(-1, 3)[i:i + 65536].contiguous(), rd.reshape(-1, 3)[i:i + 65536].contiguous(),
                                                    cutoff=CUTOFF) for i in range(0, Hv * Wv, 65536)], 0).reshape(Hv, Wv, 3))

    def render(kte, c2w, **extra):
        kw = dict(kte, near=2.0, far=6.0)
        kw.pop('ndc', None)
        kw.update(extra)
        return fastnerf.render.render(Hv, Wv, Kv, chunk=a.chunk, c2w=c2w, ndc=False, **kw)[0]

    def psnr(imgs):
        return float(np.mean([-10.0 * np.log10(float(((i - g) ** 2).mean())) for i, g in zip(imgs, gts)]))

    res = {'tool': 'time_ray_bounds', 'math': ops.get_math(), 'train_steps': a.steps, 'pilot_steps': a.pilot, 'grid_warmup': WARMUP,
           'rays_per_step': N_RAYS, 'samples': [N_SAMPLES, N_IMPORTANCE], 'view_size': [Hv, Wv], 'views': a.views, 'rounds': a.rounds,
           'pilot_occupied_coarse_per_step': {'grid': occ[0], 'grid+tighten': occ[1]}, 'N_samples_reduced': n_reduced, 'training': {},
           'rendering': {}, 'kernel': {}}
    with torch.no_grad():
        for name, r in zip(names, runs):
            ms = [e0.elapsed_time(e1) for e0, e1 in r['events']]
            c = (r['counts'].double() / max(1, r['counted'])).tolist()
            imgs = [render(r['kte'], c2w, occupancy=r['grid'], tighten=r['tighten']) for c2w in views]
            res['training'][name] = {'N_samples': r['N_samples'], 'ms_per_step': {'mean': float(np.mean(ms)), 'median': float(np.median(ms))},
                                     'occupied_coarse': c[0], 'total_coarse': c[1], 'occupied_fine': c[2], 'total_fine': c[3],
                                     'grid_occupied_fraction': r['grid'].occupied_fraction(), 'psnr_heldout': psnr(imgs)}

        # rendering: the untightened run's networks through its grid, every variant in turn
        base = runs[0]
        variants = []
        for ns in (64, 32, 16):
            variants += [('plain N_samples=%d' % ns, dict(N_samples=ns)), ('grid N_samples=%d' % ns, dict(N_samples=ns, occupancy=base['grid'])),
                         ('grid+tighten N_samples=%d' % ns, dict(N_samples=ns, occupancy=base['grid'], tighten=True))]
        ms = {name: [] for name, _ in variants}
        imgs = {name: [] for name, _ in variants}
        for name, extra in variants:
            render(base['kte'], views[0], **extra)      # warm-up
        torch.cuda.synchronize()
        for rnd in range(a.rounds):
            for c2w in views:
                for name, extra in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    rgb = render(base['kte'], c2w, **extra)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[name].append(e0.elapsed_time(e1))
                    if rnd == 0:
                        imgs[name].append(rgb)
        for name, _ in variants:
            m = ms[name]
            res['rendering'][name] = {'ms_per_image': {'mean': float(np.mean(m)), 'min': float(np.min(m)), 'max': float(np.max(m))},
                                      'psnr': psnr(imgs[name])}

        # the kernel alone
        g = base['grid']
        gen = torch.Generator().manual_seed(7)
        pix = torch.stack([torch.randint(0, 100, (N_RAYS,), generator=gen), torch.randint(0, H, (N_RAYS,), generator=gen),
                           torch.randint(0, W, (N_RAYS,), generator=gen)], 1).int()
        batches = {'4096 training rays': ops.pack_rays(*ops.gen_rays_pixels(pix.to(dev), poses, K), 2.0, 6.0),
                   'one %d x %d image' % (Hv, Wv): ops.pack_rays(*fastnerf.run_nerf_helpers.get_rays(Hv, Wv, Kv, views[0]), 2.0, 6.0)}
        for name, rays11 in batches.items():
            n = rays11.shape[0]
            bounds = torch.empty(n, 2, device=dev)
            hit = torch.empty(n, device=dev, dtype=torch.uint8)
            t = []
            for k in range(55):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(_lib.lib().fastnerf_occ_ray_bounds(ctypes.byref(g._c), None, n, rays11.data_ptr(), 0, bounds.data_ptr(),
                                                              hit.data_ptr(), _lib.stream()), 'fastnerf_occ_ray_bounds')
                e1.record()
                torch.cuda.synchronize()
                if k >= 5:
                    t.append(e0.elapsed_time(e1) * 1e3)
            kept = ((bounds[:, 1] - bounds[:, 0]) / (rays11[:, 7] - rays11[:, 6]))[hit.bool()]
            res['kernel'][name] = {'rays': n, 'us_per_launch': {'median': float(np.median(t)), 'min': float(np.min(t)), 'max': float(np.max(t))},
                                   'hit_share': float(hit.float().mean()), 'kept_of_near_far_on_hit_rays': float(kept.mean()) if kept.numel() else None}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
