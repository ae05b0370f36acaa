"""What training through an occupancy grid costs and buys per step: one JSON line.

Trains the solid-body synthetic scene (synthetic.py with the density cut off at 1.5 sigma of each blob: the scene of bench.py's
sparse leg) with the fused Trainer at 4096 rays x (64 + 128) samples, once without a grid and once per --grids entry with
OccupancyGrid.for_training(N) (defaults otherwise: warm-up 256 steps, a refresh every 16; an entry N/k refreshes a k-th of
the cells per refresh: Trainer(occupancy_cells=N^3 / k)), every run from the same seeds.  After
--steps steps it times --blocks blocks of 16 steps each with HIP events around a block (a block holds exactly one refresh, so
its mean is the amortised cost) and prints: steady-state ms per step (mean / min / max over the blocks), the time of one
grid.update alone and its share per step, the occupied share of the grid's cells and of the coarse / fine samples, and the
live share of the samples (the compacted backward's list).  The batches are drawn before the clock starts.
--outside-occupied 0 makes the grids with outside_occupied=False: samples outside the box count as empty.

--plain-only times the step without a grid and uses only calls that older checkouts have: run it there for the comparator.

usage: python tools/time_occupancy_train.py [--steps 1200] [--blocks 20] [--grids 128,128/8,256,256/8] [--plain-only] [--outside-occupied 0|1] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CUTOFF = 1.5
N_RAYS, N_SAMPLES, N_IMPORTANCE = 4096, 64, 128
FOV = 0.6911112070083618
EVERY, WARMUP = 16, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=1200)
    ap.add_argument('--blocks', type=int, default=20)
    ap.add_argument('--grids', default='128,128/8,256,256/8')
    ap.add_argument('--plain-only', action='store_true')
    ap.add_argument('--outside-occupied', type=int, default=1, help='0: samples outside the grid box count as empty (a scene known to lie inside it)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import fastnerf
    from fastnerf import ops, synthetic
    dev = torch.device('cuda')
    H = W = 800
    focal = 0.5 * W / np.tan(0.5 * FOV)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    poses = torch.stack([synthetic.pose_spherical(-180.0 + 3.6 * k, -30.0, 4.0)[:3, :4] for k in range(100)], 0).to(dev)
    args = fastnerf.run_nerf.make_args(N_importance=N_IMPORTANCE, N_samples=N_SAMPLES, perturb=1.0, white_bkgd=True, no_reload=True,
                                       lrate=5e-4, lrate_decay=500)
    gen = torch.Generator().manual_seed(1000)
    batches = []
    for _ in range(64):
        pix = torch.stack([torch.randint(0, 100, (N_RAYS,), generator=gen), torch.randint(0, H, (N_RAYS,), generator=gen),
                           torch.randint(0, W, (N_RAYS,), generator=gen)], 1).int()
        ro, rd = ops.gen_rays_pixels(pix.to(dev), poses, K)
        batches.append((ro, rd, synthetic.render_rays(ro, rd, cutoff=CUTOFF).contiguous()))

    def run(N, part=1):
        torch.manual_seed(0)
        ktr, kte, _, _, _, _ = fastnerf.run_nerf.create_nerf(args, device=dev)
        extra, grid = {}, None
        if N:
            grid = fastnerf.occupancy.OccupancyGrid.for_training(N=N, outside_occupied=bool(a.outside_occupied))
            extra = dict(occupancy=grid, occupancy_every=EVERY, occupancy_warmup=WARMUP,
                         occupancy_cells=None if part == 1 else grid.ncells // part)
        tr = fastnerf.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500, **extra)
        steps = a.steps - (a.steps - WARMUP) % EVERY if N else a.steps      # a block starts on a refresh
        for it in range(steps):
            tr.step(*batches[it % 64])
        torch.cuda.synchronize()
        ms = []
        for b in range(a.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for it in range(EVERY):
                tr.step(*batches[(steps + b * EVERY + it) % 64])
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / EVERY)
        live = tr.live_counts.tolist()
        res = {'ms_per_step': {'mean': float(np.mean(ms)), 'min': float(np.min(ms)), 'max': float(np.max(ms)), 'median': float(np.median(ms))},
               'steps_before_timing': steps, 'backward': 'compacted' if tr.last_step_live else 'plain',
               'live_share_fine': live[0] / max(1, live[1]), 'live_share_coarse': live[2] / max(1, live[3]),
               'loss_fine': float(tr.step(*batches[0])[0][0])}
        if grid is not None:
            occ = tr.occupancy_counts.tolist()
            ups = []
            for _ in range(4):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                grid.update(ktr, cells_per_call=tr.occupancy_cells)
                e1.record()
                torch.cuda.synchronize()
                ups.append(e0.elapsed_time(e1))
            res.update({'N': N, 'cells_per_refresh': grid.ncells // part, 'grid_occupied_fraction': grid.occupied_fraction(), 'occupied_share_coarse': occ[0] / occ[1],
                        'occupied_share_fine': occ[2] / occ[3], 'update_ms': float(np.median(ups)),
                        'update_ms_per_step': float(np.median(ups)) / EVERY, 'updates': grid.updates})
        return res

    out = {'tool': 'time_occupancy_train', 'math': ops.get_math(), 'rays': N_RAYS, 'samples': [N_SAMPLES, N_IMPORTANCE],
           'scene': 'three solid bodies, density zero beyond %.1f sigma' % CUTOFF, 'blocks': a.blocks, 'block_steps': EVERY,
           'no_grid': run(0)}
    if not a.plain_only:
        out['every'], out['warmup'], out['outside_occupied'] = EVERY, WARMUP, bool(a.outside_occupied)
        for spec in [x for x in a.grids.split(',') if x]:      # N, or N/k: a refresh takes a k-th of the cells
            N, part = (int(v) for v in (spec.split('/') + ['1'])[:2])
            out['grid_' + spec] = run(N, part)
        out['no_grid_again'] = run(0)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
