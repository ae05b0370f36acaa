"""What training through an occupancy cascade costs: one JSON line.

On freshly initialised networks (the refresh and the step do the same work whatever the weights hold) it times, with HIP events after
a warm-up call, mean over --reps:

  own_ms             the own lists of the cascade's levels (fastnerf_occ_cascade_own), made once per cascade
  refresh_all_ms     every cell of every level: OccupancyGrid.update level by level
  refresh_own_ms     the own cells only: OccupancyCascade.update, one cursor over all levels
  refresh_budget_ms  OccupancyCascade.update(cells_per_call=--cells)
  step_cascade_ms / step_grid_ms   Trainer.step of --rays rays, 64 + 128 samples, through a ONE-level cascade and through that grid
                     (the same launches but for the entry point: the two should agree)

and reports the cell counts beside them (cells_all, cells_own per level).  profiles/cascade_train.md holds the cost model.

usage: python tools/time_cascade_train.py [--levels 3] [--N 128] [--growth 2.0] [--dilate 1] [--cells 262144] [--rays 4096] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, reps):
    call()      # warm-up
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.mean(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--levels', type=int, default=3)
    ap.add_argument('--N', type=int, default=128)
    ap.add_argument('--growth', type=float, default=2.0)
    ap.add_argument('--dilate', type=int, default=1)
    ap.add_argument('--cells', type=int, default=1 << 18)
    ap.add_argument('--rays', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import fastnerf
    from fastnerf import ops
    from fastnerf.occupancy import OccupancyCascade, OccupancyGrid
    dev = torch.device('cuda')
    H = W = 800
    K = np.array([[1111.0, 0, 400.0], [0, 1111.0, 400.0], [0, 0, 1]])
    args = fastnerf.run_nerf.make_args(N_importance=128, N_samples=64, perturb=1.0, white_bkgd=True, no_reload=True)
    torch.manual_seed(0)
    ktr = fastnerf.run_nerf.create_nerf(args, device=dev)[0]
    geom = dict(N=a.N, bound=1.2, dilate=a.dilate)
    cascade = OccupancyCascade.for_training(levels=a.levels, growth=a.growth, **geom)
    grids = [OccupancyGrid.for_training(N=a.N, bound=1.2 * a.growth ** l, dilate=a.dilate) for l in range(a.levels)]
    res = {'tool': 'time_cascade_train', 'math': ops.get_math(), 'levels': a.levels, 'N': a.N, 'growth': a.growth, 'dilate': a.dilate,
           'cells_all': a.levels * a.N ** 3, 'cells_own': [int(cascade.own_cells(l).numel()) for l in range(a.levels)],
           'cells_per_call': a.cells, 'reps': a.reps}
    res['own_ms'] = timed(lambda: [ops.occ_cascade_own(cascade._c, l, a.dilate, dev) for l in range(a.levels)], a.reps)
    res['refresh_all_ms'] = timed(lambda: [g.update(ktr) for g in grids], a.reps)
    res['refresh_own_ms'] = timed(lambda: cascade.update(ktr), a.reps)
    res['refresh_budget_ms'] = timed(lambda: cascade.update(ktr, cells_per_call=a.cells), a.reps)
    pose = fastnerf.synthetic.pose_spherical(30.0, -30.0, 4.0)[:3, :4]
    ro, rd = fastnerf.run_nerf_helpers.get_rays(H, W, K, pose)
    sel = torch.randperm(H * W, generator=torch.Generator().manual_seed(1))[:a.rays]
    ro, rd = ro.reshape(-1, 3)[sel].contiguous().to(dev), rd.reshape(-1, 3)[sel].contiguous().to(dev)
    tgt = torch.rand(a.rays, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    for name, occ in (('step_grid_ms', OccupancyGrid.for_training(**geom)), ('step_cascade_ms', OccupancyCascade.for_training(levels=1, **geom))):
        torch.manual_seed(0)
        tr = fastnerf.run_nerf.Trainer(fastnerf.run_nerf.create_nerf(args, device=dev)[0], H, W, K, 2.0, 6.0, occupancy=occ,
                                       occupancy_warmup=10 ** 9)
        res[name] = timed(lambda: tr.step(ro, rd, tgt), a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
