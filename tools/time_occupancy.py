"""What the occupancy grid buys when a trained scene is rendered: one JSON line.

Trains the solid-body synthetic scene (synthetic.py with the density cut off at 1.5 sigma of each blob: the scene of bench.py's
sparse leg) for --steps steps of 4096 rays, 64 + 128 samples, builds OccupancyGrid.from_network with the defaults, renders the
same held-out views with and without it and prints: ms per view both ways (HIP events, one warm-up view, mean / min / max over
the views), the occupied fraction of the grid, the occupied share of the coarse and the fine samples, PSNR of either render
against the analytic ground truth, max and mean |dRGB| between the two renders, the grid's build time, and the time the
sorting kernels (count, scan, scatter of both passes) take per view.  --outside-occupied 0 builds the grid with
outside_occupied=False: samples outside the box count as empty, for a scene known to lie inside it.

--plain-only renders without the grid and uses only calls that older checkouts have: run it there for the comparator.

usage: python tools/time_occupancy.py [--steps 600] [--views 4] [--size 800] [--plain-only] [--outside-occupied 0|1] [--levels K [--growth 2.0]]
       [--N 256 | --N 256,128,128] [--out FILE]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=600)
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--size', type=int, default=800)
    ap.add_argument('--chunk', type=int, default=32768)
    ap.add_argument('--plain-only', action='store_true')
    ap.add_argument('--outside-occupied', type=int, default=1, help='0: samples outside the grid box count as empty (a scene known to lie inside it)')
    ap.add_argument('--levels', type=int, default=0, help='K >= 1: an OccupancyCascade of K levels instead of the single grid')
    ap.add_argument('--growth', type=float, default=2.0, help='box of level l = bound * growth^l (with --levels)')
    ap.add_argument('--N', default='256', help='cells per axis; with --levels also one value per level, comma separated')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.levels < 0 or a.levels > 8:
        ap.error('--levels is 1 .. 8 (0: the single grid)')
    n_values = len(a.N.split(','))
    if a.levels == 0 and (n_values != 1 or a.growth != 2.0):
        ap.error('--growth and one --N per level go with --levels K')
    if a.levels > 0 and n_values not in (1, a.levels):
        ap.error('--N is one value or one per level: got %d for --levels %d' % (n_values, a.levels))
    if a.plain_only and (a.levels or n_values != 1):
        ap.error('--plain-only renders without a grid: --levels / --N do not apply')
    import fastnerf
    from fastnerf import ops, synthetic
    dev = torch.device('cuda')
    H = W = 800
    focal = 0.5 * W / np.tan(0.5 * FOV)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    poses = torch.stack([synthetic.pose_spherical(-180.0 + 3.6 * k, -30.0, 4.0)[:3, :4] for k in range(100)], 0).to(dev)
    args = fastnerf.run_nerf.make_args(N_importance=N_IMPORTANCE, N_samples=N_SAMPLES, perturb=1.0, white_bkgd=True, no_reload=True,
                                       lrate=5e-4, lrate_decay=500)
    torch.manual_seed(0)
    ktr, kte, _, _, _, _ = fastnerf.run_nerf.create_nerf(args, device=dev)
    tr = fastnerf.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500)
    gen = torch.Generator().manual_seed(1000)
    for _ in range(a.steps):
        pix = torch.stack([torch.randint(0, 100, (N_RAYS,), generator=gen), torch.randint(0, H, (N_RAYS,), generator=gen),
                           torch.randint(0, W, (N_RAYS,), generator=gen)], 1).int()
        ro, rd = ops.gen_rays_pixels(pix.to(dev), poses, K)
        tr.step(ro, rd, synthetic.render_rays(ro, rd, cutoff=CUTOFF).contiguous())
    torch.cuda.synchronize()

    # held-out views: between the training azimuths, at another elevation
    Hv = Wv = a.size
    fv = 0.5 * Wv / np.tan(0.5 * FOV)
    Kv = np.array([[fv, 0, 0.5 * Wv], [0, fv, 0.5 * Hv], [0, 0, 1]])
    views = [synthetic.pose_spherical(-180.0 + 360.0 * (k + 0.5) / a.views + 1.8, -20.0, 4.0)[:3, :4].to(dev) for k in range(a.views)]
    kw = dict(kte, near=2.0, far=6.0)
    kw.pop('ndc', None)

    def timed_views(extra):
        imgs, ms = [], []
        with torch.no_grad():
            fastnerf.render.render(Hv, Wv, Kv, chunk=a.chunk, c2w=views[0], ndc=False, **kw, **extra)      # warm-up
            for c2w in views:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rgb = fastnerf.render.render(Hv, Wv, Kv, chunk=a.chunk, c2w=c2w, ndc=False, **kw, **extra)[0]
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
                imgs.append(rgb)
        return imgs, {'mean': float(np.mean(ms)), 'min': float(np.min(ms)), 'max': float(np.max(ms)), 'views': [round(m, 3) for m in ms]}

    def psnr(imgs, gts):
        return float(np.mean([-10.0 * np.log10(float(((i - g) ** 2).mean())) for i, g in zip(imgs, gts)]))

    gts = []
    for c2w in views:
        ro, rd = fastnerf.run_nerf_helpers.get_rays(Hv, Wv, Kv, c2w)
        gts.append(torch.cat([synthetic.render_rays(ro.reshape(-1, 3)[i:i + 65536].contiguous(), rd.reshape(-1, 3)[i:i + 65536].contiguous(),
                                                    cutoff=CUTOFF) for i in range(0, Hv * Wv, 65536)], 0).reshape(Hv, Wv, 3))
    plain, ms_plain = timed_views({})
    res = {'tool': 'time_occupancy', 'math': ops.get_math(), 'train_steps': a.steps, 'views': a.views, 'view_size': [Hv, Wv],
           'samples': [N_SAMPLES, N_IMPORTANCE], 'chunk': a.chunk, 'scene': 'three solid bodies, density zero beyond %.1f sigma' % CUTOFF,
           'ms_per_view_plain': ms_plain, 'psnr_plain': psnr(plain, gts)}
    if not a.plain_only:
        Ns = [int(v) for v in a.N.split(',')]
        gkw = dict(N=Ns[0], bound=1.2, threshold=0., dilate=1, which='both', outside_occupied=bool(a.outside_occupied))
        if a.levels > 0:
            G = fastnerf.occupancy.OccupancyCascade
            gkw.update(levels=a.levels, growth=a.growth, N=Ns[0] if len(Ns) == 1 else Ns)
        else:
            G = fastnerf.occupancy.OccupancyGrid
        G.from_network(kte, **gkw)      # warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        grid = G.from_network(kte, **gkw)
        e1.record()
        torch.cuda.synchronize()
        masked, ms_grid = timed_views({'occupancy': grid})
        counts = torch.zeros(4, dtype=torch.int64)
        decided = torch.zeros(2, a.levels + 1, dtype=torch.int64)      # cascade: samples per deciding level (last: none), coarse / fine
        ms_classify = 0.0
        with torch.no_grad():      # untimed: the occupied share of the samples of the same views
            for c2w in views:
                ro, rd = fastnerf.run_nerf_helpers.get_rays(Hv, Wv, Kv, c2w)
                rays11 = ops.pack_rays(ro, rd, 2.0, 6.0)
                for i in range(0, Hv * Wv, a.chunk):
                    o = fastnerf.render._forward_occ(rays11[i:i + a.chunk].contiguous(), kte['network_fn'], kte['network_fine'], N_SAMPLES,
                                                     N_IMPORTANCE, False, 0., True, None, None, grid)
                    counts += o['counts'].cpu().long()
                    # the sorting itself (count, scan, scatter of both passes), at the depths the render used
                    e2, e3 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    r11 = rays11[i:i + a.chunk].contiguous()
                    e2.record()
                    grid.classify(r11, o['z0'], o['raw0'])
                    grid.classify(r11, o['z_vals'], o['raw'])
                    e3.record()
                    torch.cuda.synchronize()
                    ms_classify += e2.elapsed_time(e3)
                    if a.levels > 0:
                        for k, z in enumerate((o['z0'], o['z_vals'])):
                            who = grid.decided_by(r11[:, None, 0:3] + r11[:, None, 3:6] * z[..., None]).long()
                            decided[k] += torch.bincount((who % (a.levels + 1)).reshape(-1), minlength=a.levels + 1).cpu()
        d = torch.stack([(m - p).abs() for m, p in zip(masked, plain)])
        res.update({'grid': gkw, 'classify_ms_per_view': ms_classify / a.views,
                    'grid_build_ms': e0.elapsed_time(e1), 'grid_occupied_fraction': grid.occupied_fraction(),
                    'occupied_share_coarse': float(counts[0]) / float(counts[1]), 'occupied_share_fine': float(counts[2]) / float(counts[3]),
                    'ms_per_view_grid': ms_grid, 'speedup': ms_plain['mean'] / ms_grid['mean'], 'psnr_grid': psnr(masked, gts),
                    'max_abs_drgb': float(d.max()), 'mean_abs_drgb': float(d.mean())})
        if a.levels > 0:
            res.update({'decided_share_coarse': (decided[0].double() / decided[0].sum()).tolist(),
                        'decided_share_fine': (decided[1].double() / decided[1].sum()).tolist()})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
