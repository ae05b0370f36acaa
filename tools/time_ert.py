"""What early ray termination buys when a trained scene is rendered: one JSON line.

The scene, the training and the held-out views of tools/time_occupancy.py (three solid bodies, 600 steps of 4096 rays, 64 + 128
samples, four 800 x 800 views, the default OccupancyGrid.from_network).  Variants: plain, grid, and grid + ert for eps in
{1e-3, 1e-2} and ert_block in {16, 32, 48, 64, 192 (one segment: nothing is skipped)}.  ALL variants alternate inside one process:
for every round, for every view, every variant renders that view once (HIP events around the render() call), after one untimed
warm-up view per variant -- so drift of the machine spreads over all of them.  Per variant: ms per view (mean / min / max over
rounds x views), PSNR against the analytic ground truth and its difference to the plain render's, max and mean |dRGB| against the
plain render and against the grid render; per (eps, block): the evaluated share of the fine samples (untimed, from the counters).

--existing-only times plain and grid alone and uses only calls that older checkouts have; --tree DIR imports the package from
another checkout (with its own library): together they run the comparator of the timing condition (ert=None is the parent's
render) from the same job.

usage: python tools/time_ert.py [--steps 600] [--views 4] [--rounds 2] [--size 800] [--existing-only] [--tree DIR] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTOFF = 1.5
N_RAYS, N_SAMPLES, N_IMPORTANCE = 4096, 64, 128
FOV = 0.6911112070083618
EPS = (1e-3, 1e-2)
BLOCKS = (16, 32, 48, 64, N_SAMPLES + N_IMPORTANCE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=600)
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--size', type=int, default=800)
    ap.add_argument('--chunk', type=int, default=32768)
    ap.add_argument('--existing-only', action='store_true')
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
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

    Hv = Wv = a.size
    fv = 0.5 * Wv / np.tan(0.5 * FOV)
    Kv = np.array([[fv, 0, 0.5 * Wv], [0, fv, 0.5 * Hv], [0, 0, 1]])
    views = [synthetic.pose_spherical(-180.0 + 360.0 * (k + 0.5) / a.views + 1.8, -20.0, 4.0)[:3, :4].to(dev) for k in range(a.views)]
    kw = dict(kte, near=2.0, far=6.0)
    kw.pop('ndc', None)
    grid = fastnerf.occupancy.OccupancyGrid.from_network(kte, N=256, bound=1.2, threshold=0., dilate=1, which='both', outside_occupied=True)
    variants = [('plain', {}), ('grid', {'occupancy': grid})]
    if not a.existing_only:
        variants += [('grid+ert eps=%g B=%d' % (e, b), {'occupancy': grid, 'ert': e, 'ert_block': b}) for e in EPS for b in BLOCKS]

    def render(c2w, extra):
        return fastnerf.render.render(Hv, Wv, Kv, chunk=a.chunk, c2w=c2w, ndc=False, **kw, **extra)[0]

    ms = {name: [] for name, _ in variants}
    imgs = {name: [] for name, _ in variants}
    with torch.no_grad():
        for name, extra in variants:
            render(views[0], extra)      # warm-up
        torch.cuda.synchronize()
        for rnd in range(a.rounds):
            for c2w in views:
                for name, extra in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    rgb = render(c2w, extra)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[name].append(e0.elapsed_time(e1))
                    if rnd == 0:
                        imgs[name].append(rgb)
    gts = []
    for c2w in views:
        ro, rd = fastnerf.run_nerf_helpers.get_rays(Hv, Wv, Kv, c2w)
        gts.append(torch.cat([synthetic.render_rays(ro.reshape(-1, 3)[i:i + 65536].contiguous(), rd.reshape(-1, 3)[i:i + 65536].contiguous(),
                                                    cutoff=CUTOFF) for i in range(0, Hv * Wv, 65536)], 0).reshape(Hv, Wv, 3))

    def psnr(name):
        return float(np.mean([-10.0 * np.log10(float(((i - g) ** 2).mean())) for i, g in zip(imgs[name], gts)]))

    def drgb(name, ref):
        d = torch.stack([(x - y).abs() for x, y in zip(imgs[name], imgs[ref])])
        return {'max': float(d.max()), 'mean': float(d.mean())}

    share = {}
    if not a.existing_only:
        with torch.no_grad():      # untimed: the evaluated share of the fine samples of the same views
            for c2w in views:
                ro, rd = fastnerf.run_nerf_helpers.get_rays(Hv, Wv, Kv, c2w)
                rays11 = ops.pack_rays(ro, rd, 2.0, 6.0)
                for name, extra in variants[2:]:
                    c = share.setdefault(name, torch.zeros(4, dtype=torch.int64))
                    for i in range(0, Hv * Wv, a.chunk):
                        o = fastnerf.render._forward_ert(rays11[i:i + a.chunk].contiguous(), kte['network_fn'], kte['network_fine'], N_SAMPLES,
                                                         N_IMPORTANCE, False, 0., True, None, None, extra['ert'], extra['ert_block'],
                                                         occupancy=grid, skip_dead_rgb=True)
                        c += o['counts'].cpu().long()
    res = {'tool': 'time_ert', 'tree': os.path.abspath(a.tree), 'math': ops.get_math(), 'train_steps': a.steps, 'views': a.views,
           'rounds': a.rounds, 'view_size': [Hv, Wv], 'samples': [N_SAMPLES, N_IMPORTANCE], 'chunk': a.chunk,
           'grid_occupied_fraction': grid.occupied_fraction(), 'variants': {}}
    p_plain = psnr('plain')
    for name, _ in variants:
        m = ms[name]
        v = {'ms_per_view': {'mean': float(np.mean(m)), 'min': float(np.min(m)), 'max': float(np.max(m)), 'all': [round(x, 2) for x in m]},
             'psnr': psnr(name), 'dpsnr_vs_plain': psnr(name) - p_plain, 'drgb_vs_plain': drgb(name, 'plain'), 'drgb_vs_grid': drgb(name, 'grid')}
        if name in share:
            c = share[name]
            v['occupied_share_coarse'] = float(c[0]) / float(c[1])
            v['evaluated_share_fine'] = float(c[2]) / float(c[3])
        res['variants'][name] = v
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
