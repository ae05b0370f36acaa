"""The marched render beside the hierarchical render through the grid, on a trained scene: one JSON line.

The scene, the training and the held-out views of tools/time_ert.py (three solid bodies, 600 steps of 4096 rays, 64 + 128 samples,
views the training never saw).  One grid for every variant: OccupancyGrid.from_network with outside_occupied=False (the scene lies
inside the box; with outside_occupied=True every lattice depth outside the box would be a live sample).  Variants:
  hierarchical   the 64 + 128 render through the grid, with and without ert (existing code)
  march          K in --lattice, march_cap in --caps, with and without ert
ALL variants alternate inside one process: for every round, for every view, every variant renders that view once (HIP events around the
render() call), after one untimed warm-up view per variant -- drift of the machine spreads over all of them.  Per variant: ms per view
(mean / min / max over rounds x views) and PSNR against the analytic ground truth; per marched variant also the evaluated samples
per ray and the share of rays that overflow their row (untimed, from the counters); for the hierarchical ones the evaluated samples
per ray of both passes.

usage: python tools/time_march.py [--steps 600] [--views 4] [--rounds 2] [--size 400] [--lattice 256,1024,4096] [--caps 64,128,256]
                                  [--ert 1e-2] [--ert-block 32] [--out FILE]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=600)
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--size', type=int, default=400)
    ap.add_argument('--chunk', type=int, default=32768)
    ap.add_argument('--lattice', default='256,1024,4096')
    ap.add_argument('--caps', default='64,128,256')
    ap.add_argument('--ert', type=float, default=1e-2)
    ap.add_argument('--ert-block', type=int, default=32)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
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
    grid = fastnerf.occupancy.OccupancyGrid.from_network(kte, N=256, bound=1.2, threshold=0., dilate=1, which='both', outside_occupied=False)
    ert = {'ert': a.ert, 'ert_block': a.ert_block}
    variants = [('hierarchical', {}), ('hierarchical+ert', dict(ert))]
    for k in (int(x) for x in a.lattice.split(',')):
        for c in (int(x) for x in a.caps.split(',')):
            variants.append(('march K=%d cap=%d' % (k, c), {'march': k, 'march_cap': c}))
            variants.append(('march K=%d cap=%d +ert' % (k, c), dict(ert, march=k, march_cap=c)))

    def render(c2w, extra):
        return fastnerf.render.render(Hv, Wv, Kv, chunk=a.chunk, c2w=c2w, ndc=False, occupancy=grid, **kw, **extra)[0]

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

    # untimed: the counters of the same views
    net_c, net_f = kte['network_fn'], kte['network_fine']
    stats = {}
    with torch.no_grad():
        for c2w in views:
            ro, rd = fastnerf.run_nerf_helpers.get_rays(Hv, Wv, Kv, c2w)
            rays11 = ops.pack_rays(ro, rd, 2.0, 6.0)
            for name, extra in variants:
                s = stats.setdefault(name, {'evaluated': 0, 'overflow': 0, 'rays': 0})
                for i in range(0, Hv * Wv, a.chunk):
                    r = rays11[i:i + a.chunk].contiguous()
                    if 'march' in extra:
                        o = fastnerf.render._forward_march(r, net_f, extra['march'], extra['march_cap'], False, True, grid, extra.get('ert'),
                                                           extra.get('ert_block', 32), skip_dead_rgb=True)
                        s['evaluated'] += int(o['counts'][0])
                        s['overflow'] += int(o['march_overflow'].sum())
                    elif 'ert' in extra:
                        o = fastnerf.render._forward_ert(r, net_c, net_f, N_SAMPLES, N_IMPORTANCE, False, 0., True, None, None, extra['ert'],
                                                         extra['ert_block'], occupancy=grid, skip_dead_rgb=True)
                        s['evaluated'] += int(o['counts'][0]) + int(o['counts'][2])
                    else:
                        o = fastnerf.render._forward_occ(r, net_c, net_f, N_SAMPLES, N_IMPORTANCE, False, 0., True, None, None, grid,
                                                         skip_dead_rgb=True)
                        s['evaluated'] += int(o['counts'][0]) + int(o['counts'][2])
                    s['rays'] += r.shape[0]
    res = {'tool': 'time_march', 'math': ops.get_math(), 'train_steps': a.steps, 'views': a.views, 'rounds': a.rounds,
           'view_size': [Hv, Wv], 'samples': [N_SAMPLES, N_IMPORTANCE], 'chunk': a.chunk, 'ert': [a.ert, a.ert_block],
           'grid_occupied_fraction': grid.occupied_fraction(), 'variants': {}}
    for name, extra in variants:
        m, s = ms[name], stats[name]
        v = {'ms_per_view': {'mean': float(np.mean(m)), 'min': float(np.min(m)), 'max': float(np.max(m)), 'all': [round(x, 2) for x in m]},
             'psnr': psnr(name), 'evaluated_per_ray': s['evaluated'] / s['rays']}
        if 'march' in extra:
            v['overflow_share'] = s['overflow'] / s['rays']
        res['variants'][name] = v
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
