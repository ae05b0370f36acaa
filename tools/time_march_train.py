"""Marched training beside training through the grid, on the solid-body scene: one JSON line.

The scene and the batches of tools/time_occupancy_train.py (three solid bodies, density zero beyond 1.5 sigma, 4096 rays per step, white
background).  Variants, every one from the same seeds and on a grid of its own (OccupancyGrid.for_training(N=128,
outside_occupied=False), warm-up 256 steps, a refresh every 16):
  grid           Trainer(occupancy=grid): 64 + 128 samples, two networks -- the step of the parent commit
  march K/cap    the same trainer with march=K, march_cap=cap, march_after=--march-after: from then on one network on the jittered lattice
ALL variants alternate inside one process: training advances in slices of 16 steps (one refresh each), and in every slice every variant
runs its 16 steps once, HIP events around them -- drift of the machine spreads over all of them.  Per variant: ms per step of the
slices after --march-after (mean / min / max / median), the cumulated training time, for the marched ones the evaluated samples per
ray (march_counts) and the overflow share at the end of every slice, and PSNR on held-out views every --eval-every steps (the grid
variant rendered hierarchically through its grid, a marched variant with render(march=K, march_cap=cap) through its own), which gives
PSNR at equal steps; `psnr_at_equal_time` interpolates every curve at the training time of the fastest variant's last checkpoint.
`kernels`: the entry points of ONE marched step (K, cap of the first marched variant, its state after training) called one by one
through ops, HIP events around each, median of 5 -- the launches fastnerf_train_step_march makes.

usage: python tools/time_march_train.py [--steps 1200] [--march-after 512] [--eval-every 400] [--views 2] [--size 200]
                                        [--lattice 128,256] [--caps 64,128] [--out FILE]"""
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
EVERY, WARMUP = 16, 256


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=1200)
    ap.add_argument('--march-after', type=int, default=512)
    ap.add_argument('--eval-every', type=int, default=400)
    ap.add_argument('--views', type=int, default=2)
    ap.add_argument('--size', type=int, default=200)
    ap.add_argument('--chunk', type=int, default=32768)
    ap.add_argument('--lattice', default='128,256')
    ap.add_argument('--caps', default='64,128')
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
    gen = torch.Generator().manual_seed(1000)
    batches = []
    for _ in range(64):
        pix = torch.stack([torch.randint(0, 100, (N_RAYS,), generator=gen), torch.randint(0, H, (N_RAYS,), generator=gen),
                           torch.randint(0, W, (N_RAYS,), generator=gen)], 1).int()
        ro, rd = ops.gen_rays_pixels(pix.to(dev), poses, K)
        batches.append((ro, rd, synthetic.render_rays(ro, rd, cutoff=CUTOFF).contiguous()))

    Hv = Wv = a.size
    fv = 0.5 * Wv / np.tan(0.5 * FOV)
    Kv = np.array([[fv, 0, 0.5 * Wv], [0, fv, 0.5 * Hv], [0, 0, 1]])
    views = [synthetic.pose_spherical(-180.0 + 360.0 * (k + 0.5) / a.views + 1.8, -20.0, 4.0)[:3, :4].to(dev) for k in range(a.views)]
    gts = []
    for c2w in views:
        ro, rd = fastnerf.run_nerf_helpers.get_rays(Hv, Wv, Kv, c2w)
        gts.append(torch.cat([synthetic.render_rays(ro.reshape(-1, 3)[i:i + 65536].contiguous(), rd.reshape(-1, 3)[i:i + 65536].contiguous(),
                                                    cutoff=CUTOFF) for i in range(0, Hv * Wv, 65536)], 0).reshape(Hv, Wv, 3))

    names = ['grid'] + ['march K=%d cap=%d' % (k, c) for k in (int(x) for x in a.lattice.split(',')) for c in (int(x) for x in a.caps.split(','))]
    var = {}
    for name in names:
        torch.manual_seed(0)
        ktr, kte, _, _, _, _ = fastnerf.run_nerf.create_nerf(args, device=dev)
        grid = fastnerf.occupancy.OccupancyGrid.for_training(N=128, outside_occupied=False)
        extra = {}
        if name != 'grid':
            k, c = (int(x.split('=')[1]) for x in name.split()[1:])
            extra = dict(march=k, march_cap=c, march_after=a.march_after)
        tr = fastnerf.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500, occupancy=grid, occupancy_every=EVERY,
                                       occupancy_warmup=WARMUP, **extra)
        var[name] = dict(tr=tr, kte=kte, grid=grid, extra=extra, ms=[], train_ms=0.0, curve=[], evaluated=[], overflow=[],
                         rng=torch.get_rng_state())

    def psnr(v):
        kw = dict(v['kte'], near=2.0, far=6.0)
        kw.pop('ndc', None)
        rx = {k: v['extra'][k] for k in ('march', 'march_cap') if k in v['extra']}
        with torch.no_grad():
            imgs = [fastnerf.render.render(Hv, Wv, Kv, chunk=a.chunk, c2w=c2w, ndc=False, occupancy=v['grid'], **kw, **rx)[0] for c2w in views]
        return float(np.mean([-10.0 * np.log10(float(((i - g) ** 2).mean())) for i, g in zip(imgs, gts)]))

    def slice_of(v, s0):
        for it in range(EVERY):
            _, out = v['tr'].step(*batches[(s0 + it) % 64])
        return out

    steps = a.steps - a.steps % EVERY
    for s0 in range(0, steps, EVERY):
        for name in names:
            v = var[name]
            torch.set_rng_state(v['rng'])      # every variant draws its seeds from a stream of its own
            ms, out = timed(lambda: slice_of(v, s0))
            v['rng'] = torch.get_rng_state()
            v['train_ms'] += ms
            if s0 >= a.march_after:
                v['ms'].append(ms / EVERY)
                if 'march_overflow' in out:
                    v['evaluated'].append(v['tr'].march_counts.tolist()[0] / N_RAYS)
                    v['overflow'].append(float(out['march_overflow'].float().mean()))
            if (s0 + EVERY) % a.eval_every == 0 or s0 + EVERY == steps:
                v['curve'].append([s0 + EVERY, v['train_ms'], psnr(v)])

    t_equal = min(v['curve'][-1][1] for v in var.values())
    res = {'tool': 'time_march_train', 'math': ops.get_math(), 'rays': N_RAYS, 'samples': [N_SAMPLES, N_IMPORTANCE], 'steps': steps,
           'march_after': a.march_after, 'every': EVERY, 'warmup': WARMUP, 'views': a.views, 'view_size': [Hv, Wv],
           'scene': 'three solid bodies, density zero beyond %.1f sigma' % CUTOFF, 'equal_time_ms': t_equal, 'variants': {}}
    for name in names:
        v = var[name]
        m = v['ms']
        t, p = [c[1] for c in v['curve']], [c[2] for c in v['curve']]
        r = {'ms_per_step': {'mean': float(np.mean(m)), 'min': float(np.min(m)), 'max': float(np.max(m)), 'median': float(np.median(m)),
                             'slices': len(m)},
             'train_ms': v['train_ms'], 'curve_step_ms_psnr': v['curve'], 'psnr_at_equal_time': float(np.interp(t_equal, t, p)),
             'grid_occupied_fraction': v['grid'].occupied_fraction()}
        if v['evaluated']:
            e, o = v['evaluated'], v['overflow']
            r['evaluated_per_ray'] = {'first': e[0], 'last': e[-1], 'mean': float(np.mean(e)), 'max': float(np.max(e))}
            r['overflow_share'] = {'first': o[0], 'last': o[-1], 'mean': float(np.mean(o)), 'max': float(np.max(o))}
        else:
            occ = v['tr'].occupancy_counts.tolist()
            r['occupied_per_ray'] = (occ[0] + occ[2]) / N_RAYS
        res['variants'][name] = r

    # the entry points of one marched step, one by one (the launches of fastnerf_train_step_march), on the first marched variant
    first = [n for n in names if n != 'grid']
    if first:
        v = var[first[0]]
        tr, grid = v['tr'], v['grid']
        Kl, C = v['extra']['march'], v['extra']['march_cap']
        which, net, pk = tr._marched()
        Nn = ops.NET_PARAMS
        sl = slice(which * Nn, (which + 1) * Nn)
        ro, rd, tgt = batches[0]
        n, P = N_RAYS, N_RAYS * C
        params, grad, m_, v_ = tr.flat[sl].clone(), torch.empty(Nn, device=dev), tr.m[sl].clone(), tr.v[sl].clone()
        pf, pb = ops.mlp_pack(params)
        raw = torch.empty(n, C, 4, device=dev)
        cnts = torch.zeros(2, device=dev, dtype=torch.int32)
        ws, draw = torch.empty(ops.dact_floats(P), device=dev), torch.empty(n, C, 4, device=dev)
        act, partial = torch.empty(ops.act_floats(P), device=dev), torch.empty(ops.mlp_bwd_partial_floats(), device=dev)
        st = {}
        seq = [
            ('fastnerf_pack_rays', lambda: st.update(r11=ops.pack_rays(ro, rd, 2.0, 6.0))),
            ('fastnerf_occ_march_jitter', lambda: st.update(m=ops.occ_march_jitter(grid._c, st['r11'], Kl, C, seed=12345))),
            ('fastnerf_march_list', lambda: st.update(l=ops.march_list(st['m'][1], 0, C, raw=raw, total=cnts, lattice=n * Kl))),
            ('fastnerf_mlp_*_fwd_list', lambda: ops.mlp_fwd_list(st['r11'], st['m'][0], params, pf, raw, st['l'][0], st['l'][1], flags=1)),
            ('fastnerf_raw2outputs_fwd', lambda: st.update(o=ops.raw2outputs_fwd(raw, st['m'][0], st['r11'], None, True))),
            ('fastnerf_mse_leafmax', lambda: st.update(g=ops.mse_leafmax(st['o'][0], None, tgt)[1])),
            ('fastnerf_march_mask', lambda: ops.march_mask(st['m'][2], st['g'])),
            ('fastnerf_raw2outputs_bwd', lambda: ops.raw2outputs_bwd(raw, st['m'][0], st['r11'], st['g'], None, True, draw=draw)),
            ('fastnerf_compact_live', lambda: st.update(c=ops.compact_live(draw))),
            ('fastnerf_mlp_*_fwd_live', lambda: ops.mlp_fwd_live(st['r11'], st['m'][0], params, pf, act, st['c'][0], st['c'][1])),
            ('fastnerf_mlp_*_bwd_live', lambda: ops.mlp_bwd_live(draw, act, params, pb, ws, partial, grad, st['c'][0], st['c'][1])),
            ('fastnerf_adam_step', lambda: ops.adam_step(params, grad, m_, v_, 5e-4, tr.adam_t)),
            ('pack', lambda: ops.mlp_pack(params, pf, pb)),
        ]
        times = {nm: [] for nm, _ in seq}
        for rep in range(6):
            for nm, f in seq:
                ms, _ = timed(f)
                if rep:      # the first round warms up
                    times[nm].append(ms)
        med = {nm: float(np.median(t)) for nm, t in times.items()}
        res['kernels'] = {'variant': first[0], 'ms_median_of_5': med, 'sum_ms': float(sum(med.values())),
                          'evaluated_per_ray': int(cnts[0]) / n, 'live_per_ray': int(st['c'][1][0]) / n}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
