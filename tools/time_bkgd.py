#!/usr/bin/env python3
"""What per-ray background colours cost: one JSON line.

Fused step at the bench shape (4096 rays x (64 + 128) samples, bf16x6, leaf table on, FASTNERF_COMPACT as set: the protocol of
tools/time_step_sizes.py), variants
  none | const | const+alpha | random | random+alpha        Trainer(bkgd=None / (0.2, 0.5, 0.8) / 'random'), step(alpha=) or not
every one a trainer of its own from the same seeds, ALL alternated inside one process: in every round every variant runs --slice
steps once, HIP events around them, so drift of the machine spreads over all of them.  Per variant: ms per step (median / min / max
over the rounds after the warm-up rounds), live_counts of its last step and whether that step was compacted.
`kernels`: fastnerf_bkgd_blend and fastnerf_bkgd_grad alone on the maps of 4096 rays (two passes), and fastnerf_aux_loss beside them,
median of --reps launches each, HIP events around single launches (so each figure includes the launch's own latency).
Marched step at the shape of tools/time_march_train.py (its scene and batches, K = 128, cap = 64, grid N = 128 with
outside_occupied=False, warm-up 256, refresh every 16): `none` -- that tool's trainer, white_bkgd=True, the colour its targets were
composited over -- and `random+alpha` (white_bkgd=False) trained --march-after steps through the grid, then alternated in slices of 16
marched steps.  --no-march skips it.  (The fused variants above all run with white_bkgd=False: `none` there composites over black.)

usage: python tools/time_bkgd.py [--rounds 12] [--warm 2] [--slice 10] [--reps 200] [--march-after 512] [--march-slices 8] [--no-march]
                                 [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS, N_SAMPLES, N_IMPORTANCE = 4096, 64, 128
FOV = 0.6911112070083618
COLOUR = (0.2, 0.5, 0.8)
VARIANTS = [('none', None, False), ('const', COLOUR, False), ('const+alpha', COLOUR, True), ('random', 'random', False),
            ('random+alpha', 'random', True)]


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def stats(ms):
    return {'median': float(np.median(ms)), 'min': float(np.min(ms)), 'max': float(np.max(ms)), 'n': len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=12)
    ap.add_argument('--warm', type=int, default=2)
    ap.add_argument('--slice', type=int, default=10)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--march-after', type=int, default=512)
    ap.add_argument('--march-slices', type=int, default=8)
    ap.add_argument('--no-march', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import fastnerf
    from fastnerf import ops, synthetic
    dev = torch.device('cuda')
    ops.set_math('bf16x6')
    H = W = 800
    focal = 0.5 * W / np.tan(0.5 * FOV)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    poses = torch.stack([synthetic.pose_spherical(-180.0 + 3.6 * k, -30.0, 4.0)[:3, :4] for k in range(100)], 0).to(dev)
    args = fastnerf.run_nerf.make_args(N_importance=N_IMPORTANCE, N_samples=N_SAMPLES, perturb=1.0, white_bkgd=False, no_reload=True,
                                       lrate=5e-4, lrate_decay=500, N_rand=N_RAYS)
    gen = torch.Generator().manual_seed(1000)
    batches = []
    for _ in range(16):
        pix = torch.stack([torch.randint(0, 100, (N_RAYS,), generator=gen), torch.randint(0, H, (N_RAYS,), generator=gen),
                           torch.randint(0, W, (N_RAYS,), generator=gen)], 1).int()
        ro, rd = ops.gen_rays_pixels(pix.to(dev), poses, K)
        tag = torch.stack([pix[:, 0], (pix[:, 1] // 50) * 16 + pix[:, 2] // 50], 1).int().to(dev).contiguous()
        alpha = (torch.rand(N_RAYS, generator=gen) > 0.5).float() * torch.rand(N_RAYS, generator=gen).clamp(0.5, 1.0)
        batches.append((ro, rd, torch.rand(N_RAYS, 3, generator=gen).to(dev), tag, alpha.to(dev)))
    table = torch.zeros(100 * 256, device=dev, dtype=torch.int32)

    res = {'tool': 'time_bkgd', 'fused_white_bkgd': False, 'math': ops.get_math(), 'compact': fastnerf.render.get_compact(), 'rays': N_RAYS,
           'samples': [N_SAMPLES, N_IMPORTANCE], 'slice': a.slice, 'rounds': a.rounds, 'warm_rounds': a.warm, 'fused': {}}
    var = {}
    for name, setting, use_alpha in VARIANTS:
        torch.manual_seed(0)
        ktr = fastnerf.run_nerf.create_nerf(args, device=dev)[0]
        tr = fastnerf.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500, bkgd=setting)
        var[name] = dict(tr=tr, alpha=use_alpha, ms=[], it=0, rng=torch.get_rng_state())

    def fused_slice(v):
        for _ in range(a.slice):
            ro, rd, tgt, tag, alpha = batches[v['it'] % 16]
            v['tr'].step(ro, rd, tgt, leaf_tag=tag, table=table, max_leaves=256, **({'alpha': alpha} if v['alpha'] else {}))
            v['it'] += 1

    for rnd in range(a.warm + a.rounds):
        for name, _, _ in VARIANTS:
            v = var[name]
            torch.set_rng_state(v['rng'])      # every variant draws its seeds from a stream of its own
            ms, _ = timed(lambda: fused_slice(v))
            v['rng'] = torch.get_rng_state()
            if rnd >= a.warm:
                v['ms'].append(ms / a.slice)
    for name, _, _ in VARIANTS:
        v = var[name]
        res['fused'][name] = dict(ms_per_step=stats(v['ms']), live_counts=v['tr'].live_counts.tolist(), last_step_live=bool(v['tr'].last_step_live))
    base = res['fused']['none']['ms_per_step']['median']
    for name in res['fused']:
        res['fused'][name]['delta_us_vs_none'] = 1e3 * (res['fused'][name]['ms_per_step']['median'] - base)
    res['fused_none_spread_us'] = 1e3 * (res['fused']['none']['ms_per_step']['max'] - res['fused']['none']['ms_per_step']['min'])
    del var

    # the two launches alone, and fastnerf_aux_loss beside them
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.rand(*s, generator=g).to(dev)      # noqa: E731
    rgb1, rgb0, acc1, acc0, tgt, alpha, colours = r(N_RAYS, 3), r(N_RAYS, 3), r(N_RAYS), r(N_RAYS), r(N_RAYS, 3), r(N_RAYS), r(N_RAYS, 3)
    g1, g0, depth = r(N_RAYS, 3), r(N_RAYS, 3), 2 + 4 * r(N_RAYS)
    seq = {
        'bkgd_blend injected+alpha': lambda: ops.bkgd_blend(rgb1, acc1, tgt, bkgd=colours, alpha=alpha, rgb0=rgb0, acc0=acc0),
        'bkgd_blend drawn+alpha': lambda: ops.bkgd_blend(rgb1, acc1, tgt, seed=12345, alpha=alpha, rgb0=rgb0, acc0=acc0),
        'bkgd_blend drawn': lambda: ops.bkgd_blend(rgb1, acc1, tgt, seed=12345, rgb0=rgb0, acc0=acc0),
        'bkgd_grad': lambda: ops.bkgd_grad(colours, g1, g0),
        'bkgd_grad+add': lambda: ops.bkgd_grad(colours, g1, g0, add=acc1, add0=acc0),
        'aux_loss depth+acc': lambda: ops.aux_loss(depth, acc1, depth, acc0, depth_target=depth, acc_target=alpha, lambda_depth=0.1, lambda_acc=0.1),
    }
    times = {k: [] for k in seq}
    for rep in range(a.reps + 10):
        for k, f in seq.items():
            ms, _ = timed(f)
            if rep >= 10:
                times[k].append(ms)
    res['kernels_us'] = {k: {kk: 1e3 * vv if kk != 'n' else vv for kk, vv in stats(t).items()} for k, t in times.items()}
    res['kernels_note'] = 'single launches between two HIP events, allocation of the outputs included: an upper bound of the kernel time'

    if not a.no_march:
        Kl, C, EVERY, WARMUP = 128, 64, 16, 256
        mb = []
        gen = torch.Generator().manual_seed(1000)
        for _ in range(64):
            pix = torch.stack([torch.randint(0, 100, (N_RAYS,), generator=gen), torch.randint(0, H, (N_RAYS,), generator=gen),
                               torch.randint(0, W, (N_RAYS,), generator=gen)], 1).int()
            ro, rd = ops.gen_rays_pixels(pix.to(dev), poses, K)
            t = synthetic.render_rays(ro, rd, cutoff=1.5).contiguous()
            # (the synthetic scene has no alpha channel: opaque where it is not white, for the timing's sake)
            mb.append((ro, rd, t, ((t - 1).abs().sum(-1) > 1e-3).float().contiguous()))
        mv = {}
        # `none` is the trainer of tools/time_march_train.py: white_bkgd=True, the fixed colour that the targets were composited over
        args_white = fastnerf.run_nerf.make_args(N_importance=N_IMPORTANCE, N_samples=N_SAMPLES, perturb=1.0, white_bkgd=True, no_reload=True,
                                                 lrate=5e-4, lrate_decay=500, N_rand=N_RAYS)
        for name, setting, use_alpha in (VARIANTS[0], VARIANTS[4]):
            torch.manual_seed(0)
            ktr = fastnerf.run_nerf.create_nerf(args_white if setting is None else args, device=dev)[0]
            grid = fastnerf.occupancy.OccupancyGrid.for_training(N=128, outside_occupied=False)
            tr = fastnerf.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500, occupancy=grid, occupancy_every=EVERY,
                                           occupancy_warmup=WARMUP, march=Kl, march_cap=C, march_after=a.march_after, bkgd=setting)
            mv[name] = dict(tr=tr, alpha=use_alpha, ms=[], it=0, rng=torch.get_rng_state(), out=None)

        def march_slice(v):
            for _ in range(EVERY):
                ro, rd, tgt, alpha = mb[v['it'] % 64]
                _, v['out'] = v['tr'].step(ro, rd, tgt, **({'alpha': alpha} if v['alpha'] else {}))
                v['it'] += 1

        for s in range(a.march_after // EVERY + 1 + a.march_slices):
            for name, v in mv.items():
                torch.set_rng_state(v['rng'])
                ms, _ = timed(lambda: march_slice(v))
                v['rng'] = torch.get_rng_state()
                if s > a.march_after // EVERY:
                    v['ms'].append(ms / EVERY)
        res['marched'] = {'K': Kl, 'cap': C, 'march_after': a.march_after}
        for name, v in mv.items():
            res['marched'][name] = dict(white_bkgd=bool(v['tr'].white_bkgd), ms_per_step=stats(v['ms']), evaluated_per_ray=v['tr'].march_counts.tolist()[0] / N_RAYS,
                                        overflow_share=float(v['out']['march_overflow'].float().mean()),
                                        live_counts=v['tr'].live_counts.tolist())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
