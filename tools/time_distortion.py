#!/usr/bin/env python3
"""What the distortion term costs, and what it does to a short marched run: one JSON line.

1. The fused step at the bench shape (4096 rays x (64 + 128) samples, bf16x6, leaf table on, FASTNERF_COMPACT as set: the protocol of
   tools/time_bkgd.py), arms
     parent   a Trainer of the tree under --parent (a checkout of the parent commit, built), without the argument
     off      this tree, a Trainer built without the argument
     zero     this tree, Trainer(lambda_dist=0.)
     on       this tree, Trainer(lambda_dist=--lam)
   every arm in a fresh child process (two trees cannot share one), the arms ALTERNATED --runs times in one job: parent, off, zero, on,
   parent, ...  Per run: ms per step (median / min / max over --rounds slices of --slice steps after --warm slices, HIP events around a
   slice), live_counts of the last step, whether it was compacted, and the final loss2.  Without --parent that arm is left out.
2. `kernels`: fastnerf_distortion alone on [4096, 192] and [4096, 64] weights (l and g_w, as the step calls it) and
   fastnerf_distortion_mean, HIP events around single launches, median of --reps (each figure includes the launch's own latency and the
   allocation of its outputs: an upper bound of the kernel time).
3. `marched`: the scene, batches and shape of tools/time_march_train.py (three solid bodies composited over white, K = 128, cap = 64,
   grid N = 128 with outside_occupied=False, warm-up 256, refresh every 16), one trainer without the term and one with it, from the same
   seeds, alternated in slices of 16 steps: --march-after steps through the grid, then --march-slices marched slices.  Per trainer: ms
   per marched step, evaluated samples per ray, overflowed rays, the occupied fraction of its grid, and the PSNR of a marched render of
   4096 held-out rays.  --no-march skips it.

usage: python tools/time_distortion.py [--parent DIR] [--runs 3] [--rounds 8] [--warm 2] [--slice 10] [--lam 0.01] [--reps 200]
                                       [--march-after 512] [--march-slices 8] [--march-lam 0.01] [--no-march] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS, N_SAMPLES, N_IMPORTANCE = 4096, 64, 128
FOV = 0.6911112070083618


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def stats(ms):
    return {'median': float(np.median(ms)), 'min': float(np.min(ms)), 'max': float(np.max(ms)), 'n': len(ms)}


def camera():
    H = W = 800
    focal = 0.5 * W / np.tan(0.5 * FOV)
    return H, W, np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])


def pixel_batches(ops, synthetic, count, seed, dev):
    H, W, K = camera()
    poses = torch.stack([synthetic.pose_spherical(-180.0 + 3.6 * k, -30.0, 4.0)[:3, :4] for k in range(100)], 0).to(dev)
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(count):
        pix = torch.stack([torch.randint(0, 100, (N_RAYS,), generator=gen), torch.randint(0, H, (N_RAYS,), generator=gen),
                           torch.randint(0, W, (N_RAYS,), generator=gen)], 1).int()
        ro, rd = ops.gen_rays_pixels(pix.to(dev), poses, K)
        tag = torch.stack([pix[:, 0], (pix[:, 1] // 50) * 16 + pix[:, 2] // 50], 1).int().to(dev).contiguous()
        out.append((ro, rd, tag, gen))
    return out


def run_arm(a):
    """One arm in this process, on the tree under a.root -> its JSON on stdout."""
    sys.path.insert(0, a.root)
    import fastnerf
    from fastnerf import ops, synthetic
    dev = torch.device('cuda')
    ops.set_math('bf16x6')
    H, W, K = camera()
    args = fastnerf.run_nerf.make_args(N_importance=N_IMPORTANCE, N_samples=N_SAMPLES, perturb=1.0, white_bkgd=False, no_reload=True,
                                       lrate=5e-4, lrate_decay=500, N_rand=N_RAYS)
    batches = [(ro, rd, torch.rand(N_RAYS, 3, generator=gen).to(dev), tag) for ro, rd, tag, gen in pixel_batches(ops, synthetic, 16, 1000, dev)]
    table = torch.zeros(100 * 256, device=dev, dtype=torch.int32)
    torch.manual_seed(0)
    ktr = fastnerf.run_nerf.create_nerf(args, device=dev)[0]
    kw = {'zero': dict(lambda_dist=0.), 'on': dict(lambda_dist=a.lam)}.get(a.arm, {})
    tr = fastnerf.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500, **kw)
    it, ms, loss2 = 0, [], None
    for rnd in range(a.warm + a.rounds):
        def work():
            nonlocal it, loss2
            for _ in range(a.slice):
                ro, rd, tgt, tag = batches[it % 16]
                loss2, _ = tr.step(ro, rd, tgt, leaf_tag=tag, table=table, max_leaves=256)
                it += 1
        t, _ = timed(work)
        if rnd >= a.warm:
            ms.append(t / a.slice)
    print(json.dumps(dict(arm=a.arm, ms_per_step=stats(ms), live_counts=tr.live_counts.tolist(), last_step_live=bool(tr.last_step_live),
                          loss2=loss2.tolist(), dist_losses=(tr.dist_losses.tolist() if hasattr(tr, 'dist_losses') else None))))


def kernels(ops, dev, reps):
    g = torch.Generator().manual_seed(5)
    rays11 = torch.zeros(N_RAYS, 11, device=dev)
    rays11[:, 6], rays11[:, 7] = 2.0, 6.0
    seq = {}
    for S in (N_SAMPLES + N_IMPORTANCE, N_SAMPLES):
        z = (2.0 + 4.0 * torch.rand(N_RAYS, S, generator=g).sort(dim=1).values).to(dev)
        w = (torch.rand(N_RAYS, S, generator=g) / S).to(dev)
        seq['distortion [4096,%d] l + g_w' % S] = lambda w=w, z=z: ops.distortion(w, z, rays11, coef=1e-3)
    ell = torch.rand(N_RAYS, generator=g).to(dev)
    seq['distortion_mean 2 x [4096]'] = lambda: ops.distortion_mean(ell, ell)
    times = {k: [] for k in seq}
    for rep in range(reps + 10):
        for k, f in seq.items():
            ms, _ = timed(f)
            if rep >= 10:
                times[k].append(ms)
    return {k: {kk: 1e3 * vv if kk != 'n' else vv for kk, vv in stats(t).items()} for k, t in times.items()}


def marched(fastnerf, ops, synthetic, dev, a):
    Kl, C, EVERY, WARMUP = 128, 64, 16, 256
    H, W, K = camera()
    mb = [(ro, rd, synthetic.render_rays(ro, rd, cutoff=1.5).contiguous()) for ro, rd, _, _ in pixel_batches(ops, synthetic, 64, 1000, dev)]
    held = [(ro, rd, synthetic.render_rays(ro, rd, cutoff=1.5).contiguous()) for ro, rd, _, _ in pixel_batches(ops, synthetic, 1, 77, dev)][0]
    args = fastnerf.run_nerf.make_args(N_importance=N_IMPORTANCE, N_samples=N_SAMPLES, perturb=1.0, white_bkgd=True, no_reload=True,
                                       lrate=5e-4, lrate_decay=500, N_rand=N_RAYS)
    mv = {}
    for name, lam in (('without', 0.), ('with', a.march_lam)):
        torch.manual_seed(0)
        ktr = fastnerf.run_nerf.create_nerf(args, device=dev)[0]
        grid = fastnerf.occupancy.OccupancyGrid.for_training(N=128, outside_occupied=False)
        tr = fastnerf.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500, occupancy=grid, occupancy_every=EVERY,
                                       occupancy_warmup=WARMUP, march=Kl, march_cap=C, march_after=a.march_after, lambda_dist=lam)
        mv[name] = dict(tr=tr, ktr=ktr, grid=grid, ms=[], it=0, rng=torch.get_rng_state(), out=None)

    def march_slice(v):
        for _ in range(EVERY):
            ro, rd, tgt = mb[v['it'] % 64]
            _, v['out'] = v['tr'].step(ro, rd, tgt)
            v['it'] += 1

    for s in range(a.march_after // EVERY + 1 + a.march_slices):
        for v in mv.values():
            torch.set_rng_state(v['rng'])
            ms, _ = timed(lambda: march_slice(v))
            v['rng'] = torch.get_rng_state()
            if s > a.march_after // EVERY:
                v['ms'].append(ms / EVERY)
    res = {'K': Kl, 'cap': C, 'march_after': a.march_after, 'lambda_dist': a.march_lam, 'steps': (a.march_after // EVERY + 1 + a.march_slices) * EVERY}
    for name, v in mv.items():
        tr = v['tr']
        net = v['ktr']['network_fine']
        rb = torch.cat([held[0], held[1], torch.full((N_RAYS, 1), 2.0, device=dev), torch.full((N_RAYS, 1), 6.0, device=dev),
                        torch.nn.functional.normalize(held[1], dim=-1)], -1)
        with torch.no_grad():
            img = fastnerf.render.render_rays(rb, v['ktr']['network_fn'], None, N_SAMPLES, N_importance=N_IMPORTANCE, network_fine=net,
                                              white_bkgd=True, occupancy=v['grid'], march=Kl, march_cap=C, retdist=True)
        mse = float(((img['rgb_map'] - held[2]) ** 2).mean())
        res[name] = dict(ms_per_step=stats(v['ms']), evaluated_per_ray=tr.march_counts.tolist()[0] / N_RAYS,
                         overflow_share=float(v['out']['march_overflow'].float().mean()), occupied_fraction=v['grid'].occupied_fraction(),
                         dist_losses=tr.dist_losses.tolist(), heldout_psnr=float(-10.0 * np.log10(mse)),
                         heldout_mean_distortion=float(img['dist_map'].mean()), live_counts=tr.live_counts.tolist())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--warm', type=int, default=2)
    ap.add_argument('--slice', type=int, default=10)
    ap.add_argument('--lam', type=float, default=0.01)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--march-after', type=int, default=512)
    ap.add_argument('--march-slices', type=int, default=8)
    ap.add_argument('--march-lam', type=float, default=0.01)
    ap.add_argument('--no-march', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--arm', default=None, help=argparse.SUPPRESS)      # (a child process: one arm on the tree under --root)
    ap.add_argument('--root', default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.arm:
        return run_arm(a)
    arms = ([('parent', os.path.abspath(a.parent))] if a.parent else []) + [('off', ROOT), ('zero', ROOT), ('on', ROOT)]
    res = {'tool': 'time_distortion', 'rays': N_RAYS, 'samples': [N_SAMPLES, N_IMPORTANCE], 'slice': a.slice, 'rounds': a.rounds,
           'warm_rounds': a.warm, 'lambda_dist': a.lam, 'fused': {name: [] for name, _ in arms}}
    for run in range(a.runs):
        for name, root in arms:
            cmd = [sys.executable, os.path.abspath(__file__), '--arm', name, '--root', root, '--rounds', str(a.rounds), '--warm', str(a.warm),
                   '--slice', str(a.slice), '--lam', str(a.lam)]
            p = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-4000:])
                raise SystemExit('arm %s failed with status %d: nothing further is started' % (name, p.returncode))
            res['fused'][name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print('run %d %-6s %.4f ms / step' % (run, name, res['fused'][name][-1]['ms_per_step']['median']), file=sys.stderr, flush=True)
    sys.path.insert(0, ROOT)
    import fastnerf
    from fastnerf import ops, synthetic
    dev = torch.device('cuda')
    ops.set_math('bf16x6')
    res['math'], res['compact'] = ops.get_math(), fastnerf.render.get_compact()
    res['kernels_us'] = kernels(ops, dev, a.reps)
    res['kernels_note'] = 'single launches between two HIP events, allocation of the outputs included: an upper bound of the kernel time'
    if not a.no_march:
        res['marched'] = marched(fastnerf, ops, synthetic, dev, a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
