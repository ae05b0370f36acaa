#!/usr/bin/env python3
"""What the environment map costs and what it does: writes profiles/envmap.md (or --out).

a. kernels: ops.env_lookup and ops.env_grad (its three launches: zero, scatter, finish) on two passes at n = 4096 and R = 16, 64, 128,
   and at n = 65 536 with R = 64 -- --reps calls back to back between two HIP events, every output and the scratch allocated before
   (the ops' out-parameters), so a figure is the call-to-call time on a busy stream: the launches and what the host spends between
   them, not a kernel time.
b. steps: the bench-shape step (4096 rays, 64 + 128 samples, bf16x6) with injected colours, step(bkgd=[n,3]) -- the step that exists
   without this feature, the yardstick -- beside Trainer(envmap=EnvMap(64)) on the same rays, on the fused route and on the marched
   route (96 lattice depths in rows of 128 slots through a 64^3 grid that is all occupied inside its box), the two trainers alternated
   in slices of --slice steps; medians over --rounds slices after --warm, and their ratio.
c. behaviour: one short marched run on the synthetic scene in front of an analytic sky s(d) (the RGBA quadrature of the scene
   composited over s(d) on the host side of the step), without the map and with it at three settings (the default guess, a coarse
   table, a slow table): PSNR on a held-out view, of the sky pixels and of the subject's pixels of that view apart, the grid's occupied
   fraction and the share of overflowed rows over the last 50 steps.
--fractions LOG: the lines of a pytest -s log of the environment-map tests that say how much of a bound was reached are copied in.

usage: python tools/time_envmap.py [--part a|b|c|abc] [--reps 200] [--slice 10] [--rounds 8] [--warm 2] [--steps 600] [--fractions LOG]
                                   [--out FILE]"""
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
    for n, R in ((4096, 16), (4096, 64), (4096, 128), (65536, 64)):
        table = torch.rand(R, R, 3, generator=gen).to(dev)
        rays = torch.randn(n, 11, generator=gen).to(dev)
        g1, g0 = ((torch.randn(n, 3, generator=gen) / (3 * n)).to(dev) for _ in range(2))
        a1, a0 = (torch.rand(n, generator=gen).to(dev) for _ in range(2))
        out, d_table = torch.empty(n, 3, device=dev), torch.empty(R, R, 3, device=dev)
        ws = torch.empty(R * R * 3, device=dev, dtype=torch.int64)
        dirs = rays[:, 3:6]      # read in place
        t_look = burst(lambda: ops.env_lookup(table, dirs, out=out), reps)
        t_grad = burst(lambda: ops.env_grad(R, dirs, g1, a1, g0, a0, d_table=d_table, ws=ws), reps)
        rows.append((n, R, t_look, t_grad))
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
        batches.append((ops.gen_rays_pixels(pix, base, K), torch.rand(N_RAYS, 3, generator=gen).to(dev), torch.rand(N_RAYS, 3, generator=gen).to(dev)))
    args = fn.run_nerf.make_args(N_importance=N_IMPORTANCE, N_samples=N_SAMPLES, perturb=1.0, white_bkgd=False, no_reload=True)
    arms = {}
    for name in ('injected', 'envmap'):
        torch.manual_seed(0)
        ktr = fn.run_nerf.create_nerf(args, device=dev)[0]
        kw = {}
        if march:
            kw = dict(occupancy=fn.occupancy.OccupancyGrid.for_training(N=64, bound=1.5, outside_occupied=False, device=dev),
                      occupancy_warmup=10 ** 9, march=96, march_cap=128)
        if name == 'envmap':
            kw['envmap'] = fn.envmap.EnvMap(res=64).to(dev)
        arms[name] = dict(tr=fn.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, **kw), ms=[], it=0)
    for rnd in range(a.warm + a.rounds):
        for name, v in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.slice):
                (ro, rd), tgt, colours = batches[v['it'] % len(batches)]
                v['tr'].step(ro, rd, tgt, **({} if name == 'envmap' else {'bkgd': colours}))
                v['it'] += 1
            e1.record()
            torch.cuda.synchronize()
            if rnd >= a.warm:
                v['ms'].append(e0.elapsed_time(e1) / a.slice)
    return {name: float(np.median(v['ms'])) for name, v in arms.items()}


def sky(d):
    """The analytic sky s(d) [n,3] behind the synthetic scene: smooth in the unit direction, colours in [0.2, 0.95]."""
    u = d / d.norm(dim=-1, keepdim=True)
    return torch.stack([0.55 + 0.35 * u[:, 0], 0.6 + 0.3 * u[:, 1], 0.75 + 0.2 * u[:, 2]], -1)


def scene_rgba(fn, ro, rd, near=2.0, far=6.0, n_quad=128):
    """(premultiplied colour [n,3], alpha [n]) of the analytic scene along rays: synthetic.render_rays' quadrature, the background left off."""
    S = fn.synthetic
    dev, dt_ = ro.device, ro.dtype
    t = torch.linspace(near, far, n_quad, device=dev, dtype=dt_)
    step = (far - near) / (n_quad - 1)
    pts = ro[:, None, :] + rd[:, None, :] * t[None, :, None]
    sig = torch.zeros(pts.shape[:-1], device=dev, dtype=dt_)
    col = torch.zeros(pts.shape, device=dev, dtype=dt_)
    for c, s, d, rgb in S.BLOBS:
        w = d * torch.exp(-((pts - torch.tensor(c, device=dev, dtype=dt_)) ** 2).sum(-1) / (2 * s * s))
        sig = sig + w
        col = col + w[..., None] * torch.tensor(rgb, device=dev, dtype=dt_)
    col = col / (sig[..., None] + 1e-12)
    alpha = 1 - torch.exp(-sig * step * rd.norm(dim=-1, keepdim=True))
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[..., :1]), 1 - alpha + 1e-10], -1), -1)[..., :-1]
    w = alpha * T
    return (w[..., None] * col).sum(-2), w.sum(-1)


def behaviour(fn, dev, n_steps, res=None, lrate=1e-2):
    """One marched run (res None: without the map) -> (PSNR on a held-out view: all pixels, those with alpha < 0.05, those with alpha > 0.5;
    the grid's occupied fraction; the share of overflowed rows over the last 50 steps)."""
    with_map = res is not None
    ops = fn.ops
    ops.set_math('bf16x6')
    H = W = 100
    n_img = 20
    focal = 0.5 * W / np.tan(0.5 * FOV)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    poses = torch.stack([fn.synthetic.pose_spherical(-180.0 + 360.0 * k / n_img, -30.0, 4.0)[:3, :4] for k in range(n_img)], 0).float().to(dev)
    held = fn.synthetic.pose_spherical(-171.0, -30.0, 4.0)[:3, :4].float().to(dev)

    def targets(ro, rd):
        c, a = scene_rgba(fn, ro, rd)
        return (c + (1 - a)[:, None] * sky(rd)).contiguous()
    args = fn.run_nerf.make_args(N_importance=32, N_samples=32, perturb=1.0, white_bkgd=False, no_reload=True)
    torch.manual_seed(0)
    ktr, kte = fn.run_nerf.create_nerf(args, device=dev)[:2]
    grid = fn.occupancy.OccupancyGrid.for_training(N=64, bound=1.5, threshold=0.01, outside_occupied=False, device=dev)
    env = fn.envmap.EnvMap(res=res).to(dev) if with_map else None
    tr = fn.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, lrate=1e-3, occupancy=grid, occupancy_warmup=100, occupancy_every=16, march=96,
                             march_cap=64, march_after=150, **({'envmap': env, 'envmap_lrate': lrate} if with_map else {}))
    gen = torch.Generator().manual_seed(7)
    over = []
    for k in range(n_steps):
        pix = torch.stack([torch.randint(0, n_img, (N_RAYS,), generator=gen), torch.randint(0, H, (N_RAYS,), generator=gen),
                           torch.randint(0, W, (N_RAYS,), generator=gen)], 1).int().to(dev)
        ro, rd = ops.gen_rays_pixels(pix, poses, K)
        _, out = tr.step(ro, rd, targets(ro, rd))
        if k >= n_steps - 50 and 'march_overflow' in out:
            over.append(float(out['march_overflow'].float().mean()))
    with torch.no_grad():
        ro, rd = fn.render.get_rays(H, W, K, held)
        ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
        rb = ops.pack_rays(ro, rd, 2.0, 6.0)
        got = fn.render.render_rays(rb, ktr['network_fn'], None, 32, network_fine=ktr['network_fine'], occupancy=grid, march=96, march_cap=64,
                                    **({'envmap': env} if with_map else {}))['rgb_map']
        err2 = ((got - targets(ro, rd)) ** 2).mean(-1)
        alpha = scene_rgba(fn, ro, rd)[1]
        psnr = [float(-10. * torch.log10(err2[m].mean())) for m in (torch.ones_like(alpha, dtype=torch.bool), alpha < 0.05, alpha > 0.5)]
    return psnr, float(grid.occupied_fraction()), float(np.mean(over)) if over else float('nan')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='abc')
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--slice', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--warm', type=int, default=2)
    ap.add_argument('--steps', type=int, default=600)
    ap.add_argument('--fractions', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'envmap.md'))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import fastnerf as fn
    if not torch.cuda.is_available():
        raise SystemExit('time_envmap.py measures on the GPU: none found')
    dev = torch.device('cuda')
    out = ['# Environment map: launches, kernel times, step times, bounds reached, behaviour', '',
           'Written by `tools/time_envmap.py` on %s.' % torch.cuda.get_device_name(0), '',
           '## The launches the term adds', '',
           'A step with `Trainer(envmap=)` is the step with injected colours, `step(bkgd=[n,3])`, launch for launch, and five launches more:',
           '`env_lookup_kernel` before the step\'s call; `env_zero_kernel`, `env_scatter_kernel` and `env_finish_kernel` (`ops.env_grad`) behind its',
           'forward phase, where the colour gradients stand; `adam_kernel` on the table behind the networks\' update.  The fused and the marched',
           'step are then called in two phase groups (forward | backward + update) instead of one: the same launches in the same order.', '']
    if 'a' in a.part:
        out += ['## The two ops (two passes; us per call, %d calls back to back into buffers allocated before: call-to-call time on a busy '
                'stream, not kernel time)' % a.reps, '',
                '| n | R | env_lookup | env_grad (zero + scatter + finish) |', '|---|---|---|---|']
        out += ['| %d | %d | %.1f | %.1f |' % r for r in kernels(fn, dev, a.reps)] + ['']
    if 'b' in a.part:
        out += ['## The bench-shape step with injected colours and with the map (ms per step, medians of %d slices of %d steps, bf16x6, R = 64)'
                % (a.rounds, a.slice), '', '| route | step(bkgd=[n,3]) | Trainer(envmap=) | ratio |', '|---|---|---|---|']
        for route, march in (('fused', False), ('marched', True)):
            ms = step_arms(fn, dev, a, march)
            out.append('| %s | %.3f | %.3f | %.4f |' % (route, ms['injected'], ms['envmap'], ms['envmap'] / ms['injected']))
        out.append('')
    if a.fractions:
        keep = [ln.strip().lstrip('.') for ln in open(a.fractions) if 'fraction of the bound' in ln or ln.startswith('adjoint') or ln.startswith('EnvMap fit')
                or ln.startswith('env ')]
        out += ['## Bounds reached in the tests (`pytest -s`)', '', '```'] + keep + ['```', '']
    if 'c' in a.part:
        out += ['## Behaviour: the synthetic scene in front of a sky', '',
                '20 views of 100 x 100, targets = the scene\'s RGBA quadrature over the analytic sky s(d) of this tool; %d steps of 4096 rays, 32 + 32'
                % a.steps, 'samples until step 150, then marched (96 depths, rows of 64 slots) through a 64^3 grid (threshold 0.01, refreshed every 16',
                'steps from step 100), lrate 1e-3.  Without the map the step puts nothing behind the rays.  The held-out view lies between two training',
                'views; its PSNR is given over all pixels, over the sky (alpha < 0.05) and over the subject (alpha > 0.5).', '',
                '| run | PSNR all (dB) | sky | subject | occupied fraction of the grid | overflowed rows, last 50 steps |', '|---|---|---|---|---|---|']
        for label, res, lrate in (('without the map', None, 0.), ('`EnvMap(32)`, envmap_lrate 1e-2 (the defaults\' guess)', 32, 1e-2),
                                  ('`EnvMap(8)`, envmap_lrate 1e-2', 8, 1e-2), ('`EnvMap(32)`, envmap_lrate 1e-3', 32, 1e-3)):
            psnr, occ, over = behaviour(fn, dev, a.steps, res, lrate)
            out.append('| %s | %.2f | %.2f | %.2f | %.4f | %.4f |' % ((label,) + tuple(psnr) + (occ, over)))
        out.append('')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(out))
    print('\n'.join(out))


if __name__ == '__main__':
    main()
