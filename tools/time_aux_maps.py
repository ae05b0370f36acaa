#!/usr/bin/env python3
"""What depth / opacity supervision costs at the bench shape (4096 rays x (64 + 128) samples, bf16x6, plain backward, leaf table on: the
protocol of tools/time_step_sizes.py), and that the step without targets costs what it cost before.
  python tools/time_aux_maps.py [PARENT_TREE]
Runs alternate, each in a process of its own (a library is loaded once per process), three per arm:
  parent   the step of a checkout of the parent commit, built in place, at PARENT_TREE (skipped when not given)
  branch   the step of this tree without targets (the same launches)
  aux      the step of this tree with both terms on (sparse depth: 30 % of the rays without a target)
Prints ms / step per run (HIP events around 100 steps after 10 warm-up steps), then each arm's range and median.
`python tools/time_aux_maps.py --worker TREE ARM` is one such run alone, e.g. under a kernel profiler."""
import os
import statistics
import subprocess
import sys

NS, NI, N = 64, 128, 4096
H = W = 800
WARM, STEPS = 10, 100


def worker(root, arm):
    import numpy as np
    import torch
    sys.path.insert(0, root)
    import fastnerf
    from fastnerf import ops, synthetic
    focal = 0.5 * W / np.tan(0.5 * 0.6911112070083618)
    dev = torch.device('cuda')
    ops.set_math('bf16x6')
    fastnerf.render.set_compact('0')
    args = fastnerf.run_nerf.make_args(N_importance=NI, N_samples=NS, perturb=1.0, white_bkgd=True, no_reload=True, lrate=5e-4,
                                       lrate_decay=500, N_rand=N)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    poses = torch.stack([synthetic.pose_spherical(-180.0 + 3.6 * k, -30.0, 4.0)[:3, :4] for k in range(100)], 0).to(dev)
    gen = torch.Generator().manual_seed(1000)
    batches = []
    for _ in range(16):
        pix = torch.stack([torch.randint(0, 100, (N,), generator=gen), torch.randint(0, H, (N,), generator=gen),
                           torch.randint(0, W, (N,), generator=gen)], 1).int()
        ro, rd = ops.gen_rays_pixels(pix.to(dev), poses, K)
        tag = torch.stack([pix[:, 0], (pix[:, 1] // 50) * 16 + pix[:, 2] // 50], 1).int().to(dev).contiguous()
        depth = 2 + 4 * torch.rand(N, generator=gen)
        dw = (torch.rand(N, generator=gen) > 0.3).float()
        depth[dw == 0] = float('nan')
        aux = dict(depth=depth.to(dev), depth_weight=dw.to(dev), acc=(torch.rand(N, generator=gen) > 0.4).float().to(dev))
        batches.append((ro, rd, torch.rand(N, 3, generator=gen).to(dev), tag, aux))
    torch.manual_seed(0)
    ktr = fastnerf.run_nerf.create_nerf(args, device=dev)[0]
    kw = dict(lambda_depth=0.1, lambda_acc=0.1) if arm == 'aux' else {}
    tr = fastnerf.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500, **kw)
    table = torch.zeros(100 * 256, device=dev, dtype=torch.int32)

    def step(i):
        ro, rd, tgt, tag, aux = batches[i % 16]
        return tr.step(ro, rd, tgt, leaf_tag=tag, table=table, max_leaves=256, **(aux if arm == 'aux' else {}))
    for i in range(WARM):
        step(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(STEPS):
        loss2, _ = step(WARM + i)
    e1.record()
    torch.cuda.synchronize()
    print('MS_PER_STEP %.4f loss2 %s aux %s' % (e0.elapsed_time(e1) / STEPS, loss2.tolist(),
                                                tr.aux_losses.tolist() if arm == 'aux' else None), flush=True)


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    parent = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else None
    arms = ([('parent', parent)] if parent else []) + [('branch', here), ('aux', here)]
    ms = {a: [] for a, _ in arms}
    for rnd in range(3):
        for arm, root in arms:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', root, arm], stdout=subprocess.PIPE,
                                 stderr=subprocess.STDOUT, timeout=240, check=True).stdout.decode()
            line = [ln for ln in out.splitlines() if ln.startswith('MS_PER_STEP')][-1]
            ms[arm].append(float(line.split()[1]))
            print('round %d  %-6s %s' % (rnd, arm, line), flush=True)
    for arm, v in ms.items():
        print('%-6s min %.4f  median %.4f  max %.4f ms/step' % (arm, min(v), statistics.median(v), max(v)))
    if parent:
        print('branch median - parent median = %+.4f ms (parent range %.4f)' % (
            statistics.median(ms['branch']) - statistics.median(ms['parent']), max(ms['parent']) - min(ms['parent'])))
    print('aux median - branch median = %+.4f ms = %+.2f %% of the step' % (
        statistics.median(ms['aux']) - statistics.median(ms['branch']),
        100 * (statistics.median(ms['aux']) - statistics.median(ms['branch'])) / statistics.median(ms['branch'])))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--worker':
        worker(sys.argv[2], sys.argv[3])
    else:
        main()
