"""What the density gradient costs: one JSON line per math mode.

On --points points (default 2^20) drawn uniformly in [-1.2, 1.2]^3 of a seeded default-init NeRF, in chunks of --chunk, HIP events
around each of (one warm-up pass first, then the median of --reps passes):
  density_gradient   NeRF.density_gradient: what a caller pays, the torch glue around the chunks included
  sigma_grad         ops.mlp_sigma_grad on the same chunks with a caller-owned workspace: saving forward + cotangent fill + dX
                     chain + sigma_grad_kernel, nothing else
  saving_forward     ops.mlp_fwd with `act` on the same chunks: the forward that the call starts with, alone
The dX chain has no entry point of its own to time from here; sigma_grad - saving_forward is the chain plus the new kernel.  Their
split, the new kernel's share, comes from a kernel trace of this very script:
  rocprofv3 --kernel-trace --stats -- python tools/time_sigma_grad.py --modes bf16x6
(mlp_bwd_dx_kernel / mlp_bwd_dx_bf16_kernel against sigma_grad_kernel in the stats table).  No figure here is a pass / fail
condition; profiles/sigma_grad.md records a run.

usage: python tools/time_sigma_grad.py [--points 1048576] [--chunk 65536] [--reps 5] [--modes fp32,bf16x3,bf16x6]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    """Median milliseconds of fn() over `reps` runs between device events, after one warm-up."""
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=1 << 20)
    ap.add_argument('--chunk', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--modes', default='fp32,bf16x3,bf16x6')
    a = ap.parse_args()
    import fastnerf
    from fastnerf import ops
    torch.manual_seed(0)
    net = fastnerf.model.NeRF()
    P, n0 = a.points, min(a.chunk, a.points)
    pts = torch.rand(P, 3, device='cuda') * 2.4 - 1.2
    rays = torch.zeros(P, 11, device='cuda')
    rays[:, 0:3] = pts
    z = torch.zeros(P, 1, device='cuda')
    for mode in a.modes.split(','):
        ops.set_math(mode)
        pf, pb = net.packed()
        ws = torch.empty(ops.sigma_grad_ws_floats(n0), device='cuda')
        grad = torch.empty(P, 3, device='cuda')
        raw = torch.empty(n0, 1, 4, device='cuda')
        chunks = [(p0, min(n0, P - p0)) for p0 in range(0, P, n0)]

        def kernels():
            for p0, n in chunks:
                ops.mlp_sigma_grad(rays[p0:p0 + n], z[p0:p0 + n], net.flat, pf, pb, ws=ws, grad=grad[p0:p0 + n], want_sigma=False)

        def forward():
            for p0, n in chunks:
                ops.mlp_fwd(rays[p0:p0 + n], z[p0:p0 + n], net.flat, pf, act=ws, raw=raw[:n])

        ms_all = timed(lambda: net.density_gradient(pts, chunk=n0), a.reps)
        ms_k = timed(kernels, a.reps)
        ms_f = timed(forward, a.reps)
        print(json.dumps({'mode': mode, 'points': P, 'chunk': n0, 'density_gradient_ms': round(ms_all, 3), 'sigma_grad_ms': round(ms_k, 3),
                          'saving_forward_ms': round(ms_f, 3), 'dx_chain_plus_new_kernel_ms': round(ms_k - ms_f, 3),
                          'ns_per_point': round(ms_k * 1e6 / P, 2)}), flush=True)
        del ws, grad, raw


if __name__ == '__main__':
    main()
