"""nerf-ours/extract_mesh.py on this package: load a checkpoint through create_nerf, query the fine network's density on the
(N+1)^3 grid over [-bound, bound]^3, run marching cubes at the threshold and write {basedir}/{expname}/lego_mesh.ply.
No mcubes / trimesh: the grid query and marching cubes are HIP kernels (csrc/mesh.hip), the PLY writer is numpy.

  python tools/extract_mesh.py --basedir ./logs --expname lego --N_importance 128 --use_viewdirs [--N 256] [--reference-scale] [--normals]

--reference-scale writes the reference's `vertices / N - .5` instead of world coordinates.  --normals adds per-vertex normals
(nx, ny, nz) from the density field's own gradient at the world-coordinate vertices (fastnerf.mesh.vertex_normals).  Prints the occupied fraction, V
and T, and the grid-query and marching-cubes times (device events, after one warm-up of each) as a JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import fastnerf  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--basedir', default='./logs/')
    p.add_argument('--expname', required=True)
    p.add_argument('--ft_path', default=None, help='checkpoint to load (default: the last *.tar in basedir/expname)')
    p.add_argument('--N_importance', type=int, default=0)
    p.add_argument('--N_samples', type=int, default=64)
    p.add_argument('--use_viewdirs', action='store_true')
    p.add_argument('--netchunk', type=int, default=1024 * 64)
    p.add_argument('--N', type=int, default=256, help='grid cells per axis (N + 1 points)')
    p.add_argument('--bound', type=float, default=1.2)
    p.add_argument('--threshold', type=float, default=50.)
    p.add_argument('--reference-scale', action='store_true', help="write vertices / N - .5 (the reference's scaling)")
    p.add_argument('--normals', action='store_true', help='write per-vertex normals -grad(sigma) / |grad(sigma)| (nx, ny, nz)')
    return p.parse_args(argv)


def timed(fn):
    """fn() once as a warm-up, then once between device events -> (result, ms)."""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def main(argv=None):
    a = parse_args(argv)
    args = fastnerf.run_nerf.make_args(basedir=a.basedir, expname=a.expname, ft_path=a.ft_path, N_importance=a.N_importance,
                                       N_samples=a.N_samples, use_viewdirs=a.use_viewdirs, netchunk=a.netchunk)
    _, kw_test, _, _, _, _ = fastnerf.run_nerf.create_nerf(args)
    if fastnerf.run_nerf.create_nerf.last_ckpt_path is None:
        raise SystemExit('no checkpoint found in %s' % os.path.join(a.basedir, a.expname))
    net = kw_test['network_fine'] if kw_test['network_fine'] is not None else kw_test['network_fn']
    t = torch.linspace(-a.bound, a.bound, a.N + 1, device='cuda')
    vol, ms_grid = timed(lambda: fastnerf.mesh.density_grid(net, t, t, t, network_query_fn=kw_test['network_query_fn'],
                                                            use_viewdirs=a.use_viewdirs))
    (verts, tris), ms_mc = timed(lambda: fastnerf.mesh.marching_cubes(vol, a.threshold))
    scale = (verts / a.N - .5) if a.reference_scale else (-a.bound + verts * (2 * a.bound / a.N))
    path = os.path.join(a.basedir, a.expname, 'lego_mesh.ply')
    normals, ms_normals = None, None
    if a.normals:   # always at the world-coordinate vertices: that is where the network lives
        normals, ms_normals = timed(lambda: fastnerf.mesh.vertex_normals(net, -a.bound + verts * (2 * a.bound / a.N)))
    fastnerf.mesh.export_ply(path, scale, tris, normals)
    print(json.dumps({'checkpoint': fastnerf.run_nerf.create_nerf.last_ckpt_path, 'grid': a.N + 1,
                      'fraction_occupied': float((vol > a.threshold).float().mean()), 'V': int(verts.shape[0]),
                      'T': int(tris.shape[0]), 'density_grid_ms': ms_grid, 'marching_cubes_ms': ms_mc, 'normals_ms': ms_normals,
                      'ply': path}))
    return scale, tris


if __name__ == '__main__':
    main()
