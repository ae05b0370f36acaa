"""Mesh extraction -- what nerf-ours/extract_mesh.py does (:38-86), without mcubes or trimesh.

density_grid    the fine network's relu(sigma) on a dense point grid (extract_mesh.py:38-61); a fastnerf NeRF runs the
                fused HIP forward chunk by chunk, with the points written straight into its ray rows (csrc/mesh.hip)
marching_cubes  mcubes.marching_cubes (extract_mesh.py:74) as four HIP passes (csrc/mesh.hip); vertices in index coordinates
extract_mesh    both, from a create_nerf render_kwargs, vertices in world coordinates; optionally with per-vertex normals
vertex_normals  -grad(sigma) / |grad(sigma)| of the density field at given points (csrc/sigma_grad.hip)
export_ply      trimesh's .ply export (extract_mesh.py:82-86): binary little-endian PLY, numpy only"""
import numpy as np
import torch

from . import ops
from .model import NeRF


def density_grid(network, xs, ys, zs, chunk=1024 * 64, network_query_fn=None, use_viewdirs=None):
    """[len(xs), len(ys), len(zs)] float32 grid of relu(raw[..., 3]) at the points (xs[i], ys[j], zs[k]) on the GPU.

    A fastnerf NeRF takes the fused forward (view directions 0, as extract_mesh.py:57 passes them; they do not reach sigma).
    Any other network goes through `network_query_fn(pts [n,1,3], viewdirs [n,3] or None, network)` in chunks, as the
    reference's loop does; `use_viewdirs` (default: the network's attribute, else True) decides whether zeros or None are passed."""
    xs, ys, zs = [torch.as_tensor(t, dtype=torch.float32).reshape(-1) for t in (xs, ys, zs)]
    dev = xs.device if xs.is_cuda else torch.device('cuda')
    xs, ys, zs = [t.to(dev).contiguous() for t in (xs, ys, zs)]
    ops.require_gpu(xs)
    P = xs.numel() * ys.numel() * zs.numel()
    vol = torch.empty(P, device=dev, dtype=torch.float32)
    if P == 0:
        return vol.reshape(xs.numel(), ys.numel(), zs.numel())
    net = getattr(network, 'module', network)
    n0 = min(int(chunk), P)
    rays11 = torch.empty(n0, 11, device=dev, dtype=torch.float32)
    if isinstance(net, NeRF):
        z = torch.zeros(n0, 1, device=dev, dtype=torch.float32)
        raw = torch.empty(n0, 1, 4, device=dev, dtype=torch.float32)
        packed = net.packed()[0]
        with torch.no_grad():
            for p0 in range(0, P, n0):
                n = min(n0, P - p0)
                ops.grid_points(p0, xs, ys, zs, rays11[:n])
                ops.mlp_fwd(rays11[:n], z[:n], net.flat, packed, raw=raw[:n])
                ops.grid_sigma(raw[:n], vol[p0:p0 + n])
        return vol.reshape(xs.numel(), ys.numel(), zs.numel())
    if network_query_fn is None:
        raise TypeError('density_grid with a network that is not a fastnerf NeRF needs network_query_fn(pts, viewdirs, net)')
    if use_viewdirs is None:
        use_viewdirs = getattr(net, 'use_viewdirs', True)
    with torch.no_grad():
        for p0 in range(0, P, n0):
            n = min(n0, P - p0)
            ops.grid_points(p0, xs, ys, zs, rays11[:n])
            pts = rays11[:n, 0:3]
            vd = torch.zeros_like(pts) if use_viewdirs else None
            raw = network_query_fn(pts[:, None, :], vd, network)
            vol[p0:p0 + n] = torch.relu(raw[:, 0, 3].float())
    return vol.reshape(xs.numel(), ys.numel(), zs.numel())


def marching_cubes(volume, threshold):
    """(vertices [V,3] float32, triangles [T,3] int64) cuda tensors of the `threshold` level set of `volume` [nx,ny,nz]
    (inside = value > threshold), vertices in index coordinates like mcubes.marching_cubes.  Deterministic; an empty
    result is valid.  Not a torch custom op: the output shape depends on the data."""
    if not torch.is_tensor(volume) or not volume.is_cuda:
        raise RuntimeError('marching_cubes runs on the GPU only (no CPU fallback): got a CPU array / tensor')
    if volume.dim() != 3 or min(volume.shape) < 2:
        raise ValueError('marching_cubes needs a 3-D volume with every dimension >= 2, got shape %s' % (tuple(volume.shape),))
    vol = volume.contiguous().float()
    if not bool(torch.isfinite(vol).all()):
        raise ValueError('marching_cubes: the volume holds non-finite values')
    verts, tris = ops.marching_cubes(vol, float(threshold))
    return verts, tris.long()


def vertex_normals(network, vertices, chunk=65536):
    """[V,3] unit normals of the density field at `vertices` [V,3] (world coordinates, cuda): -grad / |grad| of the density logit
    (NeRF.density_gradient: the fused forward, the dX chain and csrc/sigma_grad.hip), pointing from dense to empty space.  Exactly
    (0, 0, 0) where the gradient is zero or not finite, never NaN.  Only a fastnerf NeRF has the kernels: anything else raises."""
    net = getattr(network, 'module', network)
    if not isinstance(net, NeRF):
        raise TypeError('vertex_normals needs a fastnerf NeRF (the density gradient comes from its HIP kernels; there is no '
                        'autograd fallback), got %s' % type(net).__name__)
    _, g = net.density_gradient(vertices, chunk=chunk)
    g = g.reshape(-1, 3)
    big = g.abs().amax(-1, keepdim=True)                       # scale first: |g|^2 neither overflows nor underflows
    ok = torch.isfinite(big) & (big > 0)
    u = torch.where(ok, g / torch.where(ok, big, torch.ones_like(big)), torch.zeros_like(g))
    length = torch.linalg.vector_norm(u, dim=-1, keepdim=True)
    return torch.where(ok, -u / torch.where(ok, length, torch.ones_like(length)), torch.zeros_like(g))


def extract_mesh(render_kwargs, N=256, bound=1.2, threshold=50., which='fine', chunk=1024 * 64, normals=False):
    """extract_mesh.py:38-74 from create_nerf's render_kwargs: density on the (N+1)^3 grid linspace(-bound, bound, N+1)^3 of
    the fine network (`which='fine'`; the coarse `network_fn` when there is no fine one or `which='coarse'`), marching
    cubes at `threshold`.  -> (vertices [V,3] in world coordinates -bound + v * 2 bound / N, triangles [T,3] int64), and with
    normals=True a third result: vertex_normals of the same network at those vertices [V,3]."""
    net = render_kwargs.get('network_fine') if which == 'fine' else None
    if net is None:
        net = render_kwargs['network_fn']
    t = torch.linspace(-bound, bound, N + 1, device='cuda')   # on the device, as the reference's (default tensor type cuda, :16)
    vol = density_grid(net, t, t, t, chunk=chunk, network_query_fn=render_kwargs.get('network_query_fn'),
                       use_viewdirs=render_kwargs.get('use_viewdirs'))
    verts, tris = marching_cubes(vol, threshold)
    world = -bound + verts * (2 * bound / N)
    if not normals:
        return world, tris
    return world, tris, vertex_normals(net, world, chunk=chunk)


def export_ply(path, vertices, triangles, normals=None):
    """Binary little-endian PLY 1.0: `float x, y, z` per vertex (followed by `float nx, ny, nz` when `normals` [V,3] is given),
    `list uchar int vertex_indices` per face."""
    v = np.ascontiguousarray(torch.as_tensor(vertices).detach().cpu().numpy(), dtype='<f4').reshape(-1, 3)
    nprops = ''
    if normals is not None:
        nv = np.ascontiguousarray(torch.as_tensor(normals).detach().cpu().numpy(), dtype='<f4').reshape(-1, 3)
        if nv.shape != v.shape:
            raise ValueError('export_ply: %d normals for %d vertices' % (nv.shape[0], v.shape[0]))
        v = np.ascontiguousarray(np.concatenate([v, nv], 1))
        nprops = 'property float nx\nproperty float ny\nproperty float nz\n'
    f = np.asarray(torch.as_tensor(triangles).detach().cpu().numpy()).reshape(-1, 3)
    faces = np.empty(f.shape[0], dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    faces['n'] = 3
    faces['i'] = f
    head = ('ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n%s'
            'element face %d\nproperty list uchar int vertex_indices\nend_header\n' % (v.shape[0], nprops, f.shape[0]))
    with open(path, 'wb') as fh:
        fh.write(head.encode('ascii'))
        fh.write(v.tobytes())
        fh.write(faces.tobytes())
