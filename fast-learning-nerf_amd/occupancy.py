"""Occupancy grid: rendering that does not evaluate the networks in empty space (inference only).

    grid = fastnerf.occupancy.OccupancyGrid.from_network(render_kwargs_test)
    render_kwargs_test['occupancy'] = grid          # render / render_path / render_rays pass it through

The contract (include/fastnerf.h): a box [lo, hi) in the networks' input space, cut into nx x ny x nz cells, one
bit per cell, and `outside_occupied`.  A sample x = o + d * z lies in cell floor((x - lo) * inv) per axis (fp32, each operation
rounded, inv = n / (hi - lo) rounded once); an index outside 0 .. n-1, a non-finite point included, takes `outside_occupied`.
A sample whose bit is clear gets raw = (0, 0, 0, 0) without the network being evaluated, in the coarse and the fine pass; a
sample whose bit is set gets exactly the logits of the plain forward.  The kernels are csrc/occupancy.hip."""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops


class OccupancyGrid:
    """Bits of an nx x ny x nz grid over [lo, hi) on the GPU.  Build one with from_mask / from_density / from_network / load."""

    def __init__(self, words, shape, lo, hi, outside_occupied=True):
        ops.require_gpu(words)
        self.shape = tuple(int(s) for s in shape)
        if len(self.shape) != 3:
            raise ValueError('an occupancy grid is three-dimensional')
        assert words.dtype == torch.int32 and words.is_contiguous() and words.numel() == ops.occ_words(*self.shape)
        self.words = words
        self.lo = np.broadcast_to(np.asarray(lo, dtype=np.float32), (3,)).copy()
        self.hi = np.broadcast_to(np.asarray(hi, dtype=np.float32), (3,)).copy()
        if not (np.isfinite(self.lo).all() and np.isfinite(self.hi).all() and (self.hi > self.lo).all()):
            raise ValueError('an occupancy grid needs a finite box with hi > lo on every axis')
        # n / (hi - lo): the quotient of the fp32 bounds in double precision, rounded to fp32 once
        self.inv = (np.asarray(self.shape, np.float64) / (self.hi.astype(np.float64) - self.lo.astype(np.float64))).astype(np.float32)
        self.outside_occupied = bool(outside_occupied)
        self._c = _lib.OccGrid(words.data_ptr(), (C.c_float * 3)(*self.lo.tolist()), (C.c_float * 3)(*self.inv.tolist()),
                               (C.c_int32 * 3)(*self.shape), int(self.outside_occupied))

    # ---- constructors -----------------------------------------------------------------------------------------------
    @classmethod
    def from_mask(cls, mask, lo, hi, outside_occupied=True):
        """mask: bool cuda tensor [nx, ny, nz], True = occupied."""
        if not torch.is_tensor(mask):
            raise RuntimeError('fastnerf ops run on the GPU only (no CPU fallback): got a host array')
        return cls(ops.occ_from_mask(mask), mask.shape, lo, hi, outside_occupied)

    @classmethod
    def from_density(cls, volume, lo, hi, threshold=0., dilate=1, outside_occupied=True):
        """volume: cuda tensor [nx+1, ny+1, nz+1] of densities at the cells' corner points (mesh.density_grid).  A cell is
        occupied when the maximum of its 8 corners is > threshold; then the occupied set grows by `dilate` cells (Chebyshev
        distance, clipped at the box)."""
        if not torch.is_tensor(volume):
            raise RuntimeError('fastnerf ops run on the GPU only (no CPU fallback): got a host array')
        words = ops.occ_build(volume, threshold, dilate)
        return cls(words, [s - 1 for s in volume.shape], lo, hi, outside_occupied)

    @classmethod
    def from_network(cls, render_kwargs, N=256, bound=1.2, threshold=0., dilate=1, which='both', outside_occupied=True,
                     chunk=1024 * 64):
        """N^3 cells over [-bound, bound)^3 from relu(sigma) on linspace(-bound, bound, N+1)^3 (mesh.density_grid).  which:
        'both' (default) = the element-wise maximum of the coarse and the fine network's volumes -- the coarse pass is masked
        by the same grid -- or 'fine' / 'coarse'."""
        from . import mesh
        if which not in ('both', 'fine', 'coarse'):
            raise ValueError("which is 'both', 'fine' or 'coarse'")
        nets = []
        if which in ('both', 'coarse') or render_kwargs.get('network_fine') is None:
            nets.append(render_kwargs['network_fn'])
        if which in ('both', 'fine') and render_kwargs.get('network_fine') is not None:
            nets.append(render_kwargs['network_fine'])
        t = torch.linspace(-bound, bound, N + 1, device='cuda')
        vol = None
        for net in nets:
            v = mesh.density_grid(net, t, t, t, chunk=chunk, network_query_fn=render_kwargs.get('network_query_fn'),
                                  use_viewdirs=render_kwargs.get('use_viewdirs'))
            vol = v if vol is None else torch.maximum(vol, v)
        return cls.from_density(vol, -bound, bound, threshold, dilate, outside_occupied)

    @classmethod
    def load(cls, path, device='cuda'):
        with np.load(path) as f:
            words = torch.from_numpy(f['words'].astype(np.uint32).view(np.int32)).to(device)
            return cls(words, f['shape'].tolist(), f['lo'], f['hi'], bool(f['outside_occupied']))

    def save(self, path):
        """.npz: words (uint32; cell (i,j,k) = bit c & 31 of word c >> 5, c = (i*ny + j)*nz + k), shape, lo, hi, outside_occupied."""
        with open(path, 'wb') as fh:      # (a file object: numpy appends no suffix)
            np.savez(fh, words=self.words.cpu().numpy().view(np.uint32), shape=np.asarray(self.shape, np.int64), lo=self.lo,
                     hi=self.hi, outside_occupied=np.asarray(self.outside_occupied))

    # ---- inspection -------------------------------------------------------------------------------------------------
    def to_mask(self):
        """bool cuda tensor [nx, ny, nz]."""
        ncells = self.shape[0] * self.shape[1] * self.shape[2]
        sh = torch.arange(32, device=self.words.device, dtype=torch.int32)
        bits = (self.words[:, None] >> sh[None, :]) & 1
        return bits.reshape(-1)[:ncells].reshape(self.shape).bool()

    def query(self, points):
        """points [..., 3] (cuda) -> bool [...]: the bit a sample at that point takes."""
        if not torch.is_tensor(points):
            raise RuntimeError('fastnerf ops run on the GPU only (no CPU fallback): got a host array')
        ops.require_gpu(points)
        return ops.occ_query(self._c, points).bool().reshape(points.shape[:-1])

    def occupied_fraction(self):
        return float(self.to_mask().float().mean())

    def classify(self, rays11, z, raw=None):
        """(live_idx, counts) of ops.occ_classify for the samples o + d * z of a pass."""
        return ops.occ_classify(self._c, rays11, z, raw)
