"""Occupancy grid: rendering -- and, opted into, training -- that does not evaluate the networks in empty space.

    grid = fastnerf.occupancy.OccupancyGrid.from_network(render_kwargs_test)
    render_kwargs_test['occupancy'] = grid          # render / render_path / render_rays pass it through

The contract (include/fastnerf.h): a box [lo, hi) in the networks' input space, cut into nx x ny x nz cells, one
bit per cell, and `outside_occupied`.  A sample x = o + d * z lies in cell floor((x - lo) * inv) per axis (fp32, each operation
rounded, inv = n / (hi - lo) rounded once); an index outside 0 .. n-1, a non-finite point included, takes `outside_occupied`.
A sample whose bit is clear gets raw = (0, 0, 0, 0) without the network being evaluated, in the coarse and the fine pass; a
sample whose bit is set gets exactly the logits of the plain forward.  The kernels are csrc/occupancy.hip.

Training (opt-in): a grid made by `OccupancyGrid.for_training` starts fully occupied and carries a per-cell density `dens`;
`run_nerf.Trainer(..., occupancy=grid)` runs the first forward of its compacted step over the occupied samples only and calls
`grid.update` as training goes: dens = max(dens * decay, relu(sigma)) at a jittered point INSIDE each cell, bit = dens >
threshold, dilated.  render_rays(..., occupancy=grid) with gradients enabled still raises: the autograd route has no grid.

Cascade (rendering only): `OccupancyCascade` is an ordered list of 1 to 8 such grids, innermost first -- usually the fine grid
over the object and coarser grids over larger boxes around it.  A sample takes the bit of the FIRST grid whose box contains it
(each grid's own index arithmetic), and `outside_occupied` of the cascade when none does.  Space outside the inner box is then
skipped because it was looked at and found empty, not because it was assumed empty.

    cascade = fastnerf.occupancy.OccupancyCascade.from_network(render_kwargs_test, levels=3)
    render_kwargs_test['occupancy'] = cascade

Per-ray bounds (opt-in): `grid.ray_bounds(ray_batch)` / `grid.tighten(ray_batch)` (grids and cascades; csrc/ray_bounds.hip) clamp near
and far of every ray to the part of [near, far] outside which the lookup above calls no sample occupied, so that the coarse depths are
placed on the object; render_rays(..., occupancy=grid, tighten=True) and run_nerf.Trainer(..., occupancy=grid, tighten=True) do it
on the way.  Conservative without exceptions; stretches outside every box count as occupied when `outside_occupied` is set, so the
default grids tighten little: outside_occupied=False is the configuration this is for."""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops


def _network_volume(render_kwargs, N, bound, which='both', chunk=1024 * 64):
    """relu(sigma) of the networks of `render_kwargs` on linspace(-bound, bound, N+1)^3 (mesh.density_grid): the point volume that
    OccupancyGrid.from_network and every level of OccupancyCascade.from_network are built from.  which: 'both' = the element-wise
    maximum of the coarse and the fine network's volumes, or 'fine' / 'coarse'."""
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
    return vol


class _RayBounds:
    """ray_bounds / tighten of OccupancyGrid and OccupancyCascade (fastnerf_occ_ray_bounds through `self._c`)."""

    def _bounds(self, ray_batch):
        if not torch.is_tensor(ray_batch):
            raise RuntimeError('fastnerf ops run on the GPU only (no CPU fallback): got a host array')
        ops.require_gpu(ray_batch)
        if ray_batch.dim() != 2 or ray_batch.shape[-1] not in (8, 11):
            raise ValueError('ray batches are [N,8] (o, d, near, far) or [N,11] (+ view directions)')
        r = ray_batch.detach().float()
        if r.shape[-1] == 8:      # the kernel reads rows of 11 floats; the view directions are not looked at
            r = torch.cat([r, torch.zeros(r.shape[0], 3, device=r.device)], -1)
        return ops.occ_ray_bounds(self._c, r.contiguous())

    def ray_bounds(self, ray_batch):
        """ray_batch [n,8] or [n,11] (cuda; o, d, near, far in the space the grid lives in -- NDC space for NDC batches) ->
        (near' [n], far' [n], hit bool [n]): near <= near' < far' <= far, and every depth of [near, far] at which the grid calls the
        sample o + d * z occupied lies in [near', far'] -- no exceptions, fp32 rounding at cell faces included.  hit False: the ray
        meets nothing occupied (bounds unchanged).  Stretches outside every box count as occupied when `outside_occupied` is set,
        so such a grid tightens little: outside_occupied=False is the configuration this is for.  A ray the kernel does not walk
        (non-finite, near >= far, terms too large for fp32) keeps its bounds with hit True.  Constants: no gradient flows."""
        bounds, hit = self._bounds(ray_batch)
        return bounds[:, 0], bounds[:, 1], hit.bool()

    def tighten(self, ray_batch):
        """(a new batch of the same shape and dtype with columns 6:8 replaced by `ray_bounds`, hit bool [n]).  The input is not
        modified; the result is an ordinary ray batch for render_rays on any route (near / far are constants there, as always)."""
        bounds, hit = self._bounds(ray_batch)
        return torch.cat([ray_batch[:, :6], bounds.to(ray_batch.dtype), ray_batch[:, 8:]], -1), hit.bool()

    def march(self, ray_batch, K, cap=128, lindisp=False, u=None, seed=0):
        """ray_batch [n,8] or [n,11] (cuda) -> (z float32 [n, cap], kidx int32 [n, cap], overflow bool [n]): the packed rows of the
        marched render (fastnerf_occ_march, one round; include/fastnerf.h, "marched render").  Of the K lattice depths of every ray --
        the coarse depths for N_samples = K, perturb = 0 -- the ones this grid calls occupied are kept, run by run, each run followed
        by one closing entry (kidx -1); padding repeats the last depth with kidx -1.  overflow: the ray has more entries than `cap`
        slots, and the row holds the first cap of them.
        u (float32 [n] in [0, 1)) or seed != 0: the rows of the marched TRAINING step (fastnerf_occ_march_jitter; include/fastnerf.h,
        "marched training") -- the lattice of ray r shifted by u[r] of its spacing, u drawn from the 'mrch' stream of `seed` when not
        given.  The defaults make exactly the call made before."""
        if not torch.is_tensor(ray_batch):
            raise RuntimeError('fastnerf ops run on the GPU only (no CPU fallback): got a host array')
        ops.require_gpu(ray_batch)
        if ray_batch.dim() != 2 or ray_batch.shape[-1] not in (8, 11):
            raise ValueError('ray batches are [N,8] (o, d, near, far) or [N,11] (+ view directions)')
        r = ray_batch.detach().float()
        if r.shape[-1] == 8:
            r = torch.cat([r, torch.zeros(r.shape[0], 3, device=r.device)], -1)
        if u is None and not seed:
            z, kidx, overflow, _ = ops.occ_march(self._c, r.contiguous(), K, cap, lindisp=lindisp)
        else:
            if u is not None:
                if not torch.is_tensor(u):
                    raise RuntimeError('fastnerf ops run on the GPU only (no CPU fallback): got a host array')
                u = u.detach().float().reshape(-1).contiguous()
                if u.shape[0] != r.shape[0]:
                    raise ValueError('u holds one shift per ray')
            z, kidx, overflow, _ = ops.occ_march_jitter(self._c, r.contiguous(), K, cap, u=u, seed=int(seed), lindisp=lindisp)
        return z, kidx, overflow.bool()


class OccupancyGrid(_RayBounds):
    """Bits of an nx x ny x nz grid over [lo, hi) on the GPU.  Build one with from_mask / from_density / from_network / load,
    or for_training (a grid with a density that `update` maintains)."""
    CHUNK = 1 << 19      # cells per network launch of update()

    def __init__(self, words, shape, lo, hi, outside_occupied=True, dens=None, decay=None, threshold=0., dilate=1):
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
        # the training grid's state (None / unused for an inference grid)
        self.dens = None
        self.decay = None if decay is None else float(decay)
        self.threshold, self.dilate = float(threshold), int(dilate)
        self.updates = 0        # update() calls so far: the default seed of the next one
        self.cursor = 0         # first cell of the next slice (cells_per_call)
        self.primed = False     # every cell has been sampled at least once
        if dens is not None:
            ops.require_gpu(dens)
            assert dens.dtype == torch.float32 and dens.is_contiguous() and dens.numel() == self.ncells
            if not 0. <= self.decay <= 1.:
                raise ValueError('decay lies in [0, 1]')
            if self.dilate < 0:
                raise ValueError('dilate must be >= 0')
            self.dens = dens.reshape(-1)

    @property
    def ncells(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

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
        return cls.from_density(_network_volume(render_kwargs, N, bound, which, chunk), -bound, bound, threshold, dilate, outside_occupied)

    @classmethod
    def for_training(cls, N=128, bound=1.2, threshold=0., dilate=1, decay=0.95, outside_occupied=True, device='cuda'):
        """A grid to train through (run_nerf.Trainer(..., occupancy=grid)): N^3 cells (or N = (nx, ny, nz)) over
        [-bound, bound)^3, every bit set, and a zero density that the first `update` fills from the networks.  A cell closes
        once dens * decay^k <= threshold: with the default threshold = 0 that is never in practice (fp32 underflow, some 2000
        refreshes), so the grid then only loses cells whose sigma was never positive at any sampled point; threshold > 0
        lets cells close again."""
        shape = (int(N),) * 3 if np.ndim(N) == 0 else tuple(int(s) for s in N)
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError('N is a cell count or (nx, ny, nz), every one >= 1')
        dev = torch.device(device)
        words = ops.occ_from_mask(torch.ones(shape, dtype=torch.bool, device=dev))
        dens = torch.zeros(shape[0] * shape[1] * shape[2], device=dev, dtype=torch.float32)
        return cls(words, shape, -bound, bound, outside_occupied, dens=dens, decay=decay, threshold=threshold, dilate=dilate)

    @classmethod
    def load(cls, path, device='cuda'):
        with np.load(path) as f:
            if 'levels' in f.files:
                raise ValueError('%s holds an occupancy cascade of %d levels: load it with OccupancyCascade.load' % (path, int(f['levels'])))
            return cls._from_fields(f, '', device)

    @classmethod
    def _from_fields(cls, f, prefix, device):
        """The grid whose save() fields are f[prefix + name]."""
        get = lambda k: f[prefix + k]      # noqa: E731
        words = torch.from_numpy(get('words').astype(np.uint32).view(np.int32)).to(device)
        if prefix + 'dens' not in f.files:
            return cls(words, get('shape').tolist(), get('lo'), get('hi'), bool(get('outside_occupied')))
        g = cls(words, get('shape').tolist(), get('lo'), get('hi'), bool(get('outside_occupied')),
                dens=torch.from_numpy(get('dens').astype(np.float32)).to(device), decay=float(get('decay')),
                threshold=float(get('threshold')), dilate=int(get('dilate')))
        g.updates, g.cursor, g.primed = int(get('updates')), int(get('cursor')), bool(get('primed'))
        return g

    def _fields(self):
        fields = dict(words=self.words.cpu().numpy().view(np.uint32), shape=np.asarray(self.shape, np.int64), lo=self.lo,
                      hi=self.hi, outside_occupied=np.asarray(self.outside_occupied))
        if self.dens is not None:
            fields.update(dens=self.dens.cpu().numpy(), decay=np.asarray(self.decay, np.float64),
                          threshold=np.asarray(self.threshold, np.float64), dilate=np.asarray(self.dilate, np.int64),
                          updates=np.asarray(self.updates, np.int64), cursor=np.asarray(self.cursor, np.int64),
                          primed=np.asarray(self.primed))
        return fields

    def save(self, path):
        """.npz: words (uint32; cell (i,j,k) = bit c & 31 of word c >> 5, c = (i*ny + j)*nz + k), shape, lo, hi, outside_occupied;
        a training grid adds dens (float32 [nx*ny*nz], cell order c), decay, threshold, dilate, updates, cursor, primed."""
        with open(path, 'wb') as fh:      # (a file object: numpy appends no suffix)
            np.savez(fh, **self._fields())

    # ---- training ---------------------------------------------------------------------------------------------------
    def update(self, render_kwargs, seed=None, cells_per_call=None, _packed=None, which='both'):
        """Refresh the density and the bits from the networks of `render_kwargs` (fastnerf NeRF modules): a point inside each
        cell (fastnerf_occ_cell_points: Philox jitter keyed by (seed, cell); seed 0 = cell centres; default = 1 + the number
        of updates so far, so that every rank of a data-parallel run draws the same points), the non-saving forward of the
        coarse and of the fine network there, then dens = max(dens * decay, relu(sigma_coarse), relu(sigma_fine)) and
        bit = dens > threshold, dilated (fastnerf_occ_update).  Everything is enqueued on the current stream: no host round trip.

        cells_per_call: refresh only that many cells, a slice that rotates through the grid from call to call, so that the cost
        per call is bounded; a cell decays once per refresh of its own.  The first call always takes every cell: a cell that
        was never sampled has no density to stand on.

        which: 'both' (default), or 'coarse' / 'fine' as in from_network: the density then follows that network alone (the coarse
        one when there is no fine one) -- what a trainer that marches one network refreshes its grid from."""
        from .model import NeRF
        if self.dens is None:
            raise ValueError('update() needs a grid with a density: OccupancyGrid.for_training(...)')
        if which not in ('both', 'fine', 'coarse'):
            raise ValueError("which is 'both', 'fine' or 'coarse'")
        nets = [getattr(render_kwargs['network_fn'], 'module', render_kwargs['network_fn'])]
        fine = render_kwargs.get('network_fine')
        fine = getattr(fine, 'module', fine)
        if fine is not None and fine is not nets[0]:
            if which == 'both':
                nets.append(fine)
            elif which == 'fine':
                nets = [fine]
        if not all(isinstance(m, NeRF) for m in nets):
            raise TypeError('OccupancyGrid.update runs the fused HIP forward: it needs fastnerf NeRF networks')
        packed = _packed if _packed is not None else [m.packed()[0] for m in nets]
        seed = self.updates + 1 if seed is None else int(seed)
        total = self.ncells
        if cells_per_call is None or not self.primed or int(cells_per_call) >= total:
            ranges = [(0, total)]
            self.primed = True
        else:
            k = max(1, int(cells_per_call))
            a, b = self.cursor, self.cursor + k
            ranges = [(a, min(b, total))] + ([(0, b - total)] if b > total else [])
            self.cursor = b % total
        dev = self.dens.device
        n0 = min(self.CHUNK, max(r[1] - r[0] for r in ranges))
        rays11 = torch.empty(n0, 11, device=dev, dtype=torch.float32)
        z = torch.zeros(n0, 1, device=dev, dtype=torch.float32)
        raws = [torch.empty(n0, 1, 4, device=dev, dtype=torch.float32) for _ in nets]
        ws = torch.empty(2 * self.words.numel(), device=dev, dtype=torch.int32) if self.dilate > 0 else None
        with torch.no_grad():
            for lo, hi in ranges:
                for c0 in range(lo, hi, n0):
                    n = min(n0, hi - c0)
                    ops.occ_cell_points(self._c, c0, rays11[:n], seed)
                    for m, pk, raw in zip(nets, packed, raws):
                        ops.mlp_fwd(rays11[:n], z[:n], m.flat, pk, raw=raw[:n])
                    ops.occ_update(raws[0], raws[1] if len(raws) > 1 else None, c0, n, self.shape, self.decay, self.threshold,
                                   self.dilate, self.dens, None)
            # the bits of every cell and their dilation once, after the density of the last chunk
            ops.occ_update(None, None, 0, 0, self.shape, self.decay, self.threshold, self.dilate, self.dens, self.words, ws)
        self.updates += 1

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


class OccupancyCascade(_RayBounds):
    """An ordered list of 1 to 8 OccupancyGrids, innermost first (the cascade keeps references to them).  A point is looked up
    level by level with each grid's own index arithmetic; the first grid whose box contains it decides, and the sample takes that
    cell's bit.  A point that no box contains -- every non-finite point -- takes `outside_occupied` (None = the last grid's); the
    grids' own `outside_occupied` flags are not read.  The boxes need not be nested or concentric.  A cascade of one grid is that
    grid, bit for bit.  render / render_path / render_rays take it wherever they take a grid; training does not
    (run_nerf.Trainer raises)."""
    MAX_LEVELS = _lib.OCC_MAX_LEVELS

    def __init__(self, grids, outside_occupied=None):
        grids = list(grids)
        if not 1 <= len(grids) <= self.MAX_LEVELS:
            raise ValueError('an occupancy cascade has 1 to %d levels, got %d' % (self.MAX_LEVELS, len(grids)))
        if not all(isinstance(g, OccupancyGrid) for g in grids):
            raise TypeError('an occupancy cascade is made of OccupancyGrids')
        if len({g.words.device for g in grids}) != 1:
            raise ValueError('the levels of an occupancy cascade live on one device')
        self.grids = grids
        self.outside_occupied = grids[-1].outside_occupied if outside_occupied is None else bool(outside_occupied)
        self._c = _lib.OccCascade()
        self._c.levels = len(grids)
        for l, g in enumerate(grids):      # copies of the levels' descriptors: the words stay the grids' own
            C.memmove(C.byref(self._c.level[l]), C.byref(g._c), C.sizeof(_lib.OccGrid))
        self._c.level[len(grids) - 1].outside_occupied = int(self.outside_occupied)

    @property
    def levels(self):
        return len(self.grids)

    @classmethod
    def from_network(cls, render_kwargs, levels=3, N=256, bound=1.2, growth=2.0, threshold=0., dilate=1, which='both',
                     outside_occupied=True, chunk=1024 * 64):
        """Level l is exactly OccupancyGrid.from_network(render_kwargs, N=N_l, bound=bound * growth**l, ...): N_l^3 cells over
        [-bound * growth^l, bound * growth^l)^3, N a scalar or one value per level.  Each level is built over its WHOLE box,
        independently of the others, so level l alone equals the single grid of that box bit for bit (its cells that lie inside
        an inner level's box are built too, and never read).

        At the seams: dilation is per level and clipped at the level's box.  Outwards the coarser level's own dilation covers
        the face, because its cells over the inner box carry the inner density.  Inwards, density just outside an inner box does
        NOT open the inner level's boundary cells: a level sees only the density at its own cells' corners."""
        levels = int(levels)
        if not 1 <= levels <= cls.MAX_LEVELS:
            raise ValueError('an occupancy cascade has 1 to %d levels, got %d' % (cls.MAX_LEVELS, levels))
        Ns = [int(N)] * levels if np.ndim(N) == 0 else [int(n) for n in N]
        if len(Ns) != levels:
            raise ValueError('N is a cell count or one per level: got %d values for %d levels' % (len(Ns), levels))
        if not float(growth) > 0.:
            raise ValueError('growth must be > 0')
        grids = [OccupancyGrid.from_network(render_kwargs, N=Ns[l], bound=bound * float(growth) ** l, threshold=threshold, dilate=dilate,
                                            which=which, outside_occupied=outside_occupied, chunk=chunk) for l in range(levels)]
        return cls(grids, outside_occupied)

    @classmethod
    def load(cls, path, device='cuda'):
        with np.load(path) as f:
            if 'levels' not in f.files:
                raise ValueError('%s holds a single occupancy grid: load it with OccupancyGrid.load' % path)
            grids = [OccupancyGrid._from_fields(f, 'l%d_' % l, device) for l in range(int(f['levels']))]
            return cls(grids, bool(f['outside_occupied']))

    def save(self, path):
        """.npz: levels (int64), outside_occupied (of the cascade), and per level i the fields of OccupancyGrid.save prefixed
        `l{i}_`: l0_words (uint32; cell (i,j,k) = bit c & 31 of word c >> 5, c = (i*ny + j)*nz + k), l0_shape, l0_lo, l0_hi,
        l0_outside_occupied, l1_words, ...  OccupancyGrid.load refuses such a file."""
        fields = dict(levels=np.asarray(self.levels, np.int64), outside_occupied=np.asarray(self.outside_occupied))
        for l, g in enumerate(self.grids):
            fields.update({'l%d_%s' % (l, k): v for k, v in g._fields().items()})
        with open(path, 'wb') as fh:
            np.savez(fh, **fields)

    # ---- inspection -------------------------------------------------------------------------------------------------
    def query(self, points):
        """points [..., 3] (cuda) -> bool [...]: the bit a sample at that point takes."""
        if not torch.is_tensor(points):
            raise RuntimeError('fastnerf ops run on the GPU only (no CPU fallback): got a host array')
        ops.require_gpu(points)
        return ops.occ_query(self._c, points).bool().reshape(points.shape[:-1])

    def decided_by(self, points):
        """points [..., 3] (cuda) -> int8 [...]: the index of the level that decides the point, -1 when no box contains it.
        Torch arithmetic with the levels' own fp32 lo and inv (subtraction and product each rounded), for inspection."""
        if not torch.is_tensor(points):
            raise RuntimeError('fastnerf ops run on the GPU only (no CPU fallback): got a host array')
        ops.require_gpu(points)
        x = points.float()
        out = torch.full(x.shape[:-1], -1, device=x.device, dtype=torch.int8)
        for l in reversed(range(self.levels)):
            g = self.grids[l]
            lo, inv = (torch.from_numpy(a).to(x.device) for a in (g.lo, g.inv))
            f = torch.floor((x - lo) * inv)
            inside = ((f >= 0) & (f < torch.tensor(g.shape, device=x.device, dtype=torch.float32))).all(-1)
            out[inside] = l
        return out

    def occupied_fraction(self):
        """One fraction per level, each over the level's whole box."""
        return [g.occupied_fraction() for g in self.grids]

    def classify(self, rays11, z, raw=None):
        """(live_idx, counts) of ops.occ_classify for the samples o + d * z of a pass."""
        return ops.occ_classify(self._c, rays11, z, raw)
