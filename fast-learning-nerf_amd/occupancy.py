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

Cascade: `OccupancyCascade` is an ordered list of 1 to 8 such grids, innermost first -- usually the fine grid
over the object and coarser grids over larger boxes around it.  A sample takes the bit of the FIRST grid whose box contains it
(each grid's own index arithmetic), and `outside_occupied` of the cascade when none does.  Space outside the inner box is then
skipped because it was looked at and found empty, not because it was assumed empty.

    cascade = fastnerf.occupancy.OccupancyCascade.from_network(render_kwargs_test, levels=3)
    render_kwargs_test['occupancy'] = cascade

Training through a cascade (opt-in): `OccupancyCascade.for_training(levels=3)` -- or any cascade whose grids all carry a density, with
one `dilate` and at most 4096 cells per axis -- goes wherever a training grid goes: run_nerf.Trainer(..., occupancy=cascade), with
`tighten` and `march=`.  Its refresh (`cascade.update`) runs over the OWN cells of the levels only: a cell of level l that lies, with
a margin of dilate + 1 cells of its own and one cell of the inner level, inside the box of ONE level j < l is never read by a lookup
and is left at density 0 (`cascade.own_cells(l)`; the rule in float64: include/fastnerf.h, "cascade, trained").  One cursor rotates
over the concatenation of the levels' own lists, so `cells_per_call` bounds the cost of a refresh whatever the number of levels, and
every chunk is one network launch whatever mix of levels it holds.

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


def _update_nets(render_kwargs, which, who):
    """The networks an `update` evaluates: [coarse], [fine] or [coarse, fine] (`which`; the coarse one when there is no fine one)."""
    from .model import NeRF
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
        raise TypeError('%s.update runs the fused HIP forward: it needs fastnerf NeRF networks' % who)
    return nets


def _rotate(cursor, primed, total, cells_per_call):
    """The slice of `total` entries a refresh takes: ([(a, b), ...] one or two ascending ranges, the next cursor).  Everything while
    not primed or without a budget (the cursor stays); else cells_per_call entries from the cursor on, wrapping round."""
    if cells_per_call is None or not primed or int(cells_per_call) >= total:
        return [(0, total)], cursor
    k = max(1, int(cells_per_call))
    a, b = cursor, cursor + k
    return [(a, min(b, total))] + ([(0, b - total)] if b > total else []), b % total


def _training_fault(levels):
    """None when `levels` (objects with dens, dilate, shape) make a training cascade; else why not.  A cascade in which no or only
    some levels carry a density is a rendering cascade (''), which is no error."""
    have = [g.dens is not None for g in levels]
    if not all(have):
        return ''
    if len({int(g.dilate) for g in levels}) != 1:
        return 'the levels of a training cascade share one dilate, got %s' % ([int(g.dilate) for g in levels],)
    if max(max(g.shape) for g in levels) > OccupancyCascade.MAX_TRAIN_N:
        return 'a training cascade has at most %d cells per axis on every level' % OccupancyCascade.MAX_TRAIN_N
    return None


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
        if self.dens is None:
            raise ValueError('update() needs a grid with a density: OccupancyGrid.for_training(...)')
        nets = _update_nets(render_kwargs, which, 'OccupancyGrid')
        packed = _packed if _packed is not None else [m.packed()[0] for m in nets]
        seed = self.updates + 1 if seed is None else int(seed)
        total = self.ncells
        ranges, self.cursor = _rotate(self.cursor, self.primed, total, cells_per_call)
        self.primed = True
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
    grid, bit for bit.  render / render_path / render_rays take it wherever they take a grid.

    A cascade whose grids ALL carry a density (for_training, or made by hand from OccupancyGrid.for_training grids) is a training
    cascade: run_nerf.Trainer takes it as `occupancy=`, and `update` refreshes it over the own cells of its levels (`own_cells`).
    Its levels share one `dilate` and have at most 4096 cells per axis (ValueError otherwise).  Any other cascade is for rendering
    only (`dens` is None; run_nerf.Trainer raises)."""
    MAX_LEVELS = _lib.OCC_MAX_LEVELS
    MAX_TRAIN_N = 4096      # cells per axis of a level that is trained through: the own-cell margins rest on it
    CHUNK = 1 << 19         # positions per network launch of update()

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
        # the training cascade's state (unused for a rendering cascade): `updates`, `cursor`, `primed` as on a grid, the cursor
        # running over the concatenation of the levels' own lists
        self.updates, self.cursor, self.primed = 0, 0, False
        self._own = None
        fault = _training_fault(grids)
        if fault:
            raise ValueError(fault)
        if fault is None:      # once: the boxes do not move
            dev = grids[0].words.device
            lists = [ops.occ_cascade_own(self._c, l, grids[0].dilate, dev) for l in range(len(grids))]
            self._own = torch.cat(lists)
            self._offsets = (C.c_int64 * (len(grids) + 1))(*np.concatenate([[0], np.cumsum([x.numel() for x in lists])]).tolist())

    @property
    def levels(self):
        return len(self.grids)

    @property
    def dens(self):
        """The levels' densities (a tuple) of a training cascade, None for a rendering cascade."""
        return None if self._own is None else tuple(g.dens for g in self.grids)

    @property
    def dilate(self):
        return self.grids[0].dilate

    @property
    def offsets(self):
        """levels + 1 ints: own_cells(l) is positions offsets[l] .. offsets[l+1] of the concatenation `update` walks."""
        self._need_training()
        return [int(v) for v in self._offsets]

    def _need_training(self):
        if self._own is None:
            raise ValueError('this OccupancyCascade has levels without a density: make one to train through with '
                             'OccupancyCascade.for_training(...), or from OccupancyGrid.for_training grids')

    def own_cells(self, l):
        """Ascending int32 cell indices (c = (i*ny + j)*nz + k) of the cells of level l that a lookup can read, plus the margin
        dilation needs: every cell that is not covered by ONE inner level (include/fastnerf.h, "cascade, trained")."""
        self._need_training()
        return self._own[self._offsets[l]:self._offsets[l + 1]]

    @classmethod
    def for_training(cls, levels=3, N=128, bound=1.2, growth=2.0, threshold=0., dilate=1, decay=0.95, outside_occupied=True,
                     device='cuda'):
        """A cascade to train through (run_nerf.Trainer(..., occupancy=cascade)): level l is OccupancyGrid.for_training over
        [-bound * growth^l, bound * growth^l)^3.  N: a cell count, one per level, or one (nx, ny, nz) per level."""
        levels = int(levels)
        if not 1 <= levels <= cls.MAX_LEVELS:
            raise ValueError('an occupancy cascade has 1 to %d levels, got %d' % (cls.MAX_LEVELS, levels))
        Ns = list(N) if isinstance(N, (list, tuple, np.ndarray)) else [N] * levels
        if len(Ns) != levels or not all(np.ndim(v) == 0 or (np.ndim(v) == 1 and len(v) == 3) for v in Ns):
            raise ValueError('N is a cell count, one per level, or one (nx, ny, nz) per level: got %r for %d levels' % (N, levels))
        if not float(growth) > 0.:
            raise ValueError('growth must be > 0')
        if max(int(s) for v in Ns for s in np.atleast_1d(v)) > cls.MAX_TRAIN_N:
            raise ValueError('a training cascade has at most %d cells per axis on every level' % cls.MAX_TRAIN_N)
        grids = [OccupancyGrid.for_training(N=Ns[l], bound=bound * float(growth) ** l, threshold=threshold, dilate=dilate, decay=decay,
                                            outside_occupied=outside_occupied, device=device) for l in range(levels)]
        return cls(grids, outside_occupied)

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
            c = cls(grids, bool(f['outside_occupied']))
            if 'updates' in f.files:      # (a file from before cascades were trained through has none: a fresh cursor)
                c.updates, c.cursor, c.primed = int(f['updates']), int(f['cursor']), bool(f['primed'])
            return c

    def save(self, path):
        """.npz: levels (int64), outside_occupied (of the cascade), and per level i the fields of OccupancyGrid.save prefixed
        `l{i}_`: l0_words (uint32; cell (i,j,k) = bit c & 31 of word c >> 5, c = (i*ny + j)*nz + k), l0_shape, l0_lo, l0_hi,
        l0_outside_occupied, l1_words, ...; a training cascade adds its own updates, cursor, primed (the levels' training fields
        ride with the levels).  OccupancyGrid.load refuses such a file."""
        fields = dict(levels=np.asarray(self.levels, np.int64), outside_occupied=np.asarray(self.outside_occupied))
        if self._own is not None:
            fields.update(updates=np.asarray(self.updates, np.int64), cursor=np.asarray(self.cursor, np.int64), primed=np.asarray(self.primed))
        for l, g in enumerate(self.grids):
            fields.update({'l%d_%s' % (l, k): v for k, v in g._fields().items()})
        with open(path, 'wb') as fh:
            np.savez(fh, **fields)

    # ---- training ---------------------------------------------------------------------------------------------------
    def update(self, render_kwargs, seed=None, cells_per_call=None, which='both', _packed=None):
        """OccupancyGrid.update over the cascade's own cells: for each position of the concatenated own lists the point
        OccupancyGrid.update samples in that level's cell (same Philox key (seed, cell); fastnerf_occ_cascade_points), the non-saving
        forward of the network(s) on the chunk -- one launch per network and chunk, whatever levels the chunk spans -- then dens =
        max(dens * decay, relu(sigma)) at each position's level and cell (fastnerf_occ_cascade_update), and the bits and their dilation
        per level.  An own cell ends with the bits of density its grid's own update(seed) gives it; a covered cell keeps dens = 0.

        cells_per_call: refresh that many positions, a slice that rotates through the concatenation (level 0 first) from call to
        call; the first call takes everything.  seed, which: as for a grid (default seed = 1 + the cascade's `updates`)."""
        self._need_training()
        nets = _update_nets(render_kwargs, which, 'OccupancyCascade')
        packed = _packed if _packed is not None else [m.packed()[0] for m in nets]
        seed = self.updates + 1 if seed is None else int(seed)
        total = int(self._offsets[self.levels])
        ranges, self.cursor = _rotate(self.cursor, self.primed, total, cells_per_call)
        self.primed = True
        dev = self._own.device
        # the levels' densities and decays as they are now (a grid's decay may be set, its density rebound, between refreshes)
        dens = [g.dens for g in self.grids]
        if any(d is None or d.numel() != g.ncells or d.dtype != torch.float32 or not d.is_contiguous() or d.device != dev
               for d, g in zip(dens, self.grids)):
            raise ValueError('every level of a training cascade keeps a contiguous float32 density of its own size on the cascade\'s device')
        dens_ptrs = (C.c_void_p * self.levels)(*[d.data_ptr() for d in dens])
        decays = (C.c_float * self.levels)(*[float(g.decay) for g in self.grids])
        n0 = min(int(self.CHUNK), max(r[1] - r[0] for r in ranges))
        rays11 = torch.empty(n0, 11, device=dev, dtype=torch.float32)
        z = torch.zeros(n0, 1, device=dev, dtype=torch.float32)
        raws = [torch.empty(n0, 1, 4, device=dev, dtype=torch.float32) for _ in nets]
        with torch.no_grad():
            for lo, hi in ranges:
                for q0 in range(lo, hi, n0):
                    n = min(n0, hi - q0)
                    ops.occ_cascade_points(self._c, self._own, self._offsets, q0, rays11[:n], seed)
                    for m, pk, raw in zip(nets, packed, raws):
                        ops.mlp_fwd(rays11[:n], z[:n], m.flat, pk, raw=raw[:n])
                    ops.occ_cascade_update(self._c, raws[0], raws[1] if len(raws) > 1 else None, self._own, self._offsets, q0, n,
                                           decays, dens_ptrs)
            for g in self.grids:      # the bits of every cell of every level and their dilation, once
                ws = torch.empty(2 * g.words.numel(), device=dev, dtype=torch.int32) if g.dilate > 0 else None
                ops.occ_update(None, None, 0, 0, g.shape, g.decay, g.threshold, g.dilate, g.dens, g.words, ws)
        self.updates += 1

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
