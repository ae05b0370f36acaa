"""Volumetric renderer -- mirror of nerf-ours/render.py on the HIP kernels.

Same call surface: render (render.py:26-91), batchify_rays (:12-24), render_rays (:195-305),
raw2outputs (:149-192), render_path (:94-146).  `render_rays` runs the fused device pipeline

    sample_coarse -> mlp_fwd(coarse) -> raw2outputs -> sample_pdf_merge -> mlp_fwd(fine) -> raw2outputs

and, when autograd is recording, registers ONE autograd node whose backward runs
raw2outputs_bwd + mlp_bwd for both nets and hands the flat gradients to the NeRF parameters,
so the reference's `loss.backward(); optimizer.step()` loop works unchanged.  Networks that are not fastnerf
NeRF modules take the closure route instead (`_render_rays_closure`): the caller's `network_query_fn` runs in torch
between the same HIP sampling and compositing kernels, differentiable through torch.ops.fastnerf.raw2outputs_full.

Every map is differentiable, as under the reference's plain-torch render_rays: a loss on `disp_map`, `acc_map`, `disp0`, `acc0` (and on
`depth_map` / `depth0`, handed out with retdepth=True) reaches both networks on the fused route too -- the autograd node hands
d(loss)/d(maps) to the compositing backward (fastnerf_render_rays_bwd_maps -> raw2outputs_bwd_full); a loss on the colours alone
makes exactly the calls it made before.  `raw` and `z_std` stay non-differentiable.

Ray and pose gradients: a `ray_batch` that requires grad gets the gradient of every map with respect to its columns o, d and
viewdir on both routes (fused: ops.ray_grad after each pass's backward, `_RenderRaysRayGradFn`; it consumes d(loss)/d(raw), so the
depth / opacity terms arrive with no kernel of their own; near / far and z are constants and get zeros), and
`render(..., c2w=pose)` with a pose that requires grad carries it on to the pose (`_PoseRaysFn`).
"""
import os

import numpy as np
import torch

from . import flat_params, ops
from .model import NeRF, param_slices
from .run_nerf_helpers import compute_ssim, get_rays, to8b

_SEED_GEN = torch.Generator()


def _next_seed():
    """Key of a device-side Philox stream, drawn from torch's global CPU RNG so that torch.manual_seed governs it.  In a sharded run
    every rank draws the SAME value (parallel.sync_seed keeps the host streams in step, which the redundantly drawn pixel picks need) and
    folds its rank in: rows r::world of different ranks must not carry identical jitter patterns.  Rank 0 / a single process: unchanged."""
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    from . import parallel
    rk = parallel.rank()
    if rk:
        seed ^= (rk * 0x9E3779B97F4A7C15) & (2 ** 62 - 1)
    return seed or 1      # (0 means "deterministic" to the samplers: never hand it out as a key)


def _burn_seeds(k):
    """A rank whose shard of a batch is EMPTY skips the step's kernels but must consume the host RNG exactly like the ranks that run it:
    the redundantly drawn pixel picks of the epoch loop rely on every rank's torch CPU stream staying in step between parallel.sync_seed()
    calls."""
    for _ in range(int(k)):
        _next_seed()


def _pytest_rand(shape, device):
    np.random.seed(0)
    return torch.Tensor(np.random.rand(*shape)).to(device)


class _Workspace:
    """Scratch for the backward pass, one set per (device, stream): kernels of one stream run in order, so reuse
    across calls on that stream is safe, and two streams running backward concurrently never share a buffer."""
    _cache = {}

    @classmethod
    def _key(cls, name, device):
        return (name, str(device), torch.cuda.current_stream(device).cuda_stream)

    @classmethod
    def partial(cls, device):
        key = cls._key('partial', device)
        if key not in cls._cache:
            cls._cache[key] = torch.empty(ops.mlp_bwd_partial_floats(), device=device, dtype=torch.float32)
        return cls._cache[key]

    @classmethod
    def get(cls, name, device, count, dtype=torch.float32):
        key = cls._key(name, device)
        t = cls._cache.get(key)
        if t is None or t.numel() < count:
            cls._cache[key] = t = torch.empty(count, device=device, dtype=dtype)
        return t

    @classmethod
    def dact(cls, device, floats):
        return cls.get('dact', device, floats)


# ---- exact zero-gradient point compaction of the training backward (csrc/train.hip, render.cpp) ----
# FASTNERF_COMPACT = auto (default) | 1 | 0.  The compacted backward recomputes the forward of the live points
# (forward work 1 + f, backward work f for a live fraction f), the plain one saves every activation in the first
# forward (1, 1): compaction wins below f ~ 0.76 (split-bf16) / 0.69 (exact fp32).  `auto` starts compacted and follows
# the measured fraction.  Both math modes have the live-list kernels.
_COMPACT = os.environ.get('FASTNERF_COMPACT', 'auto')
assert _COMPACT in ('auto', '0', '1'), 'FASTNERF_COMPACT must be auto, 0 or 1'


def set_compact(mode):
    global _COMPACT
    assert mode in ('auto', '0', '1')
    _COMPACT = mode


def get_compact():
    return _COMPACT


class LivePolicy:
    """Decides per step whether the backward runs compacted; fed with the (live, total) counters of compacted steps
    through pinned-memory copies that are only read once their event has completed (never stalls the stream).

    What is live depends on the loss.  Under the colour loss alone a sample behind an opaque surface is dead (T = 0 to fp32).
    A depth or opacity term keeps the list exact -- a sample with sigma' <= 0 still has d(loss)/d(raw) == +-0 in all four
    components -- but its d(acc)/d(alpha_i) = T_end / t_i reaches EVERY sample with sigma' > 0 of a ray whose transmittance
    has not run out, so the measured fraction f (and with it the step time, 5.2 + 18.3 f ms at the bench shape) rises
    until the surfaces close; the policy follows the counters as before and needs no change."""
    MAX_LAG = 6
    EVERY, PROBE = 4, 256   # (a measurement is a 16-byte asynchronous copy: cheap enough to follow fast changes early in training)
    # break-even live fractions from the measured kernel times (forward without saving + f x (saving forward + backward)
    # against saving forward + backward): 0.76 in the split-bf16 mode, 0.69 in the exact-fp32 mode; hysteresis around them
    THRESHOLDS = {'bf16x3': (0.78, 0.70), 'fp32': (0.70, 0.62), 'bf16x6': (0.70, 0.62)}

    def __init__(self):
        self.frac = None          # last measured live fraction (both passes together)
        self.on = True
        self.step = 0
        self._pending = None      # (pinned host tensor, event)

    def available(self, net_c, net_f, N_importance):
        return N_importance == 0 or (net_f is not None and net_f is not net_c)

    def use_live(self, net_c, net_f, N_importance):
        if _COMPACT == '0' or not self.available(net_c, net_f, N_importance):
            return False
        if _COMPACT == '1':
            return True
        self.poll()
        if self.on:
            return True
        return self.step % self.PROBE == 0     # an occasional compacted step keeps the measurement alive

    def poll(self):
        # The host enqueues steps faster than the GPU runs them, so a measurement can stay "pending" for as many steps as the
        # queue is deep.  Decisions are never taken more than MAX_LAG steps blind: waiting for that event then only holds
        # the HOST back -- the GPU still has MAX_LAG steps of work queued behind it.
        if self._pending is not None and self.step - self._pending[2] >= self.MAX_LAG:
            self._pending[1].synchronize()
        if self._pending is not None and self._pending[1].query():
            c = self._pending[0].tolist()
            self._pending = None
            tot = c[1] + c[3]
            if tot > 0:
                self.frac = (c[0] + c[2]) / tot
                off, on = self.THRESHOLDS[ops.get_math()]
                if self.on and self.frac > off:
                    self.on = False
                elif not self.on and self.frac < on:
                    self.on = True

    def after_live_step(self, counts):
        if self._pending is None and (self.step % self.EVERY == 0 or not self.on):
            host = torch.empty(4, dtype=torch.int32).pin_memory()
            host.copy_(counts, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending = (host, ev, self.step)

    def tick(self):
        self.step += 1


def _maps(o, N_importance):
    """The outputs of ops.render_rays_fwd / _fwd_occ under the names of render_rays' maps."""
    if N_importance > 0:
        return dict(rgb_map=o['rgb1'], disp_map=o['disp1'], acc_map=o['acc1'], raw=o['raw1'], rgb0=o['rgb0'], disp0=o['disp0'],
                    acc0=o['acc0'], z_std=o['z_std'], weights=o['w1'], z_vals=o['z1'], depth_map=o['depth1'], depth0=o['depth0'],
                    z_samples=o['z_samples'], weights0=o['w0'], z0=o['z0'])
    return dict(rgb_map=o['rgb0'], disp_map=o['disp0'], acc_map=o['acc0'], raw=o['raw0'], weights=o['w0'], z_vals=o['z0'],
                depth_map=o['depth0'])


def _dist_maps(out, rays11, lindisp):
    """The per-ray distortion loss (ops.distortion) of the weights of a forward's image pass -> 'dist_map', and of the coarse pass of
    two -> 'dist0'.  A marched row (its depths under 'march_z') is taken with skip = its overflow flags."""
    if 'march_z' in out:
        return {'dist_map': ops.distortion(out['weights'], out['march_z'], rays11, lindisp, skip=out['march_overflow'], want=('ell',))[0]}
    d = {'dist_map': ops.distortion(out['weights'], out['z_vals'], rays11, lindisp, want=('ell',))[0]}
    if 'weights0' in out:
        d['dist0'] = ops.distortion(out['weights0'], out['z0'], rays11, lindisp, want=('ell',))[0]
    return d


def _forward_core(rays11, net_c, net_f, N_samples, N_importance, lindisp, perturb, white_bkgd, t_rand, u, noise0,
                  noise1, save, packed_c=None, packed_f=None, skip_dead_rgb=False, act_ws=False, retdist=False):
    """The fused forward.  Returns (outputs dict, saved-for-backward dict).  retdist: 'dist_map' (and 'dist0') among the outputs, and the
    weights they were taken from among the saved tensors."""
    pc = packed_c if packed_c is not None else net_c.packed()
    fine = pf = None
    if N_importance > 0:
        fine = net_f if net_f is not None else net_c
        pf = packed_f if packed_f is not None else (fine.packed() if fine is not net_c else pc)
    # act_ws (the fused Trainer: its backward runs before its next forward): the saved activations live in this stream's
    # persistent scratch instead of 11 GB of fresh allocations per step
    act_bufs = None
    if save and act_ws:
        n_ = rays11.shape[0]
        act_bufs = (_Workspace.get('act0', rays11.device, ops.act_floats(n_ * N_samples)),
                    _Workspace.get('act1', rays11.device, ops.act_floats(n_ * (N_samples + N_importance))) if N_importance > 0 else None)
    # one C-ABI call enqueues sampler -> MLP -> compositing [-> sample_pdf + merge -> MLP -> compositing]
    o = ops.render_rays_fwd(rays11, net_c.flat, pc[0], None if fine is None else fine.flat, None if pf is None else pf[0],
                            N_samples, N_importance, lindisp=lindisp, perturb=perturb, det=(perturb == 0.),
                            white_bkgd=white_bkgd, t_rand=t_rand, u=u, noise0=noise0, noise1=noise1,
                            seed0=_next_seed() if (perturb and t_rand is None) else 0,
                            seed1=_next_seed() if (N_importance > 0 and perturb and u is None) else 0, save=save,
                            skip_dead_rgb=bool(skip_dead_rgb and not save and net_c.use_viewdirs), act_bufs=act_bufs)
    # acc / depth (the disparity clamp of the map backward is decided on them) are saved as detached aliases: the maps themselves
    # are outputs of the autograd node that owns `saved`, and an output kept there would tie node -> saved -> output -> grad_fn -> node
    # into a cycle that only the cyclic collector frees -- with the saved activations in it
    saved = {'rays11': rays11, 'z0': o['z0'], 'raw0': o['raw0'], 'act0': o['act0'], 'noise0': noise0, 'white': white_bkgd,
             'net_c': net_c, 'net_f': None, 'pc': pc, 'live': not save, 'acc0': o['acc0'].detach(), 'depth0': o['depth0'].detach()}
    if N_importance > 0:
        saved.update(z1=o['z1'], raw1=o['raw1'], act1=o['act1'], noise1=noise1, net_f=fine, pf=pf, acc1=o['acc1'].detach(),
                     depth1=o['depth1'].detach())
    out = _maps(o, N_importance)
    if retdist:
        out.update(_dist_maps(out, rays11, lindisp))
        saved.update(lindisp=lindisp, w0=o['w0'].detach())
        if N_importance > 0:
            saved.update(w1=o['w1'].detach())
    return out, saved


def _forward_occ(rays11, net_c, net_f, N_samples, N_importance, lindisp, perturb, white_bkgd, t_rand, u, occupancy, skip_dead_rgb=False):
    """The fused inference forward through an occupancy grid or cascade (fastnerf_render_rays_fwd_occ / _occ_cascade, chosen by
    the type of `occupancy._c`): _forward_core(save=False) with the
    networks run on the occupied samples only.  Returns the outputs dict, plus 'counts' (device int32 [4])."""
    pc = net_c.packed()
    fine = pf = None
    if N_importance > 0:
        fine = net_f if net_f is not None else net_c
        pf = fine.packed() if fine is not net_c else pc
    o = ops.render_rays_fwd_occ(rays11, net_c.flat, pc[0], None if fine is None else fine.flat, None if pf is None else pf[0],
                                N_samples, N_importance, occupancy._c, lindisp=lindisp, perturb=perturb, det=(perturb == 0.),
                                white_bkgd=white_bkgd, t_rand=t_rand, u=u,
                                seed0=_next_seed() if (perturb and t_rand is None) else 0,
                                seed1=_next_seed() if (N_importance > 0 and perturb and u is None) else 0,
                                skip_dead_rgb=bool(skip_dead_rgb and net_c.use_viewdirs))
    return dict(_maps(o, N_importance), z0=o['z0'], raw0=o['raw0'], counts=o['counts'])


def _forward_ert(rays11, net_c, net_f, N_samples, N_importance, lindisp, perturb, white_bkgd, t_rand, u, ert, ert_block=32,
                 occupancy=None, skip_dead_rgb=False):
    """The fused inference forward with early ray termination in the pass that produces the image (fastnerf_render_rays_fwd_ert),
    optionally through an occupancy grid or cascade as well: _forward_occ with the image pass run segment by segment.  Returns
    the outputs dict, plus 'counts' (device int32 [4] = (evaluated, total) of the coarse pass, then of the fine pass; one pass: the
    first pair) and 'trans' (the image pass's final transmittance per ray)."""
    pc = net_c.packed()
    fine = pf = None
    if N_importance > 0:
        fine = net_f if net_f is not None else net_c
        pf = fine.packed() if fine is not net_c else pc
    o = ops.render_rays_fwd_ert(rays11, net_c.flat, pc[0], None if fine is None else fine.flat, None if pf is None else pf[0],
                                N_samples, N_importance, ert, ert_block, None if occupancy is None else occupancy._c, lindisp=lindisp,
                                perturb=perturb, det=(perturb == 0.), white_bkgd=white_bkgd, t_rand=t_rand, u=u,
                                seed0=_next_seed() if (perturb and t_rand is None) else 0,
                                seed1=_next_seed() if (N_importance > 0 and perturb and u is None) else 0,
                                skip_dead_rgb=bool(skip_dead_rgb and net_c.use_viewdirs))
    return dict(_maps(o, N_importance), z0=o['z0'], raw0=o['raw0'], counts=o['counts'], trans=o['trans'])


def _forward_march(rays11, net, K, cap, lindisp, white_bkgd, occupancy, ert=None, ert_block=32, skip_dead_rgb=False):
    """The marched render (fastnerf_render_rays_fwd_march): the K lattice depths of every ray that `occupancy` calls occupied, packed
    into rows of `cap` slots, one network, one compositing launch.  Returns the maps under render_rays' names plus the packed row
    (raw, march_z, march_k, weights), 'march_overflow' (bool [n]) and 'counts' (device int32 [2] = (evaluated, n * K))."""
    o = ops.render_rays_fwd_march(rays11, net.flat, net.packed()[0], K, cap, occupancy._c, eps=ert, block=ert_block, lindisp=lindisp,
                                  white_bkgd=white_bkgd, skip_dead_rgb=bool(skip_dead_rgb and net.use_viewdirs))
    return dict(rgb_map=o['rgb'], disp_map=o['disp'], acc_map=o['acc'], depth_map=o['depth'], weights=o['w'], raw=o['raw'],
                march_z=o['z'], march_k=o['kidx'], march_overflow=o['overflow'].bool(), counts=o['counts'])


def _pass_maps(maps, k):
    """(g_disp, g_acc, g_depth) of pass k ('1': the pass that produces the image, '0': the coarse pass of two) out of a dict over
    ops.MAP_GRAD_KEYS, or None when none of the three is set."""
    g = tuple((maps or {}).get(name + k) for name in ('g_disp', 'g_acc', 'g_depth'))
    return None if all(t is None for t in g) else g


def _dist_weight_grads(saved, g):
    """The cotangents of 'dist_map' / 'dist0' -> d(loss)/d(weights) of their pass under 'g_w1' / 'g_w0' (ops._weight_grads), or None when
    neither is set: the distortion kernel again, with the cotangent as its per-ray upstream gradient."""
    two = saved['net_f'] is not None
    wg = {}
    for key, k, name in (('dist_map', '1' if two else '0', 'g_w1'), ('dist0', '0', 'g_w0')):
        if g.get(key) is not None and (two or key == 'dist_map'):
            wg[name] = ops.distortion(saved['w' + k], saved['z' + k], saved['rays11'], saved['lindisp'], g_up=g[key], want=('g_w',))[1]
    return wg or None


def _backward_core(saved, g_rgb, g_rgb0, out_c=None, out_f=None, counts=None, maps=None, weight_grads=None):
    """Writes d(loss)/d(params) of the coarse (and fine) net, given d(loss)/d(rgb maps), into
    out_c / out_f (flat, parameter order; default: the nets' flat_grad buffers).  A forward that saved no activations
    (saved['live']) is followed by the compacted backward; `counts` (int32[4], device) then receives the live / total
    point counts of the fine and the coarse pass.  `maps`: None, or d(loss)/d(disp, acc, depth) of the two passes under
    ops.MAP_GRAD_KEYS (one pass: the *1 keys); without any, the calls are those of the colour loss alone.  `weight_grads`: None, or
    d(loss)/d(weights) of the passes under 'g_w1' / 'g_w0' (_dist_weight_grads)."""
    rays11 = saved['rays11']
    has1, has0 = _pass_maps(maps, '1') is not None, _pass_maps(maps, '0') is not None
    map_grads = None
    if has1 or has0:
        map_grads = dict({k: maps.get(k) for k in ops.MAP_GRAD_KEYS}, acc0=saved['acc0'], depth0=saved['depth0'],
                         acc1=saved.get('acc1'), depth1=saved.get('depth1'))
    has1, has0 = has1 or (weight_grads or {}).get('g_w1') is not None, has0 or (weight_grads or {}).get('g_w0') is not None
    dev = rays11.device
    partial = _Workspace.partial(dev)
    net_c, net_f = saved['net_c'], saved['net_f']
    out_c = out_c if out_c is not None else net_c.flat_grad
    if net_f is not None and net_f is not net_c:
        out_f = out_f if out_f is not None else net_f.flat_grad
    n, S0 = saved['z0'].shape
    if saved.get('live'):
        assert net_f is None or net_f is not net_c, 'the compacted backward needs two distinct nets (or one pass)'
        Ni = 0 if net_f is None else saved['z1'].shape[1] - S0
        P = n * (S0 + Ni)
        g_a = g_rgb if (g_rgb is not None or has1) else torch.zeros(n, 3, device=dev)
        g_b = (g_rgb0 if (g_rgb0 is not None or has0) else torch.zeros(n, 3, device=dev)) if Ni > 0 else None
        ws = _Workspace.dact(dev, ops.dact_floats(P) + P * 4)
        draw_ws = ws[ops.dact_floats(P):]
        act_ws = _Workspace.get('act', dev, ops.act_floats(P))
        live_ws = _Workspace.get('live', dev, ops.live_ws_ints(P), torch.int32)
        ops.render_rays_bwd_live(rays11, saved['white'], g_a, g_b, saved['noise0'], saved.get('noise1'), saved['z0'], saved['raw0'],
                                 saved.get('z1'), saved.get('raw1'), net_c.flat, saved['pc'], None if Ni == 0 else net_f.flat,
                                 None if Ni == 0 else saved['pf'], draw_ws, act_ws, ws, partial, live_ws, out_c,
                                 out_f if Ni > 0 else None, S0, Ni, counts=counts, map_grads=map_grads, weight_grads=weight_grads)
        return
    if net_f is None or net_f is not net_c:
        # one C-ABI call: compositing backward + MLP backward for the fine and the coarse pass
        Ni = 0 if net_f is None else saved['z1'].shape[1] - S0
        g_a = g_rgb if (g_rgb is not None or has1) else torch.zeros(n, 3, device=dev)
        g_b = (g_rgb0 if (g_rgb0 is not None or has0) else torch.zeros(n, 3, device=dev)) if Ni > 0 else None
        ws = _Workspace.dact(dev, ops.dact_floats(n * (S0 + Ni)) + n * (S0 + Ni) * 4)
        draw_ws = ws[ops.dact_floats(n * (S0 + Ni)):]
        ops.render_rays_bwd(rays11, saved['white'], g_a, g_b, saved['noise0'], saved.get('noise1'), saved['z0'], saved['raw0'],
                            saved['act0'], saved.get('z1'), saved.get('raw1'), saved.get('act1'), net_c.flat, saved['pc'][1],
                            None if Ni == 0 else net_f.flat, None if Ni == 0 else saved['pf'][1], draw_ws, ws, partial, out_c,
                            out_f if Ni > 0 else None, S0, Ni, map_grads=map_grads, weight_grads=weight_grads)
        return
    # one shared network for both passes (N_importance > 0 without network_fine): accumulate the two gradients
    _backward_passes(saved, g_rgb, g_rgb0, out_c, None, maps=maps, weight_grads=weight_grads)


def _backward_passes(saved, g_rgb, g_rgb0, out_c, out_f, d_rays=None, maps=None, weight_grads=None):
    """The backward of a saving forward pass by pass -- raw2outputs_bwd -> mlp_bwd [-> ray_grad], the fine pass, then the coarse one --
    for what the one-call ops.render_rays_bwd cannot do: one shared network (the fine pass's gradient is added to the coarse
    pass's in out_c) and ray gradients (d_rays [n,11], overwritten: ops.ray_grad reads a pass's `dact` before the next pass
    overwrites it).  Same kernels, inputs and order as the one call, so the parameter gradients are bit-identical to its.  `maps` as
    in _backward_core: a pass with a map gradient goes through raw2outputs_bwd_full, and ops.ray_grad consumes its draw, so rays and
    poses receive the depth / opacity terms (z is a constant of the backward, as in the reference).  `weight_grads` as in _backward_core:
    it travels beside the map gradients of its pass."""
    rays11 = saved['rays11']
    dev = rays11.device
    partial = _Workspace.partial(dev)
    net_c, net_f = saved['net_c'], saved['net_f']
    shared = net_f is net_c
    wg = weight_grads or {}
    # (buffers k, colour gradient, map gradients: with one pass the coarse buffers carry the image pass, whose keys are the *1 ones)
    passes = [('0', net_c, saved['pc'], g_rgb if net_f is None else g_rgb0, _pass_maps(maps, '1' if net_f is None else '0'), out_c,
               wg.get('g_w1' if net_f is None else 'g_w0'))]
    if net_f is not None:
        passes.insert(0, ('1', net_f, saved['pf'], g_rgb, _pass_maps(maps, '1'), torch.empty_like(out_c) if shared else out_f, wg.get('g_w1')))
    for i, (k, net, packed, g, gm, out, gw) in enumerate(passes):
        z, raw, noise, act = saved['z' + k], saved['raw' + k], saved['noise' + k], saved['act' + k]
        if gm is not None or gw is not None:
            gm = gm or (None, None, None)
            draw = ops.raw2outputs_bwd_full(raw, z, rays11, saved['acc' + k], saved['depth' + k], g_rgb=g, g_disp=gm[0], g_acc=gm[1],
                                            g_w=gw, g_depth=gm[2], noise=noise, white_bkgd=saved['white'])
        else:
            if g is None:
                g = torch.zeros(z.shape[0], 3, device=dev)
            draw = ops.raw2outputs_bwd(raw, z, rays11, g, noise, saved['white'])
        dact = _Workspace.dact(dev, ops.dact_floats(z.numel()))
        ops.mlp_bwd(draw, act, net.flat, packed[1], dact, partial, out)
        if d_rays is not None:
            ops.ray_grad(rays11, z, raw, noise, draw, act, dact, net.flat, d_rays=d_rays, accumulate=i > 0)
    if shared:
        out_c.add_(passes[0][5])


_POLICY = LivePolicy()   # the autograd route's policy (the fused Trainer keeps its own)


def _grad_views(flat):
    return list(flat_params.views(flat, param_slices()).values())


def _fn_keys(two, dist=False):
    return (['rgb_map', 'disp_map', 'acc_map', 'raw', 'depth_map'] + (['rgb0', 'disp0', 'acc0', 'z_std', 'depth0'] if two else [])
            + ((['dist_map'] + (['dist0'] if two else [])) if dist else []))


_MAP_OF_KEY = {'disp_map': 'g_disp1', 'acc_map': 'g_acc1', 'depth_map': 'g_depth1', 'disp0': 'g_disp0', 'acc0': 'g_acc0',
               'depth0': 'g_depth0'}


def _fn_outputs(ctx, out):
    """The outputs of the two autograd nodes: every map differentiable, `raw` and `z_std` not.  Cotangents are not materialised:
    a map no loss touches arrives as None in backward, so a loss on the colours alone reaches _backward_core with no map gradient."""
    ctx.keys = _fn_keys('rgb0' in out, 'dist_map' in out)
    outs = tuple(out[k] for k in ctx.keys)
    ctx.mark_non_differentiable(*[o for k, o in zip(ctx.keys, outs) if k in ('raw', 'z_std')])
    ctx.set_materialize_grads(False)
    return outs


def _fn_cotangents(ctx, gouts):
    """-> ({'rgb_map': ., 'rgb0': .} as given, the map gradients under ops.MAP_GRAD_KEYS or None when there is none)."""
    g = {k: (None if t is None else t.contiguous()) for k, t in zip(ctx.keys, gouts)}
    maps = {_MAP_OF_KEY[k]: t for k, t in g.items() if k in _MAP_OF_KEY and t is not None}
    return g, (maps or None)


class _RenderRaysFn(torch.autograd.Function):
    """One autograd node for the whole fused render_rays; inputs are the NeRF parameters so that
    autograd routes the flat gradients to them."""

    @staticmethod
    def forward(ctx, cfg, *params):
        live = _POLICY.use_live(cfg['net_c'], cfg['net_f'], cfg['N_importance'])
        out, saved = _forward_core(save=not live, **cfg)
        ctx.saved = saved
        ctx.n_params = len(params)
        return _fn_outputs(ctx, out)

    @staticmethod
    def backward(ctx, *gouts):
        g, maps = _fn_cotangents(ctx, gouts)
        saved = ctx.saved
        # fresh buffers: autograd accumulates the returned tensors into the parameters' .grad
        # (which may alias the nets' flat_grad), so the kernels must not write there directly
        two = saved['net_f'] is not None and saved['net_f'] is not saved['net_c']
        out_c = torch.empty_like(saved['net_c'].flat)
        out_f = torch.empty_like(saved['net_f'].flat) if two else None
        counts = _Workspace.get('counts', out_c.device, 4, torch.int32) if saved.get('live') else None
        _backward_core(saved, g.get('rgb_map'), g.get('rgb0'), out_c, out_f, counts=counts, maps=maps,
                       weight_grads=_dist_weight_grads(saved, g))
        if counts is not None:
            _POLICY.after_live_step(counts)
        _POLICY.tick()
        grads = saved['net_c'].param_grads_from(out_c) + (saved['net_f'].param_grads_from(out_f) if two else [])
        assert len(grads) == ctx.n_params
        return (None,) + tuple(grads)


class _RenderRaysRayGradFn(torch.autograd.Function):
    """_RenderRaysFn with the ray batch as a further input: the forward always saves its activations (the compacted backward has
    no ray gradients), the backward runs pass by pass (_backward_passes) and returns d(loss)/d(ray_batch) beside the parameter
    gradients, which equal the saving route's bit for bit.  Columns 6:8 (near, far) of the ray gradient are zeros: z is a constant of
    the backward (render.py:281 detaches the fine samples; the coarse ones depend on near / far alone, which are not differentiated)."""

    @staticmethod
    def forward(ctx, cfg, ray_batch, *params):
        out, saved = _forward_core(save=True, **cfg)
        ctx.saved = saved
        ctx.n_params = len(params)
        ctx.ray_like = (ray_batch.shape[-1], ray_batch.dtype)
        return _fn_outputs(ctx, out)

    @staticmethod
    def backward(ctx, *gouts):
        g, maps = _fn_cotangents(ctx, gouts)
        saved = ctx.saved
        two = saved['net_f'] is not None and saved['net_f'] is not saved['net_c']
        out_c = torch.empty_like(saved['net_c'].flat)      # (fresh buffers: see _RenderRaysFn.backward)
        out_f = torch.empty_like(saved['net_f'].flat) if two else None
        d_rays = torch.empty(saved['rays11'].shape[0], 11, device=out_c.device, dtype=torch.float32)
        _backward_passes(saved, g.get('rgb_map'), g.get('rgb0'), out_c, out_f, d_rays=d_rays, maps=maps,
                         weight_grads=_dist_weight_grads(saved, g))
        grads = saved['net_c'].param_grads_from(out_c) + (saved['net_f'].param_grads_from(out_f) if two else [])
        assert len(grads) == ctx.n_params
        width, dtype = ctx.ray_like
        return (None, d_rays[:, :width].to(dtype)) + tuple(grads)


def raw2outputs(raw, z_vals, rays_d, raw_noise_std=0, white_bkgd=False, pytest=False):
    """render.py:149-192 -> (rgb_map, disp_map, acc_map, weights, depth_map).  When `raw` requires grad, all five outputs are
    differentiable w.r.t. `raw` (torch.ops.fastnerf.raw2outputs_full, the reference's autograd formula); `z_vals` and `rays_d`
    are not differentiated (no caller in the reference needs it) and raise when they ask to be."""
    n, S = z_vals.shape
    rays11 = torch.zeros(n, 11, device=z_vals.device, dtype=torch.float32)
    rays11[:, 3:6] = rays_d.detach()
    noise = None
    if raw_noise_std > 0.:
        noise = torch.randn(n, S, device=z_vals.device) * raw_noise_std
        if pytest:
            noise = _pytest_rand((n, S), z_vals.device) * raw_noise_std
    if torch.is_grad_enabled() and raw.requires_grad:
        if z_vals.requires_grad or rays_d.requires_grad:
            raise NotImplementedError('raw2outputs differentiates w.r.t. raw only: z_vals / rays_d must not require grad')
        return torch.ops.fastnerf.raw2outputs_full(raw.float().contiguous(), z_vals.contiguous().float(), rays11, noise, white_bkgd)
    return ops.raw2outputs_fwd(raw.contiguous().float(), z_vals.contiguous().float(), rays11, noise, white_bkgd)


def _unwrap(net):
    return getattr(net, 'module', net) if net is not None else None


def _composite(raw, z, rays11, noise, white_bkgd):
    """Compositing of the closure route: the network's first four channels (a closure may return more, e.g. output_ch = 5),
    differentiable w.r.t. raw through every output when autograd records."""
    raw4 = raw[..., :4].float().contiguous()
    if torch.is_grad_enabled() and rays11.requires_grad:
        # rays that require grad: the op below does not differentiate rays11, and the points / view directions reach the rays
        # through the network in torch.  What is left is dists = dz |d| (render.py:167): relu(sigma') dz |d| = relu(sigma' s) dz |d| with
        # s = |d| / |d|.detach() = 1, so adding sigma' (s - 1) -- an exact zero -- to the logit gives d(loss)/d|d| its term
        # sum_s draw[..., 3] sigma' / |d| (csrc/ray_grad.hip header) without changing a value.  Rays with d = 0: s = 1.
        dn = torch.linalg.norm(rays11[:, 3:6], dim=-1, keepdim=True)
        s1 = torch.where(dn > 0, dn / dn.detach(), torch.ones_like(dn)) - 1.0
        sig = raw4[..., 3].detach() if noise is None else raw4[..., 3].detach() + noise
        raw4 = torch.cat([raw4[..., :3], (raw4[..., 3] + sig * s1)[..., None]], -1)
    if torch.is_grad_enabled() and raw4.requires_grad:
        return torch.ops.fastnerf.raw2outputs_full(raw4, z, rays11, noise, white_bkgd)
    return ops.raw2outputs_fwd(raw4, z, rays11, noise, white_bkgd)


def _query_occupied(network_query_fn, net, rays11, z, viewdirs, occupancy):
    """The closure route's network call through an occupancy grid or cascade: the samples are sorted by it on the device
    (fastnerf_occ_classify / _cascade), `network_query_fn` sees the occupied points only -- pts [L, 1, 3], viewdirs [L, 3] gathered per
    point -- and its rows are scattered into a zero raw [n, S, C].  One host read: the list length sizes the gather."""
    n, S = z.shape
    idx, cnt = occupancy.classify(rays11, z)
    L = int(cnt[0].item())
    live = idx[:L].long()
    ray = torch.div(live, S, rounding_mode='floor')
    pts = (rays11[ray, 0:3] + rays11[ray, 3:6] * z.reshape(-1)[live][:, None])[:, None, :]      # render.py:268, per point
    rows = network_query_fn(pts, None if viewdirs is None else viewdirs[ray], net)
    C = rows.shape[-1]      # (an empty list is an ordinary input: the network is still asked, with 0 points, for its channel count)
    raw = torch.zeros(n * S, C, device=z.device, dtype=rows.dtype)
    raw[live] = rows.reshape(L, C)
    return raw.reshape(n, S, C)


def _render_rays_closure(ray_batch, rays11, network_fn, network_fine, network_query_fn, N_samples, N_importance, retraw, lindisp,
                         perturb, white_bkgd, t_rand, u, noise0, noise1, occupancy=None, retdepth=False, retdist=False):
    """render.py:195-305 for any torch network: sampling, inverse-CDF + merge and compositing run on the HIP kernels, the
    network runs as `network_query_fn(pts, viewdirs, net)` in torch, and autograd reaches its parameters through
    raw2outputs_full.  Random draws follow the fused route (same injected tensors, same host-RNG seed draws)."""
    if network_query_fn is None:
        raise TypeError('render_rays with a network that is not a fastnerf NeRF needs network_query_fn(pts, viewdirs, net)')
    viewdirs = ray_batch[:, -3:] if ray_batch.shape[-1] > 8 else None      # render.py:218
    seed0 = _next_seed() if (perturb and t_rand is None) else 0
    z = ops.sample_coarse(rays11, N_samples, lindisp=lindisp, perturb=bool(perturb), t_rand=t_rand, seed=seed0)
    rays_o, rays_d = rays11[:, 0:3], rays11[:, 3:6]
    if occupancy is not None:
        raw = _query_occupied(network_query_fn, network_fn, rays11, z, viewdirs, occupancy)
    else:
        pts = rays_o[..., None, :] + rays_d[..., None, :] * z[..., :, None]      # render.py:268
        raw = network_query_fn(pts, viewdirs, network_fn)
    rgb, disp, acc, weights, depth = _composite(raw, z, rays11, noise0, white_bkgd)
    ret = {}
    if N_importance > 0:
        ret['rgb0'], ret['disp0'], ret['acc0'] = rgb, disp, acc
        if retdepth:
            ret['depth0'] = depth
        if retdist:
            ret['dist0'] = torch.ops.fastnerf.distortion(weights, z, rays11.detach(), lindisp, None)
        seed1 = _next_seed() if (perturb and u is None) else 0
        # sample_pdf(mid(z), weights[1:-1]) on the detached weights (render.py:279-283) + sort(cat)
        z1, _, z_std = ops.sample_pdf_merge(z, weights.detach().contiguous(), N_importance, det=(perturb == 0.), u=u, seed=seed1,
                                            want_samples=False)
        if occupancy is not None:
            raw = _query_occupied(network_query_fn, network_fine if network_fine is not None else network_fn, rays11, z1, viewdirs,
                                  occupancy)
        else:
            pts = rays_o[..., None, :] + rays_d[..., None, :] * z1[..., :, None]
            raw = network_query_fn(pts, viewdirs, network_fine if network_fine is not None else network_fn)
        z = z1
        rgb, disp, acc, weights, depth = _composite(raw, z, rays11, noise1, white_bkgd)
        ret['z_std'] = z_std
    out = {'rgb_map': rgb, 'disp_map': disp, 'acc_map': acc}
    if retdepth:
        out['depth_map'] = depth
    if retdist:
        out['dist_map'] = torch.ops.fastnerf.distortion(weights, z, rays11.detach(), lindisp, None)
    if retraw:
        out['raw'] = raw
    out.update(ret)
    return out


def render_rays(ray_batch, network_fn, network_query_fn, N_samples, retraw=False, lindisp=False, perturb=0.,
                N_importance=0, network_fine=None, white_bkgd=False, raw_noise_std=0., verbose=False, pytest=False, occupancy=None,
                tighten=False, march=None, march_cap=128, bkgd=None, envmap=None, retdist=False, retdepth=False, ert=None,
                ert_block=32):
    """render.py:195-305.  Two routes, chosen by the networks (after `.module` unwrapping):

    * fastnerf NeRF modules (8 x 256): positional encoding + MLP run fused inside the HIP kernels; `network_query_fn` is
      accepted for signature compatibility and never called.
    * any other torch network (`network_fine` too, when given): `network_query_fn(pts, viewdirs, net)` is called on the
      points of both passes, as the reference does; sampling and compositing still run on the HIP kernels, and every map is
      differentiable w.r.t. the network's parameters.

    A NeRF paired with another kind of network raises TypeError (the fused route would not train the other one).

    `occupancy` (an occupancy.OccupancyGrid or an occupancy.OccupancyCascade, whose first level that contains a sample decides;
    inference only): a sample in a cell whose bit is clear gets raw = 0 without the network being evaluated, in both passes; every
    other sample gets the logits it gets without the grid.  ValueError with
    raw_noise_std > 0 (noise is added to sigma before the relu: a zero sigma is not a dead sample) and when gradients are
    wanted (the training step must not silently change its gradients).

    `tighten=True` (with `occupancy=`; ValueError without): before the coarse depths are placed, near and far of every ray are clamped
    to the part of [near, far] outside which the grid calls no sample occupied (`occupancy.tighten`: fastnerf_occ_ray_bounds, one launch),
    so the N_samples coarse depths spread over the object instead of the scene-wide range.  Exactly render_rays(occupancy.tighten(
    ray_batch)[0], ...): both routes, and with `ert=`.  A ray that meets nothing occupied keeps its bounds and its result.  Stretches
    outside every box count as occupied when the grid's `outside_occupied` is set, so the default grids tighten little:
    outside_occupied=False is the configuration this is for.  The depths change, so the maps differ from the untightened render
    by what the two sets of samples resolve; `tighten=False` (the default) makes exactly the calls it made before.

    `retdepth=True` adds `depth_map` (and `depth0` with two passes), the expected sample distance sum_i w_i z_i of render.py:186,
    to the returned dict on both routes; the default leaves the key set as it is.

    `ert=eps` (0 <= eps < 1; inference only, fused route only) with `ert_block=B`: early ray termination in the pass that produces the
    image -- the fine pass when N_importance > 0, else the only pass.  Its sorted samples are cut into segments of B; a ray's
    transmittance T (fp32, 1 at the start) is multiplied by a segment's product of 1 - alpha + 1e-10 once the segment has its logits, and
    a sample is evaluated only when its ray's T at the start of its segment is > eps (and its occupancy bit is set, with `occupancy=`);
    every other sample gets raw = 0 without the network.  The coarse pass of two is not touched, so rgb0, disp0, acc0, z_std and the fine
    depths are bit-identical to the call without `ert`.  The skipped samples of a ray weigh at most eps in the plain render:
    |d rgb_map| <= eps per channel (white_bkgd or not), 0 <= acc_plain - acc_ert <= eps, |d depth_map| <= eps * z_max.  `disp_map`, a
    quotient of two maps, has NO such bound.  eps = 0 skips only once T is exactly 0: every map is bit-identical to the call without
    `ert`; ert_block >= the number of samples is one segment: nothing is skipped.  ValueError with raw_noise_std > 0, when gradients
    are wanted, and for eps outside [0, 1) or ert_block < 1; NotImplementedError on the closure route.  `ert=None` (the default) makes
    exactly the calls it made before.

    `march=K` (2 <= K < 2^24; with `occupancy=`; inference only, fused route only) with `march_cap=C` (2 <= C <= 512): the marched render
    (include/fastnerf.h, "marched render").  No coarse pass and no inverse-CDF: every ray walks the K unperturbed coarse depths of
    [near, far], keeps the ones the grid calls occupied, and ONE network -- `network_fine` when there is one, else `network_fn` --
    is evaluated on them, packed into rows of C slots (runs of occupied depths, each closed by one entry without logits that gives
    the run's last sample its dense width).  `N_samples` and `N_importance` are not read.  Returns rgb_map, disp_map, acc_map,
    depth_map with `retdepth`, `march_overflow` (bool [n]: the ray has more entries than C slots and was cut there), and with
    `retraw` the packed `raw` [n, C, 4], `march_z` [n, C] and `march_k` (int32 [n, C]: the lattice index, -1 for closing entries and
    padding); no coarse-pass keys.  A ray without overflow whose last lattice depth is empty gets the dense one-pass render through
    the grid at N_samples = K, up to the grouping of fp32 sums.  With `ert=` / `ert_block=` the rows are filled in segments of
    ert_block slots and a ray stops being walked once its transmittance is <= eps (the bounds above, against the marched render
    without `ert`); with `tighten=True` the lattice spans the tightened interval.  ValueError without `occupancy=`, with
    perturb > 0, raw_noise_std > 0, when gradients are wanted, and for K or C out of range; NotImplementedError on the closure route.
    `march=None` (the default) makes exactly the calls it made before.

    Every returned map except `raw` and `z_std` is differentiable w.r.t. the networks' parameters on both routes (render.py:149-192
    under the reference's autograd): rgb_map, disp_map, acc_map, depth_map and their coarse twins, in all three math modes.

    A `ray_batch` that requires grad receives the gradient of those maps w.r.t. the ray batch as the reference's plain-torch
    render_rays gives it: columns o, d (through the sample points and through dists * |d|) and viewdir; near / far (columns 6:8)
    get zeros on the fused route (they are constants there: `render` passes Python floats), and z is a constant of the backward.
    Fused route: math modes 'fp32' and 'bf16x6' (NotImplementedError under 'bf16x3'), always through the saving backward.

    `bkgd` (a colour [3] or per-ray colours [n, 3]; ValueError with white_bkgd=True): the call runs with white_bkgd=False, then
    rgb_map = rgb_map + (1 - acc_map)[:, None] * bkgd, and the same for rgb0 with acc0, in torch -- on every route, with `occupancy=`,
    `ert=` and `march=` as well.  Under autograd that is plain arithmetic on maps that are differentiable already: parameters, rays and a
    pose receive the background's gradient through acc_map.  bkgd = ones has the bits of white_bkgd=True.  `bkgd=None` (the default)
    makes exactly the calls it made before.

    `envmap` (an envmap.EnvMap; ValueError with bkgd= or white_bkgd=True): a trained background behind every ray -- the call with
    bkgd=envmap(ray_batch[:, 3:6]), the map's colours for the unnormalised directions of the batch ([N,8] or [N,11]; include/fastnerf.h,
    "environment map"), on every route.  Under autograd the map's table receives its gradient; the directions get none.

    `retdist=True` adds `dist_map` [n], the distortion loss of mip-NeRF 360 on the weights of every ray's image pass (ops.distortion;
    include/fastnerf.h has the definition), and `dist0` for the coarse pass of two: differentiable w.r.t. the networks' parameters on both
    routes, in all three math modes, through the weights alone (depths, near and far are constants).  A loss adds
    lambda * (dist_map.mean() + dist0.mean()).  With `march=` the row is taken with its overflowed rays skipped (0 there)."""
    if envmap is not None:
        if bkgd is not None or white_bkgd:
            raise ValueError('render_rays: envmap= is the background of every ray: it cannot be combined with bkgd= or white_bkgd=True')
        ops.require_gpu(ray_batch)
        if ray_batch.dim() != 2 or ray_batch.shape[-1] not in (8, 11):
            raise ValueError('ray batches are [N,8] (o, d, near, far) or [N,11] (+ view directions), render.py:216-219')
        bkgd = envmap(ray_batch[:, 3:6])
    if bkgd is not None:
        if white_bkgd:
            raise ValueError('render_rays: bkgd cannot be combined with white_bkgd=True (bkgd = ones is the white background)')
        ret = render_rays(ray_batch, network_fn, network_query_fn, N_samples, retraw=retraw, lindisp=lindisp, perturb=perturb,
                          N_importance=N_importance, network_fine=network_fine, white_bkgd=False, raw_noise_std=raw_noise_std,
                          verbose=verbose, pytest=pytest, occupancy=occupancy, tighten=tighten, march=march, march_cap=march_cap,
                          retdepth=retdepth, ert=ert, ert_block=ert_block, retdist=retdist)
        b = torch.as_tensor(bkgd, dtype=ret['rgb_map'].dtype, device=ret['rgb_map'].device)
        if b.shape != (3,) and b.shape != ret['rgb_map'].shape:
            raise ValueError('render_rays: bkgd is a colour [3] or one colour per ray [n, 3]')
        ret['rgb_map'] = ret['rgb_map'] + (1. - ret['acc_map'])[:, None] * b
        if 'rgb0' in ret:
            ret['rgb0'] = ret['rgb0'] + (1. - ret['acc0'])[:, None] * b
        return ret
    net_c = _unwrap(network_fn)
    net_f = _unwrap(network_fine)
    fused = isinstance(net_c, NeRF)
    if (net_f is not None and isinstance(net_f, NeRF) != fused):
        raise TypeError('render_rays needs either fastnerf NeRF modules for both networks (fused HIP route) or torch networks '
                        'for both, called through network_query_fn (closure route); got a NeRF paired with another network')
    if ray_batch.shape[-1] not in (8, 11):
        raise ValueError('ray batches are [N,8] (o, d, near, far) or [N,11] (+ view directions), render.py:216-219')
    if fused and ray_batch.shape[-1] == 11 and not net_c.use_viewdirs:
        raise ValueError('a ray batch with view directions needs networks built with use_viewdirs=True')
    if fused and ray_batch.shape[-1] == 8 and net_c.use_viewdirs:
        raise ValueError('networks built with use_viewdirs=True need ray batches with view directions [N,11]')
    if tighten and occupancy is None:
        raise ValueError('render_rays: tighten=True clamps near / far to an occupancy grid: it needs occupancy=')
    ops.require_gpu(ray_batch)
    if march is not None:
        K_march, cap_march = ops.check_march(march, march_cap)
        if occupancy is None:
            raise ValueError('render_rays: march= walks an occupancy grid: it needs occupancy=')
        if not fused:
            raise NotImplementedError('render_rays: the marched render (march=) runs on the fused route only (fastnerf NeRF networks); '
                                      'the closure route has none')
        if perturb > 0.:
            raise ValueError('render_rays: the marched render walks a fixed lattice of depths: perturb > 0 has no meaning there')
    if occupancy is not None:
        if raw_noise_std > 0.:
            raise ValueError('render_rays: an occupancy grid cannot be combined with raw_noise_std > 0 (sigma noise is added before '
                             'the relu, so a sample with zero sigma is not dead)')
        nets = [m for m in (net_c, net_f) if isinstance(m, torch.nn.Module)]
        if torch.is_grad_enabled() and (ray_batch.requires_grad or any(p.requires_grad for m in nets for p in m.parameters())):
            raise ValueError('render_rays: an occupancy grid is an inference feature; call it under torch.no_grad() (or with '
                             'parameters and rays that do not require grad)')
    if ert is not None:
        ops.check_ert(ert, ert_block)
        if not fused:
            raise NotImplementedError('render_rays: early ray termination (ert=) runs on the fused route only (fastnerf NeRF networks); '
                                      'the closure route has none')
        if raw_noise_std > 0.:
            raise ValueError('render_rays: early ray termination cannot be combined with raw_noise_std > 0 (sigma noise is added before '
                             'the relu, so a sample with zero sigma is not dead)')
        nets = [m for m in (net_c, net_f) if isinstance(m, torch.nn.Module)]
        if torch.is_grad_enabled() and (ray_batch.requires_grad or any(p.requires_grad for m in nets for p in m.parameters())):
            raise ValueError('render_rays: early ray termination is an inference feature; call it under torch.no_grad() (or with '
                             'parameters and rays that do not require grad)')
    if tighten:
        ray_batch = occupancy.tighten(ray_batch)[0]
    rays11 = ray_batch.contiguous().float()
    if rays11.shape[-1] == 8:      # no view directions: the kernels' direction slots stay zero (their weights are zero too)
        rays11 = torch.cat([rays11, torch.zeros(rays11.shape[0], 3, device=rays11.device)], -1)
    if march is not None:
        net = net_f if net_f is not None else net_c
        out = _forward_march(rays11, net, K_march, cap_march, lindisp, white_bkgd, occupancy, ert, ert_block, skip_dead_rgb=not retraw)
        ret = {'rgb_map': out['rgb_map'], 'disp_map': out['disp_map'], 'acc_map': out['acc_map'], 'march_overflow': out['march_overflow']}
        if retdepth:
            ret['depth_map'] = out['depth_map']
        if retraw:
            ret['raw'], ret['march_z'], ret['march_k'] = out['raw'], out['march_z'], out['march_k']
        if retdist:
            ret.update(_dist_maps(out, rays11, lindisp))
        return ret
    n = rays11.shape[0]
    dev = rays11.device
    t_rand = u = noise0 = noise1 = None
    if perturb > 0. and pytest:
        t_rand = _pytest_rand((n, N_samples), dev)
        if N_importance > 0:
            u = _pytest_rand((n, N_importance), dev)
    if raw_noise_std > 0.:
        if pytest:
            noise0 = _pytest_rand((n, N_samples), dev) * raw_noise_std
            noise1 = _pytest_rand((n, N_samples + N_importance), dev) * raw_noise_std
        else:      # one Philox launch for both passes (the injected-tensor path above stays for pytest=True)
            noise0, noise1 = ops.sigma_noise(n, N_samples, N_samples + N_importance if N_importance > 0 else 0, raw_noise_std, _next_seed(), dev)
    if not fused:
        return _render_rays_closure(ray_batch, rays11, network_fn, network_fine, network_query_fn, N_samples, N_importance, retraw,
                                    lindisp, perturb, white_bkgd, t_rand, u, noise0, noise1, occupancy=occupancy, retdepth=retdepth,
                                    retdist=retdist)
    cfg = dict(rays11=rays11, net_c=net_c, net_f=net_f, N_samples=N_samples, N_importance=N_importance,
               lindisp=lindisp, perturb=perturb, white_bkgd=white_bkgd, t_rand=t_rand, u=u, noise0=noise0,
               noise1=noise1,
               # nobody sees the colour logits of this call: tiles without a live sample may skip them (FN_FWD_SKIP_DEAD_RGB)
               skip_dead_rgb=not retraw, retdist=retdist)
    params = list(net_c.parameters()) + (list(net_f.parameters()) if (net_f is not None and net_f is not net_c) else [])
    if ert is not None:
        out = _forward_ert(rays11, net_c, net_f, N_samples, N_importance, lindisp, perturb, white_bkgd, t_rand, u, ert, ert_block,
                           occupancy=occupancy, skip_dead_rgb=not retraw)
    elif occupancy is not None:
        out = _forward_occ(rays11, net_c, net_f, N_samples, N_importance, lindisp, perturb, white_bkgd, t_rand, u, occupancy,
                           skip_dead_rgb=not retraw)
    elif torch.is_grad_enabled() and ray_batch.requires_grad:
        if ops.get_math() == 'bf16x3':
            raise NotImplementedError("render_rays: rays that require grad need the math mode 'fp32' or 'bf16x6' (FASTNERF_MATH / "
                                      "ops.set_math): 'bf16x3' has no ray-gradient kernel")
        cfg['rays11'] = rays11.detach()
        outs = _RenderRaysRayGradFn.apply(cfg, ray_batch, *params)
        out = dict(zip(_fn_keys(N_importance > 0, retdist), outs))
    elif torch.is_grad_enabled() and any(p.requires_grad for p in params):
        outs = _RenderRaysFn.apply(cfg, *params)
        out = dict(zip(_fn_keys(N_importance > 0, retdist), outs))
    else:
        out, _ = _forward_core(save=False, **cfg)
    ret = {'rgb_map': out['rgb_map'], 'disp_map': out['disp_map'], 'acc_map': out['acc_map']}
    if retdist:      # (the inference forwards through a grid / with early termination: from the weights they return)
        ret.update({k: v for k, v in (out if 'dist_map' in out else _dist_maps(out, rays11, lindisp)).items() if k in ('dist_map', 'dist0')})
    if retdepth:
        ret['depth_map'] = out['depth_map']
    if retraw:
        ret['raw'] = out['raw']
    if N_importance > 0:
        ret['rgb0'], ret['disp0'], ret['acc0'], ret['z_std'] = out['rgb0'], out['disp0'], out['acc0'], out['z_std']
        if retdepth:
            ret['depth0'] = out['depth0']
    return ret


def batchify_rays(rays_flat, chunk=1024 * 32, **kwargs):
    """render.py:12-24.  Per-ray background colours (`bkgd` [N, 3]) are sliced with the chunk."""
    all_ret = {}
    bkgd = kwargs.get('bkgd')
    per_ray = torch.is_tensor(bkgd) and bkgd.dim() == 2
    for i in range(0, rays_flat.shape[0], chunk):
        if per_ray:
            kwargs = dict(kwargs, bkgd=bkgd[i:i + chunk])
        ret = render_rays(rays_flat[i:i + chunk], **kwargs)
        for k in ret:
            all_ret.setdefault(k, []).append(ret[k])
    return {k: (v[0] if len(v) == 1 else torch.cat(v, 0)) for k, v in all_ret.items()}


class _PoseRaysFn(torch.autograd.Function):
    """The ray batch [H*W, 11] of a pinhole camera (HIP get_rays + pack_rays, ndc=False) as a function of its pose c2w [3,4]:
    o = t,  d = R dir,  viewdir v = d / |d|,  dir = ((col - cx) / fx, -(row - cy) / fy, -1)  (run_nerf_helpers.py:68-78, render.py:59-80).
    Backward, from d_rays = (d_o, d_d, ., ., d_v):  d_t = sum d_o,  d_R = sum (d_d + (I - v v^T) d_v / |d|) (x) dir -- twelve
    sums over the image, in torch: not a hot path."""

    @staticmethod
    def forward(ctx, c2w, H, W, K, near, far):
        rays_o, rays_d = get_rays(H, W, K, c2w.detach())
        ctx.cam = (H, W, float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
        ctx.save_for_backward(rays_d.reshape(-1, 3))
        ctx.like = (c2w.device, c2w.dtype)
        return ops.pack_rays(rays_o, rays_d, near, far)

    @staticmethod
    def backward(ctx, d_rays):
        d, = ctx.saved_tensors
        H, W, fx, fy, cx, cy = ctx.cam
        dev = d.device
        row, col = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                                  indexing='ij')
        dirs = torch.stack([(col - cx) / fx, -(row - cy) / fy, -torch.ones_like(col)], -1).reshape(-1, 3)
        d_rays = d_rays.float()
        dn = torch.linalg.norm(d, dim=-1, keepdim=True)
        v = d / dn
        d_v = d_rays[:, 8:11]
        g_d = d_rays[:, 3:6] + (d_v - v * (v * d_v).sum(-1, keepdim=True)) / dn
        d_c2w = torch.cat([g_d.t() @ dirs, d_rays[:, 0:3].sum(0)[:, None]], -1)
        return d_c2w.to(device=ctx.like[0], dtype=ctx.like[1]), None, None, None, None, None


def render(H, W, K, chunk=1024 * 32, rays=None, c2w=None, ndc=True, near=0., far=1., use_viewdirs=False,
           c2w_staticcam=None, **kwargs):
    """render.py:26-91 -> [rgb_map, disp_map, acc_map, extras].  A tensor `c2w` that requires grad receives the gradient of
    every differentiable map (render_rays) through the rays (_PoseRaysFn); with ndc=True or c2w_staticcam that raises NotImplementedError.
    `bkgd=` (render_rays): a colour [3], or one colour per ray in the shape of the rays ([H, W, 3] or [N, 3]).
    `envmap=` (render_rays): looked up chunk by chunk from the rays' directions; ValueError with ndc=True (NDC directions are not the
    scene's)."""
    if kwargs.get('envmap') is not None and ndc:
        raise ValueError('render: envmap= indexes the table by the ray direction: not with ndc=True (the NDC far plane is infinity)')
    bkgd = kwargs.get('bkgd')
    if bkgd is not None and not (torch.is_tensor(bkgd) and bkgd.dim() == 1):
        bkgd = torch.as_tensor(bkgd, dtype=torch.float32)
        kwargs = dict(kwargs, bkgd=bkgd if bkgd.dim() == 1 else bkgd.reshape(-1, 3))
    if torch.is_tensor(c2w) and c2w.requires_grad and torch.is_grad_enabled():
        if ndc or c2w_staticcam is not None:
            raise NotImplementedError('render: a pose that requires grad is differentiated through plain pinhole rays only '
                                      '(ndc=False, no c2w_staticcam)')
        sh = (H, W, 3)
        rays11 = _PoseRaysFn.apply(c2w[:3, :4], H, W, K, float(near), float(far))
        if not use_viewdirs:
            rays11 = rays11[:, :8]
    else:
        if c2w is not None:
            rays_o, rays_d = get_rays(H, W, K, c2w)
        else:
            rays_o, rays_d = rays
        ops.require_gpu(rays_o, rays_d)
        view_o, view_d = rays_o, rays_d
        if use_viewdirs and c2w_staticcam is not None:   # (render.py:59-66: the static camera only exists inside this branch)
            rays_o, rays_d = get_rays(H, W, K, c2w_staticcam)
        sh = rays_d.shape
        rays11 = ops.pack_rays(rays_o, rays_d, near, far, ndc=ndc, H=H, W=W, focal=float(K[0][0]))
        if not use_viewdirs:
            rays11 = rays11[:, :8].contiguous()           # [N,8]: o, d, near, far (render.py:74-78)
        elif c2w_staticcam is not None:
            # viewdirs come from the moving camera, origins/directions from the static one
            rays11[:, 8:11] = ops.pack_rays(view_o, view_d, near, far)[:, 8:11]
    all_ret = batchify_rays(rays11, chunk, **kwargs)
    for k in all_ret:
        all_ret[k] = torch.reshape(all_ret[k], list(sh[:-1]) + list(all_ret[k].shape[1:]))
    k_extract = ['rgb_map', 'disp_map', 'acc_map']
    return [all_ret[k] for k in k_extract] + [{k: all_ret[k] for k in all_ret if k not in k_extract}]


def render_path(render_poses, hwf, K, chunk, render_kwargs, gt_imgs=None, savedir=None, render_factor=0):
    """render.py:94-146 without the LPIPS dependency (external, optional in the reference env):
    renders every pose, reports PSNR and SSIM when ground truth is given, writes PNGs when imageio exists."""
    H, W, focal = hwf
    if render_factor != 0:
        H, W, focal = H // render_factor, W // render_factor, focal / render_factor
    rgbs, disps, psnrs, ssims = [], [], [], []
    with torch.no_grad():
        for i, c2w in enumerate(render_poses):
            rgb, disp, acc, _ = render(H, W, K, chunk=chunk, c2w=torch.as_tensor(c2w)[:3, :4], **render_kwargs)
            rgbs.append(rgb.cpu().numpy())
            disps.append(disp.cpu().numpy())
            if gt_imgs is not None and render_factor == 0:
                gt = gt_imgs[i].cpu().numpy() if torch.is_tensor(gt_imgs[i]) else np.asarray(gt_imgs[i])
                psnrs.append(-10. * np.log10(np.mean(np.square(rgbs[-1] - gt))))
                ssims.append(float(compute_ssim(torch.as_tensor(gt).float(), rgb.cpu())))
            if savedir is not None:
                try:
                    import imageio
                    imageio.imwrite(os.path.join(savedir, '{:03d}.png'.format(i)), to8b(rgbs[-1]))
                except ImportError:
                    np.save(os.path.join(savedir, '{:03d}.npy'.format(i)), to8b(rgbs[-1]))
    if psnrs and savedir is not None:
        with open(os.path.join(savedir, 'results.txt'), 'w') as f:
            f.write('mean PSNR: {}\nmean SSIM: {}\n'.format(np.mean(psnrs), np.mean(ssims)))
    render_path.last_psnrs = psnrs
    render_path.last_ssims = ssims
    return np.stack(rgbs, 0), np.stack(disps, 0)
