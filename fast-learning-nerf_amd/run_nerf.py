"""Training driver surface -- mirror of nerf-ours/run_nerf.py for the hot path.

create_nerf (run_nerf.py:67-153) returns the same 6-tuple and the same render_kwargs keys;
batchify / run_network (:40-64) keep their signatures.  `Trainer` is the fused,
autograd-free optimisation step (render + 2xMSE + backward + all-reduce + Adam + LR decay,
run_nerf.py:479-508) that the benchmark and `train()` use; the autograd-compatible route
(`render(...)`, `loss.backward()`, `optimizer.step()`) stays available through render.py.
Dataset readers / CLI parsing are out of scope; `train()` takes
in-memory images + poses.
"""
import ctypes
import math
import os
import time

import numpy as np
import torch

from . import _lib, flat_params, ops, parallel
from .model import NeRF, noview_slices
from .render import LivePolicy, _Workspace, get_compact, _backward_core, _backward_passes, _forward_core, _next_seed, render, render_path  # noqa: F401
from .run_nerf_helpers import get_embedder, img2mse, mse2psnr
from .tree import QuadTreeManager


def batchify(fn, chunk):
    """run_nerf.py:40-47."""
    if chunk is None:
        return fn

    def ret(inputs):
        return torch.cat([fn(inputs[i:i + chunk]) for i in range(0, inputs.shape[0], chunk)], 0)
    return ret


def run_network(inputs, viewdirs, fn, embed_fn=None, embeddirs_fn=None, netchunk=1024 * 64):
    """run_nerf.py:50-64: PE + MLP on explicit points [N,S,3] with per-ray viewdirs [N,3].
    A fastnerf NeRF runs the fused HIP forward (forward only) by expressing every point as a ray with o=pt, d=0.  Any other
    torch network runs as the reference does: flatten, `embed_fn` (get_embedder's HIP positional encoding), expanded and
    embedded viewdirs when given, `batchify(fn, netchunk)`, reshape -- differentiable w.r.t. the network's parameters."""
    net = getattr(fn, 'module', fn)
    if not isinstance(net, NeRF):
        if embed_fn is None:
            raise TypeError('run_network with a network that is not a fastnerf NeRF needs embed_fn (run_nerf.py:50-64)')
        inputs_flat = torch.reshape(inputs, [-1, inputs.shape[-1]])
        embedded = embed_fn(inputs_flat)
        if viewdirs is not None:
            if embeddirs_fn is None:
                raise TypeError('run_network: viewdirs given without embeddirs_fn')
            input_dirs = viewdirs[:, None].expand(inputs.shape)
            input_dirs_flat = torch.reshape(input_dirs, [-1, input_dirs.shape[-1]])
            embedded = torch.cat([embedded, embeddirs_fn(input_dirs_flat)], -1)
        outputs_flat = batchify(fn, netchunk)(embedded)
        return torch.reshape(outputs_flat, list(inputs.shape[:-1]) + [outputs_flat.shape[-1]])
    ops.require_gpu(inputs, viewdirs)
    if (viewdirs is not None) != net.use_viewdirs:
        raise ValueError('viewdirs must be given exactly when the network was built with use_viewdirs=True')
    sh = inputs.shape
    pts = inputs.reshape(-1, 3).float()
    P = pts.shape[0]
    rays11 = torch.zeros(P, 11, device=pts.device, dtype=torch.float32)
    rays11[:, 0:3] = pts
    if viewdirs is not None:
        rays11[:, 8:11] = viewdirs[:, None].expand(sh).reshape(-1, 3)
    z = torch.zeros(P, 1, device=pts.device, dtype=torch.float32)
    raw = ops.mlp_fwd(rays11, z, net.flat, net.packed()[0])
    return raw.reshape(list(sh[:-1]) + [4])


class _Args:
    """Defaults of argument_parser.py:4-123 for the flags the hot path reads."""
    netdepth = 8; netwidth = 256; netdepth_fine = 8; netwidth_fine = 256
    N_rand = 32 * 32 * 4; lrate = 5e-4; lrate_decay = 250; chunk = 1024 * 32; netchunk = 1024 * 64
    no_batching = True; no_reload = False; ft_path = None
    N_samples = 64; N_importance = 0; perturb = 1.; use_viewdirs = True; i_embed = 0
    multires = 10; multires_views = 4; raw_noise_std = 0.
    dataset_type = 'blender'; white_bkgd = False; no_ndc = False; lindisp = False
    random_bkgd = False      # (not in the reference's parser) RGBA training over a fresh background colour per ray
    lambda_dist = 0.         # (not in the reference's parser) weight of the distortion loss on the ray weights (Trainer(lambda_dist=))
    refine_poses = False; pose_lrate = 1e-3      # (not in the reference's parser) refine the camera poses beside the field (Trainer(poses=))
    optim_autoexpo = False; lambda_autoexpo = 1.      # (nerf++-ours' parser) fit a per-image exposure beside the field (Trainer(exposure=))
    envmap = False; envmap_res = 64; envmap_lrate = 1e-2      # (not in the reference's parser) a trained background behind every ray (Trainer(envmap=))
    band_window = None; band_start = 0; band_end = 0; band_view = True      # (not in the reference's parser) coarse-to-fine encoding: 'cosine' | 'linear' ramp of the band weights over steps band_start .. band_end (Trainer(bands=))
    n_epoch = 12; init_level = 3; rays_downscale = 1; subdivide_every = 1; subdivide_thres = 0.015
    randSamp_perc = 0.5; basedir = './logs'; expname = 'fastnerf'

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def make_args(**kw):
    return _Args(**kw)


def create_nerf(args, device='cuda'):
    """run_nerf.py:67-153 -> (render_kwargs_train, render_kwargs_test, start_epoch, start_iter,
    grad_vars, optimizer).  Both nets live in ONE flat parameter / gradient buffer (coarse first,
    as in `grad_vars`), which is what the fused Trainer and the RCCL all-reduce operate on."""
    if args.multires != 10 or (args.use_viewdirs and args.multires_views != 4) or args.i_embed != 0:
        raise NotImplementedError('HIP path implements multires=10, multires_views=4, i_embed=0')
    embed_fn, input_ch = get_embedder(args.multires, args.i_embed)
    embeddirs_fn, input_ch_views = None, 0                    # run_nerf.py:73-76
    if args.use_viewdirs:
        embeddirs_fn, input_ch_views = get_embedder(args.multires_views, args.i_embed)
    two = args.N_importance > 0
    n_nets = 2 if two else 1
    dev = torch.device(device)
    output_ch = 5 if two else 4
    N = ops.NET_PARAMS if args.use_viewdirs else noview_slices(output_ch)[1]   # parameters per net
    flat_all = torch.empty(n_nets * N, device=dev, dtype=torch.float32)
    grad_all = torch.zeros(n_nets * N, device=dev, dtype=torch.float32)
    model = NeRF(D=args.netdepth, W=args.netwidth, input_ch=input_ch, output_ch=output_ch, skips=[4],
                 input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs, device=dev, flat=flat_all[:N],
                 flat_grad=grad_all[:N])
    grad_vars = list(model.parameters())
    model_fine = None
    if two:
        model_fine = NeRF(D=args.netdepth_fine, W=args.netwidth_fine, input_ch=input_ch, output_ch=output_ch,
                          skips=[4], input_ch_views=input_ch_views, use_viewdirs=args.use_viewdirs, device=dev,
                          flat=flat_all[N:], flat_grad=grad_all[N:])
        grad_vars += list(model_fine.parameters())
    network_query_fn = lambda inputs, viewdirs, network_fn: run_network(inputs, viewdirs, network_fn,
                                                                        embed_fn=embed_fn, embeddirs_fn=embeddirs_fn,
                                                                        netchunk=args.netchunk)
    optimizer = torch.optim.Adam(params=grad_vars, lr=args.lrate, betas=(0.9, 0.999))
    start_epoch, start_iter = 0, 0
    # checkpoints: same file layout as run_nerf.py:109-127 / 532-539
    ckpts = []
    if args.ft_path is not None and args.ft_path != 'None':
        ckpts = [args.ft_path]
    else:
        d = os.path.join(args.basedir, args.expname)
        if os.path.isdir(d):
            ckpts = [os.path.join(d, f) for f in sorted(os.listdir(d)) if 'tar' in f]
    create_nerf.last_ckpt_path = None
    if len(ckpts) > 0 and not args.no_reload:
        ckpt = torch.load(ckpts[-1], map_location=dev, weights_only=False)
        create_nerf.last_ckpt_path = ckpts[-1]
        start_epoch, start_iter = ckpt['global_epoch'], ckpt['global_iter']
        optimizer.load_state_dict(ckpt['optimizer_state_dict'])
        model.load_state_dict(ckpt['network_fn_state_dict'])
        if model_fine is not None:
            model_fine.load_state_dict(ckpt['network_fine_state_dict'])
    render_kwargs_train = {
        'network_query_fn': network_query_fn, 'perturb': args.perturb, 'N_importance': args.N_importance,
        'network_fine': model_fine, 'N_samples': args.N_samples, 'network_fn': model,
        'use_viewdirs': args.use_viewdirs, 'white_bkgd': args.white_bkgd, 'raw_noise_std': args.raw_noise_std,
    }
    if args.dataset_type != 'llff' or args.no_ndc:
        render_kwargs_train['ndc'] = False
        render_kwargs_train['lindisp'] = args.lindisp
    render_kwargs_test = {k: render_kwargs_train[k] for k in render_kwargs_train}
    render_kwargs_test['perturb'] = False
    render_kwargs_test['raw_noise_std'] = 0.
    create_nerf.flat_all, create_nerf.grad_all = flat_all, grad_all
    model._flat_all, model._grad_all = flat_all, grad_all
    if args.use_viewdirs:      # NeRF.set_bands: the effective buffers of the two networks are one allocation too, laid out like flat_all
        pool = {'params': flat_all}
        for i, net in enumerate([model] + ([model_fine] if two else [])):
            net._band_pool, net._band_slot = pool, slice(i * N, (i + 1) * N)
    return render_kwargs_train, render_kwargs_test, start_epoch, start_iter, grad_vars, optimizer


def _region(block, regions, name):
    """The tensor of region `name` (_step_regions) as a view into a step's block."""
    off, shape = regions[name]
    return block[off:off + math.prod(shape)].view(shape)


class _StepOut:
    """The tensors of one fused step as a read-only mapping with the keys of render_rays' output dict (plus the extras the
    fused Trainer has always returned); views into the step's output block are built on first access."""

    def __init__(self, block, regions, names):
        self._block, self._regions, self._names, self._cache = block, regions, names, {}

    def __getitem__(self, key):
        t = self._cache.get(key)
        if t is None:
            t = self._cache[key] = _region(self._block, self._regions, self._names[key])
        return t

    def __contains__(self, key):
        return key in self._names

    def get(self, key, default=None):
        return self[key] if key in self._names else default

    def keys(self):
        return self._names.keys()

    def __iter__(self):
        return iter(self._names)

    def __len__(self):
        return len(self._names)


def _lay_out(shapes, regions, off):
    """`regions` with (name, shape) of `shapes` appended from float `off` on, each on a 256-byte boundary.  -> (regions, the end)"""
    for name, shape in shapes:
        regions[name] = (off, shape)
        off += (math.prod(shape) + 63) // 64 * 64
    return regions, off


def _step_regions(n, S0, Ni):
    """name -> (offset, shape) of the per-step tensors inside one fp32 block (every region starts on a 256-byte boundary),
    and the block's size."""
    S1 = S0 + Ni
    shapes = [('rays11', (n, 11)), ('z0', (n, S0)), ('raw0', (n, S0, 4)), ('rgb0', (n, 3)), ('disp0', (n,)), ('acc0', (n,)),
              ('w0', (n, S0)), ('depth0', (n,)), ('g_rgb', (n, 3)), ('loss2', (2,))]
    if Ni > 0:
        shapes += [('z1', (n, S1)), ('z_samples', (n, Ni)), ('z_std', (n,)), ('raw1', (n, S1, 4)), ('rgb1', (n, 3)),
                   ('disp1', (n,)), ('acc1', (n,)), ('w1', (n, S1)), ('depth1', (n,)), ('g_rgb0', (n, 3))]
    return _lay_out(shapes, {}, 0)


def _term_regions(base, size, n, S0, Ni, aux=False, bkgd=False, dist=False, expo=None):
    """The table `base` of `size` floats (_step_regions(n, S0, Ni); not built again, and handed back as it is when no term is on)
    with the tensors of the optional terms that are on behind it, in the order aux | bkgd | dist | expo: region '<term>.<member>' is
    what the pointer member of that name of the term's struct (fn_step_aux / fn_step_bkgd / fn_step_dist / fn_step_expo) points to.  expo:
    None, or (n_img, the floats of its scratch); its counts are int32 in a region of as many words.  A new term is one more list here.
    -> (regions, the block's size)"""
    shapes = []
    if aux:
        shapes += [('aux.' + k, (n,)) for k in ('g_depth1', 'g_acc1', 'g_depth0', 'g_acc0')] + [('aux.loss4', (4,))]
    if bkgd:
        shapes += [('bkgd.bkgd_used', (n, 3)), ('bkgd.target_ws', (n, 3)), ('bkgd.g_acc1', (n,)), ('bkgd.g_acc0', (n,))]
    if dist:      # (the *0 rows of aux and bkgd, and ell0, are laid out with one pass too; g_w0 would be empty)
        shapes += ([('dist.ell1', (n,)), ('dist.ell0', (n,)), ('dist.g_w1', (n, S0 + Ni))] + ([('dist.g_w0', (n, S0))] if Ni > 0 else [])
                   + [('dist.loss2d', (2,))])
    if expo:
        shapes += ([('expo.e1', (n, 3))] + ([('expo.e0', (n, 3))] if Ni > 0 else [])
                   + [('expo.ws', (expo[1],)), ('expo.d_ab', (expo[0], 2)), ('expo.counts', (expo[0],)), ('expo.loss_reg', (1,))])
    return _lay_out(shapes, dict(base), size) if shapes else (base, size)


def _term_table(regions, term):
    """The regions of one optional term under its members' names."""
    return {name[len(term) + 1:]: r for name, r in regions.items() if name.startswith(term + '.')}


def _term_struct(cls, term, block, regions, **members):
    """The ctypes struct of a term: every pointer member that has a region points into `block`; `members`: the others."""
    s, base = cls(), block.data_ptr()
    for name, (off, _) in _term_table(regions, term).items():
        setattr(s, name, base + 4 * off)
    for name, value in members.items():
        setattr(s, name, value)
    return s


def _ref(struct):
    return None if struct is None else ctypes.byref(struct)


_OUT_NAMES_2 = {'rgb_map': 'rgb1', 'disp_map': 'disp1', 'acc_map': 'acc1', 'raw': 'raw1', 'rgb0': 'rgb0', 'disp0': 'disp0',
                'acc0': 'acc0', 'z_std': 'z_std', 'weights': 'w1', 'z_vals': 'z1', 'depth_map': 'depth1',
                'z_samples': 'z_samples', 'weights0': 'w0', 'z0': 'z0'}
_OUT_NAMES_1 = {'rgb_map': 'rgb0', 'disp_map': 'disp0', 'acc_map': 'acc0', 'raw': 'raw0', 'weights': 'w0', 'z_vals': 'z0',
                'depth_map': 'depth0'}


class Trainer:
    """Fused optimisation step over rays sharded across ranks (one process per GPU).

    step(): render (perturbed, hierarchical) -> loss = mse(fine) + mse(coarse) -> analytic backward
    -> RCCL all-reduce(SUM) of the flat gradient (grads are pre-scaled by n_local/N_global, so the
    sum is the gradient of the global-batch mean) -> Adam over both nets in one launch -> LR decay
    with the reference's pre-increment rule (run_nerf.py:498-508).

    occupancy (opt-in; an occupancy.OccupancyGrid, usually OccupancyGrid.for_training(), or a training OccupancyCascade, usually
    OccupancyCascade.for_training(): wherever "grid" stands below, on the fused, `tighten` and `march=` routes and with every term,
    the cascade's lookup takes the grid's place (fastnerf_train_step_cascade / _march_cascade), its refresh runs over the own cells
    of its levels, `occupancy_cells` of them per refresh, and a one-level cascade is its grid bit for bit; a cascade in which some
    level has no density raises ValueError: it is for rendering): the first forward of each pass
    evaluates the networks on the samples in occupied cells only; a sample in an empty cell gets raw = (0, 0, 0, 0), whose
    d(loss)/d(raw) is exactly zero, so the compacted backward needs no change.  The first `occupancy_warmup` steps leave the
    grid untouched; from then on a grid with a density is refreshed (`grid.update`) every `occupancy_every` steps, by at most
    `occupancy_cells` cells per refresh when that is set.  While a grid is set the step ALWAYS takes the compacted route:
    LivePolicy still measures the live fraction but may not switch to the plain backward, which has no list to run over
    (FASTNERF_COMPACT=0, one network shared by both passes and FASTNERF_FUSED_STEP=0 are ValueErrors), and
    raw_noise_std > 0 is a ValueError (noise is added before the relu: a zero sigma is not a dead sample).
    `occupancy_counts`: device int32 [4] = (occupied, total) samples of the coarse pass, then of the fine pass, of the last step
    (None without a grid).  A step on an empty batch (a data-parallel tail) neither renders nor refreshes the grid.
    `tighten=True` (with a grid; ValueError without, or off the fused step): between packing the rays and the forward, near and far
    of every ray are clamped to the part of [near, far] outside which the grid -- its bits as they are at that step, nothing is
    cached across `grid.update` -- calls no sample occupied (fastnerf_occ_ray_bounds, FN_STEP_TIGHTEN), so the coarse depths spread
    over the object.  A ray that meets nothing occupied keeps its bounds.  Stretches outside the box count as occupied when the grid's
    `outside_occupied` is set, so the default grid tightens little: OccupancyGrid.for_training(outside_occupied=False) is the
    configuration this is for.  It raises the occupied fraction of a step's samples (`occupancy_counts`): a step may get slower
    while each sample does more.

    Depth / opacity supervision (lambda_depth, lambda_acc; step(..., depth=, depth_weight=, acc=, acc_weight=), [n] each): the step
    minimises mse(fine) + mse(coarse) + lambda_depth (Ld_fine + Ld_coarse) + lambda_acc (La_fine + La_coarse) with
    L = mean_r w_r (map[r] - target[r])^2 on depth_map / acc_map of both passes (ops.aux_loss; weights default to ones, a ray
    with weight 0 is ignored whatever its target holds -- sparse depth is "NaN where unknown, weight 0").  A term is on when its
    target is given AND its lambda is not 0; with no term on, the step is the step without these keywords, launch for launch.
    `aux_losses`: device tensor [4] = (Ld_fine, Ld_coarse, La_fine, La_coarse) of the last step, unscaled by the lambdas (zeros
    for a term that is off, and after an empty batch); the return value of step() is unchanged.  Both routes, the plain and the
    compacted backward, an occupancy grid and n_global scaling take the terms; they make every sample with positive density of a
    ray that is not yet opaque live (render.LivePolicy), so early compacted steps run over more points than under the colour loss.

    Marched training (`march=K` with `march_cap=C`, `march_after=M`; with a grid whose `outside_occupied` is False; include/fastnerf.h,
    "marched training"): the steps with `occupancy_steps < M` are the step through the grid above, launch for launch -- that is how the
    grid gets warm before the lattice relies on it.  Every later step trains ONE network, `network_fine` when there is one, else
    `network_fn` (the network render_rays(..., march=K) renders with), on the packed rows of a lattice of K depths per ray that is
    shifted per ray by u in [0, 1) of its spacing: no coarse pass, no inverse-CDF, one fastnerf_train_step_march call.  `perturb`
    switches the shift (seeded from `_next_seed()`); step(..., march_u=) injects [n] shifts.  A ray whose row overflows C slots does
    not train the field (its colour gradient is zeroed; the loss stays the mean over all rays).  The other network, its moments and
    its packed weights are left untouched, and the grid is refreshed from the marched network alone.  `march_counts`: device int32
    [2] = (evaluated samples, n * K) of the last marched step.  The step's `out` holds rgb_map, disp_map, acc_map, depth_map and
    march_overflow (bool [n]) (+ raw, weights, z_vals, march_k of the packed row).  `tighten=True` combines: the lattice spans the
    clamped interval.  ValueError: march without a grid, a grid with outside_occupied=True (every lattice point outside the box would be
    live and the rows would overflow), a depth / opacity term that is on, raw_noise_std > 0, forward_backward, a trainer off the fused
    step.  No early ray termination while training.

    Per-ray background colours (`bkgd`: None, 'random' or a colour of 3 floats; read on every step, like white_bkgd; include/fastnerf.h,
    "per-ray background colours"): the step composites with white_bkgd=False, puts a colour b_r behind every ray of both passes,
    rgb += (1 - acc) b, and -- with step(..., alpha=[n]), the alpha of an RGBA target whose colours are straight -- behind the target,
    t' = t a + (1 - a) b; the loss and the leaf-error table see the blended maps and target.  'random' draws fresh colours every step
    (one `_next_seed()` after the step's other draws), step(..., bkgd=[n,3]) injects them, a constant colour is every ray's.  Density
    where the image is transparent then always costs, which a fixed colour cannot promise.  out['bkgd'] [n,3] holds the colours used;
    out['rgb_map'] / out['rgb0'] are the blended maps.  What the blend sends back to the opacity maps, -(g_rgb . b), reaches the field
    through the full-gradient compositing backward, added to the opacity term's rows when lambda_acc is on; like that term it makes every
    sample with positive density of a ray that is not yet opaque live.  All routes take it: the fused step (plain, compacted, through a
    grid, tighten), the marched step and the call-by-call route.  ValueError: together with white_bkgd (bkgd=(1, 1, 1) is white), an
    alpha with no background on.

    Distortion loss (`lambda_dist`, read on every step; include/fastnerf.h, "distortion loss"): the step also minimises lambda_dist
    (Ldist_fine + Ldist_coarse), Ldist = the batch mean of the mip-NeRF 360 distortion loss of a pass's weights over its normalised
    intervals -- the term that removes floaters and half-transparent fog.  It reaches the field through the weights alone (depths, near
    and far are constants), as d(loss)/d(weights) rows handed to the full-gradient compositing backward of its pass.  `dist_losses`:
    device tensor [2] = (Ldist_fine, Ldist_coarse) of the last step, unscaled (the second 0 with one pass; zeros when off and after an
    empty batch); out['dist_map'] (and out['dist0']) hold the per-ray values.  All routes take it: the fused step (plain, compacted,
    through a grid, tighten), the marched step -- there on the packed row, an overflowed ray skipped -- and the call-by-call route;
    nothing else of the marched step's restrictions is lifted.  Like the opacity term it makes every sample with positive density of a ray
    that is not yet opaque live, so early compacted steps run over more points.  lambda_dist = 0 (the default): the step without it,
    launch for launch.  ValueError for a negative or non-finite lambda_dist.

    Pose refinement (`poses=` a poses.PoseTable, `pose_lrate`; include/fastnerf.h, "pose table"): step(None, None, target, pix=[n,3]
    int (image, row, col)) makes the poses from the table and the rays from the pixels (ops.pose_exp, gen_rays_pixels), steps on the
    call-by-call route with the saving backward forced and ops.ray_grad between the passes (forward_backward(d_rays=True); the fused
    step reuses the buffers ray_grad reads), carries out['d_rays'] down to `pose_grad` [n_img,6] = d(loss)/d(xi) (ops.pose_grad,
    ops.pose_exp_bwd), takes an Adam step on xi with moments of its own (`pose_m`, `pose_v`) at pose_lrate times the decay factor the
    networks' rate has, then the networks' update.  The network gradients, the loss and the maps are those of the call-by-call step on
    the same rays, bit for bit; every term above, leaf_tag / table, white_bkgd and networks without view directions pass through
    unchanged.  An image without a ray in the batch has a zero gradient.  Without `poses=` nothing changes.  ValueError: pix without
    poses= or poses= without pix, rays together with pix, occupancy= / tighten / march, data parallel.  NotImplementedError: ndc=True,
    the math mode bf16x3 (no ray gradients).

    Per-image exposure (`exposure=` an exposure.ExposureTable, `lambda_autoexpo`, `exposure_lrate`; include/fastnerf.h, "exposure
    table"): step(..., img=[n] int), the image of every ray (with pix= the default is pix[:, 0]).  The colour loss and the leaf-error table
    see e = (rgb - shift_i) / scale_i of both passes, i = img[r]; the step also minimises lambda_autoexpo times the batch mean of
    |scale_i - 1| + |shift_i|; out['rgb_map'] / out['rgb0'] stay the scene's colours.  `expo_grad` [n_img,2] = d(loss)/d(table.ab),
    `expo_counts` int32 [n_img] the rays per image and `expo_loss` [1] the unscaled penalty of the last step; then an Adam step on the
    table with moments of its own (`expo_m`, `expo_v`) at exposure_lrate (None: the networks' rate) times the networks' decay factor.  An
    image without a ray has a zero gradient; a ray whose img is outside the table is left as it is.  A fresh table (rows (0.5, 0))
    reproduces the step without it bit for bit.  All routes take it: the fused step (plain, compacted, through a grid, tighten), the
    marched step (an overflowed ray gives the table nothing), the call-by-call route and the pose step.  Without `exposure=` nothing
    changes.  ValueError: exposure= without img / pix, img without exposure=, a negative or non-finite lambda_autoexpo, data parallel.

    Environment map (`envmap=` an envmap.EnvMap, `envmap_lrate`; include/fastnerf.h, "environment map"): a trained background behind
    every ray, for captures that look past the box.  Every step looks the colours up from rays_d (ops.env_lookup; on the pose route the
    rays are made from pix first) and hands them in as the injected per-ray background above, so the step is the step with
    bkgd=env(rays_d), launch for launch; out['bkgd'] holds them.  Once the colour gradients stand -- behind the forward phase of the fused
    and the marched step, which are then called phase by phase, behind the loss launches of the call-by-call route; the exposure term
    has rescaled them by then -- ops.env_grad scatters (1 - acc) g_rgb of both passes into `env_grad` [R,R,3] = d(loss)/d(table), and the
    table takes an Adam step with moments of its own (`env_m`, `env_v`) at envmap_lrate (1e-2: a guess, not a tuned value) times the
    networks' decay factor.  A marched ray whose row overflowed has g_rgb = 0 and gives the table exactly nothing.  The table does not
    enter the pose gradient: a direction's colour is a constant of the ray.  All routes take it: the fused step (plain, compacted, through a
    grid, tighten), the marched step, the call-by-call route, the pose step, with an exposure table.  Without `envmap=` nothing changes,
    launch for launch.  ValueError, before any launch: together with bkgd= (trainer or step) or alpha= (a capture with alpha has no
    background to learn), white_bkgd, ndc=True (the NDC far plane is infinity), data parallel, a table on another device.

    Band weights (`bands=` a bands.BandSchedule; include/fastnerf.h, "band weights"; DESIGN.md, "Band weights"): coarse-to-fine positional
    encodings.  Before every step the networks get the schedule's column weights for that step (NeRF.set_bands; the step index is the
    number of steps taken, `adam_t`; uploaded only when they changed).  The kernels then run on the effective networks -- the parameters
    with the encoding columns of layer 0, the skip layer and the view layer times w -- so the fused and the marched step are called without
    FN_STEP_UPDATE on the effective buffers and `_band_update` follows: ops.band_grad into `grad` (the parameters' gradient), Adam on `flat`
    (the parameters) with `m` / `v`, the next step's weights, ops.band_apply and the re-pack; the call-by-call and the pose route end in
    `_host_update`, which calls the same.  Every term, table, grid and route above passes through untouched.  `flat`, `grad`, `m`, `v`, the
    networks' state dicts and the checkpoints are always the parameters'.  Once `bands.done(step)` the weights are cleared and the trainer
    is the trainer without bands=, launch for launch.  save_checkpoint adds `band_schedule` / `band_weights`; load_band_checkpoint takes
    them.  Networks whose weights were set by hand (NeRF.set_bands on both) train the same way.  Without `bands=` nothing changes.
    ValueError, before any launch: data parallel, one network shared by both passes, networks without view directions or of another
    class, weights on one of the two networks only."""

    def __init__(self, render_kwargs_train, H, W, K, near, far, lrate=5e-4, lrate_decay=250, decay=True,
                 beta1=0.9, beta2=0.999, eps=1e-8, occupancy=None, occupancy_every=16, occupancy_warmup=256, occupancy_cells=None,
                 lambda_depth=0., lambda_acc=0., tighten=False, march=None, march_cap=128, march_after=0, bkgd=None,
                 lambda_dist=0., poses=None, pose_lrate=1e-3, exposure=None, lambda_autoexpo=1.0, exposure_lrate=None,
                 envmap=None, envmap_lrate=1e-2, bands=None):
        kw = render_kwargs_train
        self._kw = kw
        self.net_c = kw['network_fn']
        self.net_f = kw['network_fine']
        self.N_samples, self.N_importance = kw['N_samples'], kw['N_importance']
        self.perturb, self.white_bkgd = kw['perturb'], kw['white_bkgd']
        self.raw_noise_std = kw.get('raw_noise_std', 0.)
        self.ndc, self.lindisp = kw.get('ndc', True), kw.get('lindisp', False)
        self.use_viewdirs = self.net_c.use_viewdirs
        self.H, self.W, self.K, self.near, self.far = H, W, K, near, far
        self.flat = self.net_c._flat_all
        self.grad = self.net_c._grad_all
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self.lrate, self.lrate_decay, self.decay = lrate, lrate_decay, decay
        self.lr = lrate
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        self.adam_t = 0
        self.global_iter = 0
        self.world = parallel.world_size()
        self.live = LivePolicy()   # exact zero-gradient point compaction of the backward (render.py)
        # first pass of a compacted step: tiles without a live sample skip their colour branch (FN_FWD_SKIP_DEAD_RGB; the fused
        # step never exposes raw logits, every other output and the gradients are bit-identical -- tests/test_gpu_compact.py)
        self.skip_dead_rgb = True
        self.live_counts = torch.zeros(4, device=self.flat.device, dtype=torch.int32)
        self.last_step_live = False
        # one C-ABI call per step (fastnerf_train_step) instead of ~10 calls and ~25 allocations: two distinct nets with view
        # directions (or a single pass).  FASTNERF_FUSED_STEP=0 keeps the call-by-call sequencing (same kernels, same bits).
        self.fused = (os.environ.get('FASTNERF_FUSED_STEP', '1') != '0' and self.use_viewdirs
                      and (self.N_importance == 0 or (self.net_f is not None and self.net_f is not self.net_c)))
        self.overlap_allreduce = os.environ.get('FASTNERF_OVERLAP_ALLREDUCE', '1') != '0'
        self._sa = None          # fn_step_args of the fused path
        self._cache = {}         # route -> (key, fn_step_args, its regions, their size, keep-alive list): _begin_step
        self._last = None        # (block, regions) of the last prepared step
        self.occupancy = occupancy
        self.occupancy_every, self.occupancy_warmup = max(1, int(occupancy_every)), int(occupancy_warmup)
        self.occupancy_cells = occupancy_cells
        self.occupancy_counts = None if occupancy is None else torch.zeros(4, device=self.flat.device, dtype=torch.int32)
        self.occupancy_steps = 0     # steps taken with the grid set
        self.tighten = bool(tighten)
        self.lambda_depth, self.lambda_acc = float(lambda_depth), float(lambda_acc)
        self._aux_zero = torch.zeros(4, device=self.flat.device, dtype=torch.float32)
        self.aux_losses = self._aux_zero
        self._aux = None         # fn_step_aux of the fused path's current step (None: no term on)
        self.march, self.march_cap, self.march_after = march, march_cap, march_after
        self.march_counts = None if march is None else torch.zeros(2, device=self.flat.device, dtype=torch.int32)
        self._ma = None          # fn_step_args / fn_step_march of the marched step
        self.bkgd = bkgd
        self._bk = None          # fn_step_bkgd of the current step (None: no background)
        self.lambda_dist = float(lambda_dist)
        self._dist_zero = torch.zeros(2, device=self.flat.device, dtype=torch.float32)
        self.dist_losses = self._dist_zero
        self._dist = None        # fn_step_dist of the current step (None: the term is off)
        self.poses, self.pose_lrate = poses, float(pose_lrate)
        self.pose_lr = self.pose_lrate
        self.pose_grad = None    # d(loss)/d(xi) [n_img,6] of the last pose step
        self.pose_m = self.pose_v = None
        if poses is not None:
            self.pose_m, self.pose_v = torch.zeros_like(poses.xi.data), torch.zeros_like(poses.xi.data)
        self.exposure, self.lambda_autoexpo, self.exposure_lrate = exposure, float(lambda_autoexpo), exposure_lrate
        self.expo_lr = lrate if exposure_lrate is None else float(exposure_lrate)
        self._exp = None         # fn_step_expo of the current step (None: no table)
        self._img = None         # the rays' images handed to the next _fused_prepare, which takes them and leaves None
        self.expo_grad = None    # d(loss)/d(ab) [n_img,2] of the last step with the table
        self.expo_counts = None  # int32 [n_img]: the rays of every image in that step
        self.expo_loss = torch.zeros(1, device=self.flat.device, dtype=torch.float32)
        self.expo_m = self.expo_v = None
        if exposure is not None:
            self.expo_m, self.expo_v = torch.zeros_like(exposure.ab.data), torch.zeros_like(exposure.ab.data)
        self.envmap, self.envmap_lrate = envmap, float(envmap_lrate)
        self.env_lr = self.envmap_lrate
        self.env_grad = None     # d(loss)/d(table) [R,R,3] of the last step with the map
        self.env_m = self.env_v = self._env_ws = None
        if envmap is not None:
            self.env_m, self.env_v = torch.zeros_like(envmap.table.data), torch.zeros_like(envmap.table.data)
            self.env_grad = torch.zeros_like(envmap.table.data)
            self._env_ws = torch.empty(envmap.table.numel(), device=envmap.table.device, dtype=torch.int64)
        self.bands = bands       # a bands.BandSchedule (None: the full encoding); _band_tick sets the networks' weights from it
        self._band_open = None   # the first step at which the schedule was seen done: from there on nothing is evaluated
        self._check_dist()
        self._check_poses()
        self._check_expo()
        self._check_env()
        self._check_bands()
        self._check_occupancy()
        self._check_march()
        self._band_tick(self.adam_t)
        self.repack()

    def _check_expo(self):
        """Whether the trainer has an exposure table; its refusals, before any launch (read on every step, like the other settings)."""
        if self.exposure is None:
            return False
        if not (0. <= self.lambda_autoexpo < float('inf')):
            raise ValueError('Trainer: lambda_autoexpo is a finite weight >= 0, not {!r}'.format(self.lambda_autoexpo))
        if self.world > 1:
            raise ValueError('Trainer: exposure= is not data parallel (world size {})'.format(self.world))
        return True

    def _check_env(self, alpha=None, bkgd=None):
        """Whether the trainer has an environment map; its refusals, before any launch (read on every step, like the other settings)."""
        if self.envmap is None:
            return False
        if self.bkgd is not None or bkgd is not None:
            raise ValueError('Trainer: envmap= is the background of every ray: it cannot be combined with bkgd= (trainer or step)')
        if alpha is not None:
            raise ValueError('Trainer: envmap= cannot be combined with alpha=: a capture with alpha has no background to learn')
        if self.white_bkgd:
            raise ValueError('Trainer: envmap= cannot be combined with white_bkgd=True')
        if self.ndc:
            raise ValueError('Trainer: envmap= indexes the table by the ray direction: not with ndc=True (the NDC far plane is infinity)')
        if self.world > 1:
            raise ValueError('Trainer: envmap= is not data parallel (world size {})'.format(self.world))
        if self.envmap.table.device != self.flat.device:
            raise ValueError('Trainer: the environment map is on {}, the networks on {}'.format(self.envmap.table.device, self.flat.device))
        return True

    def _env_lookup(self, rays_d):
        """-> (dirs, the map's colours [n,3] for them): what the step injects as its per-ray background."""
        ops.require_gpu(rays_d)
        dirs = ops._f32(rays_d).reshape(-1, 3)
        return dirs, ops.env_lookup(self.envmap.table.data, dirs)

    def _env_backward(self, dirs, g_rgb, acc, g_rgb0=None, acc0=None):
        """self.env_grad = d(loss)/d(table) from the step's colour gradients and opacity maps (of one pass or of two)."""
        self.env_grad = ops.env_grad(self.envmap.res, dirs, g_rgb, acc, g_rgb0, acc0, d_table=self.env_grad, ws=self._env_ws)

    def _env_backward_block(self, dirs):
        """_env_backward on the regions of the step that was just prepared, behind its forward phase."""
        block, regions = self._last
        if 'g_rgb0' in regions:
            self._env_backward(dirs, _region(block, regions, 'g_rgb'), _region(block, regions, 'acc1'), _region(block, regions, 'g_rgb0'),
                               _region(block, regions, 'acc0'))
        else:
            self._env_backward(dirs, _region(block, regions, 'g_rgb'), _region(block, regions, 'acc0'))

    # ---- band weights (bands.py; NeRF.set_bands) ---------------------------------------------------------------------------
    def _nets(self):
        return [self.net_c] + ([self.net_f] if (self.net_f is not None and self.net_f is not self.net_c) else [])

    def _check_bands(self):
        """The refusals of a trainer with a band schedule, before any launch (read on every step, like the other settings)."""
        if self.bands is None:
            return
        if self.world > 1:
            raise ValueError('Trainer: bands= is not data parallel (world size {})'.format(self.world))
        if not all(isinstance(net, NeRF) and net.use_viewdirs for net in self._nets()):
            raise ValueError('Trainer: bands= weighs the encodings of model.NeRF networks with view directions (not nerf++ nets, not '
                             'use_viewdirs=False)')
        if self.N_importance > 0 and len(self._nets()) < 2:
            raise ValueError('Trainer: bands= needs two distinct networks for two passes, not one network shared by both')

    def _banded(self):
        """Whether the networks run with band weights (all of them or none): the step then leaves the update to _band_update."""
        on = [getattr(net, '_bands', None) is not None for net in self._nets()]
        if any(on) and not all(on):
            raise ValueError('Trainer: band weights are set on one of the two networks only: set them on both (or on neither)')
        if on[0] and self.world > 1:
            raise ValueError('Trainer: networks with band weights do not train data parallel (world size {})'.format(self.world))
        return on[0]

    def _kernel_buffers(self):
        """(params, grads) the step's kernels read and write, both networks in one buffer each: the parameters' own, or with band weights
        the effective networks' (NeRF.set_bands lays them out alike)."""
        if not self._banded():
            return self.flat, self.grad
        pool = self.net_c._band_pool
        if pool is None or self.net_c.flat.data_ptr() != pool['flat'].data_ptr() or pool['flat'].numel() != self.flat.numel():
            raise ValueError('Trainer: band weights need the networks of create_nerf (one effective buffer for both)')
        return pool['flat'], pool['grad']

    def _band_tick(self, step):
        """The networks' band weights for step `step` (0-based: the steps taken so far) from the schedule -- uploaded only when they
        changed; once the schedule is done the weights are cleared and the trainer is the trainer without bands=.  -> whether the
        effective networks changed (the caller repacks)."""
        if self.bands is None or (self._band_open is not None and step >= self._band_open):
            return False
        if self.bands.done(step):
            self._band_open = step
            changed = any(net._bands is not None for net in self._nets())
            for net in self._nets():
                net.clear_bands()
            return changed
        self._band_open = None
        w = self.bands.weights(step)
        return any([net.set_bands(*w, sync=False) for net in self._nets()])

    def _band_update(self, sl, collected=False):
        """The update of a step whose kernels ran on the effective networks (called without STEP_UPDATE), over the slice `sl` of the flat
        buffer: the effective gradient to the parameters' (ops.band_grad; collected: the route has done that), Adam on the parameters
        with the trainer's moments, the next step's weights, then the effective networks anew (ops.band_apply) and their packings."""
        Nn = ops.NET_PARAMS
        nets = [net for i, net in enumerate(self._nets()) if sl.start <= i * Nn < sl.stop]
        if not collected:
            for net in nets:
                net.collect_grads()
        ops.adam_step(self.flat[sl], self.grad[sl], self.m[sl], self.v[sl], self.lr, self.adam_t, self.beta1, self.beta2, self.eps)
        if self._band_tick(self.adam_t):
            self.repack()
        else:
            for net in nets:
                net.packed(refresh=True)

    def _check_expo_step(self, img, pix, n):
        """The refusals of a step's img=, before any launch -> None without a table, else the rays' images as contiguous int32 [n]
        (the default with pix= is its first column)."""
        if not self._check_expo():
            if img is not None:
                raise ValueError('Trainer.step: img= names rows of an exposure table: it needs Trainer(exposure=)')
            return None
        if img is None:
            if pix is None:
                raise ValueError('Trainer.step: a trainer with exposure= needs the image of every ray: img= (or pix=)')
            img = pix[:, 0]
        from .exposure import check_img
        img = check_img(img)
        if img.shape[0] != n:
            raise ValueError('Trainer.step: img= holds {} rows for {} rays'.format(img.shape[0], n))
        return img

    def _check_poses(self):
        """The refusals of a trainer with a pose table, before any launch (read on every pose step, like the other settings)."""
        if self.poses is None:
            return
        if self.occupancy is not None or self.tighten or self.march is not None:
            raise ValueError('Trainer: poses= steps on the call-by-call route, which has no occupancy grid, tighten or march')
        if self.world > 1:
            raise ValueError('Trainer: poses= is not data parallel (world size {})'.format(self.world))
        if self.ndc:
            raise NotImplementedError('Trainer: poses= differentiates plain pinhole rays only (ndc=False)')
        if ops.get_math() == 'bf16x3':
            raise NotImplementedError("Trainer: poses= needs ray gradients, which exist in the math modes 'fp32' and 'bf16x6' only, "
                                      "not in 'bf16x3'")

    def _check_occupancy(self):
        if self.occupancy is None:
            if self.tighten:
                raise ValueError('Trainer: tighten=True clamps near / far to an occupancy grid: it needs occupancy=')
            return
        if self._cascade() is not None and self.occupancy.dens is None:
            raise ValueError('Trainer: this OccupancyCascade has levels without a density, so it cannot be refreshed while the networks '
                             'train: make the cascade with OccupancyCascade.for_training(...), or from OccupancyGrid.for_training grids '
                             'with one dilate; build a cascade from the networks (from_network) for rendering after training')
        if self.raw_noise_std > 0.:
            raise ValueError('Trainer: an occupancy grid cannot be combined with raw_noise_std > 0 (sigma noise is added before the '
                             'relu, so a sample with zero sigma is not dead)')
        if not self.fused:
            raise ValueError('Trainer: an occupancy grid needs the fused step (two distinct networks with view directions, or a '
                             'single pass; FASTNERF_FUSED_STEP unset)')
        if get_compact() == '0' or not self.live.available(self.net_c, self.net_f, self.N_importance):
            raise ValueError('Trainer: an occupancy grid needs the compacted step (FASTNERF_COMPACT=0 or one network shared by '
                             'both passes rules it out): the plain backward has no list')

    def _cascade(self):
        """fn_occ_cascade of the step when `occupancy` is a cascade (fn_step_args.occ is NULL then), else None."""
        from .occupancy import OccupancyCascade
        return self.occupancy._c if isinstance(self.occupancy, OccupancyCascade) else None

    def _check_march(self):
        """(K, C) of the marched step, or None when march is off; ValueError for a configuration that cannot march."""
        if self.march is None:
            return None
        if self.occupancy is None:
            raise ValueError('Trainer: march= walks an occupancy grid: it needs occupancy=')
        K, C = ops.check_march(self.march, self.march_cap)
        if self.occupancy.outside_occupied:
            raise ValueError('Trainer: march= needs a grid with outside_occupied=False: with True every lattice point outside the box '
                             'is live and the packed rows overflow')
        return K, C

    def _marched(self):
        """(which, network, its packed pair): the network the marched step trains -- network_fine when there is one."""
        if self.net_f is not None and self.net_f is not self.net_c:
            return 1, self.net_f, self.pf
        return 0, self.net_c, self.pc

    def repack(self):
        self.pc = self.net_c.packed(refresh=True)
        self.pf = self.net_f.packed(refresh=True) if self.net_f is not None else None

    def _aux_terms(self, n, depth, depth_weight, acc, acc_weight):
        """The terms that are on (target given, lambda != 0) as contiguous fp32 [n] tensors: {} or a dict with depth_target /
        depth_weight / acc_target / acc_weight (+ the lambdas)."""
        t = {}
        for name, lam, tgt, w in (('depth', self.lambda_depth, depth, depth_weight), ('acc', self.lambda_acc, acc, acc_weight)):
            if tgt is None or lam == 0.:
                continue
            ops.require_gpu(tgt, w)
            t[name + '_target'] = ops._f32(tgt).reshape(-1)
            t[name + '_weight'] = None if w is None else ops._f32(w).reshape(-1)
            assert t[name + '_target'].numel() == n and (w is None or t[name + '_weight'].numel() == n), name
        if t:
            t['lambda_depth'], t['lambda_acc'] = self.lambda_depth, self.lambda_acc
        return t

    def _bkgd_terms(self, n, dev, alpha, bkgd):
        """The background of this step: None when off, else a dict with `bkgd` (contiguous fp32 [n,3], or None: draw them, 'random')
        and `alpha` (fp32 [n] or None).  A background is on when trainer.bkgd is set or colours are injected."""
        setting = self.bkgd
        if setting is None and bkgd is None:
            if alpha is not None:
                raise ValueError('Trainer: alpha= blends the target over a background colour: it needs bkgd= (trainer or step)')
            return None
        if self.white_bkgd:
            raise ValueError('Trainer: bkgd cannot be combined with white_bkgd=True (bkgd=(1, 1, 1) is the white background)')
        ops.require_gpu(alpha, bkgd)
        if bkgd is not None:
            bkgd = ops._f32(bkgd)
            assert bkgd.shape == (n, 3), 'bkgd: [n, 3] colours'
        elif not isinstance(setting, str):
            colour = torch.as_tensor(setting, dtype=torch.float32).reshape(3)
            bkgd = colour.to(dev).expand(n, 3).contiguous()
        elif setting != 'random':
            raise ValueError("Trainer: bkgd is None, 'random' or a colour of 3 floats, not {!r}".format(setting))
        if alpha is not None:
            alpha = ops._f32(alpha).reshape(-1)
            assert alpha.numel() == n, 'alpha: [n]'
        return {'bkgd': bkgd, 'alpha': alpha}

    def _step_seeds(self, marching, t_rand=None, u=None, march_u=None, bkgd=None):
        """The seeds of one step, drawn in the step's one order -- a dense step: sigma noise, coarse jitter, fine uniforms, background; a
        marched step: shift, background (the draws of render._forward_core, then the background's) -- `_next_seed()` where the step
        wants the draw, else 0.  t_rand / u / march_u / bkgd: what the caller injects instead.  A step on an empty batch calls this too
        and drops the result: the host RNG moves alike."""
        if marching:
            wants = [('shift', self.perturb and march_u is None)]
        else:
            wants = [('noise', self.raw_noise_std > 0.), ('seed0', self.perturb and t_rand is None),
                     ('seed1', self.N_importance > 0 and self.perturb and u is None)]
        wants.append(('bkgd', bkgd is None and isinstance(self.bkgd, str) and self.bkgd == 'random'))
        return {name: _next_seed() if want else 0 for name, want in wants}

    # For inspection, of the last prepared step on either route (self._last: its block and regions): the table, the marched step's block,
    # its distortion regions (g_w1), and the blended target and the rows the background hands to the compositing backward.
    _regions = _march_regions = property(lambda self: self._last[1])
    _march_block = property(lambda self: self._last[0])
    _march_dist_regions = property(lambda self: _term_table(self._last[1], 'dist'))
    _bk_views = property(lambda self: {k: _region(*self._last, 'bkgd.' + member)
                                       for k, member in (('target', 'target_ws'), ('g_acc1', 'g_acc1'), ('g_acc0', 'g_acc0'))})

    def _check_dist(self):
        """Whether the distortion term is on; ValueError for a weight that is no weight."""
        if not (0. <= self.lambda_dist < float('inf')):
            raise ValueError('Trainer: lambda_dist is a finite weight >= 0, not {!r}'.format(self.lambda_dist))
        return self.lambda_dist != 0.

    def forward_backward(self, rays_o, rays_d, target, leaf_tag=None, table=None, max_leaves=0, t_rand=None, u=None,
                         n_global=None, alpha=None, bkgd=None, d_rays=False, img=None, depth=None, depth_weight=None, acc=None,
                         acc_weight=None):
        """d_rays=True: the saving backward is forced and runs pass by pass with ops.ray_grad between the passes
        (render._backward_passes); out['d_rays'] [n,11] is d(loss)/d(rays11).  The parameter gradients are those of the plain backward,
        bit for bit."""
        if self.march is not None:
            raise ValueError('Trainer.forward_backward: the call-by-call route has no marched step; use step()')
        if self.occupancy is not None or self.tighten:
            raise ValueError('Trainer.forward_backward: the call-by-call route has no occupancy grid; use step()')
        n = rays_o.shape[0]
        dev = rays_o.device
        img = self._check_expo_step(img, None, n)
        env_dirs = None
        if self._check_env(alpha, bkgd):
            env_dirs, bkgd = self._env_lookup(rays_d)
        bt = self._bkgd_terms(n, dev, alpha, bkgd)
        rays11 = ops.pack_rays(rays_o, rays_d, self.near, self.far, ndc=self.ndc, H=self.H, W=self.W,
                               focal=float(self.K[0][0]))
        if not self.use_viewdirs:
            rays11[:, 8:11] = 0.
        noise0 = noise1 = None
        if self.raw_noise_std > 0.:
            noise0, noise1 = ops.sigma_noise(n, self.N_samples, self.N_samples + self.N_importance, self.raw_noise_std, _next_seed(), dev)
        live = not d_rays and self.live.use_live(self.net_c, self.net_f, self.N_importance)      # (the compacted backward has no ray gradients)
        out, saved = _forward_core(rays11, self.net_c, self.net_f, self.N_samples, self.N_importance, self.lindisp,
                                   self.perturb, self.white_bkgd, t_rand, u, noise0, noise1, save=not live,
                                   packed_c=self.pc, packed_f=self.pf, skip_dead_rgb=live and self.skip_dead_rgb, act_ws=True)
        scale = 1.0 if n_global is None else float(n) / float(n_global)
        if bt is not None:      # the same launches, in the same order, as fastnerf_train_step_bkgd makes
            target, out['bkgd'] = ops.bkgd_blend(out['rgb_map'], out['acc_map'], target, bkgd=bt['bkgd'],
                                                 seed=_next_seed() if bt['bkgd'] is None else 0, alpha=bt['alpha'],
                                                 rgb0=out.get('rgb0'), acc0=out.get('acc0'))
        e1, e0 = out['rgb_map'], out.get('rgb0')
        if img is not None:      # the same launches, around the colour loss, as fastnerf_train_step_expo makes
            ab = self.exposure.ab.data
            e1, e0 = ops.expo_apply(e1, img, ab, rgb0=e0)
        loss2, g, g0 = ops.mse_leafmax(e1, e0, target, grad_scale=scale, leaf_tag=leaf_tag, max_leaves=max_leaves, table=table)
        maps = None
        self.aux_losses = self._aux_zero
        aux = self._aux_terms(n, depth, depth_weight, acc, acc_weight)
        if aux:      # the same launch, behind the colour loss, as fastnerf_train_step_aux makes
            self.aux_losses, gm = ops.aux_loss(out['depth_map'], out['acc_map'], out.get('depth0'), out.get('acc0'), grad_scale=scale, **aux)
            maps = {k: t for k, t in gm.items() if t is not None}
        if img is not None:      # g, g0 become the gradient with respect to the scene's colours, in place
            self.expo_grad, self.expo_counts, self.expo_loss = ops.expo_grad(img, ab, self.lambda_autoexpo, scale, e1, g, e0=e0, g0=g0)
        if env_dirs is not None:      # the colour gradients stand: what the blend sends back to the table
            self._env_backward(env_dirs, g, out['acc_map'], g0, out.get('acc0') if g0 is not None else None)
        if bt is not None:
            ga1, ga0 = ops.bkgd_grad(out['bkgd'], g, g0, add=(maps or {}).get('g_acc1'), add0=(maps or {}).get('g_acc0'))
            maps = dict(maps or {}, g_acc1=ga1)
            if ga0 is not None:
                maps['g_acc0'] = ga0
        wg = None
        self.dist_losses = self._dist_zero
        if self._check_dist():      # the same launches, behind the other terms', as fastnerf_train_step_dist makes
            coef = ctypes.c_float(scale).value * ctypes.c_float(self.lambda_dist).value / n
            out['dist_map'], gw1 = ops.distortion(out['weights'], out['z_vals'], rays11, self.lindisp, coef=coef)
            wg = {'g_w1': gw1}
            if 'weights0' in out:
                out['dist0'], wg['g_w0'] = ops.distortion(out['weights0'], out['z0'], rays11, self.lindisp, coef=coef)
            self.dist_losses = ops.distortion_mean(out['dist_map'], out.get('dist0'))
        if d_rays:
            out['d_rays'] = torch.empty(n, 11, device=dev, dtype=torch.float32)
            two = self.net_f is not None and self.net_f is not self.net_c
            _backward_passes(saved, g, g0, self.net_c.flat_grad, self.net_f.flat_grad if two else None, d_rays=out['d_rays'], maps=maps,
                             weight_grads=wg)
        else:
            _backward_core(saved, g, g0, counts=self.live_counts if live else None, maps=maps, weight_grads=wg)
        self.net_c.collect_grads()          # (no-ops with view directions and no band weights: the kernels write the parameters' gradients)
        if self.net_f is not None and self.net_f is not self.net_c:
            self.net_f.collect_grads()
        if live:
            self.live.after_live_step(self.live_counts)
        self.live.tick()
        self.last_step_live = live
        return loss2, out

    # ---- what preparing a step shares between the fused and the marched route ------------------------------------------
    def _follow_math(self):
        """The math mode's tag; when it changed under this trainer: repack, and drop the cached step arguments."""
        tag = ops.get_math()
        if ops.packed_tag(self.pc[0]) != tag:
            self.repack()
            self._cache.clear()
        return tag

    def _new_step_args(self, n, S0, Ni, dev):
        """A fn_step_args for n rays of the sample shape (S0, Ni), filled with what lasts while its route's key does: the network,
        moment and packed pointers, the dact | draw and partial scratch of this (device, stream) -- shared with the call-by-call
        route (render._Workspace) -- and counts.  -> (args, regions, floats of a step's block, keep-alive list)"""
        P = n * (S0 + Ni)
        a = _lib.StepArgs()
        a.n, a.net_floats, a.math_mode = n, ops.NET_PARAMS, ops.mode_id()
        a.N_samples, a.N_importance = S0, Ni
        params, grads = self._kernel_buffers()
        a.params, a.grads, a.adam_m, a.adam_v = params.data_ptr(), grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr()
        a.packed_fwd_c, a.packed_bwd_c = self.pc[0].data_ptr(), self.pc[1].data_ptr()
        if self.pf is not None:
            a.packed_fwd_f, a.packed_bwd_f = self.pf[0].data_ptr(), self.pf[1].data_ptr()
        ws = _Workspace.dact(dev, ops.dact_floats(P) + P * 4)
        a.dact_ws = ws.data_ptr()
        a.draw_ws = ws.data_ptr() + 4 * ops.dact_floats(P)
        a.partial_ws = _Workspace.partial(dev).data_ptr()
        a.counts = self.live_counts.data_ptr()
        return (a,) + _step_regions(n, S0, Ni) + ([ws],)

    @staticmethod
    def _compacted_scratch(a, keep, dev):
        """act_ws / live_ws of the compacted backward, allocated on first use."""
        if not a.act_ws:
            P = a.n * (a.N_samples + a.N_importance)
            t1 = _Workspace.get('act', dev, ops.act_floats(P))
            t2 = _Workspace.get('live', dev, ops.live_ws_ints(P), torch.int32)
            a.act_ws, a.live_ws = t1.data_ptr(), t2.data_ptr()
            keep += [t1, t2]

    def _fill_step(self, a, regions, floats, rays_o, rays_d, target, leaf_tag, table, max_leaves, n_global):
        """What every step writes into its fn_step_args: the scalar settings, one fresh block of `floats` with the region pointers,
        the batch, the leaf table and grad_scale.  -> (block, the tensors to keep referenced while the launches run)"""
        n, dev = rays_o.shape[0], rays_o.device
        # scalar settings are read from the trainer on EVERY step, like the call-by-call route does (a caller may change
        # trainer.perturb / white_bkgd / near / far between steps): a handful of ctypes stores
        a.lindisp, a.perturb = int(bool(self.lindisp)), int(bool(self.perturb))
        a.white_bkgd, a.ndc, a.H, a.W = int(bool(self.white_bkgd)), int(bool(self.ndc)), int(self.H), int(self.W)
        a.focal, a.near_plane, a.far_plane = float(self.K[0][0]), float(self.near), float(self.far)
        a.beta1, a.beta2, a.eps = self.beta1, self.beta2, self.eps
        block = torch.empty(floats, device=dev, dtype=torch.float32)
        base = block.data_ptr()
        for name, (off, _) in regions.items():
            setattr(a, name, base + 4 * off)
        ro, rd, tg = ops._f32(rays_o).reshape(-1, 3), ops._f32(rays_d).reshape(-1, 3), ops._f32(target)
        a.rays_o, a.rays_d, a.target = ro.data_ptr(), rd.data_ptr(), tg.data_ptr()
        hold = [ro, rd, tg]
        if leaf_tag is not None:
            leaf_tag = leaf_tag.contiguous()
            hold.append(leaf_tag)
        a.leaf_tag = None if leaf_tag is None else leaf_tag.data_ptr()
        a.table = None if table is None else table.data_ptr()
        a.max_leaves = int(max_leaves)
        a.grad_scale = 1.0 if n_global is None else float(n) / float(n_global)
        return block, hold

    def _begin_step(self, route, S0, Ni, extra, batch, given, alpha=None, bkgd=None, aux=(None,) * 4, img=None):
        """What preparing a step is on both routes; _fused_prepare and _march_prepare add what differs.  In order: the background's terms,
        the GPU check, the grid's refusals, the math mode; the arguments of `route` ('fused' | 'march'), cached under (n, *extra, device,
        stream, math tag); the depth / opacity terms; the step's seeds (_step_seeds); one block laid out for the terms that are on
        (_term_regions) and fn_step_args filled (_fill_step); self._aux / _bk / _dist / _exp (None: the term is off) pointing into the block,
        and aux_losses / dist_losses / expo_grad / expo_counts / expo_loss as its views.  batch: (rays_o, rays_d, target, leaf_tag, table,
        max_leaves, n_global); given: what the caller injects instead of draws, by _step_seeds' names; aux: (depth, depth_weight, acc,
        acc_weight); img: None, or the rays' images (_check_expo_step).
        -> (args, its keep-alive list, whether the args were built anew, block, regions, out key -> region of the terms' outputs, seeds,
        hold: what stays referenced until the next step is prepared -- the launches are asynchronous -- for the route to append to)"""
        n, dev = batch[0].shape[0], batch[0].device
        bt = self._bkgd_terms(n, dev, alpha, bkgd)
        ops.require_gpu(*batch[:5], *given.values())
        self._check_occupancy()
        key = (n,) + extra + (str(dev), torch.cuda.current_stream(dev).cuda_stream, self._follow_math(), self._banded())
        c = self._cache.get(route)
        fresh = c is None or c[0] != key
        if fresh:
            c = self._cache[route] = (key,) + self._new_step_args(n, S0, Ni, dev)
        _, a, base, size, keep = c
        aux = self._aux_terms(n, *aux)
        seeds = self._step_seeds(route == 'march', bkgd=bkgd, **given)
        dist = self._check_dist()
        expo = None
        if img is not None:
            ab = self.exposure.ab.data
            expo = (ab.shape[0], ops.expo_grad_ws_floats(n, ab.shape[0]))
        regions, size = _term_regions(base, size, n, S0, Ni, aux=bool(aux), bkgd=bt is not None, dist=dist, expo=expo)
        block, hold = self._fill_step(a, base, size, *batch)
        self._last = (block, regions)
        self._aux = self._bk = self._dist = self._exp = None
        self.aux_losses, self.dist_losses = self._aux_zero, self._dist_zero
        names = {}
        if aux:
            self._aux = _term_struct(_lib.StepAux, 'aux', block, regions, lambda_depth=aux['lambda_depth'], lambda_acc=aux['lambda_acc'],
                                     **{k: _lib.ptr(aux.get(k)) for k in ('depth_target', 'depth_weight', 'acc_target', 'acc_weight')})
            self.aux_losses = _region(block, regions, 'aux.loss4')
            hold += [aux, self.aux_losses]
        if bt is not None:
            self._bk = _term_struct(_lib.StepBkgd, 'bkgd', block, regions, bkgd=_lib.ptr(bt['bkgd']), seed=seeds['bkgd'], alpha=_lib.ptr(bt['alpha']))
            names['bkgd'] = 'bkgd.bkgd_used'
            hold.append(bt)
        if dist:
            self._dist = _term_struct(_lib.StepDist, 'dist', block, regions, lambda_dist=self.lambda_dist)
            self.dist_losses = _region(block, regions, 'dist.loss2d')
            names.update(dist_map='dist.ell1', **({'dist0': 'dist.ell0'} if Ni > 0 else {}))
        if expo:
            self._exp = _term_struct(_lib.StepExpo, 'expo', block, regions, img=_lib.ptr(img), ab=_lib.ptr(ab), n_img=expo[0],
                                     **{'lambda': self.lambda_autoexpo})
            self.expo_grad, self.expo_loss = _region(block, regions, 'expo.d_ab'), _region(block, regions, 'expo.loss_reg')
            self.expo_counts = _region(block, regions, 'expo.counts').view(torch.int32)
            hold += [img, ab]
        self._hold = hold
        return a, keep, fresh, block, regions, names, seeds, hold

    # ---- fused route: one fastnerf_train_step_expo call per phase group ---------------------------------------------
    def _fused_prepare(self, rays_o, rays_d, target, leaf_tag, table, max_leaves, t_rand, u, n_global, alpha=None, bkgd=None,
                       depth=None, depth_weight=None, acc=None, acc_weight=None):
        """Fill fn_step_args (and the structs of the terms that are on: _begin_step) for this batch; returns (args, out mapping, loss2,
        live).  The rays' images of a step with an exposure table come in self._img, which step() sets just before this call and which
        is taken here, once: this signature is pinned to end in the depth / opacity arguments and is called positionally up to them
        (tests/test_aux_loss_cpu.py, tests/test_gpu_step_terms.py), so it has no place for one more; a direct call sees None."""
        img, self._img = self._img, None
        n, dev = rays_o.shape[0], rays_o.device
        S0, Ni = self.N_samples, self.N_importance
        if t_rand is not None:
            t_rand = ops._f32(t_rand)
            assert t_rand.shape == (n, S0)
        if u is not None:
            u = ops._f32(u)
            assert u.shape == (n, Ni)
        a, keep, _, block, regions, names, seeds, hold = self._begin_step(
            'fused', S0, Ni, (), (rays_o, rays_d, target, leaf_tag, table, max_leaves, n_global), dict(t_rand=t_rand, u=u), alpha, bkgd,
            (depth, depth_weight, acc, acc_weight), img)
        self._sa = a
        live = self.live.use_live(self.net_c, self.net_f, Ni)
        if self.occupancy is not None or self.tighten:
            live = True             # the grid's first forward feeds the compacted backward only
        # the big buffers of the route this step takes (allocated on first use: a run that never falls back to the plain
        # backward never pays for its 11 GB of saved activations)
        if live:
            self._compacted_scratch(a, keep, dev)
        elif not a.act0:
            t1 = _Workspace.get('act0', dev, ops.act_floats(n * S0))
            a.act0 = t1.data_ptr()
            keep.append(t1)
            if Ni > 0:
                t2 = _Workspace.get('act1', dev, ops.act_floats(n * (S0 + Ni)))
                a.act1 = t2.data_ptr()
                keep.append(t2)
        a.t_rand, a.u = _lib.ptr(t_rand), _lib.ptr(u)
        noise0 = noise1 = None
        if self.raw_noise_std > 0.:
            noise0, noise1 = ops.sigma_noise(n, S0, S0 + Ni if Ni > 0 else 0, self.raw_noise_std, seeds['noise'], dev)
        a.noise0, a.noise1 = _lib.ptr(noise0), _lib.ptr(noise1)
        a.seed0, a.seed1 = seeds['seed0'], seeds['seed1']
        a.live = int(live)
        a.fwd_flags = (1 if (live and self.skip_dead_rgb and noise0 is None) else 0) | (_lib.STEP_TIGHTEN if self.tighten else 0)
        occ = self.occupancy
        if occ is not None and self.occupancy_counts is None:      # a grid set after construction
            self.occupancy_counts = torch.zeros(4, device=self.flat.device, dtype=torch.int32)
        a.occ = None if (occ is None or self._cascade() is not None) else ctypes.addressof(occ._c)
        a.occ_counts = None if occ is None else self.occupancy_counts.data_ptr()
        hold += [t_rand, u, noise0, noise1, occ]
        base_names = _OUT_NAMES_2 if Ni > 0 else _OUT_NAMES_1
        out = _StepOut(block, regions, dict(base_names, **names) if names else base_names)
        return a, out, _region(block, regions, 'loss2'), live

    def _occupancy_tick(self, marching=False):
        """Before a step with the grid set: refresh it when its turn has come (a grid without a density is never touched).  A marched
        step refreshes it from the marched network alone."""
        k = self.occupancy_steps - self.occupancy_warmup
        if self.occupancy.dens is not None and k >= 0 and k % self.occupancy_every == 0:
            self._follow_math()
            if marching:
                which, _, pk = self._marched()
                self.occupancy.update(self._kw, cells_per_call=self.occupancy_cells, _packed=[pk[0]], which='fine' if which else 'coarse')
            else:
                self.occupancy.update(self._kw, cells_per_call=self.occupancy_cells,
                                      _packed=[self.pc[0]] + ([self.pf[0]] if (self.pf is not None and self.net_f is not self.net_c) else []))
        self.occupancy_steps += 1

    # ---- marched route: one fastnerf_train_step_march_expo call per phase group -----------------------------------
    def _march_prepare(self, K, C, rays_o, rays_d, target, leaf_tag, table, max_leaves, march_u, n_global, alpha=None, bkgd=None, img=None):
        """Fill fn_step_args and fn_step_march (and the structs of the terms that are on: _begin_step) for this batch; returns (args, march,
        out dict, loss2).  out['march_overflow'] is the step's uint8 buffer here: step() hands it out as bool once the forward is enqueued."""
        n, dev = rays_o.shape[0], rays_o.device
        if march_u is not None:
            march_u = ops._f32(march_u).reshape(-1)
            assert march_u.shape == (n,)
        # the row is a single pass of C samples, always compacted
        a, keep, fresh, block, regions, names, seeds, hold = self._begin_step(
            'march', C, 0, (K, C), (rays_o, rays_d, target, leaf_tag, table, max_leaves, n_global), dict(march_u=march_u), alpha, bkgd, img=img)
        if fresh:
            x = _lib.StepMarch()
            self._ma = (a, x)
            self._compacted_scratch(a, keep, dev)
            t3 = _Workspace.get('march_list', dev, ops.step_march_ws_ints(n, C), torch.int32)
            keep.append(t3)
            a.live = 1
            x.list_ws = t3.data_ptr()
            x.counts = self.march_counts.data_ptr()
        x = self._ma[1]
        kidx = torch.empty(n, C, device=dev, dtype=torch.int32)
        overflow = torch.empty(n, device=dev, dtype=torch.uint8)
        hold += [kidx, overflow, self.occupancy, march_u]
        x.K, x.C, x.which = K, C, self._marched()[0]
        x.u, x.seed = _lib.ptr(march_u), seeds['shift']
        x.kidx, x.overflow = kidx.data_ptr(), overflow.data_ptr()
        a.fwd_flags = (1 if self.skip_dead_rgb else 0) | (_lib.STEP_TIGHTEN if self.tighten else 0)
        a.occ = None if self._cascade() is not None else ctypes.addressof(self.occupancy._c)
        view = lambda name: _region(block, regions, name)      # noqa: E731
        out = {'rgb_map': view('rgb0'), 'disp_map': view('disp0'), 'acc_map': view('acc0'), 'depth_map': view('depth0'),
               'raw': view('raw0'), 'weights': view('w0'), 'z_vals': view('z0'), 'march_k': kidx, 'march_overflow': overflow}
        out.update((key, view(name)) for key, name in names.items())
        return a, x, out, view('loss2')

    # The term structs are given in every phase call (the data-parallel step splits the phases).  NULL is "the term is off": the C side
    # then makes the launches, and names itself in errors, as the entry point without that struct does.
    def _march_call(self, a, x, phases):
        c = self._cascade()
        if c is not None:
            return _lib.check(_lib.lib().fastnerf_train_step_march_cascade(ctypes.byref(a), ctypes.byref(x), _ref(self._bk), _ref(self._dist),
                                                                           _ref(self._exp), ctypes.byref(c), int(phases), _lib.stream()),
                              'fastnerf_train_step_march_cascade')
        _lib.check(_lib.lib().fastnerf_train_step_march_expo(ctypes.byref(a), ctypes.byref(x), _ref(self._bk), _ref(self._dist), _ref(self._exp),
                                                             int(phases), _lib.stream()), 'fastnerf_train_step_march_expo')

    def _fused_call(self, a, phases):
        c = self._cascade()
        if c is not None:
            return _lib.check(_lib.lib().fastnerf_train_step_cascade(ctypes.byref(a), _ref(self._aux), _ref(self._bk), _ref(self._dist),
                                                                     _ref(self._exp), ctypes.byref(c), int(phases), _lib.stream()),
                              'fastnerf_train_step_cascade')
        _lib.check(_lib.lib().fastnerf_train_step_expo(ctypes.byref(a), _ref(self._aux), _ref(self._bk), _ref(self._dist), _ref(self._exp),
                                                       int(phases), _lib.stream()), 'fastnerf_train_step_expo')

    def _after_backward(self, live):
        if live:
            self.live.after_live_step(self.live_counts)
        self.live.tick()
        self.last_step_live = live

    def _host_update(self, sl, overlap):
        """What follows the gradient off the fused step, over the slice `sl` of the flat buffer: the collectives the stepping ranks
        issue (the fused route's two under `overlap`, so that every rank issues the same sequence), Adam, the repack.  With band
        weights (world == 1; the parameters' gradient stands): _band_update, the sequence the fused routes run then."""
        if self._banded():
            return self._band_update(sl, collected=True)
        if self.world > 1:
            Nn = ops.NET_PARAMS
            if overlap:
                parallel.wait_all(parallel.all_reduce_sum_async(self.grad[Nn:]), parallel.all_reduce_sum_async(self.grad[:Nn]))
            else:
                parallel.all_reduce_sum(self.grad[sl])
        ops.adam_step(self.flat[sl], self.grad[sl], self.m[sl], self.v[sl], self.lr, self.adam_t, self.beta1, self.beta2, self.eps)
        self.repack()

    def _empty_step(self, sl, overlap):
        """The step of a rank whose shard of a (tail) batch is empty, on every route: it renders nothing and leaves the grid alone, but
        joins the collectives with a zero gradient over the slice `sl` the step would have trained and takes the update (step() has drawn
        the seeds the step would have drawn).  -> (loss2, out)"""
        self.grad[sl].zero_()
        self.aux_losses = self._aux_zero
        self.dist_losses = self._dist_zero
        self._host_update(sl, overlap)
        return torch.zeros(2, device=self.grad.device), {}

    def step(self, rays_o, rays_d, target, leaf_tag=None, table=None, max_leaves=0, t_rand=None, u=None,
             n_global=None, decay=None, march_u=None, alpha=None, bkgd=None, pix=None, img=None, depth=None, depth_weight=None,
             acc=None, acc_weight=None):
        if pix is not None or self.poses is not None:
            pix = self._check_pose_step(rays_o, rays_d, pix)
            n = pix.shape[0]
        else:
            n = rays_o.shape[0]
        img = self._check_expo_step(img, pix, n)
        env = self._check_env(alpha, bkgd)
        Nn = ops.NET_PARAMS
        two = self.N_importance > 0 and self.net_f is not None and self.net_f is not self.net_c
        overlap = self.world > 1 and two and self.overlap_allreduce and self.grad.numel() == 2 * Nn
        KC = self._check_march()            # (read on every step, like perturb and white_bkgd)
        self._check_dist()
        if KC is not None and self._aux_terms(n, depth, depth_weight, acc, acc_weight):
            raise ValueError('Trainer: the marched step has no depth / opacity terms (lambda_depth / lambda_acc with a target)')
        marching = KC is not None and self.occupancy_steps >= int(self.march_after)
        everything = slice(0, self.grad.numel())
        self._check_bands()
        if self._band_tick(self.adam_t):      # this step's band weights (unchanged, as a rule: the last update has set them)
            self.repack()
        # with band weights the kernels run on the effective networks and the update is _band_update's (world == 1: _check_bands)
        banded = self._banded()
        update = 0 if banded else _lib.STEP_UPDATE
        self.adam_t += 1
        if self.occupancy is not None and n > 0:
            self._occupancy_tick(marching)
        if n == 0:      # an empty batch takes its own path on every route
            self._bkgd_terms(0, self.grad.device, alpha, bkgd)      # (its ValueErrors, like a step that renders)
            self._step_seeds(marching, t_rand, u, march_u, bkgd)      # (drawn like a step that renders, and dropped)
            if marching:
                which = self._marched()[0]
                loss2, out = self._empty_step(slice(which * Nn, (which + 1) * Nn), False)
            else:
                loss2, out = self._empty_step(everything, overlap)
            if pix is not None:
                self._pose_update(pix, None, None)
            if img is not None:
                self.expo_grad, self.expo_counts = torch.zeros_like(self.expo_m), torch.zeros_like(self.expo_m[:, 0], dtype=torch.int32)
                self.expo_loss = torch.zeros_like(self.expo_loss)
            if env:
                self.env_grad.zero_()
        elif pix is not None:
            # the pose step: the call-by-call route with ray gradients, then the rays' gradient down to xi and an Adam step of its own
            poses = ops.pose_exp(self.poses.base, self.poses.xi.data)
            ro, rd = ops.gen_rays_pixels(pix, poses, self.K)
            loss2, out = self.forward_backward(ro, rd, target, leaf_tag, table, max_leaves, t_rand, u, n_global, alpha=alpha, bkgd=bkgd,
                                               depth=depth, depth_weight=depth_weight, acc=acc, acc_weight=acc_weight, d_rays=True, img=img)
            self._pose_update(pix, poses, out['d_rays'])
            self._host_update(everything, overlap)
        elif marching:
            if env:
                env_dirs, bkgd = self._env_lookup(rays_d)
            a, x, out, loss2 = self._march_prepare(KC[0], KC[1], rays_o, rays_d, target, leaf_tag, table, max_leaves, march_u, n_global,
                                                   alpha, bkgd, img)
            a.lr, a.adam_t = float(self.lr), int(self.adam_t)
            if env:      # (world == 1: _check_env) phase by phase, the table's gradient behind the forward phase
                self._march_call(a, x, _lib.STEP_FORWARD)
                self._env_backward_block(env_dirs)
                self._march_call(a, x, _lib.STEP_BWD_COARSE | update)
            elif self.world == 1:
                self._march_call(a, x, _lib.STEP_FORWARD | _lib.STEP_BWD_COARSE | update)
            else:      # data parallel, not overlapped: one network, one collective over its half of the gradient
                self._march_call(a, x, _lib.STEP_FORWARD | _lib.STEP_BWD_COARSE)
                parallel.all_reduce_sum(self.grad[x.which * Nn:(x.which + 1) * Nn])
                self._march_call(a, x, _lib.STEP_UPDATE)
            if banded:
                self._band_update(slice(x.which * Nn, (x.which + 1) * Nn))
            out['march_overflow'] = out['march_overflow'].bool()
            self.live.tick()
            self.last_step_live = True
        elif self.fused:
            if env:
                env_dirs, bkgd = self._env_lookup(rays_d)
            self._img = img
            a, out, loss2, live = self._fused_prepare(rays_o, rays_d, target, leaf_tag, table, max_leaves, t_rand, u, n_global,
                                                      alpha, bkgd, depth, depth_weight, acc, acc_weight)
            a.lr, a.adam_t = float(self.lr), int(self.adam_t)
            if env:      # (world == 1: _check_env) phase by phase, the table's gradient behind the forward phase
                self._fused_call(a, _lib.STEP_FORWARD)
                self._env_backward_block(env_dirs)
                self._fused_call(a, _lib.STEP_BWD_FINE | _lib.STEP_BWD_COARSE | update)
                self._after_backward(live)
            elif self.world == 1:
                self._fused_call(a, _lib.STEP_FORWARD | _lib.STEP_BWD_FINE | _lib.STEP_BWD_COARSE | update)
                self._after_backward(live)
            else:
                # data parallel: the fine net's gradient (the second half of the flat buffer) is final after the fine pass and is
                # all-reduced while the coarse pass's backward runs (the collective has its own stream; `wait` orders ours behind it)
                if overlap:
                    self._fused_call(a, _lib.STEP_FORWARD | _lib.STEP_BWD_FINE)
                    w1 = parallel.all_reduce_sum_async(self.grad[Nn:])
                    self._fused_call(a, _lib.STEP_BWD_COARSE)
                    w0 = parallel.all_reduce_sum_async(self.grad[:Nn])
                    parallel.wait_all(w1, w0)
                else:
                    self._fused_call(a, _lib.STEP_FORWARD | _lib.STEP_BWD_FINE | _lib.STEP_BWD_COARSE)
                    parallel.all_reduce_sum(self.grad)
                self._after_backward(live)
                self._fused_call(a, _lib.STEP_UPDATE)
            if banded:
                self._band_update(everything)
        else:
            loss2, out = self.forward_backward(rays_o, rays_d, target, leaf_tag, table, max_leaves, t_rand, u, n_global,
                                               alpha=alpha, bkgd=bkgd, depth=depth, depth_weight=depth_weight, acc=acc, acc_weight=acc_weight,
                                               img=img)
            self._host_update(everything, overlap)
        if img is not None:      # Adam on the table with moments of its own, as _pose_update does for xi
            ops.adam_step(self.exposure.ab.data, self.expo_grad, self.expo_m, self.expo_v, self.expo_lr, self.adam_t, self.beta1, self.beta2,
                          self.eps)
        if env:      # and on the environment map
            ops.adam_step(self.envmap.table.data, self.env_grad, self.env_m, self.env_v, self.env_lr, self.adam_t, self.beta1, self.beta2,
                          self.eps)
        if (self.decay if decay is None else decay):
            factor = 0.1 ** (self.global_iter / (self.lrate_decay * 1000))
            self.lr = self.lrate * factor
            self.pose_lr = self.pose_lrate * factor
            self.expo_lr = (self.lrate if self.exposure_lrate is None else float(self.exposure_lrate)) * factor
            self.env_lr = self.envmap_lrate * factor
            self.global_iter += 1
        return loss2, out

    def _check_pose_step(self, rays_o, rays_d, pix):
        """The refusals of a pose step, before any launch -> pix as contiguous int32 [n,3]."""
        if self.poses is None:
            raise ValueError('Trainer.step: pix= names pixels of the images of a pose table: it needs Trainer(poses=)')
        if pix is None:
            raise ValueError('Trainer.step: a trainer with poses= makes its rays from the table: it needs pix=, not rays')
        if rays_o is not None or rays_d is not None:
            raise ValueError('Trainer.step: give rays or pix=, not both: with pix= the rays come from the pose table (rays_o = rays_d = None)')
        self._check_poses()
        from .poses import check_pix
        return check_pix(pix)

    def _pose_update(self, pix, poses, d_rays):
        """d_rays -> d_poses -> self.pose_grad = d(loss)/d(xi), then Adam on xi with the table's own moments at pose_lr (pose_lrate times
        the decay factor the networks' rate has).  An empty batch (poses None): a zero gradient, and the update Adam makes of it."""
        xi = self.poses.xi.data
        if poses is None:
            self.pose_grad = torch.zeros_like(xi)
        else:
            d_poses = ops.pose_grad(pix, poses, self.K, d_rays)
            self.pose_grad = ops.pose_exp_bwd(self.poses.base, xi, d_poses)
        ops.adam_step(xi, self.pose_grad, self.pose_m, self.pose_v, self.pose_lr, self.adam_t, self.beta1, self.beta2, self.eps)

    def state_dict(self):
        sd = {'m': self.m, 'v': self.v, 'adam_t': self.adam_t, 'global_iter': self.global_iter, 'lr': self.lr}
        if self.poses is not None:
            sd.update(pose_m=self.pose_m, pose_v=self.pose_v, pose_lr=self.pose_lr)
        if self.exposure is not None:
            sd.update(expo_m=self.expo_m, expo_v=self.expo_v, expo_lr=self.expo_lr)
        if self.envmap is not None:
            sd.update(env_m=self.env_m, env_v=self.env_v, env_lr=self.env_lr)
        return sd

    # ---- interchange with torch.optim.Adam (the optimizer_state_dict of the reference's .tar, run_nerf.py:121,537) ----
    def _param_list(self):
        ps = list(self.net_c.parameters())
        if self.net_f is not None and self.net_f is not self.net_c:
            ps += list(self.net_f.parameters())
        return ps

    def torch_optimizer_state_dict(self):
        """State in torch.optim.Adam's format over grad_vars (coarse then fine parameters, parameters() order = the
        flat buffer's order): loadable by the reference's `optimizer.load_state_dict`."""
        return flat_params.adam_state_to_torch(self._param_list(), self.m, self.v, self.adam_t, self.lr, (self.beta1, self.beta2), self.eps)

    def load_torch_optimizer(self, opt):
        """Take over the moments / step count / lr of a torch.optim.Adam (or its state_dict) over the same
        parameters, e.g. the optimizer create_nerf restored from a reference checkpoint."""
        self.adam_t, lr = flat_params.adam_state_from_torch(self._param_list(), self.m, self.v, opt)
        self.lr = float(lr)
        if self.bands is not None:      # (as in load_state_dict)
            self._band_open = None
            self._band_tick(self.adam_t)
            self.repack()

    def load_pose_checkpoint(self, ckpt):
        """Take xi and its moments from a checkpoint of save_checkpoint (the loaded dict, or its path).  A checkpoint without a pose
        table leaves the table untouched; one whose base poses are not this table's is a ValueError."""
        if self.poses is None:
            return False
        if not isinstance(ckpt, dict):
            ckpt = torch.load(ckpt, map_location=self.poses.xi.device, weights_only=False)
        if 'pose_xi' not in ckpt:
            return False
        base = ckpt['pose_base'].to(self.poses.base.device)
        if base.shape != self.poses.base.shape or not torch.equal(base, self.poses.base):
            raise ValueError('Trainer.load_pose_checkpoint: the checkpoint refines other base poses than this table holds')
        self.poses.xi.data.copy_(ckpt['pose_xi'])
        self.pose_m.copy_(ckpt['pose_m']); self.pose_v.copy_(ckpt['pose_v'])
        return True

    def load_expo_checkpoint(self, ckpt):
        """Take the exposure table and its moments from a checkpoint of save_checkpoint (the loaded dict, or its path).  A checkpoint
        without one leaves the table untouched; one for another number of images is a ValueError."""
        if self.exposure is None:
            return False
        ab = self.exposure.ab.data
        if not isinstance(ckpt, dict):
            ckpt = torch.load(ckpt, map_location=ab.device, weights_only=False)
        if 'expo_ab' not in ckpt:
            return False
        if ckpt['expo_ab'].shape != ab.shape:
            raise ValueError('Trainer.load_expo_checkpoint: the checkpoint holds exposures of {} images, this table of {}'.format(
                ckpt['expo_ab'].shape[0], ab.shape[0]))
        ab.copy_(ckpt['expo_ab'])
        self.expo_m.copy_(ckpt['expo_m']); self.expo_v.copy_(ckpt['expo_v'])
        return True

    def load_env_checkpoint(self, ckpt):
        """Take the environment map and its moments from a checkpoint of save_checkpoint (the loaded dict, or its path).  A checkpoint
        without one leaves the table untouched; one of another resolution is a ValueError."""
        if self.envmap is None:
            return False
        table = self.envmap.table.data
        if not isinstance(ckpt, dict):
            ckpt = torch.load(ckpt, map_location=table.device, weights_only=False)
        if 'env_table' not in ckpt:
            return False
        if ckpt['env_table'].shape != table.shape:
            raise ValueError('Trainer.load_env_checkpoint: the checkpoint holds a map of resolution {}, this one has {}'.format(
                ckpt['env_table'].shape[0], table.shape[0]))
        table.copy_(ckpt['env_table'])
        self.env_m.copy_(ckpt['env_m']); self.env_v.copy_(ckpt['env_v'])
        return True

    def load_state_dict(self, sd):
        self.m.copy_(sd['m']); self.v.copy_(sd['v'])
        self.adam_t, self.global_iter, self.lr = sd['adam_t'], sd['global_iter'], sd['lr']
        if self.poses is not None and 'pose_m' in sd:      # (a state without them: the table's moments stay as they are)
            self.pose_m.copy_(sd['pose_m']); self.pose_v.copy_(sd['pose_v'])
            self.pose_lr = sd.get('pose_lr', self.pose_lr)
        if self.exposure is not None and 'expo_m' in sd:
            self.expo_m.copy_(sd['expo_m']); self.expo_v.copy_(sd['expo_v'])
            self.expo_lr = sd.get('expo_lr', self.expo_lr)
        if self.envmap is not None and 'env_m' in sd:
            self.env_m.copy_(sd['env_m']); self.env_v.copy_(sd['env_v'])
            self.env_lr = sd.get('env_lr', self.env_lr)
        if self.bands is not None:      # the step count moved: the band weights of the step that comes next, on the networks as they are
            self._band_open = None
            self._band_tick(self.adam_t)
            self.repack()

    def load_band_checkpoint(self, ckpt):
        """Take the band schedule from a checkpoint of save_checkpoint (the loaded dict, or its path): the trainer then ramps as the
        run that wrote it did; the weights of the next step follow from the step count (load_torch_optimizer / load_state_dict first).
        A checkpoint without a schedule leaves the trainer untouched."""
        if not isinstance(ckpt, dict):
            ckpt = torch.load(ckpt, map_location=self.flat.device, weights_only=False)
        if 'band_schedule' not in ckpt:
            return False
        from .bands import BandSchedule
        self.bands = BandSchedule.from_settings(ckpt['band_schedule'], ckpt.get('band_weights'))
        self._check_bands()
        self._band_open = None
        self._band_tick(self.adam_t)
        self.repack()
        return True


def reference_state_dict(net):
    """state_dict with the `module.` prefix of the nn.DataParallel wrapper the reference saves and strictly loads
    (run_nerf.py:82,90,124-126,535-536)."""
    return flat_params.add_prefix(net.state_dict())


def tree_pkl_path(args, epoch):
    """run_nerf.py:339,542."""
    return os.path.join(args.basedir, args.expname, 'treeDivide_{:04d}.pkl'.format(epoch))


def save_checkpoint(args, epoch_id, trainer, kw_train, mgr):
    """run_nerf.py:532-544: `{epoch:03d}.tar` (global_epoch, global_iter, the two DataParallel state_dicts, the Adam
    state in torch.optim's format) + `treeDivide_{epoch:04d}.pkl`.  Both files load in the reference."""
    d = os.path.join(args.basedir, args.expname)
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, '{:03d}.tar'.format(epoch_id))
    ckpt = {'global_epoch': epoch_id, 'global_iter': trainer.global_iter,
            'network_fn_state_dict': reference_state_dict(kw_train['network_fn']),
            'network_fine_state_dict': (None if kw_train['network_fine'] is None    # N_importance = 0: run_nerf.py:536 fails
                                        else reference_state_dict(kw_train['network_fine'])),   # on None.state_dict(); None is kept
            'optimizer_state_dict': trainer.torch_optimizer_state_dict()}
    if trainer.poses is not None:      # the pose table beside them (keys the reference does not read)
        ckpt.update(pose_xi=trainer.poses.xi.data, pose_base=trainer.poses.base, pose_m=trainer.pose_m, pose_v=trainer.pose_v)
    if trainer.exposure is not None:      # and the exposure table
        ckpt.update(expo_ab=trainer.exposure.ab.data, expo_m=trainer.expo_m, expo_v=trainer.expo_v)
    if trainer.envmap is not None:      # and the environment map
        ckpt.update(env_table=trainer.envmap.table.data, env_m=trainer.env_m, env_v=trainer.env_v)
    if trainer.bands is not None:      # and the band schedule, with the weights of the step that comes next (the state dicts above are the
        # parameters themselves, never the effective networks: after the ramp this is a plain checkpoint of the reference's)
        ckpt.update(band_schedule=trainer.bands.settings(), band_weights=trainer.bands.weights(trainer.adam_t))
    torch.save(ckpt, path)
    mgr.save_trees(tree_pkl_path(args, epoch_id))
    return path


def load_dataset(args):
    """The data-loading branch of the reference's train() (run_nerf.py:160-241) for the two dataset types on this path:
    -> dict(images [n,H,W,3], poses [n,3,4], render_poses, hwf [H,W,focal], K, i_train, i_val, i_test, near, far).
    `args` needs dataset_type, datadir and the matching options (blender: half_res, testskip, white_bkgd; llff: factor,
    spherify, llffhold, no_ndc); render_test swaps the render poses for the test poses like the reference.
    args.random_bkgd (no such flag in the reference's parser; default off): a blender set keeps its alpha, images [n,H,W,4] with
    straight colours, for `train` to composite over a fresh colour per ray (Trainer(bkgd='random')); ValueError with white_bkgd."""
    K = None
    if args.dataset_type == 'llff':
        from .load_llff import load_llff_data
        images, poses, bds, render_poses, i_test = load_llff_data(args.datadir, getattr(args, 'factor', 8), recenter=True,
                                                                  bd_factor=.75, spherify=getattr(args, 'spherify', False))
        hwf = poses[0, :3, -1]
        poses = poses[:, :3, :4]
        i_test = i_test if isinstance(i_test, list) else [i_test]
        if getattr(args, 'llffhold', 8) > 0:
            i_test = np.arange(images.shape[0])[::getattr(args, 'llffhold', 8)]
        i_val = i_test
        i_train = np.array([i for i in np.arange(int(images.shape[0])) if (i not in i_test and i not in i_val)])
        if args.no_ndc:
            near, far = np.ndarray.min(bds) * .9, np.ndarray.max(bds) * 1.
        else:
            near, far = 0., 1.
    elif args.dataset_type == 'blender':
        from .load_blender import load_blender_data
        images, poses, render_poses, hwf, i_split = load_blender_data(args.datadir, getattr(args, 'half_res', False),
                                                                      getattr(args, 'testskip', 8))
        i_train, i_val, i_test = i_split
        near, far = 2., 6.
        if getattr(args, 'random_bkgd', False):
            if args.white_bkgd:
                raise ValueError('load_dataset: random_bkgd keeps the alpha channel for per-ray backgrounds; white_bkgd composites it away')
        elif args.white_bkgd:
            images = images[..., :3] * images[..., -1:] + (1. - images[..., -1:])
        else:
            images = images[..., :3]
        poses = poses[:, :3, :4]
    else:
        raise ValueError('Unknown dataset type {!r} (this build reads blender and llff)'.format(args.dataset_type))
    H, W, focal = hwf
    H, W = int(H), int(W)
    if K is None:
        K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    if getattr(args, 'render_test', False):
        render_poses = np.array(poses[i_test])
    return dict(images=images, poses=poses, render_poses=render_poses, hwf=[H, W, focal], K=K, i_train=i_train, i_val=i_val,
                i_test=i_test, near=near, far=far)


def train(images, poses, H, W, focal, args, near=2., far=6., device='cuda', log=print, max_iters_per_epoch=None,
          compat_rng=False):
    """Epoch loop of run_nerf.py:train() (:337-546) on in-memory data: center-crop warm-up, per-epoch
    quadtree ray generation, fused steps with the on-device leaf-loss table, tree adjustment every
    `subdivide_every` epochs, checkpoints in the reference's file format.  images [n,H,W,3] (CPU or
    GPU tensor), poses [n,3,4].  args.random_bkgd: images [n,H,W,4] with straight colours (load_dataset); every step composites
    prediction and target over a fresh colour per ray (Trainer(bkgd='random'), alpha taken at the rays' own pixels)."""
    dev = torch.device(device)
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    kw_train, kw_test, start_epoch, global_iter, grad_vars, optimizer = create_nerf(args, device=dev)
    bds_dict = {'near': near, 'far': far}   # run_nerf.py:267-272: the bounds travel in both kwargs dicts
    kw_train.update(bds_dict)
    kw_test.update(bds_dict)
    occ_kw = {}
    if getattr(args, 'occupancy_train', False):     # opt-in (no such flag in the reference's parser): train through an occupancy grid
        from .occupancy import OccupancyCascade, OccupancyGrid
        geom = dict(N=getattr(args, 'occupancy_N', 128), bound=getattr(args, 'occupancy_bound', 1.2),
                    outside_occupied=getattr(args, 'occupancy_outside_occupied', True), device=dev)
        # args.occupancy_levels (default: a single grid): a cascade of that many levels, level l over occupancy_bound * occupancy_growth^l;
        # occupancy_N is then a cell count, a list of one per level, or a list of (nx, ny, nz) per level
        levels = getattr(args, 'occupancy_levels', None)
        occ = (OccupancyGrid.for_training(**geom) if not levels else
               OccupancyCascade.for_training(levels=int(levels), growth=float(getattr(args, 'occupancy_growth', 2.0)), **geom))
        occ_kw = dict(occupancy=occ,
                      tighten=getattr(args, 'occupancy_tighten', False),     # (matters with occupancy_outside_occupied=False)
                      # marched training (needs occupancy_outside_occupied=False): steps from march_after on train the fine network alone
                      march=getattr(args, 'march', None), march_cap=getattr(args, 'march_cap', 128), march_after=getattr(args, 'march_after', 0),
                      occupancy_every=getattr(args, 'occupancy_every', 16), occupancy_warmup=getattr(args, 'occupancy_warmup', 256))
    random_bkgd = bool(getattr(args, 'random_bkgd', False))
    # args.refine_poses (no such flag in the reference's parser; default off): the poses are a PoseTable that every step refines beside
    # the networks, at args.pose_lrate; the steps get the rows' pixels instead of rays.  The table is trainer.poses.
    refine_poses = bool(getattr(args, 'refine_poses', False))
    pose_kw = {}
    if refine_poses:
        from .poses import PoseTable
        pose_kw = dict(poses=PoseTable(torch.as_tensor(poses, dtype=torch.float32)[:, :3, :4]).to(dev),
                       pose_lrate=float(getattr(args, 'pose_lrate', 1e-3)))
    # args.optim_autoexpo, args.lambda_autoexpo (the reference's names, nerf++-ours ddp_train_nerf.py; default off): an ExposureTable with a
    # row per image is fitted beside the networks; the steps get the image of every row.  The table is trainer.exposure.
    autoexpo = bool(getattr(args, 'optim_autoexpo', False))
    expo_kw = {}
    if autoexpo:
        from .exposure import ExposureTable
        expo_kw = dict(exposure=ExposureTable(len(images)).to(dev), lambda_autoexpo=float(getattr(args, 'lambda_autoexpo', 1.)))
    # args.envmap, args.envmap_res, args.envmap_lrate (no such flags in the reference's parser; default off): an EnvMap is fitted beside the
    # networks as the background of every ray, and the test-time kwargs render over it.  The map is trainer.envmap.
    env_kw = {}
    if bool(getattr(args, 'envmap', False)):
        from .envmap import EnvMap
        env_kw = dict(envmap=EnvMap(res=int(getattr(args, 'envmap_res', 64))).to(dev), envmap_lrate=float(getattr(args, 'envmap_lrate', 1e-2)))
        kw_test['envmap'] = env_kw['envmap']
    # args.band_window, args.band_start, args.band_end, args.band_view (no such flags in the reference's parser; default off): the band
    # weights of the encodings ramp from low to high frequency over the steps band_start .. band_end (bands.BandSchedule)
    band_kw = {}
    if getattr(args, 'band_window', None):
        from .bands import BandSchedule
        band_kw = dict(bands=BandSchedule(args.band_window, getattr(args, 'band_start', 0), getattr(args, 'band_end', 0),
                                          view=bool(getattr(args, 'band_view', True))))
    trainer = Trainer(kw_train, H, W, K, near, far, lrate=args.lrate, lrate_decay=args.lrate_decay, bkgd='random' if random_bkgd else None,
                      lambda_dist=float(getattr(args, 'lambda_dist', 0.)), **occ_kw, **pose_kw, **expo_kw, **env_kw, **band_kw)
    trainer.global_iter = global_iter
    if len(optimizer.state_dict()['state']) > 0:   # create_nerf restored a checkpoint (ours or the reference's)
        trainer.load_torch_optimizer(optimizer)
        if refine_poses and create_nerf.last_ckpt_path is not None:
            trainer.load_pose_checkpoint(create_nerf.last_ckpt_path)
        if autoexpo and create_nerf.last_ckpt_path is not None:
            trainer.load_expo_checkpoint(create_nerf.last_ckpt_path)
        if env_kw and create_nerf.last_ckpt_path is not None:
            trainer.load_env_checkpoint(create_nerf.last_ckpt_path)
    images = torch.as_tensor(images, dtype=torch.float32)
    alpha_img = None
    if random_bkgd:      # the quadtree manager (and the leaf-error picks) see the straight colours; alpha travels beside them
        if images.shape[-1] != 4:
            raise ValueError('train: random_bkgd needs RGBA images [n,H,W,4] (load_dataset with args.random_bkgd)')
        alpha_img = images[..., 3].contiguous().to(dev)
        images = images[..., :3].contiguous()

    def alpha_at(pix):
        """alpha [N] at the pixels (image, row, col) of an epoch's rows, or None without random_bkgd."""
        if alpha_img is None:
            return None
        p = pix.to(dev).long()
        return alpha_img[p[:, 0], p[:, 1], p[:, 2]].contiguous()
    poses = torch.as_tensor(poses, dtype=torch.float32)[:, :3, :4]
    mgr = QuadTreeManager(H, W, K, images, poses, mseThres=0.0, max_depth=args.init_level, device=dev)
    # like the model, the subdivided trees of the checkpointed epoch are reloaded (run_nerf.py:338-345)
    if os.path.exists(tree_pkl_path(args, start_epoch)):
        mgr.load_trees(tree_pkl_path(args, start_epoch), cur_level=start_epoch)
        log("load '" + tree_pkl_path(args, start_epoch) + "'")
    N_rand = args.N_rand
    rank, world = parallel.rank(), parallel.world_size()
    history = []

    def run_batches(rays_o, rays_d, tgt, tags, decay, table, max_leaves, local_of=None, alpha=None, pix=None, img=None):
        """local_of = N: the tensors hold only THIS rank's rows of an epoch of N rows (gen_rays_device(shard=...)), batch after batch.
        pix (refine_poses): the rows' pixels [N,3]; the steps get them instead of the rays.  img (optim_autoexpo): the rows' images [N]."""
        if pix is not None:
            pix = pix.to(dev).int()
        if img is not None:
            img = img.to(dev).int()
        n_total = rays_o.shape[0] if local_of is None else local_of
        it = 0
        lo = 0
        for b0 in range(0, n_total, N_rand):
            b1 = min(b0 + N_rand, n_total)
            if local_of is None:
                sl = slice(b0 + rank, b1, world) if world > 1 else slice(b0, b1)
            else:
                cnt = parallel.shard_count(b1 - b0, N_rand, rank, world)
                sl = slice(lo, lo + cnt)
                lo += cnt
            # (a rank's rows r::world of the global batch are a strided view: the kernels take contiguous buffers)
            loss2, _ = trainer.step(None if pix is not None else rays_o[sl].contiguous(), None if pix is not None else rays_d[sl].contiguous(),
                                    tgt[sl].contiguous(), leaf_tag=None if tags is None else tags[sl].contiguous(),
                                    table=table, max_leaves=max_leaves, n_global=(b1 - b0) if world > 1 else None,
                                    decay=decay, alpha=None if alpha is None else alpha[sl].contiguous(),
                                    **({} if pix is None else {'pix': pix[sl].contiguous()}),
                                    **({} if img is None else {'img': img[sl].contiguous()}))
            it += 1
            if max_iters_per_epoch is not None and it >= max_iters_per_epoch:
                break
        return loss2, it

    parallel.sync_seed()   # every rank draws the same pixel lists (rows rank::world of ONE global batch)
    if start_epoch == 0:
        # center-crop warm-up (run_nerf.py:367-423): one coordinate set shared by all images, no LR decay
        dH, dW = H // 4, W // 4
        rows = torch.arange(H // 2 - dH, H // 2 + dH)
        cols = torch.arange(W // 2 - dW, W // 2 + dW)
        coords = torch.stack(torch.meshgrid(rows, cols, indexing='ij'), -1).reshape(-1, 2)
        randNum = min(int(N_rand * 500 / mgr.n_images), coords.shape[0])
        sel = coords[np.random.choice(coords.shape[0], size=[randNum], replace=False)]
        pix = torch.cat([torch.cat([torch.full((randNum, 1), i, dtype=torch.int64), sel], 1)
                         for i in range(mgr.n_images)], 0)
        ro, rd, tgt = mgr.gather(pix)
        loss2, it = run_batches(ro, rd, tgt, None, False, None, 0, alpha=alpha_at(pix), pix=pix if refine_poses else None,
                                img=pix[:, 0] if autoexpo else None)
        log('warm-up: {} iters, fine/coarse mse {}'.format(it, loss2.tolist()))

    for epoch_id in range(start_epoch + 1, args.n_epoch + 1):
        t0 = time.time()
        parallel.sync_seed()
        last = epoch_id == args.n_epoch
        if last:
            mgr.epoch_size = mgr.n_images * mgr.h * mgr.w
        # data parallel with the device generator: every rank generates ONLY the rows it steps (rows rank :: world of every batch; the seed is
        # the same on every rank after sync_seed, and the row -> ray map is a bijection of the row index: the union is the one epoch)
        sharded_gen = world > 1 and not compat_rng and dev.type == 'cuda'
        ro, rd, tgt = mgr.gen_rays_v3_multiThread(down_scale=1, prob=False, randSamp_proc=args.randSamp_perc,
                                                  last_epoch=last, compat_rng=compat_rng,
                                                  shard=(rank, world, N_rand) if sharded_gen else None, want_pix=random_bkgd or refine_poses or autoexpo)
        tags = mgr.result_leaf_tag
        max_leaves = mgr.max_leaves()
        table = torch.zeros(mgr.n_images * max_leaves, device=dev, dtype=torch.int32)
        loss2, it = run_batches(ro, rd, tgt, tags, True, table, max_leaves, local_of=mgr.epoch_rows if sharded_gen else None,
                                alpha=alpha_at(mgr.result_pix) if random_bkgd else None, pix=mgr.result_pix if refine_poses else None,
                                img=mgr.result_pix[:, 0] if autoexpo else None)
        psnr = mse2psnr(loss2[:1].cpu())
        history.append((epoch_id, it, float(loss2[0]), float(psnr[0]), time.time() - t0))
        log('epoch {}: {} iters, fine mse {:.5f} psnr {:.2f}, {:.1f}s'.format(*history[-1]) +
            ('' if trainer.live.frac is None else ' (live samples {:.2f}, backward {})'.format(
                trainer.live.frac, 'compacted' if trainer.live.on else 'plain')))
        if args.subdivide_every > 0 and epoch_id % args.subdivide_every == 0 and epoch_id < args.n_epoch - 1:
            if world > 1:
                parallel.all_reduce_max_int(table)
            mgr.adjust_tree_from_table(table.view(mgr.n_images, max_leaves), thres=args.subdivide_thres)
        if rank == 0 and getattr(args, 'save_ckpt', False):
            save_checkpoint(args, epoch_id, trainer, kw_train, mgr)
    return kw_train, kw_test, trainer, mgr, history
