"""PyTorch custom-op registration of the C-ABI entry points (`torch.ops.fastnerf.*`).

The product boundary is the C ABI (include/fastnerf.h, bound with ctypes in _lib.py); this module puts the SAME calls into
PyTorch's operator registry -- schemas, fake-tensor (shape) implementations, and autograd formulas where the reference
differentiates through the op -- so that they are visible to the dispatcher, `torch.compile` tracing and
`torch.library.opcheck` like any other PyTorch-ROCm custom op.  Nothing here computes: every implementation is one call into
ops.py (device pointers + the current HIP stream), and there is no CPU kernel registered -- a CPU tensor raises, as everywhere
in this package.

    torch.ops.fastnerf.gen_rays_pixels(pix, poses, fx, fy, cx, cy)          -> (rays_o, rays_d)   run_nerf_helpers.py:68-78
    torch.ops.fastnerf.pack_rays(rays_o, rays_d, near, far, ndc, H, W, focal) -> rays11             render.py:59-80
    torch.ops.fastnerf.sample_coarse(rays11, S, lindisp, perturb, t_rand, seed) -> z                 render.py:244-266
    torch.ops.fastnerf.posenc(x, L)                                            -> enc                run_nerf_helpers.py:15-63
    torch.ops.fastnerf.mlp_fwd(rays11, z, params, packed_fwd)                  -> raw                model.py:38-63 (+ PE)
    torch.ops.fastnerf.raw2outputs(raw, z, rays11, noise, white_bkgd)          -> (rgb, disp, acc, weights, depth)   render.py:149-192
                                                                                  differentiable w.r.t. raw through rgb
    torch.ops.fastnerf.raw2outputs_full(raw, z, rays11, noise, white_bkgd)     -> (rgb, disp, acc, weights, depth)   render.py:149-192
                                                                                  differentiable w.r.t. raw through all five
    torch.ops.fastnerf.distortion(w, z, rays11, lindisp, skip)                 -> ell [n]            the distortion loss of mip-NeRF 360
                                                                                  differentiable w.r.t. w (z, near, far are constants)
    torch.ops.fastnerf.sample_pdf_merge(z, weights, Ni, det, u, seed)          -> (z_all, z_samples, z_std)          run_nerf_helpers.py:112-155 + render.py:283
    torch.ops.fastnerf.mse_leafmax(rgb, rgb0, target, grad_scale, leaf_tag, max_leaves, table) -> (loss2, g_rgb, g_rgb0)   (table mutated)
    torch.ops.fastnerf.adam_step(params, grads, m, v, lr, step, beta1, beta2, eps)             -> ()  (params, m, v mutated)
    torch.ops.fastnerf.compact_live(draw)                                      -> (live_idx, counts)
"""
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import ops

_lib_def = torch.library.custom_op


@_lib_def('fastnerf::gen_rays_pixels', mutates_args=())
def gen_rays_pixels(pix: Tensor, poses: Tensor, fx: float, fy: float, cx: float, cy: float) -> Tuple[Tensor, Tensor]:
    K = [[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]
    return ops.gen_rays_pixels(pix, poses, K)


@gen_rays_pixels.register_fake
def _(pix, poses, fx, fy, cx, cy):
    return pix.new_empty((pix.shape[0], 3), dtype=torch.float32), pix.new_empty((pix.shape[0], 3), dtype=torch.float32)


@_lib_def('fastnerf::pack_rays', mutates_args=())
def pack_rays(rays_o: Tensor, rays_d: Tensor, near: float, far: float, ndc: bool, H: int, W: int, focal: float) -> Tensor:
    return ops.pack_rays(rays_o, rays_d, near, far, ndc=ndc, H=H, W=W, focal=focal)


@pack_rays.register_fake
def _(rays_o, rays_d, near, far, ndc, H, W, focal):
    return rays_o.new_empty((rays_o.numel() // 3, 11))


@_lib_def('fastnerf::sample_coarse', mutates_args=())
def sample_coarse(rays11: Tensor, S: int, lindisp: bool, perturb: bool, t_rand: Optional[Tensor], seed: int) -> Tensor:
    return ops.sample_coarse(rays11, S, lindisp=lindisp, perturb=perturb, t_rand=t_rand, seed=seed)


@sample_coarse.register_fake
def _(rays11, S, lindisp, perturb, t_rand, seed):
    return rays11.new_empty((rays11.shape[0], S))


@_lib_def('fastnerf::posenc', mutates_args=())
def posenc(x: Tensor, L: int) -> Tensor:
    return ops.posenc(x, L)


@posenc.register_fake
def _(x, L):
    return x.new_empty(tuple(x.shape[:-1]) + (3 + 6 * L,))


@_lib_def('fastnerf::mlp_fwd', mutates_args=())
def mlp_fwd(rays11: Tensor, z: Tensor, params: Tensor, packed_fwd: Tensor) -> Tensor:
    # (the tensor objects the dispatcher hands over carry no Python attributes: ops.mlp_fwd finds the math mode packed_fwd
    # was produced under in ops.mlp_pack's registry by storage address, and raises when it is not the current mode)
    return ops.mlp_fwd(rays11, z, params, packed_fwd)


@mlp_fwd.register_fake
def _(rays11, z, params, packed_fwd):
    return z.new_empty(tuple(z.shape) + (4,))


@_lib_def('fastnerf::raw2outputs', mutates_args=())
def raw2outputs(raw: Tensor, z: Tensor, rays11: Tensor, noise: Optional[Tensor], white_bkgd: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    return ops.raw2outputs_fwd(raw.contiguous(), z.contiguous(), rays11, noise, white_bkgd)


@raw2outputs.register_fake
def _(raw, z, rays11, noise, white_bkgd):
    n, S = z.shape
    return z.new_empty((n, 3)), z.new_empty((n,)), z.new_empty((n,)), z.new_empty((n, S)), z.new_empty((n,))


@_lib_def('fastnerf::raw2outputs_bwd', mutates_args=())
def raw2outputs_bwd(raw: Tensor, z: Tensor, rays11: Tensor, g_rgb: Tensor, noise: Optional[Tensor], white_bkgd: bool) -> Tensor:
    return ops.raw2outputs_bwd(raw.contiguous(), z.contiguous(), rays11, g_rgb.contiguous(), noise, white_bkgd)


@raw2outputs_bwd.register_fake
def _(raw, z, rays11, g_rgb, noise, white_bkgd):
    return raw.new_empty(raw.shape)


def _r2o_setup(ctx, inputs, output):
    raw, z, rays11, noise, white_bkgd = inputs
    ctx.save_for_backward(raw, z, rays11, noise if noise is not None else raw.new_empty(0))
    ctx.has_noise, ctx.white = noise is not None, white_bkgd


def _r2o_backward(ctx, g_rgb, g_disp, g_acc, g_w, g_depth):
    # the training loss reaches the network through the colour map only (run_nerf.py:482-490): that is the implemented formula
    raw, z, rays11, noise = ctx.saved_tensors
    for name, g in (('disp', g_disp), ('acc', g_acc), ('weights', g_w), ('depth', g_depth)):
        if g is not None and bool((g != 0).any()):
            raise NotImplementedError('torch.ops.fastnerf.raw2outputs is differentiable through the colour map only; got a non-zero '
                                      'gradient for ' + name)
    draw = torch.ops.fastnerf.raw2outputs_bwd(raw, z, rays11, g_rgb, noise if ctx.has_noise else None, ctx.white)
    return draw, None, None, None, None


raw2outputs.register_autograd(_r2o_backward, setup_context=_r2o_setup)


@_lib_def('fastnerf::raw2outputs_full', mutates_args=())
def raw2outputs_full(raw: Tensor, z: Tensor, rays11: Tensor, noise: Optional[Tensor], white_bkgd: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    return ops.raw2outputs_fwd(raw.contiguous(), z.contiguous(), rays11, noise, white_bkgd)


@raw2outputs_full.register_fake
def _(raw, z, rays11, noise, white_bkgd):
    n, S = z.shape
    return z.new_empty((n, 3)), z.new_empty((n,)), z.new_empty((n,)), z.new_empty((n, S)), z.new_empty((n,))


@_lib_def('fastnerf::raw2outputs_bwd_full', mutates_args=())
def raw2outputs_bwd_full(raw: Tensor, z: Tensor, rays11: Tensor, acc: Tensor, depth: Tensor, g_rgb: Optional[Tensor],
                         g_disp: Optional[Tensor], g_acc: Optional[Tensor], g_w: Optional[Tensor], g_depth: Optional[Tensor],
                         noise: Optional[Tensor], white_bkgd: bool) -> Tensor:
    return ops.raw2outputs_bwd_full(raw.contiguous(), z.contiguous(), rays11, acc, depth, g_rgb, g_disp, g_acc, g_w, g_depth,
                                    noise, white_bkgd)


@raw2outputs_bwd_full.register_fake
def _(raw, z, rays11, acc, depth, g_rgb, g_disp, g_acc, g_w, g_depth, noise, white_bkgd):
    return raw.new_empty(raw.shape)


def _r2o_full_setup(ctx, inputs, output):
    raw, z, rays11, noise, white_bkgd = inputs
    _, _, acc, _, depth = output
    ctx.save_for_backward(raw, z, rays11, noise if noise is not None else raw.new_empty(0), acc, depth)
    ctx.has_noise, ctx.white = noise is not None, white_bkgd
    ctx.set_materialize_grads(False)      # an output nobody differentiates arrives as None: the kernel skips its read


def _r2o_full_backward(ctx, g_rgb, g_disp, g_acc, g_w, g_depth):
    # every output of render.py:149-192 reaches raw, as in the reference's autograd (z and rays_d are not differentiated)
    raw, z, rays11, noise, acc, depth = ctx.saved_tensors
    if all(g is None for g in (g_rgb, g_disp, g_acc, g_w, g_depth)):
        return None, None, None, None, None
    draw = torch.ops.fastnerf.raw2outputs_bwd_full(raw, z, rays11, acc, depth, g_rgb, g_disp, g_acc, g_w, g_depth,
                                                   noise if ctx.has_noise else None, ctx.white)
    return draw, None, None, None, None


raw2outputs_full.register_autograd(_r2o_full_backward, setup_context=_r2o_full_setup)


@_lib_def('fastnerf::distortion', mutates_args=())
def distortion(w: Tensor, z: Tensor, rays11: Tensor, lindisp: bool, skip: Optional[Tensor]) -> Tensor:
    return ops.distortion(w.contiguous(), z.contiguous(), rays11.contiguous(), lindisp, skip, want=('ell',))[0]


@distortion.register_fake
def _(w, z, rays11, lindisp, skip):
    return z.new_empty((z.shape[0],))


@_lib_def('fastnerf::distortion_bwd', mutates_args=())
def distortion_bwd(w: Tensor, z: Tensor, rays11: Tensor, lindisp: bool, skip: Optional[Tensor], g_ell: Tensor) -> Tensor:
    return ops.distortion(w.contiguous(), z.contiguous(), rays11.contiguous(), lindisp, skip, g_up=g_ell.contiguous(), want=('g_w',))[1]


@distortion_bwd.register_fake
def _(w, z, rays11, lindisp, skip, g_ell):
    return z.new_empty(z.shape)


def _dist_setup(ctx, inputs, output):
    w, z, rays11, lindisp, skip = inputs
    ctx.save_for_backward(w, z, rays11, skip if skip is not None else w.new_empty(0, dtype=torch.uint8))
    ctx.has_skip, ctx.lindisp = skip is not None, lindisp


def _dist_backward(ctx, g_ell):
    # the same kernel with the upstream gradient per ray: g_w[r][i] = g_ell[r] dl_r/dw_i (depths, near and far are constants)
    w, z, rays11, skip = ctx.saved_tensors
    return torch.ops.fastnerf.distortion_bwd(w, z, rays11, ctx.lindisp, skip if ctx.has_skip else None, g_ell), None, None, None, None


distortion.register_autograd(_dist_backward, setup_context=_dist_setup)


@_lib_def('fastnerf::sample_pdf_merge', mutates_args=())
def sample_pdf_merge(z: Tensor, weights: Tensor, Ni: int, det: bool, u: Optional[Tensor], seed: int) -> Tuple[Tensor, Tensor, Tensor]:
    return ops.sample_pdf_merge(z, weights, Ni, det=det, u=u, seed=seed)


@sample_pdf_merge.register_fake
def _(z, weights, Ni, det, u, seed):
    n, S = z.shape
    return z.new_empty((n, S + Ni)), z.new_empty((n, Ni)), z.new_empty((n,))


@_lib_def('fastnerf::mse_leafmax', mutates_args=('table',))
def mse_leafmax(rgb: Tensor, rgb0: Tensor, target: Tensor, grad_scale: float, leaf_tag: Optional[Tensor], max_leaves: int,
                table: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    return ops.mse_leafmax(rgb, rgb0, target, grad_scale=grad_scale, leaf_tag=leaf_tag, max_leaves=max_leaves, table=table)


@mse_leafmax.register_fake
def _(rgb, rgb0, target, grad_scale, leaf_tag, max_leaves, table):
    return rgb.new_empty((2,)), rgb.new_empty(rgb.shape), rgb.new_empty(rgb.shape)


@_lib_def('fastnerf::adam_step', mutates_args=('params', 'm', 'v'))
def adam_step(params: Tensor, grads: Tensor, m: Tensor, v: Tensor, lr: float, step: int, beta1: float, beta2: float, eps: float) -> None:
    ops.adam_step(params, grads, m, v, lr, step, beta1, beta2, eps)


@_lib_def('fastnerf::compact_live', mutates_args=())
def compact_live(draw: Tensor) -> Tuple[Tensor, Tensor]:
    return ops.compact_live(draw)


@compact_live.register_fake
def _(draw):
    return draw.new_empty((draw.numel() // 4,), dtype=torch.int32), draw.new_empty((2,), dtype=torch.int32)


OPS = ['gen_rays_pixels', 'pack_rays', 'sample_coarse', 'posenc', 'mlp_fwd', 'raw2outputs', 'raw2outputs_bwd', 'raw2outputs_full',
       'raw2outputs_bwd_full', 'distortion', 'distortion_bwd', 'sample_pdf_merge', 'mse_leafmax', 'adam_step', 'compact_live']
