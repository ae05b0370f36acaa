"""Thin tensor-level wrappers over the C ABI (one per entry point).

PyTorch is plumbing here: it owns device memory and the stream; every op calls
straight into libfastnerf.so with raw pointers.  No op has a CPU fallback."""
import ctypes
import os
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, require_gpu, stream  # noqa: F401 (re-exported: tree.py uses ops.ptr / ops.stream)

NET_PARAMS = 595844
DACT_FLOATS = 2432


# ---- matrix-core math mode of the 8x256 MLP kernels ---------------------------------------------
# 'fp32'   : v_mfma_f32_32x32x2_f32 (csrc/mlp_*.hip), every kind: the products and sums of an fp32 FMA chain
# 'bf16x6' : csrc/mlp_*.hip MM_X6 -- every fp32 operand decomposed EXACTLY into three bf16 pieces, a product = its six piece
#            products of weight >= 2^-16, fp32 accumulation on v_mfma_f32_16x16x32_bf16: fp32-WIDTH products (the dropped terms
#            are <= 2^-24 of the product) at 2.67x the matrix rate of the fp32 instruction; same buffers as 'fp32' except the
#            packed weights (three bf16 planes)
# 'bf16x3' : 3-term split-bf16 (two pieces, 16 significand bits) on the same instruction (csrc/mlp_bf16.hip): NARROWER than
#            fp32 (products ~2^-17 relative), ~2.5x the rate of 'fp32'; rendered RGB still within 1e-6 of the fp32 kernels
# (the two-fp16-piece 'f16x3' experiment of round 4 was deleted in round 6: unguarded fp16 range; its record is profiles/r04_f16x3_*)
MATH_MODES = ('fp32', 'bf16x3', 'bf16x6')
_MODE_ID = {'fp32': 0, 'bf16x3': 1, 'bf16x6': 2}
_MATH = os.environ.get('FASTNERF_MATH', 'bf16x6')   # default: the reference's arithmetic width
assert _MATH in MATH_MODES, 'FASTNERF_MATH must be one of ' + ', '.join(MATH_MODES)


def get_math():
    return _MATH


def set_math(mode):
    """Switch the math mode.  Packed weights / saved activations are mode-specific: models re-pack on their
    next packed() call; do not mix buffers produced under different modes."""
    global _MATH
    assert mode in MATH_MODES
    _MATH = mode


def mode_id():
    """math_mode argument of the fused C-ABI entry points (fastnerf_render_rays_*, fastnerf_train_step)."""
    return _MODE_ID[_MATH]


# math mode a packed-weight buffer was produced under: a Python attribute on the tensor object AND a registry by storage
# address (a tensor that went through the PyTorch dispatcher -- torch.ops.fastnerf.mlp_fwd -- is a fresh object without the
# attribute), so that weights packed under one mode and used under the other are an error, never garbage
_PACK_TAGS = {}


def _tag_packed(t, tag):
    """Tag a packed-weight buffer with its math mode.  The persistent buffers of NeRF.packed() / NerfNet.packed() are re-packed in
    place on every step: ONE finalizer per tensor object (a token the object carries), later calls only update the tag."""
    t._fn_math = tag
    key = (t.device.index, t.data_ptr(), t.numel())
    token = getattr(t, '_fn_token', None)
    entry = _PACK_TAGS.get(key)
    if token is not None and entry is not None and entry[1] is token:
        if entry[0] != tag:
            _PACK_TAGS[key] = (tag, token)
        return
    token = object()
    t._fn_token = token
    _PACK_TAGS[key] = (tag, token)
    # the entry lives as long as the tensor object mlp_pack handed out: a freed block that the caching allocator hands to an
    # unrelated tensor must not inherit the tag
    weakref.finalize(t, _drop_tag, key, token)


def _drop_tag(key, token):
    entry = _PACK_TAGS.get(key)
    if entry is not None and entry[1] is token:
        del _PACK_TAGS[key]


def packed_tag(t):
    tag = getattr(t, '_fn_math', None)
    if tag:
        return tag
    entry = _PACK_TAGS.get((t.device.index, t.data_ptr(), t.numel()))
    return entry[0] if entry else None


# The MLP entry points of each family (include/fastnerf.h), by operation: the one place that knows their names.  The plain
# forward is the odd one out: only fastnerf_mlp_x6_fwd takes `flags` (after `act`).
_MLP = {
    'fp32': dict(pack='fastnerf_mlp_pack_ex', fwd='fastnerf_mlp_fwd_ex', bwd='fastnerf_mlp_bwd_ex', fwd_live='fastnerf_mlp_fwd_live_ex',
                 bwd_live='fastnerf_mlp_bwd_live_ex', fwd_list='fastnerf_mlp_fwd_list_ex'),
    'bf16x3': dict(pack='fastnerf_mlp_bf16_pack', fwd='fastnerf_mlp_bf16_fwd', bwd='fastnerf_mlp_bf16_bwd',
                   fwd_live='fastnerf_mlp_bf16_fwd_live', bwd_live='fastnerf_mlp_bf16_bwd_live', fwd_list='fastnerf_mlp_bf16_fwd_list'),
    'bf16x6': dict(pack='fastnerf_mlp_x6_pack', fwd='fastnerf_mlp_x6_fwd', bwd='fastnerf_mlp_x6_bwd', fwd_live='fastnerf_mlp_x6_fwd_live',
                   bwd_live='fastnerf_mlp_x6_bwd_live', fwd_list='fastnerf_mlp_x6_fwd_list'),
}


def _family(kind):
    """The kernel family that serves a net of this kind under the current math mode: the split-bf16 kernels exist for kinds
    0 to 2 only, any other kind runs on the exact-fp32 ones under 'bf16x3'."""
    if _MATH == 'bf16x3' and int(kind) not in (0, 1, 2):
        return 'fp32'
    return _MATH


def _mlp(op, kind):
    """(ctypes function, its name) of the MLP operation `op` for a net of this kind under the current math mode."""
    name = _MLP[_family(kind)][op]
    return getattr(lib(), name), name


def act_floats(P, kind=0):
    """Size (floats) of the saved-activation buffer for P points of a net of the given kind."""
    if _family(kind) == 'bf16x3':
        return int(lib().fastnerf_mlp_bf16_floats(int(kind), 3, int(P)))
    return int(lib().fastnerf_mlp_act_floats(int(kind), int(P)))


def dact_floats(P, kind=0):
    """Size (floats) of the pre-activation-gradient workspace for P points."""
    if _family(kind) == 'bf16x3':
        return int(lib().fastnerf_mlp_bf16_floats(int(kind), 4, int(P)))
    return int(P) * DACT_FLOATS


def packed_floats(kind, which):
    """which: 1 forward, 2 backward packed-weight buffer (floats) under the current math mode."""
    family = _family(kind)
    if family == 'bf16x3':
        return int(lib().fastnerf_mlp_bf16_floats(int(kind), int(which), 0))
    if family == 'bf16x6':
        return int(lib().fastnerf_mlp_x6_packed_floats(int(kind), int(which)))
    return net_floats(kind, which)


def net_floats(kind, what=0):
    """what: 0 parameters, 1 packed-forward, 2 packed-backward, 3 padded PE width."""
    return int(lib().fastnerf_net_floats(int(kind), int(what)))


def _f32(t):
    """t as contiguous fp32: t itself, or a new tensor.  Bind a new one to a name until the call is enqueued: a temporary inside the
    argument list is freed as soon as its pointer is taken, and the allocator hands its block to the next temporary of that list,
    whose conversion then overwrites it before the kernel reads either."""
    return t.contiguous().float()


def _need_f32(name, t, *shape):
    """Refuse, before any launch, a tensor that the library would read as fp32 [*shape] and that is something else (ptr() only
    checks contiguity: a float64 tensor would be read as twice as many fp32 values, a wrong shape beyond its end)."""
    if t.dtype != torch.float32:
        raise TypeError(f'{name} must be float32, got {t.dtype}')
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name} must have shape {tuple(shape)}, got {tuple(t.shape)}')


def gen_rays(H, W, K, c2w):
    """get_rays (run_nerf_helpers.py:68-78) for every pixel of one camera -> ([H,W,3], [H,W,3])."""
    c2w_t = torch.as_tensor(c2w, dtype=torch.float32)
    dev = c2w_t.device if c2w_t.is_cuda else torch.device('cuda')
    host = np.ascontiguousarray(c2w_t.detach().cpu().numpy()[:3, :4], dtype=np.float32)
    ro = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
    rd = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
    check(lib().fastnerf_gen_rays(H, W, float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]),
                                  host.ctypes.data, ptr(ro), ptr(rd), stream()), 'fastnerf_gen_rays')
    return ro, rd


def gen_rays_pixels(pix, poses, K):
    """Rays for selected (image,row,col) pixels; pix [n,3] int32 cuda, poses [n_img,3,4] cuda."""
    require_gpu(pix, poses)
    n = pix.shape[0]
    ro = torch.empty(n, 3, device=pix.device, dtype=torch.float32)
    rd = torch.empty(n, 3, device=pix.device, dtype=torch.float32)
    pix, poses = pix.contiguous().int(), _f32(poses)      # (named: see _f32)
    check(lib().fastnerf_gen_rays_pixels(n, ptr(pix), ptr(poses), float(K[0][0]),
                                         float(K[1][1]), float(K[0][2]), float(K[1][2]), ptr(ro), ptr(rd), stream()),
          'fastnerf_gen_rays_pixels')
    return ro, rd


def ndc_rays(H, W, focal, near, rays_o, rays_d):
    require_gpu(rays_o, rays_d)
    sh = rays_o.shape
    ro, rd = _f32(rays_o).reshape(-1, 3), _f32(rays_d).reshape(-1, 3)
    oo, od = torch.empty_like(ro), torch.empty_like(rd)
    check(lib().fastnerf_ndc_rays(ro.shape[0], H, W, float(focal), float(near), ptr(ro), ptr(rd), ptr(oo), ptr(od),
                                  stream()), 'fastnerf_ndc_rays')
    return oo.reshape(sh), od.reshape(sh)


def pack_rays(rays_o, rays_d, near, far, ndc=False, H=0, W=0, focal=1.0):
    require_gpu(rays_o, rays_d)
    ro, rd = _f32(rays_o).reshape(-1, 3), _f32(rays_d).reshape(-1, 3)
    out = torch.empty(ro.shape[0], 11, device=ro.device, dtype=torch.float32)
    check(lib().fastnerf_pack_rays(ro.shape[0], ptr(ro), ptr(rd), float(near), float(far), int(bool(ndc)), int(H),
                                   int(W), float(focal), ptr(out), stream()), 'fastnerf_pack_rays')
    return out


def sample_coarse(rays11, S, lindisp=False, perturb=False, t_rand=None, seed=0):
    require_gpu(rays11, t_rand)
    n = rays11.shape[0]
    _need_f32('rays11', rays11, n, 11)
    z = torch.empty(n, S, device=rays11.device, dtype=torch.float32)
    if t_rand is not None:
        t_rand = _f32(t_rand)
        assert t_rand.shape == (n, S)
    check(lib().fastnerf_sample_coarse(n, S, ptr(rays11), int(bool(lindisp)), int(bool(perturb) or t_rand is not None),
                                       ptr(t_rand), int(seed), ptr(z), stream()), 'fastnerf_sample_coarse')
    return z


def posenc(x, L):
    require_gpu(x)
    sh = x.shape
    xf = _f32(x).reshape(-1, 3)
    out = torch.empty(xf.shape[0], 3 + 6 * L, device=x.device, dtype=torch.float32)
    check(lib().fastnerf_posenc(xf.shape[0], L, ptr(xf), ptr(out), stream()), 'fastnerf_posenc')
    return out.reshape(list(sh[:-1]) + [3 + 6 * L])


def mlp_pack(params, packed_fwd=None, packed_bwd=None, kind=0):
    require_gpu(params)
    assert params.numel() == net_floats(kind, 0) and params.is_contiguous()
    if packed_fwd is None:
        packed_fwd = torch.empty(packed_floats(kind, 1), device=params.device, dtype=torch.float32)
    if packed_bwd is None:
        packed_bwd = torch.empty(packed_floats(kind, 2), device=params.device, dtype=torch.float32)
    assert packed_fwd.numel() == packed_floats(kind, 1) and packed_bwd.numel() == packed_floats(kind, 2), \
        'packed buffers were sized under a different math mode'
    # the two modes' buffers can have the same size: tag them so that a mix-up is an error, not garbage
    for t in (packed_fwd, packed_bwd):
        _tag_packed(t, _MATH)
    fn, name = _mlp('pack', kind)
    check(fn(int(kind), ptr(params), ptr(packed_fwd), ptr(packed_bwd), stream()), name)
    return packed_fwd, packed_bwd


def mlp_fwd(rays11, z, params, packed_fwd, act=None, raw=None, kind=0):
    """kind 0/1: points o + d*z; kind 2 (nerf++ background): inverted-sphere points of depth z, consumed
    far->near (raw[:, s] belongs to z[:, S-1-s])."""
    require_gpu(rays11, z, params, packed_fwd)
    n, S = z.shape
    if raw is None:
        raw = torch.empty(n, S, 4, device=z.device, dtype=torch.float32)
    if act is not None:
        assert act.numel() >= act_floats(n * S, kind)
    assert packed_fwd.numel() == packed_floats(kind, 1) and packed_tag(packed_fwd) == _MATH, \
        'packed weights were not produced by mlp_pack under the current math mode'
    fn, name = _mlp('fwd', kind)
    flags = (0,) if name == 'fastnerf_mlp_x6_fwd' else ()
    check(fn(int(kind), n, S, ptr(rays11), ptr(z), ptr(params), ptr(packed_fwd), ptr(raw), ptr(act), *flags, stream()), name)
    return raw


def mlp_bwd_partial_floats():
    return max(int(lib().fastnerf_mlp_bwd_partial_floats()), int(lib().fastnerf_mlp_bf16_partial_floats()))


def mlp_bwd(draw, act, params, packed_bwd, dact, partial, grads, kind=0):
    require_gpu(draw, act, params, packed_bwd, dact, partial, grads)
    n, S = draw.shape[0], draw.shape[1]
    assert dact.numel() >= dact_floats(n * S, kind) and grads.numel() == net_floats(kind, 0)
    assert packed_bwd.numel() == packed_floats(kind, 2) and packed_tag(packed_bwd) == _MATH, \
        'packed weights were not produced by mlp_pack under the current math mode'
    fn, name = _mlp('bwd', kind)
    check(fn(int(kind), n, S, ptr(draw), ptr(act), ptr(params), ptr(packed_bwd), ptr(dact), ptr(partial), ptr(grads), stream()), name)
    return grads


def sigma_grad_ws_floats(P):
    """Floats of scratch one mlp_sigma_grad call over P points needs under the current math mode (about 20 KB per point)."""
    return int(check(lib().fastnerf_mlp_sigma_grad_ws_floats(mode_id(), int(P)), 'fastnerf_mlp_sigma_grad_ws_floats'))


def mlp_sigma_grad(rays11, z, params, packed_fwd, packed_bwd, ws=None, grad=None, want_sigma=True):
    """(sigma [n,S], grad [n,S,3]): the density logit raw[..., 3] of the current math mode's forward at the points o + d*z and its
    gradient with respect to the point -- both BEFORE the ReLU of raw2outputs (fastnerf_mlp_sigma_grad, kind 0).  sigma equals
    mlp_fwd(...)[..., 3] bit for bit; it is None with want_sigma=False.  ws: caller-owned scratch of >= sigma_grad_ws_floats(n*S)
    floats (default: allocated here); grad: caller-owned output of >= n*S*3 floats, only its first n*S rows are written."""
    require_gpu(rays11, z, params, packed_fwd, packed_bwd, ws, grad)
    n, S = z.shape
    P = n * S
    assert rays11.shape == (n, 11) and z.dtype == torch.float32 and params.numel() == net_floats(0, 0)
    assert packed_fwd.numel() == packed_floats(0, 1) and packed_bwd.numel() == packed_floats(0, 2) \
        and packed_tag(packed_fwd) == _MATH and packed_tag(packed_bwd) == _MATH, \
        'packed weights were not produced by mlp_pack under the current math mode'
    dev = z.device
    if ws is None:
        ws = torch.empty(sigma_grad_ws_floats(P), device=dev, dtype=torch.float32)
    assert ws.dtype == torch.float32 and ws.numel() >= sigma_grad_ws_floats(P)
    if grad is None:
        grad = torch.empty(P * 3, device=dev, dtype=torch.float32)
    assert grad.dtype == torch.float32 and grad.numel() >= P * 3
    sigma = torch.empty(n, S, device=dev, dtype=torch.float32) if want_sigma else None
    check(lib().fastnerf_mlp_sigma_grad(mode_id(), 0, n, S, ptr(rays11), ptr(z), ptr(params), ptr(packed_fwd), ptr(packed_bwd), ptr(ws),
                                        ptr(sigma), ptr(grad), stream()), 'fastnerf_mlp_sigma_grad')
    return sigma, grad.reshape(-1)[:P * 3].view(n, S, 3)


def ray_grad_ws_floats(n, S):
    """Floats of scratch one ray_grad call over n rays of S samples needs (the per-point gradient, 12 bytes per sample)."""
    return int(check(lib().fastnerf_ray_grad_ws_floats(mode_id(), int(n), int(S)), 'fastnerf_ray_grad_ws_floats'))


def ray_grad(rays11, z, raw, noise, draw, act, dact, params, d_rays=None, accumulate=False, ws=None, kind=0):
    """d_rays [n,11]: the gradient of a loss with respect to the rays (o, d, near, far, viewdir) of ONE pass of render_rays
    (fastnerf_ray_grad, kind 0, math modes fp32 and bf16x6).  Call it after raw2outputs_bwd (-> draw) and mlp_bwd on that draw,
    with the same `act` and `dact`: it reads the pre-activation gradients the backward left there.  rays11, z, raw, noise: what the
    pass's raw2outputs_bwd got.  Columns 6:8 (near, far) are exact zeros: they are constants of this gradient.
    accumulate=True adds to `d_rays` (a second pass on top of the first); otherwise its n rows are overwritten (default: allocated
    here).  bf16x3 raises NotImplementedError: its saved tensors have no ray-gradient kernel, and a partial gradient is worse than none."""
    if _MATH == 'bf16x3':
        raise NotImplementedError("ray gradients exist in the math modes 'fp32' and 'bf16x6' only (FASTNERF_MATH / ops.set_math), "
                                  "not in 'bf16x3'")
    require_gpu(rays11, z, raw, noise, draw, act, dact, params, d_rays, ws)
    n, S = z.shape
    P = n * S
    f32 = torch.float32
    assert rays11.shape == (n, 11) and rays11.dtype == f32 and z.dtype == f32 and params.numel() == net_floats(0, 0)
    assert raw.numel() == P * 4 and draw.numel() == P * 4 and raw.dtype == f32 and draw.dtype == f32
    assert noise is None or (noise.numel() == P and noise.dtype == f32)
    assert act.dtype == f32 and dact.dtype == f32 and act.numel() >= act_floats(P) and dact.numel() >= dact_floats(P)
    if d_rays is None:
        assert not accumulate, 'accumulate=True needs the d_rays to add to'
        d_rays = torch.empty(n, 11, device=z.device, dtype=f32)
    assert d_rays.dtype == f32 and d_rays.numel() >= n * 11
    if ws is None:
        ws = torch.empty(ray_grad_ws_floats(n, S), device=z.device, dtype=f32)
    assert ws.dtype == f32 and ws.numel() >= ray_grad_ws_floats(n, S)
    check(lib().fastnerf_ray_grad(mode_id(), int(kind), n, S, ptr(rays11), ptr(z), ptr(raw), ptr(noise), ptr(draw), ptr(act), ptr(dact),
                                  ptr(params), ptr(ws), int(bool(accumulate)), ptr(d_rays), stream()), 'fastnerf_ray_grad')
    return d_rays.reshape(-1)[:n * 11].view(n, 11)


# ---- pose table (csrc/pose.hip; include/fastnerf.h, "pose table") --------------------------------
def _need_pix(pix):
    """Refuse a pixel list that fastnerf_pose_grad would not read as int32 [n,3] rows (no value is read here: rows must name
    existing images, as for gen_rays_pixels)."""
    if pix.dtype != torch.int32:
        raise TypeError(f'pix must be int32, got {pix.dtype}')
    if pix.dim() != 2 or pix.shape[1] != 3:
        raise ValueError(f'pix must have shape (n, 3), got {tuple(pix.shape)}')


def pose_exp(base, xi=None, out=None):
    """poses [n_img,3,4] = (exp(hat(omega)) R0 | t0 + tau) of the base poses [n_img,3,4] and xi [n_img,6] = (omega, tau)
    (fastnerf_pose_exp).  xi=None, or a zero row, gives the base pose bit for bit."""
    require_gpu(base, xi, out)
    n_img = base.shape[0]
    _need_f32('base', base, n_img, 3, 4)
    if n_img < 1:
        raise ValueError('pose_exp: at least one image')
    if xi is not None:
        _need_f32('xi', xi, n_img, 6)
    if out is None:
        out = torch.empty_like(base)
    _need_f32('out', out, n_img, 3, 4)
    check(lib().fastnerf_pose_exp(n_img, ptr(base), ptr(xi), ptr(out), stream()), 'fastnerf_pose_exp')
    return out


def pose_exp_bwd(base, xi, d_poses, d_xi=None):
    """d_xi [n_img,6] = d(loss)/d(xi) from d_poses [n_img,3,4] = d(loss)/d(pose_exp(base, xi)) (fastnerf_pose_exp_bwd)."""
    require_gpu(base, xi, d_poses, d_xi)
    n_img = base.shape[0]
    _need_f32('base', base, n_img, 3, 4)
    if n_img < 1:
        raise ValueError('pose_exp_bwd: at least one image')
    if xi is not None:
        _need_f32('xi', xi, n_img, 6)
    _need_f32('d_poses', d_poses, n_img, 3, 4)
    if d_xi is None:
        d_xi = torch.empty(n_img, 6, device=base.device, dtype=torch.float32)
    _need_f32('d_xi', d_xi, n_img, 6)
    check(lib().fastnerf_pose_exp_bwd(n_img, ptr(base), ptr(xi), ptr(d_poses), ptr(d_xi), stream()), 'fastnerf_pose_exp_bwd')
    return d_xi


def pose_grad_ws_floats(n, n_img):
    """Floats of scratch one pose_grad call over n rays of n_img images needs (0 for a small batch)."""
    return int(check(lib().fastnerf_pose_grad_ws_floats(int(n), int(n_img)), 'fastnerf_pose_grad_ws_floats'))


def pose_grad(pix, poses, K, d_rays, d_poses=None, ws=None):
    """d_poses [n_img,3,4]: the gradient with respect to the poses of a loss whose gradient with respect to the pinhole rays of the
    pixels pix [n,3] int32 = (image, row, col) is d_rays [n,11] (ops.ray_grad; columns 6:8 ignored) -- fastnerf_pose_grad, a
    segmented sum without atomics.  An image without a ray gets zeros."""
    require_gpu(pix, poses, d_rays, d_poses, ws)
    n_img = poses.shape[0]
    _need_f32('poses', poses, n_img, 3, 4)
    if n_img < 1:
        raise ValueError('pose_grad: at least one image')
    _need_pix(pix)
    n = pix.shape[0]
    _need_f32('d_rays', d_rays, n, 11)
    if d_poses is None:
        d_poses = torch.empty(n_img, 3, 4, device=poses.device, dtype=torch.float32)
    _need_f32('d_poses', d_poses, n_img, 3, 4)
    need = pose_grad_ws_floats(n, n_img)
    if ws is None and need > 0:
        ws = torch.empty(need, device=poses.device, dtype=torch.float32)
    assert need == 0 or (ws.dtype == torch.float32 and ws.numel() >= need)
    check(lib().fastnerf_pose_grad(n, n_img, ptr(pix), ptr(poses), float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]),
                                   ptr(d_rays), ptr(ws), ptr(d_poses), stream()), 'fastnerf_pose_grad')
    return d_poses


# ---- exposure table (csrc/exposure.hip; include/fastnerf.h, "exposure table") ---------------------
def _need_img(img, n):
    """Refuse an image list that the exposure kernels would not read as int32 [n] (no value is read here: a row outside the table is
    defined behaviour, the ray is left untouched)."""
    if img.dtype != torch.int32:
        raise TypeError(f'img must be int32, got {img.dtype}')
    if tuple(img.shape) != (n,):
        raise ValueError(f'img must have shape {(n,)}, got {tuple(img.shape)}')


def _need_ab(ab):
    if ab.dim() != 2 or ab.shape[0] < 1:
        raise ValueError(f'ab must have shape (n_img >= 1, 2), got {tuple(ab.shape)}')
    _need_f32('ab', ab, ab.shape[0], 2)
    return ab.shape[0]


def expo_apply(rgb, img, ab, rgb0=None, out=None, out0=None):
    """e [n,3] = (rgb - shift_i) / scale_i, i = img[r], scale_i = |ab[i,0]| + 0.5, shift_i = ab[i,1] (fastnerf_expo_apply): the colours
    the loss sees.  rgb0: the coarse pass's map of a two-pass render.  A ray whose img is outside the table keeps rgb's bits.
    out / out0: [n,3] buffers to write instead of new ones.  -> (e, e0 or None)"""
    require_gpu(rgb, img, ab, rgb0, out, out0)
    n_img, n = _need_ab(ab), rgb.shape[0]
    _need_f32('rgb', rgb, n, 3)
    _need_img(img, n)
    if rgb0 is not None:
        _need_f32('rgb0', rgb0, n, 3)
    e = torch.empty_like(rgb, memory_format=torch.contiguous_format) if out is None else out
    e0 = None if rgb0 is None else (torch.empty_like(e) if out0 is None else out0)
    for name, t in (('out', e), ('out0', e0)):
        if t is not None:
            _need_f32(name, t, n, 3)
    check(lib().fastnerf_expo_apply(n, n_img, ptr(img), ptr(ab), ptr(rgb), ptr(rgb0), ptr(e), ptr(e0), stream()), 'fastnerf_expo_apply')
    return e, e0


def expo_grad_ws_floats(n, n_img):
    """Floats of scratch one expo_grad call over n rays of n_img images needs."""
    return int(check(lib().fastnerf_expo_grad_ws_floats(int(n), int(n_img)), 'fastnerf_expo_grad_ws_floats'))


def expo_grad(img, ab, lam, grad_scale, e, g, e0=None, g0=None, d_ab=None, counts=None, ws=None, loss_reg=None):
    """The backward of expo_apply under a loss whose gradient with respect to e / e0 is g / g0 [n,3] (fastnerf_expo_grad): g and g0 are
    divided by their ray's scale IN PLACE (they become the gradient with respect to rgb / rgb0), and
    -> (d_ab [n_img,2], counts [n_img] int32 = rays per image, loss_reg [1] = the batch mean of |scale - 1| + |shift|), d_ab with the
    gradient of lam * grad_scale * loss_reg in it.  A segmented sum without atomics; an image without a ray gets an exact zero row.
    d_ab / counts / ws / loss_reg: buffers to use instead of new ones."""
    require_gpu(img, ab, e, g, e0, g0, d_ab, counts, ws, loss_reg)
    n_img, n = _need_ab(ab), g.shape[0]
    _need_img(img, n)
    for name, t in (('e', e), ('g', g), ('e0', e0), ('g0', g0)):
        if t is not None:
            _need_f32(name, t, n, 3)
    if (e0 is None) != (g0 is None):
        raise ValueError('expo_grad: e0 and g0 go together')
    if not (0. <= float(lam) < float('inf')):
        raise ValueError(f'expo_grad: lam is a finite weight >= 0, not {lam!r}')
    dev = ab.device
    if d_ab is None:
        d_ab = torch.empty(n_img, 2, device=dev, dtype=torch.float32)
    _need_f32('d_ab', d_ab, n_img, 2)
    if counts is None:
        counts = torch.empty(n_img, device=dev, dtype=torch.int32)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (n_img,)
    need = expo_grad_ws_floats(n, n_img)
    if ws is None and need > 0:
        ws = torch.empty(need, device=dev, dtype=torch.float32)
    assert need == 0 or (ws.dtype == torch.float32 and ws.numel() >= need)
    if loss_reg is None:
        loss_reg = torch.empty(1, device=dev, dtype=torch.float32)
    _need_f32('loss_reg', loss_reg, 1)
    check(lib().fastnerf_expo_grad(n, n_img, ptr(img), ptr(ab), float(lam), float(grad_scale), ptr(e), ptr(e0), ptr(g), ptr(g0), ptr(ws),
                                   ptr(d_ab), ptr(counts), ptr(loss_reg), stream()), 'fastnerf_expo_grad')
    return d_ab, counts, loss_reg


# ---- environment map (csrc/envmap.hip; include/fastnerf.h, "environment map") ---------------------
def _need_table(table):
    """Refuse a table that the kernels would not read as fp32 [R,R,3], R >= 2 -> R."""
    if table.dim() != 3 or table.shape[0] != table.shape[1] or table.shape[0] < 2:
        raise ValueError(f'table must have shape (R, R, 3) with R >= 2, got {tuple(table.shape)}')
    _need_f32('table', table, table.shape[0], table.shape[0], 3)
    return table.shape[0]


def _need_dirs(dirs):
    """Refuse directions that the kernels would not read as fp32 rows of three at a fixed stride -> (n, stride): a contiguous [n,3], or a
    column view such as rays[:, 3:6] of a contiguous batch, which is read in place."""
    if dirs.dtype != torch.float32:
        raise TypeError(f'dirs must be float32, got {dirs.dtype}')
    if dirs.dim() != 2 or dirs.shape[1] != 3:
        raise ValueError(f'dirs must have shape (n, 3), got {tuple(dirs.shape)}')
    n = dirs.shape[0]
    if n <= 1 and dirs.stride(1) == 1:
        return n, 3      # (a single row: its stride is never used)
    if dirs.stride(1) != 1 or dirs.stride(0) < 3:
        raise ValueError(f'dirs must be rows of three contiguous floats, got strides {tuple(dirs.stride())}')
    return n, dirs.stride(0)


def env_lookup(table, dirs, out=None):
    """The environment map's colours [n,3] for directions dirs [n,3] of any length (fastnerf_env_lookup): the bilinear sample of the
    octahedral table [R,R,3] with the mirror wrap at its border.  dirs may be a column view of a ray batch (rays[:, 3:6]).
    out: an [n,3] buffer to write instead of a new one."""
    require_gpu(table, dirs, out)
    R = _need_table(table)
    n, stride = _need_dirs(dirs)
    if out is None:
        out = torch.empty(n, 3, device=table.device, dtype=torch.float32)
    _need_f32('out', out, n, 3)
    check(lib().fastnerf_env_lookup(n, dirs.data_ptr() if n else None, stride, ptr(table), R, ptr(out), stream()), 'fastnerf_env_lookup')
    return out


def env_grad_ws_bytes(R):
    """Bytes of scratch one env_grad call on an [R,R,3] table needs."""
    return int(check(lib().fastnerf_env_grad_ws_bytes(int(R)), 'fastnerf_env_grad_ws_bytes'))


def env_grad(R, dirs, g_rgb, acc, g_rgb0=None, acc0=None, d_table=None, ws=None):
    """d_table [R,R,3]: what rgb += (1 - acc) env(dirs) (and the same for rgb0 / acc0 of a two-pass render) sends back to the table
    under colour gradients g_rgb / g_rgb0 [n,3] (fastnerf_env_grad).  A scatter in 64-bit fixed point: the same bits whatever the order
    of the rays.  d_table / ws (int64, R*R*3 words): buffers to use instead of new ones."""
    require_gpu(dirs, g_rgb, acc, g_rgb0, acc0, d_table, ws)
    R = int(R)
    if R < 2:
        raise ValueError(f'env_grad: R >= 2, got {R}')
    n, stride = _need_dirs(dirs)
    _need_f32('g_rgb', g_rgb, n, 3)
    _need_f32('acc', acc, n)
    if (g_rgb0 is None) != (acc0 is None):
        raise ValueError('env_grad: g_rgb0 and acc0 go together')
    if g_rgb0 is not None:
        _need_f32('g_rgb0', g_rgb0, n, 3)
        _need_f32('acc0', acc0, n)
    dev = g_rgb.device
    if d_table is None:
        d_table = torch.empty(R, R, 3, device=dev, dtype=torch.float32)
    _need_f32('d_table', d_table, R, R, 3)
    if ws is None:
        ws = torch.empty(R * R * 3, device=dev, dtype=torch.int64)
    if ws.dtype != torch.int64 or not ws.is_contiguous() or ws.numel() * 8 < env_grad_ws_bytes(R):
        raise ValueError(f'env_grad: ws must be contiguous int64 with at least {R * R * 3} words')
    check(lib().fastnerf_env_grad(n, dirs.data_ptr() if n else None, stride, R, ptr(g_rgb), ptr(acc), ptr(g_rgb0), ptr(acc0), ptr(ws),
                                  ptr(d_table), stream()), 'fastnerf_env_grad')
    return d_table


# ---- band weights (csrc/bands.hip; include/fastnerf.h, "band weights") ---------------------------
BAND_VIEW_COLS = 27


def band_pos_cols(kind=0):
    """Columns of the point encoding of a net of this kind: 63, or 84 for kind 2."""
    return 84 if int(kind) == 2 else 63


def _need_bands(kind, w_pos, w_view, *buffers):
    """Refuse, before any launch, what fastnerf_band_apply / _grad would misread: a kind outside 0..2, weights that are not contiguous
    fp32 [in_pe] / [27], net buffers that are not contiguous fp32 of the kind's size, tensors on different devices."""
    kind = int(kind)
    if kind not in (0, 1, 2):
        raise ValueError(f'kind must be 0, 1 or 2, got {kind}')
    require_gpu(w_pos, w_view, *buffers)
    _need_f32('w_pos', w_pos, band_pos_cols(kind))
    _need_f32('w_view', w_view, BAND_VIEW_COLS)
    n = net_floats(kind, 0)
    for name, t in zip(('the first net buffer', 'the second net buffer'), buffers):
        _need_f32(name, t, n)
    for name, t in (('w_pos', w_pos), ('w_view', w_view)) + tuple(zip(('the first net buffer', 'the second net buffer'), buffers)):
        if not t.is_contiguous():
            raise ValueError(f'{name} must be contiguous, got strides {tuple(t.stride())}')
        if t.device != buffers[0].device:
            raise ValueError(f'{name} is on {t.device}, the net on {buffers[0].device}')
    return kind


def band_apply(w_pos, w_view, master, effective=None, kind=0):
    """effective (a new buffer when None) = the network whose encoding columns are the master's times the band weights
    (fastnerf_band_apply): LW[0][:, :in_pe] and LW[5][:, :in_pe] times w_pos [in_pe], VW[:, 256:283] times w_view [27], every other
    float copied bit for bit.  master and effective: flat fp32 nets of layout `kind`, two buffers."""
    if effective is None:
        effective = torch.empty_like(master)
    kind = _need_bands(kind, w_pos, w_view, master, effective)
    if master.data_ptr() == effective.data_ptr():
        raise ValueError('band_apply: master and effective must be two buffers')
    check(lib().fastnerf_band_apply(kind, ptr(w_pos), ptr(w_view), ptr(master), ptr(effective), stream()), 'fastnerf_band_apply')
    return effective


def band_grad(w_pos, w_view, grads, kind=0):
    """In place: the encoding columns of a flat gradient buffer of the effective network times the band weights, which makes it the
    master's gradient (fastnerf_band_grad).  No other float is touched."""
    kind = _need_bands(kind, w_pos, w_view, grads)
    check(lib().fastnerf_band_grad(kind, ptr(w_pos), ptr(w_view), ptr(grads), stream()), 'fastnerf_band_grad')
    return grads


def raw2outputs_fwd(raw, z, rays11, noise=None, white_bkgd=False):
    require_gpu(raw, z, rays11, noise)
    n = rays11.shape[0]
    _need_f32('rays11', rays11, n, 11)
    S = z.shape[-1]
    _need_f32('z', z, n, S)
    _need_f32('raw', raw, n, S, 4)
    dev = z.device
    rgb = torch.empty(n, 3, device=dev, dtype=torch.float32)
    disp = torch.empty(n, device=dev, dtype=torch.float32)
    acc = torch.empty(n, device=dev, dtype=torch.float32)
    weights = torch.empty(n, S, device=dev, dtype=torch.float32)
    depth = torch.empty(n, device=dev, dtype=torch.float32)
    check(lib().fastnerf_raw2outputs_fwd(n, S, ptr(raw), ptr(z), ptr(rays11), ptr(noise), int(bool(white_bkgd)),
                                         ptr(rgb), ptr(disp), ptr(acc), ptr(weights), ptr(depth), stream()),
          'fastnerf_raw2outputs_fwd')
    return rgb, disp, acc, weights, depth


def _rr_fwd_outputs(rays11, packed_c, packed_f, N_samples, N_importance, t_rand, u, act_buf=lambda k, P: None):
    """What render_rays_fwd and render_rays_fwd_occ do before their call: the packed-weight and random-draw checks, and the dict of
    output tensors (act0 / act1 from act_buf(pass, points)).  Returns (outputs, t_rand, u)."""
    n = rays11.shape[0]
    f32 = dict(device=rays11.device, dtype=torch.float32)
    assert packed_tag(packed_c) == _MATH and (packed_f is None or packed_tag(packed_f) == _MATH), \
        'packed weights were not produced by mlp_pack under the current math mode'
    if t_rand is not None:
        t_rand = _f32(t_rand)
        assert t_rand.shape == (n, N_samples)
    if u is not None:
        u = _f32(u)
        assert u.shape == (n, N_importance)
    o = {'z0': torch.empty(n, N_samples, **f32), 'raw0': torch.empty(n, N_samples, 4, **f32),
         'act0': act_buf(0, n * N_samples),
         'rgb0': torch.empty(n, 3, **f32), 'disp0': torch.empty(n, **f32), 'acc0': torch.empty(n, **f32),
         'w0': torch.empty(n, N_samples, **f32), 'depth0': torch.empty(n, **f32)}
    S1 = N_samples + N_importance
    if N_importance > 0:
        o.update({'z1': torch.empty(n, S1, **f32), 'z_samples': torch.empty(n, N_importance, **f32), 'z_std': torch.empty(n, **f32),
                  'raw1': torch.empty(n, S1, 4, **f32), 'act1': act_buf(1, n * S1),
                  'rgb1': torch.empty(n, 3, **f32), 'disp1': torch.empty(n, **f32), 'acc1': torch.empty(n, **f32),
                  'w1': torch.empty(n, S1, **f32), 'depth1': torch.empty(n, **f32)})
    return o, t_rand, u


def _rr_fwd_ptrs(o, rays11, params_c, packed_c, params_f, packed_f, N_samples, N_importance, lindisp, perturb, det, white_bkgd, t_rand,
                 u, seed0, seed1, with_act):
    """The arguments the forward entry points have in common, in their order: (mode .. u, seed0 .. packed_f, the outputs); the
    plain entry point has noise0 / noise1 between the first two and takes act0 / act1 among the outputs (with_act)."""
    head = [mode_id(), rays11.shape[0], int(N_samples), int(N_importance), ptr(rays11), int(bool(lindisp)),
            int(bool(perturb) or t_rand is not None), int(bool(det)), int(bool(white_bkgd)), ptr(t_rand), ptr(u)]
    nets = [int(seed0), int(seed1), ptr(params_c), ptr(packed_c), ptr(params_f), ptr(packed_f)]
    keys = ['z0', 'raw0', 'act0', 'rgb0', 'disp0', 'acc0', 'w0', 'depth0', 'z1', 'z_samples', 'z_std', 'raw1', 'act1', 'rgb1', 'disp1',
            'acc1', 'w1', 'depth1']
    return head, nets, [ptr(o.get(k)) for k in keys if with_act or not k.startswith('act')]


def render_rays_fwd(rays11, params_c, packed_c, params_f, packed_f, N_samples, N_importance, lindisp=False, perturb=False,
                    det=True, white_bkgd=False, t_rand=None, u=None, noise0=None, noise1=None, seed0=0, seed1=0, save=False, skip_dead_rgb=False, act_bufs=None):
    """One C-ABI call for the whole forward of render_rays (render.py:238-299).  Returns a dict of the tensors the
    step-by-step ops would have produced (same kernels, same results).  params_f / packed_f may be None when
    N_importance == 0."""
    require_gpu(rays11, params_c, packed_c, params_f, packed_f, t_rand, u, noise0, noise1)
    dev = rays11.device
    # act_bufs = (buffer for the coarse pass, buffer for the fine pass): caller-owned scratch for the saved activations (11 GB at
    # the bench size) instead of fresh allocations -- for callers whose backward follows before the next forward
    def act_buf(k, P):
        if not save:
            return None
        count = act_floats(P)
        if act_bufs is not None and act_bufs[k] is not None:
            assert act_bufs[k].numel() >= count and act_bufs[k].dtype == torch.float32 and act_bufs[k].device == dev
            return act_bufs[k]
        return torch.empty(count, device=dev, dtype=torch.float32)
    o, t_rand, u = _rr_fwd_outputs(rays11, packed_c, packed_f, N_samples, N_importance, t_rand, u, act_buf)
    head, nets, outs = _rr_fwd_ptrs(o, rays11, params_c, packed_c, params_f, packed_f, N_samples, N_importance, lindisp, perturb, det,
                                    white_bkgd, t_rand, u, seed0, seed1, with_act=True)
    # skip_dead_rgb (FN_FWD_SKIP_DEAD_RGB): the inference launches may leave the colour logits of tiles without a live sample at
    # zero -- every other output is bit-identical; only callers that never expose `raw0` / `raw1` ask for it
    check(lib().fastnerf_render_rays_fwd_ex(*head, ptr(noise0), ptr(noise1), *nets, *outs, 1 if skip_dead_rgb else 0, stream()),
          'fastnerf_render_rays_fwd_ex')
    return o


MAP_GRAD_KEYS = ('g_disp1', 'g_acc1', 'g_depth1', 'g_disp0', 'g_acc0', 'g_depth0')


def _map_grads(map_grads, n):
    """map_grads of render_rays_bwd / _bwd_live -> (None, []) when no map gradient is set (the plain entry point is called, as
    ever), else ([acc0, depth0, acc1, depth1 pointers, byref(fn_map_grads)], tensors to keep alive over the call)."""
    if not map_grads or all(map_grads.get(k) is None for k in MAP_GRAD_KEYS):
        return None, []
    unknown = set(map_grads) - set(MAP_GRAD_KEYS) - {'acc0', 'depth0', 'acc1', 'depth1'}
    assert not unknown, unknown
    keep = {k: (None if map_grads.get(k) is None else _f32(map_grads[k]))
            for k in MAP_GRAD_KEYS + ('acc0', 'depth0', 'acc1', 'depth1')}
    require_gpu(*keep.values())
    for k, t in keep.items():
        assert t is None or t.numel() == n, (k, tuple(t.shape))
    mg = _lib.MapGrads(**{k: ptr(keep[k]) for k in MAP_GRAD_KEYS})
    return [ptr(keep['acc0']), ptr(keep['depth0']), ptr(keep['acc1']), ptr(keep['depth1']), ctypes.byref(mg)], [keep, mg]


def _weight_grads(weight_grads, n, N_samples, N_importance):
    """weight_grads of render_rays_bwd / _bwd_live -> (None, []) when no weight gradient is set, else (byref(fn_weight_grads), tensors to
    keep alive over the call).  'g_w1': the image pass's [n, N_samples + N_importance] ([n, N_samples] with one pass), 'g_w0': the coarse
    pass's of two [n, N_samples]."""
    if not weight_grads or all(weight_grads.get(k) is None for k in ('g_w1', 'g_w0')):
        return None, []
    assert not set(weight_grads) - {'g_w1', 'g_w0'}, set(weight_grads)
    keep = {k: (None if weight_grads.get(k) is None else _f32(weight_grads[k])) for k in ('g_w1', 'g_w0')}
    require_gpu(*keep.values())
    assert keep['g_w1'] is None or tuple(keep['g_w1'].shape) == (n, N_samples + N_importance), tuple(keep['g_w1'].shape)
    assert keep['g_w0'] is None or (N_importance > 0 and tuple(keep['g_w0'].shape) == (n, N_samples)), tuple(keep['g_w0'].shape)
    wg = _lib.WeightGrads(ptr(keep['g_w1']), ptr(keep['g_w0']))
    return ctypes.byref(wg), [keep, wg]


def render_rays_bwd(rays11, white_bkgd, g_rgb, g_rgb0, noise0, noise1, z0, raw0, act0, z1, raw1, act1, params_c, packed_bwd_c,
                    params_f, packed_bwd_f, draw_ws, dact_ws, partial, grads_c, grads_f, N_samples, N_importance, map_grads=None,
                    weight_grads=None):
    """One C-ABI call for the backward of render_rays w.r.t. the parameters of the (distinct) coarse / fine nets.
    map_grads: None, or a dict with d(loss)/d(disp, acc, depth) of the fine (1) and coarse (0) pass under MAP_GRAD_KEYS ([n] each,
    absent / None = zero; one pass: the *1 keys) and the forward's 'acc0', 'depth0', 'acc1', 'depth1' (needed for a g_disp*):
    fastnerf_render_rays_bwd_maps.  A pass with a map gradient may have g_rgb / g_rgb0 None.
    weight_grads: None, or a dict with d(loss)/d(weights) under 'g_w1' / 'g_w0' (_weight_grads): fastnerf_render_rays_bwd_w."""
    require_gpu(rays11, g_rgb, g_rgb0, z0, raw0, act0, z1, raw1, act1, params_c, packed_bwd_c, params_f, packed_bwd_f, draw_ws,
                dact_ws, partial, grads_c, grads_f)
    n = rays11.shape[0]
    S1 = N_samples + N_importance
    tag = _MATH
    assert packed_tag(packed_bwd_c) == tag and (packed_bwd_f is None or packed_tag(packed_bwd_f) == tag), \
        'packed weights were not produced by mlp_pack under the current math mode'
    assert draw_ws.numel() >= n * S1 * 4 and dact_ws.numel() >= dact_floats(n * S1)
    args = [mode_id(), n, int(N_samples), int(N_importance), ptr(rays11), int(bool(white_bkgd)), ptr(g_rgb), ptr(g_rgb0),
            ptr(noise0), ptr(noise1), ptr(z0), ptr(raw0), ptr(act0), ptr(z1), ptr(raw1), ptr(act1), ptr(params_c), ptr(packed_bwd_c),
            ptr(params_f), ptr(packed_bwd_f), ptr(draw_ws), ptr(dact_ws), ptr(partial), ptr(grads_c), ptr(grads_f)]
    maps, _keep = _map_grads(map_grads, n)
    wg, _keep_w = _weight_grads(weight_grads, n, int(N_samples), int(N_importance))
    if wg is not None:
        check(lib().fastnerf_render_rays_bwd_w(*args, *(maps or [None] * 5), wg, stream()), 'fastnerf_render_rays_bwd_w')
    elif maps is None:
        check(lib().fastnerf_render_rays_bwd(*args, stream()), 'fastnerf_render_rays_bwd')
    else:
        check(lib().fastnerf_render_rays_bwd_maps(*args, *maps, stream()), 'fastnerf_render_rays_bwd_maps')


def compact_live(draw):
    """Indices (ascending, int32) of the points whose d(loss)/d(raw) is not exactly zero, and the [live, total] counts --
    both stay on the device.  draw: [n, S, 4] or [P, 4]."""
    require_gpu(draw)
    P = draw.numel() // 4
    idx = torch.empty(P, device=draw.device, dtype=torch.int32)
    cnt = torch.empty(2, device=draw.device, dtype=torch.int32)
    ws = torch.empty(int(lib().fastnerf_compact_ws_ints(P)), device=draw.device, dtype=torch.int32)
    check(lib().fastnerf_compact_live(P, ptr(_f32(draw)), ptr(idx), ptr(cnt), ptr(ws), stream()), 'fastnerf_compact_live')
    return idx, cnt


def mlp_fwd_live(rays11, z, params, packed_fwd, act, live_idx, live_cnt, kind=0):
    """Training forward over a live list: saves the activations of points live_idx[0:live_cnt[0]] (current math mode)."""
    require_gpu(rays11, z, params, packed_fwd, act, live_idx, live_cnt)
    n, S = z.shape
    tag = _MATH
    assert act.numel() >= act_floats(n * S, kind) and live_idx.dtype == torch.int32 and live_cnt.dtype == torch.int32
    assert packed_fwd.numel() == packed_floats(kind, 1) and packed_tag(packed_fwd) == tag
    fn, name = _mlp('fwd_live', kind)
    check(fn(int(kind), n, S, ptr(rays11), ptr(z), ptr(params), ptr(packed_fwd), ptr(act), ptr(live_idx), ptr(live_cnt), stream()), name)


def mlp_bwd_live(draw, act, params, packed_bwd, dact, partial, grads, live_idx, live_cnt, kind=0):
    require_gpu(draw, act, params, packed_bwd, dact, partial, grads, live_idx, live_cnt)
    n, S = draw.shape[0], draw.shape[1]
    tag = _MATH
    assert dact.numel() >= dact_floats(n * S, kind) and grads.numel() == net_floats(kind, 0)
    assert packed_bwd.numel() == packed_floats(kind, 2) and packed_tag(packed_bwd) == tag
    fn, name = _mlp('bwd_live', kind)
    check(fn(int(kind), n, S, ptr(draw), ptr(act), ptr(params), ptr(packed_bwd), ptr(dact), ptr(partial), ptr(grads), ptr(live_idx),
             ptr(live_cnt), stream()), name)
    return grads


def live_ws_ints(P):
    return 4 + int(P) + int(lib().fastnerf_compact_ws_ints(int(P)))


def render_rays_bwd_live(rays11, white_bkgd, g_rgb, g_rgb0, noise0, noise1, z0, raw0, z1, raw1, params_c, packed_c,
                         params_f, packed_f, draw_ws, act_ws, dact_ws, partial, live_ws, grads_c, grads_f, N_samples,
                         N_importance, counts=None, map_grads=None, weight_grads=None):
    """One C-ABI call: backward of render_rays with exact zero-gradient point compaction, for a forward that saved
    nothing.  packed_c / packed_f: the (forward, backward) packed-weight pairs.  counts: optional int32[4] device
    tensor receiving (live, total) of the fine and of the coarse pass.  map_grads, weight_grads: as render_rays_bwd
    (fastnerf_render_rays_bwd_live_maps, fastnerf_render_rays_bwd_live_w)."""
    require_gpu(rays11, g_rgb, g_rgb0, z0, raw0, z1, raw1, params_c, params_f, draw_ws, act_ws, dact_ws, partial, live_ws,
                grads_c, grads_f, counts)
    n = rays11.shape[0]
    S1 = N_samples + N_importance
    tag = _MATH
    for pk in (packed_c, packed_f):
        assert pk is None or all(packed_tag(t) == tag for t in pk)
    assert draw_ws.numel() >= n * S1 * 4 and dact_ws.numel() >= dact_floats(n * S1) and act_ws.numel() >= act_floats(n * S1)
    assert live_ws.dtype == torch.int32 and live_ws.numel() >= live_ws_ints(n * S1)
    args = [mode_id(), n, int(N_samples), int(N_importance), ptr(rays11), int(bool(white_bkgd)), ptr(g_rgb), ptr(g_rgb0), ptr(noise0),
            ptr(noise1), ptr(z0), ptr(raw0), ptr(z1), ptr(raw1), ptr(params_c), ptr(packed_c[0]), ptr(packed_c[1]),
            ptr(params_f), ptr(None if packed_f is None else packed_f[0]), ptr(None if packed_f is None else packed_f[1]),
            ptr(draw_ws), ptr(act_ws), ptr(dact_ws), ptr(partial), ptr(live_ws), ptr(grads_c), ptr(grads_f), ptr(counts)]
    maps, _keep = _map_grads(map_grads, n)
    wg, _keep_w = _weight_grads(weight_grads, n, int(N_samples), int(N_importance))
    if wg is not None:
        check(lib().fastnerf_render_rays_bwd_live_w(*args, *(maps or [None] * 5), wg, stream()), 'fastnerf_render_rays_bwd_live_w')
    elif maps is None:
        check(lib().fastnerf_render_rays_bwd_live(*args, stream()), 'fastnerf_render_rays_bwd_live')
    else:
        check(lib().fastnerf_render_rays_bwd_live_maps(*args, *maps, stream()), 'fastnerf_render_rays_bwd_live_maps')


def raw2outputs_bwd(raw, z, rays11, g_rgb, noise=None, white_bkgd=False, draw=None):
    require_gpu(raw, z, rays11, g_rgb, noise)
    n, S = z.shape
    if draw is None:
        draw = torch.empty(n, S, 4, device=z.device, dtype=torch.float32)
    check(lib().fastnerf_raw2outputs_bwd(n, S, ptr(raw), ptr(z), ptr(rays11), ptr(noise), int(bool(white_bkgd)),
                                         ptr(_f32(g_rgb)), ptr(draw), stream()), 'fastnerf_raw2outputs_bwd')
    return draw


def raw2outputs_bwd_full(raw, z, rays11, acc, depth, g_rgb=None, g_disp=None, g_acc=None, g_w=None, g_depth=None, noise=None,
                         white_bkgd=False, draw=None):
    """d(rgb, disp, acc, weights, depth)/d(raw) [n,S,4] (render.py:149-192).  acc / depth: the forward's outputs; every upstream
    gradient may be None (= zero).  With only g_rgb, bit-identical to raw2outputs_bwd."""
    require_gpu(raw, z, rays11, acc, depth, g_rgb, g_disp, g_acc, g_w, g_depth, noise)
    n, S = z.shape
    if draw is None:
        draw = torch.empty(n, S, 4, device=z.device, dtype=torch.float32)
    g = [None if t is None else _f32(t) for t in (g_rgb, g_disp, g_acc, g_w, g_depth)]
    for t, shp in zip(g, ((n, 3), (n,), (n,), (n, S), (n,))):
        assert t is None or tuple(t.shape) == shp, (tuple(t.shape), shp)
    check(lib().fastnerf_raw2outputs_bwd_full(n, S, ptr(raw), ptr(z), ptr(rays11), ptr(noise), int(bool(white_bkgd)),
                                              ptr(None if acc is None else _f32(acc)), ptr(None if depth is None else _f32(depth)),
                                              *[ptr(t) for t in g], ptr(draw), stream()), 'fastnerf_raw2outputs_bwd_full')
    return draw


def sample_pdf_merge(z, weights, Ni, det=False, u=None, seed=0, want_samples=True):
    require_gpu(z, weights, u)
    n, S = z.shape
    dev = z.device
    z_out = torch.empty(n, S + Ni, device=dev, dtype=torch.float32)
    z_samples = torch.empty(n, Ni, device=dev, dtype=torch.float32) if want_samples else None
    z_std = torch.empty(n, device=dev, dtype=torch.float32)
    if u is not None:
        u = _f32(u)
        assert u.shape == (n, Ni)
    check(lib().fastnerf_sample_pdf_merge(n, S, Ni, ptr(z), ptr(weights), int(bool(det)), ptr(u), int(seed),
                                          ptr(z_out), ptr(z_samples), ptr(z_std), stream()),
          'fastnerf_sample_pdf_merge')
    return z_out, z_samples, z_std


def sample_pdf(bins, weights, Ni, det=False, u=None, seed=0):
    require_gpu(bins, weights, u)
    n, M = bins.shape
    out = torch.empty(n, Ni, device=bins.device, dtype=torch.float32)
    if u is not None:
        u = _f32(u)
    bins, weights = _f32(bins), _f32(weights)
    check(lib().fastnerf_sample_pdf(n, M, Ni, ptr(bins), ptr(weights), int(bool(det)), ptr(u), int(seed),
                                    ptr(out), stream()), 'fastnerf_sample_pdf')
    return out


def leaf_table_reset(table):
    """Zero the per-(image, leaf) error table on the device (fastnerf_leaf_table_reset)."""
    require_gpu(table)
    assert table.dtype == torch.int32 and table.is_contiguous()
    check(lib().fastnerf_leaf_table_reset(ptr(table), table.numel(), stream()), 'fastnerf_leaf_table_reset')
    return table


def leaf_table_read(table):
    """The table as host floats (max |gt - pred| per leaf), waited for: what the split rule of tree.py:629-652 consumes."""
    require_gpu(table)
    assert table.dtype == torch.int32 and table.is_contiguous()
    out = torch.empty(table.shape, dtype=torch.float32)
    check(lib().fastnerf_leaf_table_read(ptr(table), out.data_ptr(), table.numel(), stream()), 'fastnerf_leaf_table_read')
    return out


def mse_leafmax(rgb, rgb0, target, grad_scale=1.0, want_grads=True, leaf_tag=None, max_leaves=0, table=None):
    require_gpu(rgb, rgb0, target, leaf_tag, table)
    rgb, target = _f32(rgb), _f32(target)
    rgb0 = None if rgb0 is None else _f32(rgb0)
    leaf_tag = None if leaf_tag is None else leaf_tag.contiguous()
    n = rgb.shape[0]
    dev = rgb.device
    g = torch.empty(n, 3, device=dev, dtype=torch.float32) if want_grads else None
    g0 = torch.empty(n, 3, device=dev, dtype=torch.float32) if (want_grads and rgb0 is not None) else None
    loss2 = torch.empty(2, device=dev, dtype=torch.float32)
    check(lib().fastnerf_mse_leafmax(n, ptr(rgb), ptr(rgb0), ptr(target), float(grad_scale), ptr(g), ptr(g0),
                                     ptr(loss2), ptr(leaf_tag), int(max_leaves), ptr(table), stream()),
          'fastnerf_mse_leafmax')
    return loss2, g, g0


def aux_loss(depth, acc, depth0=None, acc0=None, depth_target=None, depth_weight=None, acc_target=None, acc_weight=None,
             lambda_depth=0., lambda_acc=0., grad_scale=1.0, want_grads=True):
    """Depth / opacity losses of the maps of one render (fastnerf_aux_loss): depth / acc are the image pass's maps, depth0 / acc0
    the coarse pass's of a two-pass render (None with one pass).  Returns (loss4, grads): loss4 = (Ld_fine, Ld_coarse, La_fine,
    La_coarse) on the device, unscaled by the lambdas; grads = dict g_depth1, g_acc1, g_depth0, g_acc0 ([n] each; None for a term
    whose target is None, for the coarse pass with one pass, and with want_grads=False) = grad_scale lambda 2 w (map - target) / n.
    Weights None = ones; a ray with weight 0 contributes exactly 0 and gets +0 whatever its target holds."""
    t = {k: (None if v is None else _f32(v).reshape(-1)) for k, v in dict(
        depth1=depth, acc1=acc, depth0=depth0, acc0=acc0, dt=depth_target, dw=depth_weight, at=acc_target, aw=acc_weight).items()}
    assert t['depth1'] is not None or t['acc1'] is not None, 'aux_loss needs the depth map or the opacity map'
    require_gpu(*t.values())
    ref = t['depth1'] if t['depth1'] is not None else t['acc1']
    n, dev = ref.numel(), ref.device
    for k, v in t.items():
        assert v is None or v.numel() == n, (k, v.numel(), n)
    assert t['dt'] is None or t['depth1'] is not None, 'a depth target needs the depth map'
    assert t['at'] is None or t['acc1'] is not None, 'an opacity target needs the opacity map'
    new = lambda on: torch.empty(n, device=dev, dtype=torch.float32) if (want_grads and on) else None      # noqa: E731
    g = {'g_depth1': new(t['dt'] is not None), 'g_acc1': new(t['at'] is not None),
         'g_depth0': new(t['dt'] is not None and t['depth0'] is not None), 'g_acc0': new(t['at'] is not None and t['acc0'] is not None)}
    loss4 = torch.empty(4, device=dev, dtype=torch.float32)
    check(lib().fastnerf_aux_loss(n, ptr(t['depth1']), ptr(t['acc1']), ptr(t['depth0']), ptr(t['acc0']), ptr(t['dt']), ptr(t['dw']),
                                  ptr(t['at']), ptr(t['aw']), float(lambda_depth), float(lambda_acc), float(grad_scale),
                                  ptr(g['g_depth1']), ptr(g['g_acc1']), ptr(g['g_depth0']), ptr(g['g_acc0']), ptr(loss4), stream()),
          'fastnerf_aux_loss')
    return loss4, g


def distortion(w, z, rays11, lindisp=False, skip=None, coef=1.0, g_up=None, want=('ell', 'g_w')):
    """The distortion loss of the weights of every ray and its gradient in them (fastnerf_distortion; include/fastnerf.h has the
    definition).  w, z [n,S] (1 <= S <= 512), near / far = columns 6 / 7 of rays11.  skip: [n] bytes (uint8 or bool), a non-zero one gives
    its ray l = 0 and a zero row.  -> (ell [n] or None, g_w [n,S] or None) as `want` names them; g_w = coef * (g_up[r] or 1) * dl_r/dw_i."""
    require_gpu(w, z, rays11, skip, g_up)
    w, z, rays11 = _f32(w), _f32(z), _f32(rays11)
    n, S = z.shape
    assert tuple(w.shape) == (n, S) and tuple(rays11.shape) == (n, 11), (tuple(w.shape), tuple(z.shape), tuple(rays11.shape))
    assert want and not set(want) - {'ell', 'g_w'}, want
    if skip is not None:
        skip = skip.to(torch.uint8).contiguous()
        assert skip.numel() == n
    if g_up is not None:
        g_up = _f32(g_up).reshape(-1)
        assert g_up.numel() == n
    ell = torch.empty(n, device=z.device, dtype=torch.float32) if 'ell' in want else None
    g_w = torch.empty(n, S, device=z.device, dtype=torch.float32) if 'g_w' in want else None
    check(lib().fastnerf_distortion(n, S, ptr(w), ptr(z), ptr(rays11), int(bool(lindisp)), ptr(skip), float(coef), ptr(g_up), ptr(ell),
                                    ptr(g_w), stream()), 'fastnerf_distortion')
    return ell, g_w


def distortion_mean(ell1, ell0=None):
    """The batch means of the per-ray distortion losses of the image pass and, when given, the coarse pass (fastnerf_distortion_mean):
    -> loss2d [2] on the device (the second 0 without ell0); one workgroup, fixed order, fp64: bit-identical from call to call."""
    require_gpu(ell1, ell0)
    ell1 = _f32(ell1).reshape(-1)
    ell0 = None if ell0 is None else _f32(ell0).reshape(-1)
    assert ell0 is None or ell0.numel() == ell1.numel()
    loss2d = torch.empty(2, device=ell1.device, dtype=torch.float32)
    check(lib().fastnerf_distortion_mean(ell1.numel(), ptr(ell1), ptr(ell0), ptr(loss2d), stream()), 'fastnerf_distortion_mean')
    return loss2d


def bkgd_blend(rgb, acc, target, bkgd=None, seed=0, alpha=None, rgb0=None, acc0=None):
    """Per-ray background colours behind the colour maps of one render and behind its target (fastnerf_bkgd_blend).  rgb [n,3] / acc [n]
    are the image pass's maps composited with white_bkgd=False, rgb0 / acc0 the coarse pass's of a two-pass render; rgb and rgb0 are
    blended IN PLACE: rgb += (1 - acc) b.  bkgd: [n,3] injected colours, or None with seed != 0: drawn from the 'bkgd' stream.  alpha:
    [n] or None; the blended target is target * alpha + (1 - alpha) b, or the target's bits without an alpha.
    -> (target_out [n,3], bkgd_used [n,3])."""
    require_gpu(rgb, acc, target, bkgd, alpha, rgb0, acc0)
    n, dev = rgb.shape[0], rgb.device
    for t, shape in ((rgb, (n, 3)), (rgb0, (n, 3)), (acc, (n,)), (acc0, (n,))):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.shape == shape and t.device == dev), shape
    assert (rgb0 is None) == (acc0 is None), 'rgb0 and acc0 go together'
    target = _f32(target)
    bkgd = None if bkgd is None else _f32(bkgd)
    alpha = None if alpha is None else _f32(alpha).reshape(-1)
    assert target.shape == (n, 3) and (bkgd is None or bkgd.shape == (n, 3)) and (alpha is None or alpha.shape == (n,))
    target_out = torch.empty(n, 3, device=dev, dtype=torch.float32)
    used = torch.empty(n, 3, device=dev, dtype=torch.float32)
    check(lib().fastnerf_bkgd_blend(n, ptr(bkgd), int(seed), ptr(alpha), ptr(acc), ptr(acc0), ptr(rgb), ptr(rgb0), ptr(target),
                                    ptr(target_out), ptr(used), stream()), 'fastnerf_bkgd_blend')
    return target_out, used


def bkgd_grad(bkgd_used, g_rgb, g_rgb0=None, add=None, add0=None):
    """What bkgd_blend sends back to the opacity maps (fastnerf_bkgd_grad): g_acc[r] = (add[r] or 0) - (g_rgb[r] . bkgd_used[r]), [n], and
    the same for the coarse pass from g_rgb0 / add0.  add / add0: another term's d(loss)/d(acc) rows (the opacity term's), or None.
    -> (g_acc, g_acc0 or None): the rows that raw2outputs_bwd_full takes beside g_rgb (white_bkgd=False)."""
    require_gpu(bkgd_used, g_rgb, g_rgb0, add, add0)
    n, dev = g_rgb.shape[0], g_rgb.device
    t = [None if x is None else _f32(x) for x in (bkgd_used, g_rgb, g_rgb0, add, add0)]
    assert t[0].shape == (n, 3) and t[1].shape == (n, 3) and (t[2] is None or t[2].shape == (n, 3))
    assert (t[3] is None or t[3].shape == (n,)) and (t[4] is None or t[4].shape == (n,))
    g_acc = torch.empty(n, device=dev, dtype=torch.float32)
    g_acc0 = None if g_rgb0 is None else torch.empty(n, device=dev, dtype=torch.float32)
    check(lib().fastnerf_bkgd_grad(n, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), ptr(t[4]), ptr(g_acc), ptr(g_acc0), stream()),
          'fastnerf_bkgd_grad')
    return g_acc, g_acc0


def sigma_noise(n, S0, S1, std, seed, device):
    """(noise0 [n, S0], noise1 [n, S1] or None when S1 == 0): N(0, std^2) sigma noise of both passes of one render_rays call
    (render.py:162), one launch into one allocation (csrc/train.hip gauss_noise_kernel)."""
    tot0 = (n * S0 + 3) // 4 * 4          # (keeps the second view 16-byte aligned)
    buf = torch.empty(tot0 + n * S1, device=device, dtype=torch.float32)
    require_gpu(buf)
    check(lib().fastnerf_gauss_noise(buf.numel(), float(std), int(seed), ptr(buf), stream()), 'fastnerf_gauss_noise')
    return buf[:n * S0].view(n, S0), (buf[tot0:].view(n, S1) if S1 > 0 else None)


def adam_step(params, grads, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    require_gpu(params, grads, m, v)
    check(lib().fastnerf_adam_step(params.numel(), ptr(params), ptr(grads), ptr(m), ptr(v), float(lr), float(beta1),
                                   float(beta2), float(eps), int(step), stream()), 'fastnerf_adam_step')


# ---- nerf++-ours additions -------------------------------------------------------------------
def pp_intersect_sphere(rays11, check_inside=True):
    """ddp_train_nerf.py:54-69.  Raises (like the reference) when a camera is outside the unit sphere;
    check_inside=False skips the device->host read of the counter."""
    require_gpu(rays11)
    n = rays11.shape[0]
    _need_f32('rays11', rays11, n, 11)
    fg_far = torch.empty(n, device=rays11.device, dtype=torch.float32)
    cnt = torch.zeros(1, device=rays11.device, dtype=torch.int32) if check_inside else None
    check(lib().fastnerf_pp_intersect_sphere(n, ptr(rays11), ptr(fg_far), ptr(cnt), stream()),
          'fastnerf_pp_intersect_sphere')
    if check_inside and int(cnt.item()) > 0:
        raise Exception('Not all your cameras are bounded by the unit sphere; please make sure the cameras are '
                        'normalized properly!')
    return fg_far


def pp_fg_depths(fg_far, S, near=1e-4, perturb=True, t_rand=None, seed=0):
    require_gpu(fg_far, t_rand)
    n = fg_far.shape[0]
    _need_f32('fg_far', fg_far, n)
    z = torch.empty(n, S, device=fg_far.device, dtype=torch.float32)
    if t_rand is not None:
        t_rand = _f32(t_rand)
        assert t_rand.shape == (n, S)
    check(lib().fastnerf_pp_fg_depths(n, S, float(near), ptr(fg_far), int(bool(perturb) or t_rand is not None),
                                      ptr(t_rand), int(seed), ptr(z), stream()), 'fastnerf_pp_fg_depths')
    return z


def pp_sample_pdf_merge(z, weights, Ni, det=False, u=None, seed=0):
    require_gpu(z, weights, u)
    n, S = z.shape
    z_out = torch.empty(n, S + Ni, device=z.device, dtype=torch.float32)
    z_samples = torch.empty(n, Ni, device=z.device, dtype=torch.float32)
    if u is not None:
        u = _f32(u)
    check(lib().fastnerf_pp_sample_pdf_merge(n, S, Ni, ptr(z), ptr(weights), int(bool(det)), ptr(u), int(seed),
                                             ptr(z_out), ptr(z_samples), stream()), 'fastnerf_pp_sample_pdf_merge')
    return z_out, z_samples


def pp_perturb_samples(z, t_rand=None, seed=0):
    """perturb_samples (ddp_train_nerf.py:72-81) on [n,S] sorted depths."""
    require_gpu(z, t_rand)
    z = _f32(z)
    n, S = z.shape
    out = torch.empty_like(z)
    if t_rand is not None:
        t_rand = _f32(t_rand)
        assert t_rand.shape == z.shape
    check(lib().fastnerf_pp_perturb_samples(n, S, ptr(z), ptr(t_rand), int(seed), ptr(out), stream()), 'fastnerf_pp_perturb_samples')
    return out


def pp_sample_pdf(bins, weights, Ni, det=False, u=None, seed=0):
    """nerf++ sample_pdf (ddp_train_nerf.py:84-133): bins [n,M], weights [n,M-1] -> [n,Ni]."""
    require_gpu(bins, weights, u)
    n, M = bins.shape
    out = torch.empty(n, Ni, device=bins.device, dtype=torch.float32)
    if u is not None:
        u = _f32(u)
    bins, weights = _f32(bins), _f32(weights)
    check(lib().fastnerf_pp_sample_pdf(n, M, Ni, ptr(bins), ptr(weights), int(bool(det)), ptr(u), int(seed), ptr(out),
                                       stream()), 'fastnerf_pp_sample_pdf')
    return out


def pp_depth2pts_outside(ray_o, ray_d, depth):
    """depth2pts_outside (ddp_model.py:16-45): ray_o / ray_d [n,3], depth [n,S] -> (pts [n,S,4], depth_real [n,S])."""
    require_gpu(ray_o, ray_d, depth)
    depth = _f32(depth)
    n, S = depth.shape
    pts = torch.empty(n, S, 4, device=depth.device, dtype=torch.float32)
    dr = torch.empty(n, S, device=depth.device, dtype=torch.float32)
    ray_o, ray_d = _f32(ray_o), _f32(ray_d)
    check(lib().fastnerf_pp_depth2pts_outside(n, S, ptr(ray_o), ptr(ray_d), ptr(depth), ptr(pts), ptr(dr), stream()),
          'fastnerf_pp_depth2pts_outside')
    return pts, dr


def pp_composite_fwd(part, raw, z, rays11, fg_far=None):
    require_gpu(raw, z, rays11, fg_far)
    n, S = z.shape
    dev = z.device
    rgb = torch.empty(n, 3, device=dev, dtype=torch.float32)
    w = torch.empty(n, S, device=dev, dtype=torch.float32)
    depth = torch.empty(n, device=dev, dtype=torch.float32)
    lam = torch.empty(n, device=dev, dtype=torch.float32) if part == 0 else None
    check(lib().fastnerf_pp_composite_fwd(n, S, int(part), ptr(raw), ptr(z), ptr(rays11), ptr(fg_far), ptr(rgb), ptr(w),
                                          ptr(depth), ptr(lam), stream()), 'fastnerf_pp_composite_fwd')
    return rgb, w, depth, lam


def pp_composite_bwd(part, raw, z, rays11, g_rgb, fg_far=None, g_lambda=None):
    require_gpu(raw, z, rays11, g_rgb, fg_far, g_lambda)
    n, S = z.shape
    draw = torch.empty(n, S, 4, device=z.device, dtype=torch.float32)
    g_rgb, g_lambda = _f32(g_rgb), None if g_lambda is None else _f32(g_lambda)
    check(lib().fastnerf_pp_composite_bwd(n, S, int(part), ptr(raw), ptr(z), ptr(rays11), ptr(fg_far), ptr(g_rgb),
                                          ptr(g_lambda), ptr(draw), stream()),
          'fastnerf_pp_composite_bwd')
    return draw


def leaf_sumcount(rgb, target, leaf_tag, max_leaves, sums, counts):
    """Accumulate per-(image, leaf) fp64 sums of |gt-pred| (rays x channels) and ray counts."""
    require_gpu(rgb, target, leaf_tag, sums, counts)
    assert sums.dtype == torch.float64 and counts.dtype == torch.int32
    rgb, target = _f32(rgb), _f32(target)
    check(lib().fastnerf_leaf_sumcount(rgb.shape[0], ptr(rgb), ptr(target), ptr(leaf_tag), int(max_leaves),
                                       ptr(sums), ptr(counts), stream()), 'fastnerf_leaf_sumcount')


def pp_gen_rays(H, W, intrinsics, c2w, device='cuda'):
    """get_rays_single_image (nerf_sample_ray_split.py:10-34) -> rays_o, rays_d [H*W,3] on the device."""
    K = np.ascontiguousarray(np.asarray(intrinsics, dtype=np.float64).reshape(4, 4))
    M = np.ascontiguousarray(np.asarray(c2w, dtype=np.float64).reshape(4, 4))
    ro = torch.empty(H * W, 3, device=device, dtype=torch.float32)
    rd = torch.empty(H * W, 3, device=device, dtype=torch.float32)
    check(lib().fastnerf_pp_gen_rays(int(H), int(W), K.ctypes.data, M.ctypes.data, ptr(ro), ptr(rd), stream()),
          'fastnerf_pp_gen_rays')
    return ro, rd


MC_TRI_STRIDE = 16   # FASTNERF_MC_TRI_STRIDE


def grid_points(p0, xs, ys, zs, rays11):
    """Rows p0 .. p0 + len(rays11) - 1 of the (xs, ys, zs) point grid (meshgrid 'ij' order) as rays11 rows o = point, rest 0."""
    require_gpu(xs, ys, zs, rays11)
    check(lib().fastnerf_grid_points(int(p0), rays11.shape[0], ptr(xs), xs.numel(), ptr(ys), ys.numel(), ptr(zs), zs.numel(),
                                     ptr(rays11), stream()), 'fastnerf_grid_points')


def grid_sigma(raw, out):
    """out[q] = relu(raw[q, .., 3]) for the len(out) rows of an MLP output [n, 1, 4]."""
    require_gpu(raw, out)
    assert raw.numel() == 4 * out.numel()
    check(lib().fastnerf_grid_sigma(out.numel(), ptr(raw), ptr(out), stream()), 'fastnerf_grid_sigma')


def mc_tables():
    """(tri [256, MC_TRI_STRIDE] int8, edge [256] uint16): the marching-cubes tables the kernels use (host call, no GPU)."""
    tri = np.zeros((256, MC_TRI_STRIDE), np.int8)
    edge = np.zeros(256, np.uint16)
    check(lib().fastnerf_mc_tables(tri.ctypes.data, edge.ctypes.data), 'fastnerf_mc_tables')
    return tri, edge


def marching_cubes(vol, threshold):
    """vol: contiguous float32 [nx, ny, nz] cuda tensor -> (verts [V, 3] float32, tris [T, 3] int32), the contract of
    include/fastnerf.h.  One host synchronisation (the counts)."""
    require_gpu(vol)
    nx, ny, nz = vol.shape
    ws = torch.empty(int(check(lib().fastnerf_mc_ws_bytes(nx, ny, nz), 'fastnerf_mc_ws_bytes')), device=vol.device, dtype=torch.uint8)
    counts = np.zeros(2, np.int64)
    check(lib().fastnerf_mc_count(ptr(vol), nx, ny, nz, float(threshold), ptr(ws), counts.ctypes.data, stream()), 'fastnerf_mc_count')
    V, T = int(counts[0]), int(counts[1])
    verts = torch.empty(V, 3, device=vol.device, dtype=torch.float32)
    tris = torch.empty(T, 3, device=vol.device, dtype=torch.int32)
    if V > 0:
        check(lib().fastnerf_mc_emit(ptr(vol), nx, ny, nz, float(threshold), ptr(ws), ptr(verts), ptr(tris), stream()),
              'fastnerf_mc_emit')
    return verts, tris


# ---- occupancy grid (csrc/occupancy.hip) ---------------------------------------------------------------------------
def occ_words(nx, ny, nz):
    """Number of uint32 words (held as int32) of the packed bits of an nx x ny x nz grid."""
    return int(check(lib().fastnerf_occ_words(int(nx), int(ny), int(nz)), 'fastnerf_occ_words'))


def occ_build(vol, threshold=0., dilate=1):
    """Point volume [nx+1, ny+1, nz+1] -> packed bits: corner maximum > threshold, then dilation by `dilate` cells."""
    require_gpu(vol)
    if vol.dim() != 3 or min(vol.shape) < 2:
        raise ValueError('an occupancy grid needs a point volume [nx+1, ny+1, nz+1] with every dimension >= 2, got %s' % (tuple(vol.shape),))
    if int(dilate) < 0:
        raise ValueError('dilate must be >= 0')
    vol = _f32(vol)
    nx, ny, nz = (int(s) - 1 for s in vol.shape)
    nw = occ_words(nx, ny, nz)
    words = torch.empty(nw, device=vol.device, dtype=torch.int32)
    ws = torch.empty(2 * nw, device=vol.device, dtype=torch.int32) if int(dilate) > 0 else None
    check(lib().fastnerf_occ_build(ptr(vol), nx, ny, nz, float(threshold), int(dilate), ptr(words), ptr(ws), stream()), 'fastnerf_occ_build')
    return words


def occ_from_mask(mask):
    """Bool / byte mask [nx, ny, nz] -> packed bits."""
    require_gpu(mask)
    if mask.dim() != 3 or min(mask.shape) < 1:
        raise ValueError('an occupancy mask is [nx, ny, nz] with every dimension >= 1, got %s' % (tuple(mask.shape),))
    m = (mask != 0).to(torch.uint8).contiguous()
    nx, ny, nz = (int(s) for s in m.shape)
    words = torch.empty(occ_words(nx, ny, nz), device=m.device, dtype=torch.int32)
    check(lib().fastnerf_occ_from_mask(ptr(m), nx, ny, nz, ptr(words), stream()), 'fastnerf_occ_from_mask')
    return words


def _occ_entry(cgrid, name):
    """The entry point `name` for a _lib.OccGrid, its `_cascade` form for a _lib.OccCascade: (function, its name).  The
    descriptor itself is wanted (OccupancyGrid._c / OccupancyCascade._c): a ctypes.byref() or POINTER() of one, which ctypes
    alone would convert, does not say which entry point it is for and raises TypeError."""
    if isinstance(cgrid, _lib.OccCascade):
        name += '_cascade'
    elif not isinstance(cgrid, _lib.OccGrid):
        raise TypeError('expected a _lib.OccGrid or a _lib.OccCascade, got %s' % type(cgrid).__name__)
    return getattr(lib(), name), name


def occ_query(cgrid, pts):
    """cgrid: _lib.OccGrid or _lib.OccCascade; pts [n, 3] -> uint8 [n]."""
    require_gpu(pts)
    pts = _f32(pts).reshape(-1, 3)
    out = torch.empty(pts.shape[0], device=pts.device, dtype=torch.uint8)
    fn, name = _occ_entry(cgrid, 'fastnerf_occ_query')
    check(fn(cgrid, pts.shape[0], ptr(pts), ptr(out), stream()), name)
    return out


def occ_classify(cgrid, rays11, z, raw=None):
    """The samples o + d * z of a pass sorted by the grid (or the cascade): (live_idx int32 [n*S], counts int32 [2] = (occupied, n*S)), both on
    the device; live_idx[:occupied] ascends.  raw ([n, S, 4], optional) is zeroed at the other samples, untouched elsewhere."""
    require_gpu(rays11, z, raw)
    n, S = z.shape
    P = n * S
    assert rays11.shape == (n, 11) and rays11.is_contiguous() and z.is_contiguous() and z.dtype == torch.float32
    assert raw is None or (raw.numel() == P * 4 and raw.is_contiguous() and raw.dtype == torch.float32)
    idx = torch.empty(P, device=z.device, dtype=torch.int32)
    cnt = torch.empty(2, device=z.device, dtype=torch.int32)
    ws = torch.empty(int(lib().fastnerf_compact_ws_ints(P)), device=z.device, dtype=torch.int32)
    fn, name = _occ_entry(cgrid, 'fastnerf_occ_classify')
    check(fn(cgrid, n, S, ptr(rays11), ptr(z), ptr(idx), ptr(cnt), ptr(raw), ptr(ws), stream()), name)
    return idx, cnt


def occ_ray_bounds(cgrid, rays11, write_back=False):
    """Per ray of rays11 [n, 11] the part [near', far'] of [near, far] (columns 6:8) outside which the grid (cgrid a _lib.OccGrid) or the
    cascade (a _lib.OccCascade) calls no sample o + d * z occupied: (bounds float32 [n, 2], hit uint8 [n]); a ray with hit = 0 meets
    nothing occupied and keeps its bounds.  Conservative without exceptions, `outside_occupied` honoured (fastnerf_occ_ray_bounds).
    write_back=True also stores near' / far' into columns 6:8 of rays11, in place; no other column is written."""
    require_gpu(rays11)
    assert rays11.dim() == 2 and rays11.shape[1] == 11 and rays11.is_contiguous() and rays11.dtype == torch.float32
    n = rays11.shape[0]
    bounds = torch.empty(n, 2, device=rays11.device, dtype=torch.float32)
    hit = torch.empty(n, device=rays11.device, dtype=torch.uint8)
    grid, cascade = _ert_grid_args(cgrid)
    if grid is None and cascade is None:
        raise TypeError('expected a _lib.OccGrid or a _lib.OccCascade, got None')
    check(lib().fastnerf_occ_ray_bounds(grid, cascade, n, ptr(rays11), 1 if write_back else 0, ptr(bounds), ptr(hit), stream()),
          'fastnerf_occ_ray_bounds')
    return bounds, hit


def occ_cell_points(cgrid, c0, rays11, seed=0):
    """One point inside each of the cells c0 .. c0 + len(rays11) - 1 of the grid as rays11 rows (o = point, rest 0): the cell's
    centre (seed 0) or a Philox-jittered point keyed by (seed, cell)."""
    require_gpu(rays11)
    assert rays11.dim() == 2 and rays11.shape[1] == 11 and rays11.is_contiguous() and rays11.dtype == torch.float32
    check(lib().fastnerf_occ_cell_points(cgrid, int(c0), rays11.shape[0], int(seed), ptr(rays11), stream()), 'fastnerf_occ_cell_points')
    return rays11


def occ_update(raw_c, raw_f, c0, n, shape, decay, threshold, dilate, dens, words, ws=None):
    """dens = max(dens * decay, relu(sigma of raw_c), relu(sigma of raw_f)) on the cells c0 .. c0 + n - 1, then words = dens >
    threshold over the whole grid, dilated by `dilate` cells.  words=None: the density only; n=0: the bits only.  In place; no host
    round trip."""
    require_gpu(raw_c, raw_f, dens, words, ws)
    nx, ny, nz = (int(s) for s in shape)
    nw = occ_words(nx, ny, nz)
    assert dens.dtype == torch.float32 and dens.is_contiguous() and dens.numel() == nx * ny * nz
    assert words is None or (words.dtype == torch.int32 and words.is_contiguous() and words.numel() == nw)
    for r in (raw_c, raw_f):
        assert r is None or (r.dtype == torch.float32 and r.is_contiguous() and r.numel() >= 4 * int(n))
    if int(dilate) > 0 and ws is None and words is not None:
        ws = torch.empty(2 * nw, device=dens.device, dtype=torch.int32)
    assert ws is None or (ws.dtype == torch.int32 and ws.numel() >= 2 * nw)
    check(lib().fastnerf_occ_update(ptr(raw_c), ptr(raw_f), int(c0), int(n), nx, ny, nz, float(decay), float(threshold), int(dilate),
                                    ptr(dens), ptr(words), ptr(ws), stream()), 'fastnerf_occ_update')


def occ_cascade_own(ccascade, level, dilate, device):
    """The own cells of level `level` of a training cascade (ccascade a _lib.OccCascade): ascending int32 cell indices
    (fastnerf_occ_cascade_own).  One host read of the count: it runs once, when the cascade is made."""
    g = ccascade.level[int(level)]
    ncells = int(g.n[0]) * int(g.n[1]) * int(g.n[2])
    if not 0 < ncells < 2 ** 31:
        raise ValueError('a level has 1 to 2^31 - 1 cells')
    lst = torch.empty(ncells, device=device, dtype=torch.int32)
    cnt = torch.empty(2, device=device, dtype=torch.int32)
    ws = torch.empty(int(lib().fastnerf_compact_ws_ints(ncells)), device=device, dtype=torch.int32)
    check(lib().fastnerf_occ_cascade_own(ccascade, int(level), int(dilate), ptr(lst), ptr(cnt), ptr(ws), stream()), 'fastnerf_occ_cascade_own')
    return lst[:int(cnt[0])].clone()


def occ_cascade_points(ccascade, own, offsets, q0, rays11, seed=0):
    """One point per position q0 .. q0 + len(rays11) - 1 of the concatenated own lists (`own` int32 on the device, `offsets` a ctypes
    int64 array of levels + 1 entries): the point occ_cell_points makes for that level's grid and that cell."""
    require_gpu(own, rays11)
    assert rays11.dim() == 2 and rays11.shape[1] == 11 and rays11.is_contiguous() and rays11.dtype == torch.float32
    assert own.dtype == torch.int32 and own.is_contiguous() and own.numel() >= int(offsets[ccascade.levels])
    check(lib().fastnerf_occ_cascade_points(ccascade, ptr(own), offsets, int(q0), rays11.shape[0], int(seed), ptr(rays11), stream()),
          'fastnerf_occ_cascade_points')
    return rays11


def occ_cascade_update(ccascade, raw_c, raw_f, own, offsets, q0, n, decay, dens):
    """dens = max(dens * decay, relu(sigma of raw_c), relu(sigma of raw_f)) at the level and cell of the positions q0 .. q0 + n - 1.
    decay: ctypes float array, dens: ctypes void-pointer array, one entry per level (the caller keeps the tensors alive)."""
    require_gpu(raw_c, raw_f, own)
    for r in (raw_c, raw_f):
        assert r is None or (r.dtype == torch.float32 and r.is_contiguous() and r.numel() >= 4 * int(n))
    assert own.dtype == torch.int32 and own.is_contiguous() and own.numel() >= int(offsets[ccascade.levels])
    check(lib().fastnerf_occ_cascade_update(ccascade, ptr(raw_c), ptr(raw_f), ptr(own), offsets, int(q0), int(n), decay, dens, stream()),
          'fastnerf_occ_cascade_update')


def mlp_fwd_list(rays11, z, params, packed_fwd, raw, live_idx, live_cnt, flags=0):
    """Inference forward over a point list (current math mode): raw[live_idx[j]] = logits of point live_idx[j], j < live_cnt[0]."""
    require_gpu(rays11, z, params, packed_fwd, raw, live_idx, live_cnt)
    n, S = z.shape
    assert raw.numel() == n * S * 4 and raw.is_contiguous() and live_idx.dtype == torch.int32 and live_cnt.dtype == torch.int32
    assert packed_fwd.numel() == packed_floats(0, 1) and packed_tag(packed_fwd) == _MATH, \
        'packed weights were not produced by mlp_pack under the current math mode'
    fn, name = _mlp('fwd_list', 0)
    check(fn(0, n, S, ptr(rays11), ptr(z), ptr(params), ptr(packed_fwd), ptr(raw), ptr(live_idx), ptr(live_cnt), int(flags), stream()), name)
    return raw


def render_rays_fwd_occ(rays11, params_c, packed_c, params_f, packed_f, N_samples, N_importance, cgrid, lindisp=False, perturb=False,
                        det=True, white_bkgd=False, t_rand=None, u=None, seed0=0, seed1=0, skip_dead_rgb=False):
    """render_rays_fwd (inference, no sigma noise) through an occupancy grid (cgrid a _lib.OccGrid) or a cascade (a
    _lib.OccCascade: fastnerf_render_rays_fwd_occ_cascade): one C-ABI call.  Same dict, act0 / act1 None,
    plus 'counts': int32 [4] on the device = (occupied, total) samples of the coarse pass, then of the fine pass."""
    require_gpu(rays11, params_c, packed_c, params_f, packed_f, t_rand, u)
    dev = rays11.device
    o, t_rand, u = _rr_fwd_outputs(rays11, packed_c, packed_f, N_samples, N_importance, t_rand, u)
    o['counts'] = torch.zeros(4, device=dev, dtype=torch.int32)
    P1 = rays11.shape[0] * (N_samples + N_importance)
    live_ws = torch.empty(max(1, P1 + int(lib().fastnerf_compact_ws_ints(max(1, P1)))), device=dev, dtype=torch.int32)
    head, nets, outs = _rr_fwd_ptrs(o, rays11, params_c, packed_c, params_f, packed_f, N_samples, N_importance, lindisp, perturb, det,
                                    white_bkgd, t_rand, u, seed0, seed1, with_act=False)
    fn, name = _occ_entry(cgrid, 'fastnerf_render_rays_fwd_occ')
    check(fn(*head, *nets, cgrid, ptr(live_ws), ptr(o['counts']), *outs, 1 if skip_dead_rgb else 0, stream()), name)
    return o


# ---- early ray termination (csrc/occupancy.hip, csrc/composite.hip, render.cpp) ----------------------------------------------
def _ert_grid_args(cgrid, required=False):
    """(grid, cascade) arguments of the fastnerf_ert_* / march entry points for None (unless `required`), a _lib.OccGrid or a
    _lib.OccCascade."""
    if cgrid is None:
        if required:
            raise TypeError('expected a _lib.OccGrid or a _lib.OccCascade, got None')
        return None, None
    if isinstance(cgrid, _lib.OccCascade):
        return None, cgrid
    if isinstance(cgrid, _lib.OccGrid):
        return cgrid, None
    raise TypeError('expected None, a _lib.OccGrid or a _lib.OccCascade, got %s' % type(cgrid).__name__)


def check_ert(ert, ert_block):
    """(eps, block) as numbers, or ValueError: 0 <= eps < 1 (fp32, as the kernels compare it), block >= 1."""
    eps, block = float(np.float32(ert)), int(ert_block)
    if not (0. <= eps < 1.) or block < 1 or block != ert_block:
        raise ValueError('early ray termination needs 0 <= ert < 1 and an integer ert_block >= 1, got ert=%r, ert_block=%r' % (ert, ert_block))
    return eps, block


def ert_classify(rays11, z, s0, s1, trans, eps, cgrid=None, raw=None):
    """The segment [s0, s1) of the samples of a pass sorted by trans[ray] > eps (trans None: every ray) and by cgrid (None, a
    _lib.OccGrid or a _lib.OccCascade): (live_idx int32 [n * (s1 - s0)], counts int32 [2] = (evaluated, n * (s1 - s0))), both on the
    device; live_idx[:evaluated] ascends and holds indices ray * S + s.  raw ([n, S, 4], optional) is zeroed at the segment's other
    samples and untouched elsewhere."""
    require_gpu(rays11, z, trans, raw)
    n, S = z.shape
    s0, s1 = int(s0), int(s1)
    assert rays11.shape == (n, 11) and rays11.is_contiguous() and z.is_contiguous() and z.dtype == torch.float32
    assert rays11.dtype == torch.float32 and rays11.device == z.device
    assert trans is None or (trans.shape == (n,) and trans.dtype == torch.float32 and trans.is_contiguous() and trans.device == z.device)
    assert raw is None or raw.device == z.device
    assert raw is None or (raw.numel() == n * S * 4 and raw.is_contiguous() and raw.dtype == torch.float32)
    Q = max(1, n * max(0, s1 - s0))
    idx = torch.empty(Q, device=z.device, dtype=torch.int32)
    cnt = torch.empty(2, device=z.device, dtype=torch.int32)
    ws = torch.empty(int(lib().fastnerf_compact_ws_ints(Q)), device=z.device, dtype=torch.int32)
    grid, cascade = _ert_grid_args(cgrid)
    check(lib().fastnerf_ert_classify(grid, cascade, n, S, s0, s1, ptr(rays11), ptr(z), ptr(trans), float(eps), ptr(idx), ptr(cnt),
                                      ptr(raw), ptr(ws), stream()), 'fastnerf_ert_classify')
    return idx, cnt


def ert_advance(raw, z, rays11, s0, s1, trans, first=False, seg_count=None, total=None):
    """trans[ray] (float32 [n], in place; taken as 1 when first) *= the product over the samples s0 <= s < s1 of 1 - alpha + 1e-10, as
    raw2outputs forms alpha.  total (int32 [2], optional): total[0] (0 when first) += seg_count[0], total[1] = n * S."""
    require_gpu(raw, z, rays11, trans, seg_count, total)
    n, S = z.shape
    assert raw.shape == (n, S, 4) and raw.is_contiguous() and raw.dtype == torch.float32 and z.is_contiguous() and z.dtype == torch.float32
    assert rays11.shape == (n, 11) and rays11.is_contiguous() and rays11.dtype == torch.float32
    assert trans.shape == (n,) and trans.dtype == torch.float32 and trans.is_contiguous()
    assert total is None or (seg_count is not None and total.dtype == torch.int32 and seg_count.dtype == torch.int32 and
                             total.is_contiguous() and seg_count.is_contiguous() and total.numel() >= 2 and seg_count.numel() >= 1)
    assert all(t is None or t.device == z.device for t in (raw, rays11, trans, seg_count, total))
    check(lib().fastnerf_ert_advance(n, S, int(s0), int(s1), ptr(raw), ptr(z), ptr(rays11), 1 if first else 0, ptr(trans), ptr(seg_count),
                                     ptr(total), stream()), 'fastnerf_ert_advance')
    return trans


# ---- marched render (csrc/march.hip, csrc/occupancy.hip, render.cpp) ------------------------------------------------------------
MARCH_K_MAX = (1 << 24) - 1      # lattice depths per ray: 2 <= K < 2^24
MARCH_CAP_MAX = 512              # slots of a packed row: 2 <= C <= 512 (the compositing kernels' limit)


def check_march(march, march_cap):
    """(K, C) as numbers, or ValueError: integers with 2 <= K < 2^24 and 2 <= C <= 512."""
    ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (march, march_cap))
    if not ok or not (2 <= march <= MARCH_K_MAX) or not (2 <= march_cap <= MARCH_CAP_MAX):
        raise ValueError('the marched render needs integers 2 <= march < 2^24 and 2 <= march_cap <= 512, got march=%r, march_cap=%r'
                         % (march, march_cap))
    return int(march), int(march_cap)


def occ_march(cgrid, rays11, K, C, s0=0, s1=None, trans=None, eps=0., lindisp=False, state=None, z=None, kidx=None, overflow=None,
              jitter=None):
    """One round [s0, s1) of fastnerf_occ_march over the rays of rays11 [n, 11], through cgrid (a _lib.OccGrid or a _lib.OccCascade):
    -> (z float32 [n, C], kidx int32 [n, C], overflow uint8 [n], state int32 [n, 2]).  The first round (s0 == 0) allocates what is not
    given; a later round takes the four tensors of the round before it and writes in place.  trans (float32 [n], optional): a ray
    with trans <= eps (or NaN) is cut.  jitter = (u, seed): the call goes to fastnerf_occ_march_jitter (occ_march_jitter below)."""
    require_gpu(rays11, trans, state, z, kidx, overflow)
    K, C = check_march(K, C)
    s0 = int(s0)
    s1 = C if s1 is None else int(s1)
    assert rays11.dim() == 2 and rays11.shape[1] == 11 and rays11.is_contiguous() and rays11.dtype == torch.float32
    n, dev = rays11.shape[0], rays11.device
    if s0 > 0 and any(t is None for t in (state, z, kidx, overflow)):
        raise ValueError('a round with s0 > 0 continues the state, z, kidx and overflow of the round before it')
    z = torch.empty(n, C, device=dev, dtype=torch.float32) if z is None else z
    kidx = torch.empty(n, C, device=dev, dtype=torch.int32) if kidx is None else kidx
    overflow = torch.empty(n, device=dev, dtype=torch.uint8) if overflow is None else overflow
    state = torch.empty(n, 2, device=dev, dtype=torch.int32) if state is None else state
    assert z.shape == (n, C) and z.dtype == torch.float32 and z.is_contiguous() and z.device == dev
    assert kidx.shape == (n, C) and kidx.dtype == torch.int32 and kidx.is_contiguous() and kidx.device == dev
    assert overflow.shape == (n,) and overflow.dtype == torch.uint8 and overflow.is_contiguous() and overflow.device == dev
    assert state.shape == (n, 2) and state.dtype == torch.int32 and state.is_contiguous() and state.device == dev
    assert trans is None or (trans.shape == (n,) and trans.dtype == torch.float32 and trans.is_contiguous() and trans.device == dev)
    grid, cascade = _ert_grid_args(cgrid, required=True)
    name, shift = 'fastnerf_occ_march', ()
    if jitter is not None:      # the same list with (u, seed) behind eps
        u, seed = jitter
        require_gpu(u)
        assert u is None or (u.shape == (n,) and u.dtype == torch.float32 and u.is_contiguous() and u.device == dev)
        name, shift = 'fastnerf_occ_march_jitter', (ptr(u), int(seed))
    check(getattr(lib(), name)(grid, cascade, n, K, 1 if lindisp else 0, ptr(rays11), C, s0, s1, 1 if s0 == 0 else 0, ptr(trans),
                               float(eps), *shift, ptr(state), ptr(z), ptr(kidx), ptr(overflow), stream()), name)
    return z, kidx, overflow, state


def occ_march_jitter(cgrid, rays11, K, C, u=None, seed=0, **kw):
    """occ_march through fastnerf_occ_march_jitter (include/fastnerf.h, "marched training"): the lattice of ray r shifted by u[r] in
    [0, 1) of its spacing.  u: float32 [n] or None; with None, seed != 0 draws the shifts from the 'mrch' stream and seed == 0 is the
    unshifted lattice.  The other keywords and the result are occ_march's."""
    return occ_march(cgrid, rays11, K, C, jitter=(u, seed), **kw)


def march_mask(overflow, g_rgb):
    """fastnerf_march_mask, in place: the rows of g_rgb [n, 3] of the rays with overflow[r] != 0 are zeroed.  -> g_rgb."""
    require_gpu(overflow, g_rgb)
    n = overflow.shape[0]
    assert overflow.dtype == torch.uint8 and overflow.is_contiguous() and overflow.shape == (n,)
    assert g_rgb.dtype == torch.float32 and g_rgb.is_contiguous() and g_rgb.shape == (n, 3) and g_rgb.device == overflow.device
    check(lib().fastnerf_march_mask(n, ptr(overflow), ptr(g_rgb), stream()), 'fastnerf_march_mask')
    return g_rgb


def step_march_ws_ints(n, C):
    """int32 count of fn_step_march.list_ws for n rays and rows of C slots."""
    return int(check(lib().fastnerf_step_march_ws_ints(int(n), int(C)), 'fastnerf_step_march_ws_ints'))


def march_list(kidx, s0, s1, raw=None, total=None, lattice=0):
    """The live list of the segment [s0, s1) of packed rows kidx [n, C]: (live_idx int32 [n * (s1 - s0)], counts int32 [2] = (live,
    n * (s1 - s0))), on the device; live_idx[:live] ascends and holds ray * C + slot.  raw ([n, C, 4], optional) is zeroed at the
    segment's other slots."""
    require_gpu(kidx, raw, total)
    n, C = kidx.shape
    s0, s1 = int(s0), int(s1)
    assert kidx.dtype == torch.int32 and kidx.is_contiguous()
    assert raw is None or (raw.numel() == n * C * 4 and raw.is_contiguous() and raw.dtype == torch.float32 and raw.device == kidx.device)
    assert total is None or (total.dtype == torch.int32 and total.is_contiguous() and total.numel() >= 2 and total.device == kidx.device)
    Q = max(1, n * max(0, s1 - s0))
    idx = torch.empty(Q, device=kidx.device, dtype=torch.int32)
    cnt = torch.empty(2, device=kidx.device, dtype=torch.int32)
    ws = torch.empty(int(lib().fastnerf_compact_ws_ints(Q)), device=kidx.device, dtype=torch.int32)
    check(lib().fastnerf_march_list(n, C, s0, s1, ptr(kidx), ptr(idx), ptr(cnt), ptr(raw), ptr(ws), ptr(total), int(lattice), stream()),
          'fastnerf_march_list')
    return idx, cnt


def render_rays_fwd_march(rays11, params, packed, K, C, cgrid, eps=None, block=32, lindisp=False, white_bkgd=False, skip_dead_rgb=False):
    """The marched render (fastnerf_render_rays_fwd_march): one C-ABI call.  -> dict of rgb, disp, acc, depth, w [n, C] (the maps and
    the weights of the packed row), raw [n, C, 4], z [n, C], kidx int32 [n, C], overflow uint8 [n], counts int32 [2] = (evaluated
    samples, n * K).  eps None: no early ray termination."""
    require_gpu(rays11, params, packed)
    K, C = check_march(K, C)
    if eps is None:
        eps, block = 0., 0
    else:
        eps, block = check_ert(eps, block)
    assert rays11.dim() == 2 and rays11.shape[1] == 11 and rays11.is_contiguous() and rays11.dtype == torch.float32
    assert packed.numel() == packed_floats(0, 1) and packed_tag(packed) == _MATH, \
        'packed weights were not produced by mlp_pack under the current math mode'
    n, dev = rays11.shape[0], rays11.device
    f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)      # noqa: E731
    o = dict(rgb=f(n, 3), disp=f(n), acc=f(n), depth=f(n), w=f(n, C), raw=f(n, C, 4), z=f(n, C),
             kidx=torch.empty(n, C, device=dev, dtype=torch.int32), overflow=torch.empty(n, device=dev, dtype=torch.uint8),
             counts=torch.zeros(2, device=dev, dtype=torch.int32))
    grid, cascade = _ert_grid_args(cgrid, required=True)
    check(lib().fastnerf_render_rays_fwd_march(mode_id(), n, K, C, ptr(rays11), 1 if lindisp else 0, 1 if white_bkgd else 0, ptr(params),
                                               ptr(packed), grid, cascade, eps, block, ptr(o['counts']), ptr(o['z']), ptr(o['kidx']),
                                               ptr(o['overflow']), ptr(o['raw']), ptr(o['rgb']), ptr(o['disp']), ptr(o['acc']), ptr(o['w']),
                                               ptr(o['depth']), 1 if skip_dead_rgb else 0, stream()), 'fastnerf_render_rays_fwd_march')
    return o


def render_rays_fwd_ert(rays11, params_c, packed_c, params_f, packed_f, N_samples, N_importance, eps, block, cgrid=None, lindisp=False,
                        perturb=False, det=True, white_bkgd=False, t_rand=None, u=None, seed0=0, seed1=0, skip_dead_rgb=False):
    """render_rays_fwd_occ with early ray termination in the pass that produces the image (fastnerf_render_rays_fwd_ert; cgrid may be
    None): same dict, 'counts' = (evaluated, total) samples of the coarse pass, then of the fine pass, plus 'trans': float32 [n], the
    image pass's transmittance per ray after its last segment."""
    require_gpu(rays11, params_c, packed_c, params_f, packed_f, t_rand, u)
    dev = rays11.device
    eps, block = check_ert(eps, block)
    o, t_rand, u = _rr_fwd_outputs(rays11, packed_c, packed_f, N_samples, N_importance, t_rand, u)
    o['counts'] = torch.zeros(4, device=dev, dtype=torch.int32)
    n = rays11.shape[0]
    if cgrid is None and N_importance > 0:      # a plain coarse pass evaluates every sample: the library leaves that pair to the caller
        o['counts'][:2] = n * N_samples
    o['trans'] = torch.empty(n, device=dev, dtype=torch.float32)
    P1 = n * (N_samples + N_importance)
    live_ws = torch.empty(max(1, P1 + int(lib().fastnerf_compact_ws_ints(max(1, P1)))) + 2, device=dev, dtype=torch.int32)
    head, nets, outs = _rr_fwd_ptrs(o, rays11, params_c, packed_c, params_f, packed_f, N_samples, N_importance, lindisp, perturb, det,
                                    white_bkgd, t_rand, u, seed0, seed1, with_act=False)
    grid, cascade = _ert_grid_args(cgrid)
    check(lib().fastnerf_render_rays_fwd_ert(*head, *nets, grid, cascade, eps, block, ptr(o['trans']), ptr(live_ws), ptr(o['counts']),
                                             *outs, 1 if skip_dead_rgb else 0, stream()), 'fastnerf_render_rays_fwd_ert')
    return o
