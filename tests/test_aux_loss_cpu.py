"""Depth / opacity supervision without a GPU: the torch restatement of the loss (tests/aux_loss_ref.py) against float64
autograd of the plain formula, the zero-weight / NaN-target rule, the new C-ABI symbols and the struct sizes."""
import ctypes as C
import inspect
import os
import re

import torch

import aux_loss_ref as A
from fastnerf import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('fastnerf_aux_loss', 'fastnerf_render_rays_bwd_maps', 'fastnerf_render_rays_bwd_live_maps', 'fastnerf_step_aux_size',
       'fastnerf_train_step_aux')


def _inputs(n, seed, sparse):
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(n, generator=gen, dtype=torch.float64)      # noqa: E731
    maps = dict(depth1=2 + 4 * r(), acc1=r(), depth0=2 + 4 * r(), acc0=r())
    tg = dict(depth_target=2 + 4 * r(), depth_weight=0.5 + r(), acc_target=(r() > 0.5).double(), acc_weight=0.5 + r())
    if sparse:
        off = r() < 0.3
        tg['depth_weight'][off] = 0.
        tg['depth_target'][off] = float('nan')
        tg['acc_weight'][~off] = 0.
        tg['acc_target'][~off] = float('nan')
    return maps, tg


def test_restatement_against_float64_autograd():
    """g = grad_scale * lambda * d(L)/d(map), with L written out plainly (weights multiply: no zero weights here)."""
    n, lam_d, lam_a, scale = 37, 0.7, 0.3, 0.5
    maps, tg = _inputs(n, 1, sparse=False)
    leaves = {k: v.clone().requires_grad_(True) for k, v in maps.items()}
    Ld = lambda x: (tg['depth_weight'] * (x - tg['depth_target']) ** 2).mean()      # noqa: E731
    La = lambda x: (tg['acc_weight'] * (x - tg['acc_target']) ** 2).mean()      # noqa: E731
    plain = [Ld(leaves['depth1']), Ld(leaves['depth0']), La(leaves['acc1']), La(leaves['acc0'])]
    loss = A.f32(scale) * (A.f32(lam_d) * (plain[0] + plain[1]) + A.f32(lam_a) * (plain[2] + plain[3]))
    ref = torch.autograd.grad(loss, [leaves[k] for k in ('depth1', 'acc1', 'depth0', 'acc0')])
    loss4, g = A.aux_loss(**maps, **tg, lambda_depth=lam_d, lambda_acc=lam_a, grad_scale=scale)
    torch.testing.assert_close(loss4, torch.stack(plain).detach(), rtol=1e-14, atol=0)
    for got, want in zip((g['g_depth1'], g['g_acc1'], g['g_depth0'], g['g_acc0']), ref):
        torch.testing.assert_close(got, want, rtol=1e-14, atol=0)
    # unweighted = weights of one
    a, ga = A.aux_loss(**maps, depth_target=tg['depth_target'], lambda_depth=lam_d)
    b, gb = A.aux_loss(**maps, depth_target=tg['depth_target'], depth_weight=torch.ones(n), lambda_depth=lam_d)
    assert torch.equal(a, b) and torch.equal(ga['g_depth1'], gb['g_depth1'])
    assert ga['g_acc1'] is None and float(a[2]) == 0 and float(a[3]) == 0, 'a missing target switches its term off'


def test_zero_weight_rays_are_selected_out():
    """A weight of 0 gives exactly 0 and +0 whatever the target holds, NaN included; the rest equals the dense result on the kept rays."""
    n = 41
    maps, tg = _inputs(n, 2, sparse=True)
    loss4, g = A.aux_loss(**maps, **tg, lambda_depth=0.7, lambda_acc=0.3)
    assert torch.isfinite(loss4).all()
    for name, w in (('g_depth1', tg['depth_weight']), ('g_depth0', tg['depth_weight']), ('g_acc1', tg['acc_weight']),
                    ('g_acc0', tg['acc_weight'])):
        assert torch.isfinite(g[name]).all()
        z = g[name][w == 0]
        assert z.numel() > 0 and (z == 0).all() and not torch.signbit(z).any(), name
    keep = tg['depth_weight'] != 0
    dense = (tg['depth_weight'][keep] * (maps['depth1'][keep] - tg['depth_target'][keep]) ** 2).sum() / n
    torch.testing.assert_close(loss4[0], dense, rtol=1e-14, atol=0)
    # in float32 too (what the Trainer's targets are)
    l32, g32 = A.aux_loss(**maps, **tg, lambda_depth=0.7, lambda_acc=0.3, dtype=torch.float32)
    assert l32.dtype == torch.float32 and torch.isfinite(l32).all() and all(torch.isfinite(t).all() for t in g32.values())


def test_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, 'include', 'fastnerf.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, src), name + ' is not declared in fastnerf.h'
        assert hasattr(lib, name), name + ' is not exported'
        assert name in _lib.SIGNATURES
    I, L, P, F = C.c_int, C.c_int64, C.c_void_p, C.c_float
    # n, 4 maps, 2 x (target, weight), lambda_depth, lambda_acc, grad_scale, 4 gradients, loss4, stream
    assert _lib.SIGNATURES['fastnerf_aux_loss'] == (I, [L] + [P] * 8 + [F] * 3 + [P] * 6)
    # the existing lists + acc0, depth0, acc1, depth1 + const fn_map_grads* (before the stream)
    for plain in ('fastnerf_render_rays_bwd', 'fastnerf_render_rays_bwd_live'):
        res, args = _lib.SIGNATURES[plain]
        assert _lib.SIGNATURES[plain + '_maps'] == (res, args[:-1] + [P] * 4 + [C.POINTER(_lib.MapGrads), P])
    assert _lib.SIGNATURES['fastnerf_train_step_aux'] == (I, [C.POINTER(_lib.StepArgs), C.POINTER(_lib.StepAux), I, P])
    for name in ('struct fn_map_grads', 'struct fn_step_aux'):
        assert name in src


def test_struct_sizes():
    lib = _lib.lib()
    assert lib.fastnerf_step_aux_size() == C.sizeof(_lib.StepAux) == 80      # 9 pointers + 2 floats
    assert C.sizeof(_lib.MapGrads) == 48
    assert lib.fastnerf_step_args_size() == C.sizeof(_lib.StepArgs) == 512, 'fn_step_args does not grow'


def test_argument_checks_come_before_any_launch():
    lib = _lib.lib()
    null = C.c_void_p(None)
    assert lib.fastnerf_aux_loss(0, *([null] * 8), 1.0, 1.0, 1.0, *([null] * 6)) == -1
    one = C.c_void_p(16)      # never dereferenced: the call fails on its arguments
    assert lib.fastnerf_aux_loss(4, null, null, null, null, one, null, null, null, 1.0, 1.0, 1.0, *([null] * 6)) == -1
    assert b'depth' in lib.fastnerf_last_error()
    a = _lib.StepArgs()
    assert lib.fastnerf_train_step_aux(C.byref(a), None, 1, None) == -1      # the checks of fastnerf_train_step, with and without aux
    assert lib.fastnerf_train_step_aux(C.byref(a), C.byref(_lib.StepAux()), 1, None) == -1


def test_python_surface():
    from fastnerf import ops, render, run_nerf
    assert callable(ops.aux_loss)
    assert 'map_grads' in inspect.signature(ops.render_rays_bwd).parameters
    assert 'map_grads' in inspect.signature(ops.render_rays_bwd_live).parameters
    assert inspect.signature(render.render_rays).parameters['retdepth'].default is False
    for fn_, tail in ((run_nerf.Trainer.step, 4), (run_nerf.Trainer.forward_backward, 4), (run_nerf.Trainer._fused_prepare, 4)):
        names = list(inspect.signature(fn_).parameters)
        assert names[-tail:] == ['depth', 'depth_weight', 'acc', 'acc_weight'], names      # appended, with defaults
        assert all(inspect.signature(fn_).parameters[k].default is None for k in names[-tail:])
    init = inspect.signature(run_nerf.Trainer.__init__).parameters
    assert init['lambda_depth'].default == 0. and init['lambda_acc'].default == 0.
    assert 'stay non-differentiable' not in render.render_rays.__doc__
