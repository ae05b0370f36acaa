"""Per-ray background colours without a device: the restatement of the two kernels (tests/bkgd_ref.py) against autograd and against the
white composite, the 'bkgd' stream, the argument checks of the library that come before anything touches a GPU, the Trainer's refusals
and the loader's flag."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import bkgd_ref as B
import philox_numpy as P

F32 = np.float32


def test_blend_sends_minus_g_dot_b_to_acc():
    gen = torch.Generator().manual_seed(1)
    n = 37
    rgb = torch.rand(n, 3, generator=gen, dtype=torch.float64)
    acc = torch.rand(n, generator=gen, dtype=torch.float64).requires_grad_()
    b = torch.rand(n, 3, generator=gen, dtype=torch.float64)
    g = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    (B.blend_torch(rgb, acc, b) * g).sum().backward()
    want = -(g * b).sum(-1)
    assert torch.allclose(acc.grad, want, rtol=1e-14, atol=0)
    # the float32 restatement of fastnerf_bkgd_grad is that number, to the roundings of three products and two sums
    got, none = B.grad(b.numpy(), g.numpy())
    assert none is None and got.dtype == F32
    bound = 8 * 2.0 ** -24 * (g.abs() * b).sum(-1).numpy()
    assert (np.abs(got.astype(np.float64) - want.numpy()) <= bound).all()
    add = torch.randn(n, generator=gen).numpy()
    with_add, with_add0 = B.grad(b.numpy(), g.numpy(), g.numpy(), add, add)
    assert np.array_equal(with_add, (add + got).astype(F32)) and np.array_equal(with_add, with_add0)      # add - x == add + (-x)
    detached = torch.autograd.grad((B.blend_torch(rgb, acc, b, detach_acc=True) * g).sum() + 0 * acc.sum(), acc)[0]
    assert (detached == 0).all()


def test_white_is_the_loaders_composite_bit_for_bit():
    rs = np.random.RandomState(2)
    n = 1000
    rgb, a = rs.rand(n, 3).astype(F32), rs.rand(n).astype(F32)
    a[:5] = [0, 1, 0.5, 0, 1]
    acc = rs.rand(n).astype(F32)
    ones = np.ones((n, 3), F32)
    out1, out0, tout, used = B.blend(rgb, acc, rgb, bkgd=ones, alpha=a, rgb0=rgb, acc0=a)
    loader = rgb * a[:, None] + (1. - a[:, None])       # run_nerf.load_dataset, white_bkgd
    assert loader.dtype == F32 and np.array_equal(tout.view(np.int32), loader.view(np.int32))
    white = rgb + (F32(1) - acc)[:, None]               # the white branch of raw2outputs: rgb + (1 - acc)
    assert np.array_equal(out1.view(np.int32), white.astype(F32).view(np.int32))
    assert np.array_equal(out0, (rgb + (F32(1) - a)[:, None]).astype(F32)) and np.array_equal(used, ones)
    # without an alpha the target keeps its bits; a transparent pixel becomes the colour, an opaque one stays
    b = rs.rand(n, 3).astype(F32)
    _, _, t_plain, _ = B.blend(rgb, acc, rgb, bkgd=b)
    assert np.array_equal(t_plain.view(np.int32), rgb.view(np.int32))
    _, _, t_b, _ = B.blend(rgb, acc, rgb, bkgd=b, alpha=a)
    assert np.array_equal(t_b[0], b[0]) and np.array_equal(t_b[1], rgb[1])


def test_the_bkgd_stream():
    import march_train_numpy as MT
    words = [getattr(P, k) for k in ('COAR', 'FGDP', 'PRTB', 'PDFS', 'NOIS', 'OCCG', 'EPIX')] + [MT.MRCH]
    assert B.BKGD == int.from_bytes(b'bkgd', 'big') == 0x626b6764 and B.BKGD not in words
    a, b = B.draw(1000, 1), B.draw(1000, (1 << 40) + 1)
    for x in (a, b):
        assert x.dtype == F32 and x.shape == (1000, 3) and x.min() >= 0 and x.max() < 1 and 0.45 < x.mean() < 0.55
    assert (a != b).mean() > 0.99 and np.array_equal(B.draw(10, 1), a[:10]), 'the counter is the ray: a prefix is a prefix'
    assert not np.array_equal(a[:, 0], MT.draw_u(1000, 1)), 'a stream of its own'
    w = P.stream_words(B.BKGD, np.arange(1000, dtype=P.U64), 1)
    assert np.array_equal(a[:, 2], P.u01(w[2]))
    with pytest.raises(AssertionError):
        B.blend(a, a[:, 0], a)            # neither colours nor a seed
    with pytest.raises(AssertionError):
        B.blend(a, a[:, 0], a, bkgd=a, seed=3)


def _step_args(**over):
    from fastnerf import _lib
    a = _lib.StepArgs()
    a.n, a.net_floats, a.math_mode, a.N_samples, a.N_importance, a.live, a.adam_t = 4, 1000, 0, 8, 8, 1, 1
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _bk(**over):
    from fastnerf import _lib
    k = _lib.StepBkgd()
    k.bkgd, k.seed, k.bkgd_used, k.target_ws, k.g_acc1, k.g_acc0 = 16, 0, 16, 16, 16, 16      # never dereferenced
    for name, v in over.items():
        setattr(k, name, v)
    return k


def test_argument_checks_come_before_any_launch():
    """On a host without a GPU a launch fails with -2, an argument check with -1: the refusals touch no pointer (every buffer of
    fn_step_args is NULL here) and come first."""
    from fastnerf import _lib
    lib = _lib.lib()
    assert lib.fastnerf_step_bkgd_size() == C.sizeof(_lib.StepBkgd) == 56
    assert lib.fastnerf_step_args_size() == C.sizeof(_lib.StepArgs) == 512, 'fn_step_args does not grow'
    one = C.c_void_p(16)
    # fastnerf_bkgd_blend: exactly one of bkgd / seed
    blend = lambda n, bkgd, seed: lib.fastnerf_bkgd_blend(n, bkgd, seed, None, one, None, one, None, one, one, one, None)      # noqa: E731
    for n in (0, 4):
        assert blend(n, one, 5) == -1 and lib.fastnerf_last_error().startswith(b'fastnerf_bkgd_blend:')
        assert blend(n, None, 0) == -1 and lib.fastnerf_last_error().startswith(b'fastnerf_bkgd_blend:')
    assert blend(0, one, 0) == 0 and blend(0, None, 1 << 40) == 0, 'no rays, no work'
    assert blend(-1, one, 0) == -1
    assert lib.fastnerf_bkgd_blend(4, one, 0, None, None, None, one, None, one, one, one, None) == -1
    assert lib.fastnerf_bkgd_blend(4, one, 0, None, one, None, one, one, one, one, one, None) == -1, 'rgb0 without acc0'
    assert lib.fastnerf_bkgd_grad(0, None, None, None, None, None, None, None, None) == 0
    assert lib.fastnerf_bkgd_grad(4, one, one, one, None, None, one, None, None) == -1, 'g_rgb0 without g_acc0'
    assert lib.fastnerf_bkgd_grad(4, None, one, None, None, None, one, None, None) == -1
    assert lib.fastnerf_bkgd_grad(-1, one, one, None, None, None, one, None, None) == -1
    # the two steps: white_bkgd with bk, a null member of bk, both / neither of bkgd and seed -- under their own names
    x = _lib.StepMarch()
    x.K, x.C, x.which = 64, 16, 1
    fused = lambda a, k, ph=15: lib.fastnerf_train_step_bkgd(C.byref(a), None, C.byref(k), ph, None)                  # noqa: E731
    march = lambda a, k, ph=15: lib.fastnerf_train_step_march_bkgd(C.byref(a), C.byref(x), C.byref(k), ph, None)      # noqa: E731
    for call, prefix in ((fused, b'fastnerf_train_step_bkgd:'), (march, b'fastnerf_train_step_march_bkgd:')):
        assert call(_step_args(white_bkgd=1), _bk()) == -1
        msg = lib.fastnerf_last_error()
        assert msg.startswith(prefix) and b'white_bkgd' in msg, msg
        members = ['bkgd_used', 'target_ws', 'g_acc1'] + (['g_acc0'] if call is fused else [])
        for member in members:
            assert call(_step_args(), _bk(**{member: None})) == -1, member
            msg = lib.fastnerf_last_error()
            assert msg.startswith(prefix) and b'null member' in msg, (member, msg)
        for kw in (dict(bkgd=None, seed=0), dict(bkgd=16, seed=7)):
            assert call(_step_args(), _bk(**kw)) == -1, kw
            msg = lib.fastnerf_last_error()
            assert msg.startswith(prefix) and b'exactly one' in msg, (kw, msg)
        # a backward phase needs its g_acc row and nothing of the forward's; the update phase needs none of bk
        assert call(_step_args(), _bk(g_acc1=None), 4) == -1 and lib.fastnerf_last_error().startswith(prefix + b' null member')
        assert call(_step_args(), _bk(bkgd_used=None, target_ws=None, bkgd=None), 4) == -1
        assert b'null member' not in lib.fastnerf_last_error() and lib.fastnerf_last_error().startswith(prefix), 'the step\'s own checks, by name'
    # one pass: g_acc0 is not needed
    assert fused(_step_args(N_importance=0), _bk(g_acc0=None)) == -1 and b'null member' not in lib.fastnerf_last_error()
    # bk == NULL: the entry points without _bkgd, by name
    a = _step_args()
    assert lib.fastnerf_train_step_bkgd(C.byref(a), None, None, 15, None) == -1
    assert lib.fastnerf_last_error().startswith(b'fastnerf_train_step:')
    assert lib.fastnerf_train_step_march_bkgd(C.byref(a), C.byref(x), None, 15, None) == -1
    assert lib.fastnerf_last_error().startswith(b'fastnerf_train_step_march:')


def test_backward_and_update_refusals_come_before_the_forward():
    """A call with every phase: the null gradient buffer of a depth / opacity term (a backward phase's check) and the missing Adam
    state (the update phase's) are refused under the entry point's own name before the forward launches -- on a host without a GPU a
    launch would return -2, and the batch buffers are NULL here."""
    from fastnerf import _lib
    lib = _lib.lib()
    nets = dict(params=16, grads=16, packed_fwd_c=16, packed_bwd_c=16, packed_fwd_f=16, packed_bwd_f=16, live=0)
    aux = _lib.StepAux()
    aux.depth_target = 16
    a = _step_args(adam_m=16, adam_v=16, **nets)
    assert lib.fastnerf_train_step_bkgd(C.byref(a), C.byref(aux), C.byref(_bk()), 15, None) == -1
    assert lib.fastnerf_last_error().startswith(b'fastnerf_train_step_bkgd: null gradient buffer of a term'), lib.fastnerf_last_error()
    assert lib.fastnerf_train_step_aux(C.byref(a), C.byref(aux), 15, None) == -1
    assert lib.fastnerf_last_error().startswith(b'fastnerf_train_step_aux: null gradient buffer of a term'), lib.fastnerf_last_error()
    aux.acc_target, aux.g_depth1, aux.g_depth0 = 16, 16, 16      # with a background the opacity term's rows are needed in the forward
    assert lib.fastnerf_train_step_bkgd(C.byref(a), C.byref(aux), C.byref(_bk()), 15, None) == -1
    assert lib.fastnerf_last_error().startswith(b'fastnerf_train_step_bkgd: null gradient buffer of the opacity term')
    assert lib.fastnerf_train_step_bkgd(C.byref(a), C.byref(aux), C.byref(_bk()), 6, None) == -1
    assert lib.fastnerf_last_error().startswith(b'fastnerf_train_step_bkgd: null gradient buffer of a term')
    a = _step_args(**nets)
    assert lib.fastnerf_train_step_bkgd(C.byref(a), None, C.byref(_bk()), 15, None) == -1
    assert lib.fastnerf_last_error().startswith(b'fastnerf_train_step_bkgd: update phase needs'), lib.fastnerf_last_error()


def test_refusals_that_need_no_device():
    """The ValueErrors of the Trainer's background (Trainer._bkgd_terms reads `bkgd` and `white_bkgd` of the trainer, nothing else) and
    of render_rays come before anything asks for a GPU."""
    import types
    import fastnerf as fn
    terms = fn.run_nerf.Trainer._bkgd_terms
    S = lambda bkgd, white=False: types.SimpleNamespace(bkgd=bkgd, white_bkgd=white)      # noqa: E731
    e3, e1 = torch.zeros(4, 3), torch.zeros(4)
    assert terms(S(None), 4, 'cpu', None, None) is None, 'no background: nothing'
    with pytest.raises(ValueError, match='alpha'):
        terms(S(None), 4, 'cpu', e1, None)
    for setting in ('random', (0.5, 0.5, 0.5)):
        with pytest.raises(ValueError, match='white_bkgd'):
            terms(S(setting, True), 4, 'cpu', e1, None)
    with pytest.raises(ValueError, match='white_bkgd'):
        terms(S(None, True), 4, 'cpu', None, e3)
    with pytest.raises(ValueError, match='random'):
        terms(S('blue'), 4, 'cpu', None, None)
    ktr = fn.run_nerf.create_nerf(fn.run_nerf.make_args(N_importance=8, N_samples=8, use_viewdirs=True, no_reload=True), device='cpu')[0]
    with pytest.raises(ValueError, match='white_bkgd'):
        fn.render.render_rays(torch.zeros(4, 11), ktr['network_fn'], None, 8, white_bkgd=True, bkgd=torch.ones(3))


def test_python_surface():
    import inspect
    from fastnerf import ops, render, run_nerf, tree
    assert callable(ops.bkgd_blend) and callable(ops.bkgd_grad)
    assert inspect.signature(run_nerf.Trainer.__init__).parameters['bkgd'].default is None
    for f in (run_nerf.Trainer.step, run_nerf.Trainer.forward_backward, run_nerf.Trainer._fused_prepare, run_nerf.Trainer._march_prepare):
        sig = inspect.signature(f).parameters
        assert sig['alpha'].default is None and sig['bkgd'].default is None
    assert inspect.signature(render.render_rays).parameters['bkgd'].default is None
    assert inspect.signature(tree.QuadTreeManager.gen_rays_v3_multiThread).parameters['want_pix'].default is False
    assert run_nerf.make_args().random_bkgd is False


def test_load_dataset_keeps_alpha_under_the_flag(golden_dir, tmp_path):
    PIL = pytest.importorskip('PIL.Image')
    import fastnerf
    g = np.load(os.path.join(golden_dir, 'g15_loaders.npz'))
    d = str(tmp_path / 'blender')
    for split in ('train', 'val', 'test'):
        os.makedirs(os.path.join(d, split))
        imgs, mats = g['blender.%s.imgs' % split], g['blender.%s.mats' % split]
        frames = []
        for i in range(imgs.shape[0]):
            PIL.fromarray(imgs[i], 'RGBA').save(os.path.join(d, split, 'r_%d.png' % i))
            frames.append({'file_path': './%s/r_%d' % (split, i), 'transform_matrix': mats[i].tolist()})
        json.dump({'camera_angle_x': float(g['blender.%s.angle' % split]), 'frames': frames},
                  open(os.path.join(d, 'transforms_%s.json' % split), 'w'))
    rgba = g['blender.out1.imgs']
    A = lambda **kw: fastnerf.run_nerf.make_args(dataset_type='blender', datadir=d, half_res=False, testskip=1, **kw)      # noqa: E731
    ds = fastnerf.run_nerf.load_dataset(A(random_bkgd=True))
    assert ds['images'].shape == rgba.shape and ds['images'].shape[-1] == 4 and np.array_equal(ds['images'], rgba)
    assert ds['poses'].shape == (12, 3, 4) and (ds['near'], ds['far']) == (2., 6.)
    # without the flag (absent or False): what it always returned
    for kw in (dict(), dict(random_bkgd=False)):
        assert np.array_equal(fastnerf.run_nerf.load_dataset(A(**kw))['images'], rgba[..., :3])
        white = fastnerf.run_nerf.load_dataset(A(white_bkgd=True, **kw))['images']
        assert np.array_equal(white, rgba[..., :3] * rgba[..., -1:] + (1. - rgba[..., -1:]))
    with pytest.raises(ValueError, match='random_bkgd'):
        fastnerf.run_nerf.load_dataset(A(random_bkgd=True, white_bkgd=True))
