"""Early ray termination without a GPU: the float64 restatement (tests/ert_numpy.py) against the oracle's compositing, the new
C-ABI symbols and their argument checks, the Python surface, and the scene of tests/test_gpu_ert.py validated on the CPU oracle
alone -- it terminates, it saves what the GPU test expects it to save, and no decision sits where the GPU's expf could flip it."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ert_numpy as E
import occ_numpy as R
from fastnerf import _lib
from oracle import nerf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('fastnerf_ert_classify', 'fastnerf_ert_advance', 'fastnerf_render_rays_fwd_ert')


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------
def _random_pass(n, S, seed):
    rs = np.random.RandomState(seed)
    raw = (rs.randn(n, S, 4) * 3).astype(np.float32)
    raw[rs.rand(n, S) < 0.1, 3] = 1e4      # huge sigma
    z = np.sort(2.0 + 4.0 * rs.rand(n, S).astype(np.float32), -1)
    rays = np.zeros((n, 11), np.float32)
    rays[:, 3:6] = rs.randn(n, 3)
    return raw, z, rays


@pytest.mark.parametrize('B', [1, 5, 16, 64])
def test_chained_segments_are_the_transmittance_of_raw2outputs(B):
    n, S = 23, 37
    raw, z, rays = _random_pass(n, S, B)
    _, _, acc, w, _ = O.raw2outputs(torch.from_numpy(raw).double(), torch.from_numpy(z).double(), torch.from_numpy(rays[:, 3:6]).double())
    w64 = E.weights64(raw, z, rays)
    np.testing.assert_allclose(w64, w.numpy(), rtol=1e-12, atol=1e-300)
    T = np.ones(n)
    for s0, s1 in E.segments(S, B):
        T = E.advance(T, raw, z, rays, s0, s1)
    # sum of the weights = 1 - prod (1 - alpha) up to the 1e-10 terms
    np.testing.assert_allclose(1.0 - T, acc.numpy(), atol=S * 2e-10)
    assert E.segments(7, 2) == [(0, 2), (2, 4), (4, 6), (6, 7)] and E.segments(7, 7) == [(0, 7)] and E.segments(7, 100) == [(0, 7)]


def test_classify_compares_in_float32_and_ands_the_bits():
    eps = np.float32(1e-2)
    trans = np.array([1.0, eps, np.nextafter(eps, np.float32(1)), np.nextafter(eps, np.float32(0)), 0.0, np.nan], np.float32)
    bits = np.random.RandomState(0).rand(6, 9) < 0.5
    keep = E.classify(trans, eps, 9, 3, 7, bits)
    assert keep.shape == (6, 4) and np.array_equal(keep, np.array([1, 0, 1, 0, 0, 0], bool)[:, None] & bits[:, 3:7])
    assert np.array_equal(E.classify(None, eps, 9, 0, 9, bits), bits) and E.classify(trans, eps, 9, 0, 2).all(-1).tolist() == [True, False, True, False, False, False]
    assert np.array_equal(E.live_list(keep, 9, 3), np.nonzero(np.pad(keep, ((0, 0), (3, 2))).reshape(-1))[0])


def test_terminate_is_classify_and_advance_chained():
    n, S, B, eps = 31, 29, 4, 1e-2
    raw, z, rays = _random_pass(n, S, 3)
    bits = np.random.RandomState(1).rand(n, S) < 0.7
    raw = raw * bits[..., None]
    t = E.terminate(raw, z, rays, eps, B, bits)
    T = np.ones(n)
    for k, (s0, s1) in enumerate(E.segments(S, B)):
        keep = (T > float(np.float32(eps)))[:, None] & bits[:, s0:s1]
        assert np.array_equal(t['keep'][:, s0:s1], keep) and np.array_equal(t['t_start'][:, k], T)
        T = E.advance(T, raw * t['keep'][..., None], z, rays, s0, s1)
    assert np.array_equal(t['t_final'], T)
    assert 0 < t['keep'].sum() < bits.sum(), 'some rays terminate, some samples remain'
    # the skipped samples of a ray weigh at most its T at the start of the first skipped segment
    w = E.weights64(raw, z, rays)
    assert ((w * ~t['keep']).sum(-1) <= float(np.float32(eps)) * (1 + S * 1e-10)).all()
    one = E.terminate(raw, z, rays, eps, S, bits)
    assert np.array_equal(one['keep'], bits), 'one segment: nothing is skipped'


# ---- 2. the C ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, 'include', 'fastnerf.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    lib = _lib.lib()
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, src), name + ' is not declared in fastnerf.h'
        assert hasattr(lib, name), name + ' is not exported'
        assert name in _lib.SIGNATURES
    I, L, P, F = C.c_int, C.c_int64, C.c_void_p, C.c_float
    G, K = C.POINTER(_lib.OccGrid), C.POINTER(_lib.OccCascade)
    # grid, cascade, n, S, s0, s1, rays11, z, trans, eps, live_idx, count_out, raw, ws, stream
    assert _lib.SIGNATURES['fastnerf_ert_classify'] == (I, [G, K, L, I, I, I, P, P, P, F, P, P, P, P, P])
    # n, S, s0, s1, raw, z, rays11, first, trans, seg_count, total, stream
    assert _lib.SIGNATURES['fastnerf_ert_advance'] == (I, [L, I, I, I, P, P, P, I, P, P, P, P])
    # the arguments of fastnerf_render_rays_fwd_occ with (grid, cascade, eps, block, trans_ws) where its grid is
    res, occ = _lib.SIGNATURES['fastnerf_render_rays_fwd_occ']
    k = occ.index(G)
    assert _lib.SIGNATURES['fastnerf_render_rays_fwd_ert'] == (res, occ[:k] + [G, K, F, I, P] + occ[k + 1:])


def test_existing_structs_and_signatures_keep_their_sizes():
    lib = _lib.lib()
    assert C.sizeof(_lib.OccGrid) == 48 and C.sizeof(_lib.OccCascade) == 8 + 8 * 48
    assert lib.fastnerf_step_args_size() == C.sizeof(_lib.StepArgs) == 512, 'the training step does not learn about ert'
    assert not any(f[0].startswith('ert') for f in _lib.StepArgs._fields_)


def _ert_args(n=4, NS=8, NI=8, eps=1e-2, block=4, grid=None, cascade=None, null=()):
    one = C.c_void_p(16)      # never dereferenced: the call fails on its arguments
    p = lambda k: None if k in null else one      # noqa: E731
    head = [0, n, NS, NI, p('rays11'), 0, 0, 1, 0, None, None, 0, 0, p('params_c'), p('packed_c'), p('params_f'), p('packed_f')]
    outs = [p(k) for k in ('z0', 'raw0', 'rgb0', 'disp0', 'acc0', 'w0', 'depth0', 'z1', 'z_samples', 'z_std', 'raw1', 'rgb1', 'disp1',
                           'acc1', 'w1', 'depth1')]
    return head + [grid, cascade, eps, block, p('trans_ws'), p('live_ws'), p('counts')] + outs + [0, None]


def test_argument_checks_come_before_any_launch():
    """Every one of these calls would enqueue the coarse sampler first if its check came late: on a host without a GPU that launch
    fails with -2, an argument check with -1."""
    lib = _lib.lib()
    f = lib.fastnerf_render_rays_fwd_ert
    for kw, word in ((dict(eps=1.0), b'eps'), (dict(eps=-1e-3), b'eps'), (dict(eps=float('nan')), b'eps'), (dict(block=0), b'block'),
                     (dict(null=('trans_ws',)), b'null'), (dict(null=('live_ws',)), b'null'), (dict(null=('counts',)), b'null'),
                     (dict(null=('raw1',)), b'fine'), (dict(null=('params_f',)), b'fine'), (dict(n=2 ** 24, NS=64, NI=64), b'2^31'),
                     (dict(grid=C.pointer(_lib.OccGrid()), cascade=C.pointer(_lib.OccCascade())), b'at most one'),
                     (dict(cascade=C.pointer(_lib.OccCascade())), b'levels'), (dict(grid=C.pointer(_lib.OccGrid())), b'words')):
        assert f(*_ert_args(**kw)) == -1, kw
        assert word in lib.fastnerf_last_error(), (kw, lib.fastnerf_last_error())
    assert f(*_ert_args(n=0)) == 0      # an empty batch is no error, as in the other forward entry points
    one = C.c_void_p(16)
    cl = lambda **k: lib.fastnerf_ert_classify(k.get('grid'), k.get('cascade'), k.get('n', 4), k.get('S', 8), k.get('s0', 0), k.get('s1', 4),      # noqa: E731
                                               one, one, one, k.get('eps', 1e-2), k.get('idx', one), one, one, one, None)
    for kw in (dict(eps=1.0), dict(eps=-1.0), dict(s0=4, s1=4), dict(s1=9), dict(s0=-1), dict(n=0), dict(n=2 ** 28), dict(idx=None),
               dict(grid=C.pointer(_lib.OccGrid())), dict(cascade=C.pointer(_lib.OccCascade())),
               dict(grid=C.pointer(_lib.OccGrid()), cascade=C.pointer(_lib.OccCascade()))):
        assert cl(**kw) == -1, kw
    ad = lambda **k: lib.fastnerf_ert_advance(k.get('n', 4), k.get('S', 8), k.get('s0', 0), k.get('s1', 4), one, one, one, 0,      # noqa: E731
                                              k.get('trans', one), k.get('seg'), k.get('total'), None)
    for kw in (dict(s0=4, s1=4), dict(s1=9), dict(S=513, s1=513), dict(n=0), dict(trans=None), dict(total=one)):
        assert ad(**kw) == -1, kw


# ---- 3. the Python surface -------------------------------------------------------------------------------------------------------
def test_python_surface():
    from fastnerf import ops, render
    sig = inspect.signature(render.render_rays).parameters
    names = list(sig)
    assert names[-3:] == ['retdepth', 'ert', 'ert_block'], names      # appended, with defaults
    assert sig['ert'].default is None and sig['ert_block'].default == 32
    assert callable(render._forward_ert) and callable(ops.ert_classify) and callable(ops.ert_advance) and callable(ops.render_rays_fwd_ert)
    doc = render.render_rays.__doc__
    assert 'ert' in doc and 'disp_map' in doc and 'NO such bound' in doc
    for bad in ((1.0, 32), (-0.1, 32), (float('nan'), 32), (1e-2, 0), (1e-2, 2.5)):
        with pytest.raises(ValueError):
            ops.check_ert(*bad)
    assert ops.check_ert(0, 1) == (0.0, 1) and ops.check_ert(1e-2, 64) == (float(np.float32(1e-2)), 64)


# ---- 4. the scene of the GPU tests, on the oracle alone -------------------------------------------------------------------------
@functools.lru_cache(None)
def scene(case):
    """case: 'plain' / 'ball' (64 + 128 samples) or 'one' (one pass of 192 samples) -> (raw, z, rays, bits, occupied share)."""
    rays = E.scene_rays(O)
    sdc, sdf = E.scene_networks(O)
    grid = R.scene_grids()['ball'] if case == 'ball' else None
    with torch.no_grad():
        raw, z, bits = E.oracle_pass(O, rays, sdc, sdf, grid, 192 if case == 'one' else E.NS, 0 if case == 'one' else E.NI)
    return raw, z, rays, bits, (1.0 if bits is None else float(bits.mean()))


def test_oracle_pass_is_the_masked_render_of_occ_numpy():
    rays = E.scene_rays(O)
    sdc, sdf = E.scene_networks(O)
    m, lo, hi, oo = R.scene_grids()['ball']
    with torch.no_grad():
        ref = R.render_rays_masked(O, rays, sdc, sdf, m, lo, hi, oo, E.NS, E.NI)
    raw, z, _, bits, _ = scene('ball')
    assert rays.shape == (169, 11) and z.shape == (169, 192)
    assert np.array_equal(bits, ref['bits1']) and np.array_equal(raw, ref['raw1'].numpy())


@pytest.mark.parametrize('case', ['plain', 'one'])
def test_every_ray_of_the_scene_terminates(case):
    raw, z, rays, _, _ = scene(case)
    T = E.terminate(raw, z, rays, 0.0, 16)['t_final']
    print('%s: largest final T = %.3g' % (case, T.max()))
    assert (T <= 1e-2).all()      # (a)


def test_evaluated_shares():
    share = {}
    for case in ('plain', 'ball', 'one'):
        raw, z, rays, bits, occ = scene(case)
        share[case] = (float(E.terminate(raw, z, rays, 1e-2, 16, bits)['keep'].mean()), occ)
        print('%s: evaluated share of the image pass at B = 16, eps = 1e-2: %.3f (occupied %.3f)' % ((case,) + share[case]))
    assert share['plain'][0] <= 0.75                          # (b)
    assert share['ball'][0] < share['ball'][1] < 1.0          # (b), with the grid
    assert share['one'][0] <= 0.25                            # (c)


@pytest.mark.parametrize('case', ['plain', 'ball', 'one'])
def test_no_decision_sits_on_the_threshold_and_the_bound_holds(case):
    raw, z, rays, bits, _ = scene(case)
    w = E.weights64(raw, z, rays)
    for eps in (1e-3, 1e-2):
        e = float(np.float32(eps))
        for B in (16, 32, 48):
            t = E.terminate(raw, z, rays, eps, B, bits)
            gap = np.abs(t['t_start'] / e - 1.0).min()
            skipped = (w * ~t['keep']).sum(-1).max()
            print('%s eps %g B %d: closest segment-start T to eps: relative %.3g; largest skipped weight %.3g' % (case, eps, B, gap, skipped))
            assert gap > 1e-3                                 # (d)
            assert skipped <= e                               # (e)
            assert 0 < t['keep'].sum() < (z.size if bits is None else bits.sum())
