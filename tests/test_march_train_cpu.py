"""Marched training without a device: the restatement of the jittered lattice (tests/march_train_numpy.py) against the unshifted one of
tests/march_numpy.py and against its own contract, the 'mrch' draw, the overflow mask, and the argument checks of the library and of
run_nerf.Trainer that come before anything touches a GPU."""
import types

import numpy as np
import pytest

import march_numpy as M
import march_train_numpy as MT
import occ_numpy as R
from oracle import nerf_oracle as O

F32 = np.float32
SCENES = ['ball', 'random', 'two_shells', 'cascade']
SHAPES = [(13, 5), (64, 32), (256, 64)]


@pytest.fixture(scope='module')
def rays():
    return R.scene_rays(O, side=10)      # 100 rays


@pytest.mark.parametrize('name', SCENES)
@pytest.mark.parametrize('K,C', SHAPES)
@pytest.mark.parametrize('lindisp', [False, True])
def test_zero_shift_is_the_unshifted_march(rays, name, K, C, lindisp):
    grid = M.scene_grids()[name]
    zlat = M.lattice(rays, K, lindisp)
    zu = MT.jittered_lattice(rays, K, np.zeros(rays.shape[0], F32), lindisp)
    assert np.array_equal(zu.view(np.int32), zlat.view(np.int32)), 'u = 0: every depth has the bits of the lattice, z_K included'
    want = M.march(M.live_bits(grid, rays, zlat[:, :K]), zlat, C)
    for B in (None, 2, 16):
        got, _ = MT.march(grid, rays, K, C, np.zeros(rays.shape[0], F32), lindisp, B)
        for g, w, what in zip(got, want, ('z', 'kidx', 'overflow', 'state')):
            assert np.array_equal(g, w), (what, B)
    assert (want[1] >= 0).any()


@pytest.mark.parametrize('name', SCENES)
@pytest.mark.parametrize('K,C', SHAPES)
@pytest.mark.parametrize('lindisp', [False, True])
def test_shifted_rows_are_ordered_and_stay_inside_their_lattice_interval(rays, name, K, C, lindisp):
    grid = M.scene_grids()[name]
    n = rays.shape[0]
    u = np.random.RandomState(K + C).rand(n).astype(F32)
    u[:3] = [0.0, np.nextafter(F32(1), F32(0)), 0.5]
    assert u.min() >= 0 and u.max() < 1
    zlat, zu = M.lattice(rays, K, lindisp), MT.jittered_lattice(rays, K, u, lindisp)
    if not lindisp:      # z_k <= z_k(u) <= z_{k+1}
        assert (zlat[:, :K] <= zu[:, :K]).all() and (zu[:, :K] <= zlat[:, 1:]).all()
    assert (np.diff(zu, axis=1) >= 0).all(), 'the shifted lattice is non-decreasing, its closing depth included'
    (z, kidx, overflow, _), live = MT.march(grid, rays, K, C, u, lindisp)
    assert (np.diff(z, axis=1) >= 0).all(), 'z is non-decreasing along a row'
    # the rows are the contract's (march_numpy.packed) on the shifted lattice, and rounds reproduce the single round
    cz, ck, co = M.packed(live, zu, C)
    assert np.array_equal(z.view(np.int32), cz.view(np.int32)) and np.array_equal(kidx, ck) and np.array_equal(overflow.astype(bool), co)
    for B in (2, 16):
        again, _ = MT.march(grid, rays, K, C, u, lindisp, B)
        assert all(np.array_equal(a, b) for a, b in zip(again[:3], (z, kidx, overflow)))
    # a live slot holds the shifted depth of its lattice point, a closing entry that of the next one
    r, s = np.nonzero(kidx >= 0)
    assert np.array_equal(z[r, s], zu[r, kidx[r, s]])
    close = (kidx[:, 1:] < 0) & (kidx[:, :-1] >= 0)
    r, s = np.nonzero(close)
    assert r.size and np.array_equal(z[r, s + 1], zu[r, kidx[r, s] + 1])
    assert (kidx >= 0).any()


def test_the_mrch_draws():
    a, b = MT.draw_u(1000, 1), MT.draw_u(1000, 2)
    for u in (a, b):
        assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1
        assert 0.4 < u.mean() < 0.6 and np.unique(u).size > 990
    assert (a != b).mean() > 0.99
    assert np.array_equal(MT.draw_u(10, 1), a[:10]), 'the counter is the ray: a prefix is a prefix'
    import philox_numpy as P
    assert not np.array_equal(a, P.stream_u(P.COAR, (1000,), 1)), "a stream of its own"
    assert MT.MRCH == int.from_bytes(b'mrch', 'big')
    with pytest.raises(AssertionError):
        MT.draw_u(4, 0)


def test_the_mask():
    g = np.random.RandomState(0).randn(7, 3).astype(F32)
    ov = np.array([0, 1, 0, 0, 2, 0, 1], np.uint8)
    m = MT.mask(ov, g)
    assert (m[ov != 0] == 0).all() and np.array_equal(m[ov == 0].view(np.int32), g[ov == 0].view(np.int32))
    assert np.array_equal(MT.mask(np.zeros(7, np.uint8), g), g)


# ---- the library's argument checks and the Python surface (no device needed) ---------------------------------------------------------
def _good_grid():
    import ctypes as C
    from fastnerf import _lib
    return _lib.OccGrid(16, (C.c_float * 3)(-1.5, -1.5, -1.5), (C.c_float * 3)(8.0, 8.0, 8.0), (C.c_int32 * 3)(24, 24, 24), 0)      # words never read


def test_argument_checks_come_before_any_launch():
    """On a host without a GPU a launch fails with -2, an argument check with -1: every check precedes the first launch."""
    import ctypes as C
    from fastnerf import _lib
    lib = _lib.lib()
    assert lib.fastnerf_step_march_size() == C.sizeof(_lib.StepMarch)
    one = C.c_void_p(16)      # never dereferenced
    grid = C.pointer(_good_grid())

    def march(n=4, K=64, cap=16, s0=0, s1=16, first=1, grid=grid, cascade=None, trans=None, eps=0.0, state=one, u=one, seed=0):
        return lib.fastnerf_occ_march_jitter(grid, cascade, n, K, 0, one, cap, s0, s1, first, trans, eps, u, seed, state, one, one, one, None)

    for src in (dict(), dict(u=None, seed=5), dict(u=None, seed=0)):
        for kw in (dict(K=1), dict(K=1 << 24), dict(cap=1), dict(cap=513, s1=513), dict(s1=17), dict(s0=4, s1=4), dict(s0=-1),
                   dict(s0=4, first=1), dict(first=0), dict(n=-1), dict(n=1 << 23, cap=256, s1=256), dict(grid=None),
                   dict(cascade=C.pointer(_lib.OccCascade())), dict(grid=C.pointer(_lib.OccGrid())), dict(trans=one, eps=1.0),
                   dict(trans=one, eps=-1.0), dict(state=None)):
            assert march(**dict(src, **kw)) == -1, (src, kw)
        assert march(n=0, **src) == 0
    assert lib.fastnerf_march_mask(-1, one, one, None) == -1 and lib.fastnerf_march_mask(4, None, one, None) == -1
    assert lib.fastnerf_march_mask(4, one, None, None) == -1 and lib.fastnerf_march_mask(0, None, None, None) == 0
    assert lib.fastnerf_step_march_ws_ints(0, 16) == -1 and lib.fastnerf_step_march_ws_ints(4, 513) == -1
    assert lib.fastnerf_step_march_ws_ints(4, 16) == 4 * 16 + lib.fastnerf_compact_ws_ints(4 * 16) + 2 + 2 * 4

    def step(phases=15, march=True, **over):
        a, x = _lib.StepArgs(), _lib.StepMarch()
        for k, t in _lib.StepArgs._fields_:
            if t is _lib.P and k not in ('t_rand', 'u', 'noise0', 'noise1', 'leaf_tag', 'table', 'occ', 'occ_counts'):
                setattr(a, k, 16)
        a.n, a.net_floats, a.math_mode, a.live, a.adam_t = 4, 1000, 0, 1, 1
        a.occ = C.addressof(grid.contents)
        x.K, x.C, x.which, x.kidx, x.overflow, x.list_ws, x.counts = 64, 16, 1, 16, 16, 16, 16
        for k, v in over.items():
            setattr(x if k in ('K', 'C', 'which', 'kidx', 'overflow', 'list_ws', 'counts') else a, k, v)
        return lib.fastnerf_train_step_march(C.byref(a), C.byref(x) if march else None, phases, None)

    bad_grid = _lib.OccGrid()
    for kw, word in ((dict(occ=None), b'occ'), (dict(live=0), b'live'), (dict(noise0=16), b'noise'), (dict(noise1=16), b'noise'),
                     (dict(K=1), b'K'), (dict(K=1 << 24), b'K'), (dict(C=1), b'C'), (dict(C=513), b'C'), (dict(n=1 << 23, C=256), b'2^31'),
                     (dict(n=1 << 20, K=1 << 12), b'2^31'), (dict(which=2), b'which'), (dict(which=-1), b'which'), (dict(math_mode=3), b'math_mode'),
                     (dict(n=0), b'n > 0'), (dict(march=False), b'march'), (dict(occ=C.addressof(bad_grid)), b'words'),
                     (dict(kidx=None), b'null'), (dict(overflow=None), b'null'), (dict(list_ws=None), b'null'), (dict(counts=None), b'null'),
                     (dict(z0=None), b'null'), (dict(raw0=None), b'null'), (dict(g_rgb=None), b'null'), (dict(packed_fwd_f=None), b'null'),
                     (dict(packed_bwd_f=None), b'null'), (dict(params=None), b'null'), (dict(grads=None), b'null'),
                     (dict(phases=1, target=None), b'null'), (dict(phases=1, w0=None), b'null'), (dict(phases=1, loss2=None), b'null'),
                     (dict(phases=4, live_ws=None), b'null'), (dict(phases=4, act_ws=None), b'null'), (dict(phases=4, draw_ws=None), b'null'),
                     (dict(phases=8, adam_m=None), b'adam'), (dict(phases=8, adam_t=0), b'adam')):
        assert step(**kw) == -1, kw
        msg = lib.fastnerf_last_error()
        assert msg.startswith(b'fastnerf_train_step_march:') and word in msg, (kw, msg)
    # the unmarched half may be absent, a phase that is not asked for needs none of its buffers, and no phase is no launch
    assert step(phases=0, packed_fwd_c=None, packed_bwd_c=None, target=None, live_ws=None, adam_m=None) == 0
    assert step(phases=2) == 0, 'FN_STEP_BWD_FINE is a no-op'


def _cpu_networks(fn, **over):
    kw = dict(N_importance=8, N_samples=8, use_viewdirs=True, no_reload=True)
    kw.update(over)
    return fn.run_nerf.create_nerf(fn.run_nerf.make_args(**kw), device='cpu')[0]


def test_trainer_refusals_that_need_no_device(monkeypatch):
    import fastnerf as fn
    K = np.array([[14.0, 0, 4.0], [0, 14.0, 4.0], [0, 0, 1]])
    grid = types.SimpleNamespace(outside_occupied=False, dens=None)      # the checks read no more of a grid than this
    T = lambda ktr, **kw: fn.run_nerf.Trainer(ktr, 8, 8, K, 2.0, 6.0, **kw)      # noqa: E731
    ktr = _cpu_networks(fn)
    with pytest.raises(ValueError, match='needs occupancy'):
        T(ktr, march=64)
    with pytest.raises(ValueError, match='outside_occupied=False'):
        T(ktr, march=64, occupancy=types.SimpleNamespace(outside_occupied=True, dens=None))
    for bad in (dict(march=1), dict(march=1 << 24), dict(march=64, march_cap=1), dict(march=64, march_cap=513), dict(march=64.0)):
        with pytest.raises(ValueError, match='2 <= march'):
            T(ktr, occupancy=grid, **bad)
    with pytest.raises(ValueError, match='raw_noise_std'):
        T(_cpu_networks(fn, raw_noise_std=1.0), march=64, occupancy=grid)
    monkeypatch.setenv('FASTNERF_FUSED_STEP', '0')
    with pytest.raises(ValueError, match='fused step'):
        T(ktr, march=64, occupancy=grid)


def test_python_surface():
    import inspect
    from fastnerf import occupancy, ops, run_nerf
    sig = inspect.signature(run_nerf.Trainer.__init__).parameters
    assert sig['march'].default is None and sig['march_cap'].default == 128 and sig['march_after'].default == 0
    assert inspect.signature(run_nerf.Trainer.step).parameters['march_u'].default is None
    assert inspect.signature(occupancy.OccupancyGrid.update).parameters['which'].default == 'both'
    sig = inspect.signature(occupancy.OccupancyGrid.march).parameters
    assert sig['u'].default is None and sig['seed'].default == 0
    assert callable(ops.occ_march_jitter) and callable(ops.march_mask) and callable(ops.step_march_ws_ints)
    assert 'march_after' in run_nerf.Trainer.__doc__ and 'march_overflow' in run_nerf.Trainer.__doc__
