"""The marched render on the CPU alone: the kernel restatement of tests/march_numpy.py (march_round, the oracle of csrc/march.hip) against
the contract of include/fastnerf.h restated from its definition (runs -> sequence -> packed row), and the consequence of the contract --
a packed row composites to what the dense row with zeros composites to -- in float64.

Conditions on the inputs, asserted below: at least a quarter of the two_shells rays have three or more runs; no ray of the equality
tests overflows or has lattice point K - 1 live."""
import numpy as np
import pytest

import march_numpy as M
import occ_numpy as R
from oracle import nerf_oracle as O

F32 = np.float32
K, C = 128, 160
SCENES = ['ball', 'random', 'two_shells', 'cascade']


@pytest.fixture(scope='module')
def rays():
    return R.scene_rays(O, side=12)      # 144 rays


@pytest.fixture(scope='module')
def scenes(rays):
    """name -> (live [n, K], zlat [n, K + 1], one round's (z, kidx, overflow, state)): computed once, never modified."""
    out = {}
    zlat = M.lattice(rays, K)
    for name, grid in M.scene_grids().items():
        live = M.live_bits(grid, rays, zlat[:, :K])
        out[name] = (live, zlat, M.march(live, zlat, C))
    return out


def n_runs(live):
    return np.array([len(M.runs(row)) for row in live])


def test_lattice_is_the_coarse_sampler(rays):
    import torch
    rb = torch.as_tensor(rays)
    for lindisp in (False, True):
        zlat = M.lattice(rays, 64, lindisp)
        ref = O.coarse_z(rb[:, 6:7], rb[:, 7:8], 64, lindisp, None).numpy()
        assert np.allclose(zlat[:, :64], ref, rtol=3e-7, atol=0), 'the lattice is the reference\'s coarse depths up to the rounding of linspace'
        assert (np.diff(zlat, axis=-1) > 0).all()
        assert np.array_equal(zlat[:, 64], (zlat[:, 63] + (zlat[:, 63] - zlat[:, 62]).astype(F32)).astype(F32))


def test_input_conditions(scenes):
    runs = n_runs(scenes['two_shells'][0])
    assert (runs >= 3).mean() >= 0.25, 'at least a quarter of the two_shells rays have three or more runs'
    assert (runs >= 4).any(), 'central rays cross both shells twice (a ray that grazes a voxelised shell may have more)'
    for name in SCENES:
        live, _, (_, _, overflow, _) = scenes[name]
        assert not overflow.any() and not live[:, K - 1].any(), name + ': no ray of the equality tests overflows or has K - 1 live'
        assert live.any(1).mean() > 0.3 and not live.all(1).any(), name


@pytest.mark.parametrize('name', SCENES)
def test_live_set_and_rows_are_the_contract(scenes, name):
    live, zlat, (z, kidx, overflow, state) = scenes[name]
    # the live (ray, k) set of the rows = the dense classify of the lattice
    got = np.zeros_like(live)
    r, s = np.nonzero(kidx >= 0)
    got[r, kidx[r, s]] = True
    assert np.array_equal(got, live)
    assert (np.diff(np.where(kidx >= 0, kidx, K + 1).astype(np.int64), axis=-1)[(kidx[:, :-1] >= 0) & (kidx[:, 1:] >= 0)] == 1).all()
    # the rows = the sequence of the definition, cut and padded
    cz, ck, co = M.packed(live, zlat, C)
    assert np.array_equal(z.view(np.int32), cz.view(np.int32)) and np.array_equal(kidx, ck) and np.array_equal(overflow.astype(bool), co)
    assert (np.diff(z, axis=-1) >= 0).all(), 'z is non-decreasing along a row'
    assert (kidx[:, C - 1] == -1).all()
    assert ((state[:, 1] & 1) == 0).all(), 'no close is owed after the last round'


@pytest.mark.parametrize('name', SCENES)
def test_float64_composite_of_the_packed_row_is_the_dense_one(scenes, rays, name):
    live, zlat, (z, kidx, _, _) = scenes[name]
    n = live.shape[0]
    raw_dense = (np.random.RandomState(3).rand(n, K, 4).astype(F32) * 4 + F32(0.05)) * live[..., None]      # random, positive, zeros where empty
    dense = M.composite64(raw_dense, zlat[:, :K], rays)
    pk = M.composite64(M.pack_raw(raw_dense, kidx), z, rays)
    assert float(dense['acc'].max()) > 0.9 and float(dense['acc'].min()) == 0.0
    for k in ('rgb', 'acc', 'depth'):
        assert np.abs(dense[k] - pk[k]).max() <= 1e-12, k
    hit = dense['acc'] > 0
    assert np.abs(dense['disp'][hit] / pk['disp'][hit] - 1).max() <= 1e-12
    # every live sample has the width of the dense pass: the same bits
    r, s = np.nonzero(kidx >= 0)
    kk = kidx[r, s]
    assert np.array_equal((z[r, s + 1] - z[r, s]).astype(F32), (zlat[r, kk + 1] - zlat[r, kk]).astype(F32))
    assert np.array_equal(z[r, s], zlat[r, kk])


def test_cap_overflow_padding_and_the_empty_ray(scenes):
    live, zlat, _ = scenes['two_shells']
    L = np.array([len(M.sequence(live[r], zlat[r])) for r in range(live.shape[0])])
    empty = np.nonzero(L == 0)[0]
    assert empty.size > 0 and L.max() > 20
    for cap in (2, 5, int(L.max()) - 1, int(L.max())):
        z, kidx, overflow, _ = M.march(live, zlat, cap)
        cz, ck, co = M.packed(live, zlat, cap)
        assert np.array_equal(z.view(np.int32), cz.view(np.int32)) and np.array_equal(kidx, ck), cap
        assert np.array_equal(overflow.astype(bool), L > cap) and np.array_equal(co, L > cap), cap
        assert (kidx[:, cap - 1] == -1).all(), 'slot C - 1 never holds a live sample'
        over = np.nonzero(L > cap)[0]
        for r in over[:8]:      # the first C entries of the sequence: z stays, the last kept entry loses its index
            seq = M.sequence(live[r], zlat[r])
            assert [a for a, _ in seq[:cap]] == z[r].tolist() and [b for _, b in seq[:cap - 1]] == kidx[r, :cap - 1].tolist()
        assert (z[empty] == zlat[empty, :1]).all() and (kidx[empty] == -1).all(), 'a ray without a live lattice point holds (z_0, -1)'
    assert (L > int(L.max()) - 1).sum() >= 1 and not (L > int(L.max())).any()
    # padding: (z of the slot before, -1)
    z, kidx, _, _ = M.march(live, zlat, C)
    for r in np.nonzero((L > 0) & (L < C))[0]:
        assert (z[r, L[r]:] == z[r, L[r] - 1]).all() and (kidx[r, L[r]:] == -1).all()


def test_a_live_last_lattice_point_is_closed_at_z_K(rays):
    grid = M.cascade2(outside_occupied=True)      # the far end of every ray lies outside both boxes: occupied
    zlat = M.lattice(rays, K)
    live = M.live_bits(grid, rays, zlat[:, :K])
    assert live[:, K - 1].all()
    z, kidx, overflow, _ = M.march(live, zlat, 160)
    ok = ~overflow.astype(bool)
    assert ok.sum() > 10
    for r in np.nonzero(ok)[0]:
        s = int(np.nonzero(kidx[r] == K - 1)[0][0])
        assert z[r, s + 1] == zlat[r, K] and kidx[r, s + 1] == -1
        assert (z[r, s + 1:] == zlat[r, K]).all()
    cz, ck, co = M.packed(live, zlat, 160)
    assert np.array_equal(z.view(np.int32), cz.view(np.int32)) and np.array_equal(kidx, ck) and np.array_equal(overflow.astype(bool), co)


@pytest.mark.parametrize('name', SCENES)
@pytest.mark.parametrize('B', [1, 7, 16, 159, 160, 300])
def test_rounds_without_a_cut_reproduce_the_single_round(scenes, name, B):
    live, zlat, one = scenes[name]
    n = live.shape[0]
    for trans_of in (None, lambda j, z, k: np.full(n, 0.5, F32)):      # every T > eps
        got = M.march(live, zlat, C, B=B, trans_of=trans_of, eps=1e-2)
        assert np.array_equal(got[0].view(np.int32), one[0].view(np.int32)) and np.array_equal(got[1], one[1]), B
        assert np.array_equal(got[2], one[2])
    # a smaller cap, where most rays overflow: the flag and the rows survive the rounds too
    one5 = M.march(live, zlat, 5)
    got5 = M.march(live, zlat, 5, B=2)
    assert all(np.array_equal(a, b) for a, b in zip(one5[:3], got5[:3]))


def test_every_round_leaves_the_next_depth_in_place(scenes):
    """z[s1] after a round is the depth of the row's next entry when slot s1 - 1 is live -- what fastnerf_ert_advance reads for that
    sample's width -- whether or not the ray goes on."""
    live, zlat, one = scenes['two_shells']
    B = 4
    cur = None
    seen = 0
    for s0 in range(0, C, B):
        cur = M.march_round(live, zlat, C, s0, s0 + B, cur)
        if s0 + B < C:
            z, kidx = cur[0], cur[1]
            lv = kidx[:, s0 + B - 1] >= 0
            seen += int(lv.sum())
            assert np.array_equal(z[lv, s0 + B], one[0][lv, s0 + B])
            assert np.array_equal(z[lv, s0 + B], zlat[lv, kidx[lv, s0 + B - 1] + 1])
            assert np.array_equal(z[~lv, s0 + B], z[~lv, s0 + B - 1])
    assert seen > 50


def test_a_cut_ray_keeps_its_pending_close(scenes):
    live, zlat, one = scenes['two_shells']
    n = live.shape[0]
    B = 4
    for j in (1, 2, 5):
        s0 = j * B
        cur = None
        for a in range(0, s0, B):
            cur = M.march_round(live, zlat, C, a, a + B, cur)
        state_before = cur[3].copy()
        trans = np.where(np.arange(n) % 2 == 0, F32(1e-3), F32(0.5)).astype(F32)
        trans[1] = np.nan      # a NaN is not > eps
        z, kidx, overflow, state = M.march_round(live, zlat, C, s0, s0 + B, cur, trans=trans, eps=1e-2)
        cutr = np.nonzero(~(trans > F32(1e-2)))[0]
        pending = cutr[cur[1][cutr, s0 - 1] >= 0]
        assert pending.size > 3 and (cutr.size - pending.size) > 3, 'both kinds of cut rays occur'
        for r in cutr:
            if cur[1][r, s0 - 1] >= 0:      # the segment before ended in live sample k: slot jB = (z_{k+1}, -1), then padding
                k = cur[1][r, s0 - 1]
                assert z[r, s0] == zlat[r, k + 1] and kidx[r, s0] == -1
                assert (z[r, s0 + 1:s0 + B + 1] == zlat[r, k + 1]).all()
            else:
                assert (z[r, s0:s0 + B + 1] == z[r, s0 - 1]).all()
            assert (kidx[r, s0:s0 + B] == -1).all()
            assert state[r, 0] == state_before[r, 0], 'the lattice position does not advance'
            assert np.array_equal(z[r, :s0], cur[0][r, :s0]) and np.array_equal(kidx[r, :s0], cur[1][r, :s0])
        go = np.setdiff1d(np.arange(n), cutr)
        assert np.array_equal(z[go, :s0 + B], one[0][go, :s0 + B]) and np.array_equal(kidx[go, :s0 + B], one[1][go, :s0 + B])
        # cut once, cut for good: the later rounds pad
        nxt = M.march_round(live, zlat, C, s0 + B, s0 + 2 * B, (z, kidx, overflow, state), trans=trans, eps=1e-2)
        assert (nxt[1][cutr, s0 + B:s0 + 2 * B] == -1).all()
        assert np.array_equal(nxt[0][cutr, s0 + B:s0 + 2 * B], np.repeat(z[cutr, s0 + B - 1:s0 + B], B, 1))


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
    one = C.c_void_p(16)      # never dereferenced
    grid = C.pointer(_good_grid())

    def render(mode=0, n=4, K=64, cap=16, grid=grid, cascade=None, eps=0.0, block=0, null=()):
        p = lambda k: None if k in null else one      # noqa: E731
        outs = [p(k) for k in ('counts', 'z', 'kidx', 'overflow', 'raw', 'rgb', 'disp', 'acc', 'w', 'depth')]
        return lib.fastnerf_render_rays_fwd_march(mode, n, K, cap, p('rays11'), 0, 0, p('params'), p('packed'), grid, cascade, eps, block, *outs, 0, None)

    for kw, word in ((dict(mode=3), b'math_mode'), (dict(K=1), b'K'), (dict(K=1 << 24), b'K'), (dict(cap=1), b'C'), (dict(cap=513), b'C'),
                     (dict(eps=1.0, block=4), b'eps'), (dict(eps=float('nan'), block=4), b'eps'), (dict(block=-1), b'block'),
                     (dict(grid=None), b'exactly one'), (dict(cascade=C.pointer(_lib.OccCascade())), b'exactly one'),
                     (dict(grid=None, cascade=C.pointer(_lib.OccCascade())), b'levels'), (dict(grid=C.pointer(_lib.OccGrid())), b'words'),
                     (dict(n=1 << 23, cap=256), b'2^31'), (dict(n=1 << 20, K=1 << 12), b'2^31'),
                     (dict(null=('rays11',)), b'null'), (dict(null=('kidx',)), b'null'), (dict(null=('counts',)), b'null')):
        assert render(**kw) == -1, kw
        msg = lib.fastnerf_last_error()
        assert msg.startswith(b'fastnerf_render_rays_fwd_march:') and word in msg, (kw, msg)
    assert render(n=0) == 0

    def march(n=4, K=64, cap=16, s0=0, s1=16, first=1, grid=grid, cascade=None, trans=None, eps=0.0, state=one):
        return lib.fastnerf_occ_march(grid, cascade, n, K, 0, one, cap, s0, s1, first, trans, eps, state, one, one, one, None)

    for kw in (dict(K=1), dict(K=1 << 24), dict(cap=1), dict(cap=513, s1=513), dict(s1=17), dict(s0=4, s1=4), dict(s0=-1), dict(s0=4, first=1),
               dict(first=0), dict(n=-1), dict(n=1 << 23, cap=256, s1=256), dict(grid=None), dict(cascade=C.pointer(_lib.OccCascade())),
               dict(grid=C.pointer(_lib.OccGrid())), dict(trans=one, eps=1.0), dict(trans=one, eps=-1.0), dict(state=None)):
        assert march(**kw) == -1, kw
    assert march(n=0) == 0
    lst = lambda **k: lib.fastnerf_march_list(k.get('n', 4), k.get('C', 16), k.get('s0', 0), k.get('s1', 8), k.get('kidx', one), one, one, None,      # noqa: E731
                                              one, None, 0, None)
    for kw in (dict(n=0), dict(s1=17), dict(s0=8), dict(kidx=None), dict(n=1 << 28)):
        assert lst(**kw) == -1, kw


def test_python_surface():
    import inspect
    from fastnerf import occupancy, ops, render
    sig = inspect.signature(render.render_rays).parameters
    assert sig['march'].default is None and sig['march_cap'].default == 128
    assert callable(render._forward_march) and callable(ops.occ_march) and callable(ops.march_list) and callable(ops.render_rays_fwd_march)
    assert callable(occupancy.OccupancyGrid.march) and callable(occupancy.OccupancyCascade.march)
    doc = render.render_rays.__doc__
    assert 'march=K' in doc and 'march_overflow' in doc
    for bad in ((1, 128), (1 << 24, 128), (256, 1), (256, 513), (256.0, 128), (True, 128), (256, None)):
        with pytest.raises(ValueError):
            ops.check_march(*bad)
    assert ops.check_march(2, 2) == (2, 2) and ops.check_march(np.int64(4096), 512) == (4096, 512)
