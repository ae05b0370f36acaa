"""Training through an occupancy cascade, the part that needs no GPU: the numpy restatement of the covered rule
(tests/occ_cascade_train_numpy.py) against the lookup of tests/occ_cascade_numpy.py, the cursor arithmetic, the signatures and the
refusals, and that cascade files written before the feature still load."""
import inspect
import types

import numpy as np
import pytest

import fastnerf as fn

import occ_cascade_numpy as RC
import occ_cascade_train_numpy as T
import occ_numpy as R

F32 = np.float32
DILATES = (0, 1, 2)
SCENES = T.scenes()


def with_masks(levels):
    return [(np.ones(shape, bool), lo, hi) for shape, lo, hi in levels]


def test_concentric_scene_has_covered_cells_on_every_outer_level():
    """By the rule, at growth 2 and N = 16: level l covers indices i with -2.4 + (i - m) 0.3 >= -1.05 and -2.4 + (i + 1 + m) 0.3 <=
    1.05 (level 1; level 2 alike against level 1, and nothing of level 2 reaches into level 0's margins that level 1 does not hold):
    {7, 8} per axis at dilate 1, so 8 cells; {6 .. 9} at dilate 0, so 64; none at dilate 2."""
    levels = SCENES['concentric']
    for dilate, want in ((0, 64), (1, 8), (2, 0)):
        assert T.covered(levels, 0, dilate).sum() == 0
        for l in (1, 2):
            cov = T.covered(levels, l, dilate)
            assert cov.sum() == want, (dilate, l, int(cov.sum()))
            if dilate == 1:
                assert np.array_equal(np.argwhere(cov), np.array([[i, j, k] for i in (7, 8) for j in (7, 8) for k in (7, 8)]))
    own, off = T.concatenation(levels, 1)
    assert off.tolist() == [0, 4096, 4096 + 4088, 4096 + 2 * 4088] and own.size == off[-1]


def test_buried_level_may_own_nothing():
    levels = SCENES['buried']
    assert T.own_cells(levels, 1, 0).size == 0 and T.own_cells(levels, 1, 1).size == 0
    assert 0 < T.own_cells(levels, 1, 2).size < 64      # the margin of 3 cells reaches past the inner box's last cell
    assert T.own_cells(levels, 0, 1).size == 16 ** 3      # level 0 owns all its cells
    # the outer level is covered by level 0 ONLY: a union with the buried box adds nothing, and the buried box itself is too small
    only0 = T.covered([levels[0], levels[2]], 1, 1)
    assert np.array_equal(T.covered(levels, 2, 1), only0) and only0.any()


def test_own_lists_ascend_and_partition_the_level():
    for name, levels in SCENES.items():
        for dilate in DILATES:
            for l in range(len(levels)):
                own = T.own_cells(levels, l, dilate)
                cov = T.covered(levels, l, dilate).reshape(-1)
                assert own.dtype == np.int32 and (np.diff(own) > 0).all()
                assert own.size + cov.sum() == cov.size and not cov[own].any()
                if dilate:      # a larger margin covers no more
                    assert not (cov & ~T.covered(levels, l, dilate - 1).reshape(-1)).any()


@pytest.mark.parametrize('name', sorted(SCENES))
def test_no_point_is_decided_by_a_covered_cell(name):
    """The invariant the refresh rests on: a point that level l decides (the lookup's own fp32 arithmetic) never falls in a covered
    cell of l, for any dilate."""
    levels = SCENES[name]
    pts = T.points(levels, 100000, seed=sorted(SCENES).index(name))
    who = RC.decided_by(with_masks(levels), pts)
    assert all((who == l).sum() > 100 for l in range(len(levels)) if not (name == 'buried' and l == 1))
    assert (who == -1).any()
    for l, (shape, lo, hi) in enumerate(levels):
        mine = pts[who == l]
        idx = R.cell_index(mine, shape, lo, hi).astype(np.int64)
        for dilate in DILATES:
            cov = T.covered(levels, l, dilate)
            assert not cov[idx[:, 0], idx[:, 1], idx[:, 2]].any(), (name, l, dilate)


def test_points_sit_on_faces():
    """The snapped half of the points really lands on both sides of faces: the two neighbours of a face fall in different cells."""
    levels = SCENES['concentric']
    pts = T.points(levels, 100000, seed=0)
    shape, lo, hi = levels[1]
    f = (np.float64(lo[0]) + (np.float64(hi[0]) - lo[0]) * np.arange(17) / 16).astype(F32)
    on = np.isin(pts[:, 0], f).sum()
    below = np.isin(pts[:, 0], np.nextafter(f, F32(-np.inf))).sum()
    assert on > 500 and below > 500


def test_cursor_arithmetic_equals_the_package():
    total = 37
    for k in (None, 1, 5, 36, 37, 100):
        cursor, primed, seen = 0, False, np.zeros(total, np.int64)
        for call in range(12):
            want, nxt = T.refresh_slice(cursor, primed, total, k)
            ranges, got_next = fn.occupancy._rotate(cursor, primed, total, k)
            got = np.concatenate([np.arange(a, b) for a, b in ranges])
            assert np.array_equal(got, want) and got_next == nxt, (k, call)
            assert all(0 <= a < b <= total for a, b in ranges)
            if primed:
                seen[want] += 1
            cursor, primed = nxt, True
            if k is not None and k < total and call == -(-total // k):      # ceil(total / k) budgeted calls past priming
                assert (seen >= 1).all() and seen.sum() == k * call
    own, off = T.concatenation(SCENES['noncubic'], 1)
    l, i = T.level_of(off, np.arange(own.size))
    assert np.array_equal(np.bincount(l, minlength=3), np.diff(off)) and (i[off[:-1]] == 0).all()


def test_signatures():
    C = fn.occupancy.OccupancyCascade
    p = inspect.signature(C.for_training).parameters
    assert [(k, v.default) for k, v in p.items()] == [('levels', 3), ('N', 128), ('bound', 1.2), ('growth', 2.0), ('threshold', 0.),
                                                      ('dilate', 1), ('decay', 0.95), ('outside_occupied', True), ('device', 'cuda')]
    p = inspect.signature(C.update).parameters
    assert [(k, v.default) for k, v in list(p.items())[1:5]] == [('render_kwargs', inspect.Parameter.empty), ('seed', None),
                                                                 ('cells_per_call', None), ('which', 'both')]
    assert list(inspect.signature(C.own_cells).parameters) == ['self', 'l']
    assert C.MAX_TRAIN_N == T.MAX_TRAIN_N == 4096
    _lib = fn._lib
    assert len(_lib.SIGNATURES['fastnerf_train_step_cascade'][1]) == len(_lib.SIGNATURES['fastnerf_train_step_expo'][1]) + 1
    assert len(_lib.SIGNATURES['fastnerf_train_step_march_cascade'][1]) == len(_lib.SIGNATURES['fastnerf_train_step_march_expo'][1]) + 1


def test_refusals():
    fault = fn.occupancy._training_fault
    g = lambda dens=1, dilate=1, shape=(8, 8, 8): types.SimpleNamespace(dens=dens, dilate=dilate, shape=shape)      # noqa: E731
    assert fault([g(), g(), g()]) is None
    assert fault([g(), g(dens=None)]) == '' and fault([g(dens=None)]) == ''      # a rendering cascade: no error, not trained through
    assert 'dilate' in fault([g(), g(dilate=2)])
    assert '4096' in fault([g(), g(shape=(8, 4097, 8))])
    assert fault([g(shape=(4096, 1, 1))]) is None
    with pytest.raises(ValueError, match='4096'):
        fn.occupancy.OccupancyCascade.for_training(levels=2, N=[16, 5000], device='cpu')
    with pytest.raises(ValueError):
        fn.occupancy.OccupancyCascade.for_training(levels=3, N=[16, 16], device='cpu')
    with pytest.raises(ValueError, match='per level'):      # a ragged N is refused in this function's own words
        fn.occupancy.OccupancyCascade.for_training(levels=2, N=[16, (5, 5, 4, 3)], device='cpu')
    with pytest.raises(ValueError):
        fn.occupancy.OccupancyCascade.for_training(levels=9, device='cpu')
    with pytest.raises(ValueError):
        fn.occupancy.OccupancyCascade.for_training(levels=2, growth=0., device='cpu')
    # the C side: refused before anything is enqueued (no GPU is touched)
    _lib = fn._lib
    lib = _lib.lib()
    c = _lib.OccCascade()
    c.levels = 1
    c.level[0].n[:] = [8, 4097, 8]
    c.level[0].inv[:] = [1.0, 1.0, 1.0]
    assert lib.fastnerf_occ_cascade_own(c, 0, 1, None, None, None, None) == -1
    assert b'4096' in lib.fastnerf_last_error()
    c.level[0].n[:] = [8, 8, 8]
    assert lib.fastnerf_occ_cascade_own(c, 1, 1, None, None, None, None) == -1      # level out of range
    assert lib.fastnerf_occ_cascade_own(c, 0, 1, None, None, None, None) == -1      # null pointers
    import ctypes
    off = (ctypes.c_int64 * 2)(0, 513)
    assert lib.fastnerf_occ_cascade_points(c, None, off, 0, 1, 0, None, None) == -1      # more entries than the level has cells
    off = (ctypes.c_int64 * 2)(0, 512)
    assert lib.fastnerf_occ_cascade_points(c, None, off, 500, 13, 0, None, None) == -1      # a range past the concatenation
    assert lib.fastnerf_occ_cascade_points(c, None, off, 512, 0, 0, None, None) == 0        # nothing to do
    # the step: a cascade beside args->occ is refused, whatever else the arguments hold
    a = _lib.StepArgs()
    a.n, a.N_samples, a.occ = 4, 8, 1
    assert lib.fastnerf_train_step_cascade(ctypes.byref(a), None, None, None, None, ctypes.byref(c), 1, None) == -1
    assert b'occ == NULL' in lib.fastnerf_last_error()


def test_cascade_files_from_before_still_load(tmp_path, monkeypatch):
    """A cascade file as save() wrote it before cascades were trained through (no updates / cursor / primed) loads, with a fresh
    cursor.  The grids' constructor wants device tensors; here it is let through on the host, which the lookup-free load allows."""
    monkeypatch.setattr(fn.ops, 'require_gpu', lambda *a: None)
    fields = dict(levels=np.asarray(2, np.int64), outside_occupied=np.asarray(False))
    rs = np.random.RandomState(0)
    for l, n in enumerate((4, 6)):
        nw = (n ** 3 + 31) // 32
        fields.update({'l%d_words' % l: rs.randint(0, 2 ** 32, nw, dtype=np.uint64).astype(np.uint32), 'l%d_shape' % l: np.asarray((n,) * 3, np.int64),
                       'l%d_lo' % l: np.full(3, -1.0 - l, F32), 'l%d_hi' % l: np.full(3, 1.0 + l, F32),
                       'l%d_outside_occupied' % l: np.asarray(True)})
    p = str(tmp_path / 'old.npz')
    with open(p, 'wb') as fh:
        np.savez(fh, **fields)
    c = fn.occupancy.OccupancyCascade.load(p, device='cpu')
    assert c.levels == 2 and c.outside_occupied is False and c.dens is None
    assert (c.updates, c.cursor, c.primed) == (0, 0, False)
    assert np.array_equal(c.grids[1].words.numpy().view(np.uint32), fields['l1_words'])
    with pytest.raises(ValueError, match='for_training'):
        c.own_cells(0)
    q = str(tmp_path / 'new.npz')
    c.save(q)
    with np.load(q) as f:
        assert 'updates' not in f.files      # a rendering cascade writes the file it wrote before
