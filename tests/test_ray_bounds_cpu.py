"""fastnerf_occ_ray_bounds, the part that needs no GPU: the float32 restatement of tests/ray_bounds_numpy.py is conservative (C)
and tight (T) against the lookup of tests/occ_numpy.py / occ_cascade_numpy.py on every grid and ray set the GPU tests use, keeps
the contract's edge cases, and the new export is in the header, the library and the binding.

(C) every probe depth that the lookup calls occupied lies in [near', far'] and its ray has hit = 1: zero exceptions.
(T) with M+ the mask dilated by one cell: every hit ray has an occupied probe under M+, and near' >= zmin(M+) - s,
    far' <= zmax(M+) + s, s = sqrt(3) h_max / |d| + 2 probe spacings: zero exceptions.
4096 probes per ray; every combination has rays with hit = 1 and (the grids with outside_occupied=False) rays with hit = 0."""
import ctypes
import os
import re

import numpy as np
import pytest

import occ_cascade_numpy as RC
import occ_numpy as R
import ray_bounds_numpy as RB
from oracle import nerf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
GRIDS = R.scene_grids()
RAYS = RB.ray_sets(O)
_cache = {}


def grid_case(gname, rname):
    """(rays, z, bounds of the restatement, live under M, live under M+, h_max), computed once per combination."""
    key = (gname, rname)
    if key not in _cache:
        mask, lo, hi, outside = GRIDS[gname]
        rays = RAYS[rname]
        z = RB.probe_depths(rays)
        live = R.classify(mask, lo, hi, outside, rays, z)
        plus = R.classify(R.dilated(mask, 1), lo, hi, outside, rays, z)
        _cache[key] = (rays, z, RB.ray_bounds_grid(mask, lo, hi, outside, rays), live, plus, RB.cell_edges(mask.shape, lo, hi).max())
    return _cache[key]


@pytest.mark.parametrize('rname', sorted(RAYS))
@pytest.mark.parametrize('gname', sorted(GRIDS))
def test_conservative_and_tight(gname, rname):
    rays, z, (n2, f2, hit), live, plus, h_max = grid_case(gname, rname)
    assert rays.shape == (144, 11) and z.shape == (144, RB.PROBES)
    print('%s / %s: hit %d of 144, mean kept %.3f of [near, far] on the hit rays' % (
        gname, rname, hit.sum(), float(((f2 - n2) / (rays[:, 7] - rays[:, 6]))[hit == 1].mean())))
    assert (rays[:, 6] <= n2).all() and (n2 < f2).all() and (f2 <= rays[:, 7]).all()
    assert RB.check_conservative(live, z, n2, f2, hit) == 0
    assert RB.check_tight(plus, z, rays, n2, f2, hit, h_max) == 0
    assert 0 < int(hit.sum()) and (GRIDS[gname][3] or int(hit.sum()) < 144)
    miss = hit == 0
    assert (n2[miss] == rays[miss, 6]).all() and (f2[miss] == rays[miss, 7]).all()


def test_outside_occupied_false_tightens_and_true_hardly_does():
    rays = RAYS['camera']
    for gname, lo_frac, hi_frac in (('ball', 0.2, 0.6), ('random', 0.3, 0.7)):
        _, _, (n2, f2, hit), _, _, _ = grid_case(gname, 'camera')
        kept = float(((f2 - n2) / (rays[:, 7] - rays[:, 6]))[hit == 1].mean())
        assert lo_frac < kept < hi_frac, (gname, kept)
    # outside_occupied=True: whatever of [near, far] lies outside the box stays, whatever the bits say
    mask, lo, hi, _ = GRIDS['ball']
    z = RB.probe_depths(rays)
    beyond = ~R.query(np.ones_like(mask), lo, hi, False, R.sample_points(rays, z))
    n2, f2, hit = RB.ray_bounds_grid(mask, lo, hi, True, rays)
    assert beyond.any(1).all() and hit.all()
    assert RB.check_conservative(beyond, z, n2, f2, hit) == 0
    assert float(((f2 - n2) / (rays[:, 7] - rays[:, 6])).mean()) > 0.6


# ---- the edge cases of the contract ----------------------------------------------------------------------------------------------
def one(gname, o, d, near, far, **kw):
    mask, lo, hi, outside = GRIDS[gname]
    return RB.ray_bounds_one([(mask, lo, hi)], kw.get('outside', outside), np.asarray(o, F32), np.asarray(d, F32), near, far, kw.get('cap'))


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_non_finite_rays_keep_their_bounds_with_hit(bad):
    for col in range(6):
        v = [0.1, 0.2, -3.0, 0.0, 0.1, 1.0]
        v[col] = bad
        assert one('ball', v[:3], v[3:], 0.5, 6.0) == (F32(0.5), F32(6.0), 1)
    n2, f2, hit = one('ball', [0, 0, -3], [0, 0, 1], bad, 6.0)
    assert hit == 1 and f2 == F32(6.0) and (n2 == F32(bad) or n2 != n2)
    n2, f2, hit = one('ball', [0, 0, -3], [0, 0, 1], 0.5, bad)
    assert hit == 1 and n2 == F32(0.5) and (f2 == F32(bad) or f2 != f2)


def test_near_not_below_far_keeps_the_bounds_with_hit():
    assert one('ball', [0, 0, -3], [0, 0, 1], 4.0, 4.0) == (F32(4.0), F32(4.0), 1)
    assert one('ball', [0, 0, -3], [0, 0, 1], 5.0, 2.0) == (F32(5.0), F32(2.0), 1)


def test_a_ray_that_misses_the_box():
    assert one('ball', [0, 5, -3], [0, 0, 1], 0.5, 6.0) == (F32(0.5), F32(6.0), 0)
    assert one('ball', [0, 5, -3], [0, 0, 1], 0.5, 6.0, outside=True) == (F32(0.5), F32(6.0), 1)
    assert one('ball', [0, 0, -3], [0, 0, -1], 0.5, 6.0) == (F32(0.5), F32(6.0), 0)      # points away from it
    assert one('ball', [0, 0, -9], [0, 0, 1], 0.5, 6.0) == (F32(0.5), F32(6.0), 0)       # [near, far] ends before it


def test_a_ray_through_the_ball_and_parallel_to_a_face():
    # along z through the centre: the ball of radius 1.2 in cells of 3/32, the ray on the face x = 0 between two cells
    n2, f2, hit = one('ball', [0, 0, -3], [0, 0, 1], 0.5, 6.0)
    assert hit == 1 and 1.6 < n2 < 1.85 and 4.15 < f2 < 4.4
    n2, f2, hit = one('ball', [0.01, 0.02, -3], [0, 0, 2], 0.25, 3.0)                      # two zero components, |d| = 2
    assert hit == 1 and 0.8 < n2 < 0.925 and 2.075 < f2 < 2.2
    # in the plane of the box's own face x = lo: the samples may fall on either side of it
    mask, lo, hi, _ = GRIDS['ball']
    rays = np.array([[-1.5, 0.05, -3, 0, 0, 1, 0.5, 6.0, 0, 0, 1]], F32)
    z = RB.probe_depths(rays)
    n2, f2, hit = RB.ray_bounds_grid(mask, lo, hi, False, rays)
    assert RB.check_conservative(R.classify(mask, lo, hi, False, rays, z), z, n2, f2, hit) == 0


def test_the_iteration_cap_keeps_the_bounds_with_hit():
    assert one('ball', [0.3, 0.2, -3], [0.01, 0.02, 1], 0.5, 6.0, cap=5) == (F32(0.5), F32(6.0), 1)
    assert RB.iteration_cap([(32, 32, 32)]) == 2 * 96 + 32
    assert RB.iteration_cap([(12, 16, 20), (8, 8, 8)]) == 2 * 72 + 48


def test_terms_too_large_for_the_error_bound_keep_the_bounds_with_hit():
    assert one('ball', [0, 0, -3e7], [0, 0, 1], 0.5, 6.0) == (F32(0.5), F32(6.0), 1)
    assert one('ball', [0, 0, -3], [0, 0, 1], 0.5, 3e30) == (F32(0.5), F32(3e30), 1)


# ---- cascades ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gname', sorted(GRIDS))
def test_a_cascade_of_one_level_is_the_grid(gname):
    mask, lo, hi, outside = GRIDS[gname]
    a = RB.ray_bounds_grid(mask, lo, hi, outside, RAYS['random'])
    b = RB.ray_bounds([(mask, lo, hi)], outside, RAYS['random'])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def cascade_case(which, rname, outside):
    key = ('cascade', which, rname, outside)
    if key not in _cache:
        levels = RB.cascade_fixtures()[which]
        rays = RAYS[rname]
        z = RB.probe_depths(rays)
        live = RC.classify(levels, outside, rays, z)
        plus = RC.classify([(R.dilated(m, 1), lo, hi) for m, lo, hi in levels], outside, rays, z)
        h_max = max(RB.cell_edges(m.shape, lo, hi).max() for m, lo, hi in levels)
        _cache[key] = (levels, rays, z, RB.ray_bounds(levels, outside, rays), live, plus, h_max)
    return _cache[key]


@pytest.mark.parametrize('outside', [False, True])
@pytest.mark.parametrize('rname', sorted(RAYS))
def test_three_level_cascade_is_conservative(rname, outside):
    levels, rays, z, (n2, f2, hit), live, _, _ = cascade_case(0, rname, outside)
    who = RC.decided_by(levels, R.sample_points(rays, z))
    print('cascade / %s: hit %d of 144, probes decided by level 0 / 1 / 2 / none: %s' % (rname, hit.sum(), RC.shares(who, 3)))
    assert all((who == l).any() for l in (0, 1, 2)) and (rname == 'camera' or (who == -1).any())
    assert (rays[:, 6] <= n2).all() and (n2 < f2).all() and (f2 <= rays[:, 7]).all()
    assert RB.check_conservative(live, z, n2, f2, hit) == 0
    assert 0 < hit.sum() and (outside or rname == 'camera' or hit.sum() < 144)


@pytest.mark.parametrize('rname', sorted(RAYS))
def test_three_level_cascade_is_tight_away_from_the_seams(rname):
    levels, rays, z, (n2, f2, hit), live, plus, h_max = cascade_case(1, rname, False)
    assert all(m.any() for m, _, _ in levels)
    assert RB.check_conservative(live, z, n2, f2, hit) == 0
    assert RB.check_tight(plus, z, rays, n2, f2, hit, h_max) == 0
    assert 0 < hit.sum() < 144


# ---- the export in header, library and binding ---------------------------------------------------------------------------------
def test_export_in_header_and_binding():
    import fastnerf
    from fastnerf import _lib
    with open(os.path.join(ROOT, 'include', 'fastnerf.h')) as f:
        header = f.read()
    assert re.search(r'\bint fastnerf_occ_ray_bounds\(const fn_occ_grid\* grid, const fn_occ_cascade\* cascade', header)
    assert re.search(r'#define FN_STEP_TIGHTEN 2\b', header)
    res, args = _lib.SIGNATURES['fastnerf_occ_ray_bounds']
    assert res is ctypes.c_int and len(args) == 8
    assert hasattr(fastnerf.ops, 'occ_ray_bounds')
    for cls in (fastnerf.occupancy.OccupancyGrid, fastnerf.occupancy.OccupancyCascade):
        assert callable(getattr(cls, 'ray_bounds')) and callable(getattr(cls, 'tighten'))


def test_argument_errors_need_no_gpu():
    """The checks that come before any launch: exactly one of grid / cascade, n >= 0, pointers."""
    from fastnerf import _lib
    lib = _lib.lib()
    g = _lib.OccGrid(8, (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(2, 2, 2), (ctypes.c_int32 * 3)(4, 4, 4), 0)
    c = _lib.OccCascade()
    assert lib.fastnerf_occ_ray_bounds(None, None, 1, 8, 0, 8, 8, None) == -1
    assert b'exactly one' in lib.fastnerf_last_error()
    assert lib.fastnerf_occ_ray_bounds(ctypes.byref(g), ctypes.byref(c), 1, 8, 0, 8, 8, None) == -1
    assert lib.fastnerf_occ_ray_bounds(ctypes.byref(g), None, -1, 8, 0, 8, 8, None) == -1
    assert lib.fastnerf_occ_ray_bounds(ctypes.byref(g), None, 1, None, 0, 8, 8, None) == -1
    assert lib.fastnerf_occ_ray_bounds(None, ctypes.byref(c), 1, 8, 0, 8, 8, None) == -1       # levels == 0
    assert lib.fastnerf_occ_ray_bounds(ctypes.byref(g), None, 0, None, 0, None, None, None) == 0   # nothing to do


def test_tighten_without_a_grid_raises_before_anything_runs():
    import fastnerf
    import torch
    with pytest.raises(ValueError, match='tighten'):
        fastnerf.render.render_rays(torch.zeros(4, 11), network_fn=None, network_query_fn=None, N_samples=4, tighten=True)
