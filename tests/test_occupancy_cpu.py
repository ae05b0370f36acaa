"""Occupancy grid, the part that needs no GPU: properties of the restatement the GPU tests compare against (tests/occ_numpy.py),
the .npz format, the new symbols in header / library / binding, and the check that the grids and seeds of the masked-render GPU
tests mask enough to matter (on the CPU oracle alone)."""
import os
import re

import numpy as np
import pytest
import torch

import occ_numpy as R
from oracle import nerf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['fastnerf_occ_words', 'fastnerf_occ_build', 'fastnerf_occ_from_mask', 'fastnerf_occ_query', 'fastnerf_occ_classify',
               'fastnerf_mlp_fwd_list_ex', 'fastnerf_mlp_bf16_fwd_list', 'fastnerf_mlp_x6_fwd_list', 'fastnerf_render_rays_fwd_occ']


def test_dilation_composes():
    m = np.random.RandomState(1).rand(9, 7, 11) < 0.03
    for a, b in ((1, 1), (1, 2), (2, 1), (0, 3)):
        assert np.array_equal(R.dilated(m, a + b), R.dilated(R.dilated(m, a), b))
    assert np.array_equal(R.dilated(m, 0), m)
    one = np.zeros((5, 5, 5), bool)
    one[0, 2, 4] = True
    d = R.dilated(one, 1)
    assert d.sum() == 2 * 3 * 2 and d[1, 3, 3] and not d[2, 2, 4]      # clipped at the box


def test_build_is_monotone_in_the_threshold_and_strict():
    v = np.random.RandomState(2).rand(6, 5, 7).astype(np.float32)
    prev = None
    for thr in (0.99, 0.9, 0.5, 0.1, -1.0):
        cur = R.build(v, thr, 1)
        assert prev is None or not (prev & ~cur).any()
        prev = cur
    assert R.build(v, -1.0, 0).all() and not R.build(v, 1.0, 3).any()
    flat = np.full((3, 3, 3), 0.25, np.float32)
    assert not R.build(flat, 0.25, 0).any() and R.build(flat, np.nextafter(np.float32(0.25), np.float32(0)), 0).all()
    corner = np.zeros((3, 3, 3), np.float32)
    corner[1, 1, 1] = 1.0                                              # the one point all 8 cells share
    assert R.build(corner, 0.5, 0).all()


def test_face_points_go_to_the_upper_cell_and_outside_rules():
    mask = np.zeros((4, 4, 4), bool)
    mask[2, 1, 3] = True
    lo, hi = np.float32(-1.0), np.float32(1.0)
    pt = lambda *c: np.array(c, np.float32)
    assert R.query(mask, lo, hi, False, pt(0.0, -0.5, 0.5))            # on three lower faces of cell (2, 1, 3)
    assert not R.query(mask, lo, hi, False, pt(-2.0 ** -23, -0.5, 0.5))      # (x - lo is exact here)
    assert not R.query(mask, lo, hi, False, pt(0.5, -0.5, 0.5))        # the upper face belongs to cell 3
    assert R.cell_index(pt(-1.0, -1.0, -1.0), mask.shape, lo, hi).tolist() == [0, 0, 0]
    for oo in (False, True):
        for p in (pt(1.0, 0.0, 0.0), pt(0.0, -1.0001, 0.0), pt(np.nan, 0.0, 0.0), pt(0.0, np.inf, 0.0), pt(0.0, 0.0, -np.inf)):
            assert bool(R.query(mask, lo, hi, oo, p)) == oo
    full = np.ones((4, 4, 4), bool)
    assert R.query(full, lo, hi, False, pt(-1.0, -1.0, -1.0)) and not R.query(full, lo, hi, False, pt(1.0, 1.0, 1.0))


def test_sample_points_round_twice():
    r = np.zeros((1, 11), np.float32)
    r[0, 0], r[0, 3] = np.float32(-(1.0 + 2.0 ** -11)), np.float32(1.0 + 2.0 ** -12)
    z = np.array([[1.0 + 2.0 ** -12]], np.float32)      # d * z = 1 + 2^-11 + 2^-24: the last term is lost to the first rounding
    x = R.sample_points(r, z)[0, 0, 0]
    assert x == np.float32(0.0)
    assert np.float32(np.float64(r[0, 3]) * np.float64(z[0, 0]) + np.float64(r[0, 0])) == np.float32(2.0 ** -24)      # a fused multiply-add


def test_npz_layout_is_readable_with_numpy_alone(tmp_path):
    m = np.random.RandomState(3).rand(5, 6, 7) < 0.4
    flat = np.zeros((m.size + 31) // 32 * 32, np.uint32)
    flat[:m.size] = m.reshape(-1)
    words = (flat.reshape(-1, 32) << np.arange(32, dtype=np.uint32)).sum(1).astype(np.uint32)
    p = str(tmp_path / 'g.npz')
    with open(p, 'wb') as fh:
        np.savez(fh, words=words, shape=np.asarray(m.shape, np.int64), lo=np.zeros(3, np.float32), hi=np.ones(3, np.float32),
                 outside_occupied=np.asarray(True))
    with np.load(p) as f:
        assert sorted(f.files) == ['hi', 'lo', 'outside_occupied', 'shape', 'words']
        assert np.array_equal(R.words_to_mask(f['words'], f['shape']), m)


def test_new_symbols_in_header_library_and_binding():
    from fastnerf import _lib
    src = open(os.path.join(ROOT, 'include', 'fastnerf.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(fastnerf_\w+)\s*\(', src))
    lib = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert 'fn_occ_grid' in src
    import ctypes
    assert ctypes.sizeof(_lib.OccGrid) == 8 + 4 * 10
    assert lib.fastnerf_occ_words(256, 256, 256) == 256 ** 3 // 32 and lib.fastnerf_occ_words(1, 1, 1) == 1
    assert lib.fastnerf_occ_words(0, 4, 4) == -1 and b'fastnerf_occ_words' in lib.fastnerf_last_error()
    assert lib.fastnerf_occ_words(2048, 2048, 2048) == -1


def test_surface_refuses_cpu_tensors_without_a_gpu():
    import fastnerf
    assert hasattr(fastnerf, 'occupancy')
    G = fastnerf.occupancy.OccupancyGrid
    with pytest.raises(RuntimeError):
        G.from_mask(torch.ones(4, 4, 4, dtype=torch.bool), -1.0, 1.0)
    with pytest.raises(RuntimeError):
        G.from_density(torch.ones(5, 5, 5), -1.0, 1.0)
    import inspect
    assert inspect.signature(fastnerf.render.render_rays).parameters['occupancy'].default is None


@pytest.mark.parametrize('white_bkgd', [False, True])
@pytest.mark.parametrize('perturb', [0, 1])
def test_the_gpu_tests_grids_mask_enough_to_matter(white_bkgd, perturb):
    """The grids, networks and seeds test_gpu_occupancy.py fixes, on the CPU oracle alone: in each pass between 0.2 and 0.9 of
    the samples are masked, and the masked image differs from the plain one by more than 1e-2 somewhere."""
    rays = R.scene_rays(O)
    sdc, sdf = R.scene_networks(O)
    tr, u = R.scene_randoms(rays.shape[0], 64, 128, perturb)
    tr, u = (None if t is None else torch.from_numpy(t) for t in (tr, u))
    plain = R.render_rays_masked(O, rays, sdc, sdf, None, 0, 1, True, 64, 128, white_bkgd, tr, u)
    for name, (m, lo, hi, oo) in R.scene_grids().items():
        r = R.render_rays_masked(O, rays, sdc, sdf, m, lo, hi, oo, 64, 128, white_bkgd, tr, u)
        for b in (r['bits0'], r['bits1']):
            assert 0.2 < 1.0 - b.mean() < 0.9, (name, 1.0 - b.mean())
        assert float((r['rgb_map'] - plain['rgb_map']).abs().max()) > 1e-2, name
        assert ((r['raw0'] == 0).all(-1).numpy() == ~r['bits0']).all()
