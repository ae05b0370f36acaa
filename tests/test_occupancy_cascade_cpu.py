"""Occupancy cascade, the part that needs no GPU: the restatement of tests/occ_cascade_numpy.py against a brute-force loop, the
.npz layout, the new symbols and the struct in header / library / binding, the argument errors of the new entry points, and the
check that the cascade the masked-render GPU tests fix puts every level -- and the 'no level' outcome -- in play."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import occ_cascade_numpy as RC
import occ_numpy as R
from oracle import nerf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['fastnerf_occ_query_cascade', 'fastnerf_occ_classify_cascade', 'fastnerf_render_rays_fwd_occ_cascade']
F32 = np.float32


# ---- the restatement against a brute-force loop ------------------------------------------------------------------------------
def brute(levels, outside, p):
    """One point, one level at a time, one axis at a time, in numpy float32 scalars."""
    for mask, lo, hi in levels:
        lo3, hi3 = np.broadcast_to(np.asarray(lo, F32), (3,)), np.broadcast_to(np.asarray(hi, F32), (3,))
        idx = []
        for a in range(3):
            inv = F32(np.float64(mask.shape[a]) / (np.float64(hi3[a]) - np.float64(lo3[a])))
            with np.errstate(invalid='ignore', over='ignore'):
                f = np.floor(F32(F32(p[a] - lo3[a]) * inv))
            if not (f >= 0 and f < mask.shape[a]):
                break
            idx.append(int(f))
        if len(idx) == 3:
            return bool(mask[idx[0], idx[1], idx[2]])
    return bool(outside)


def special_points(levels, rs):
    pts = []
    for mask, lo, hi in levels:
        lo3, hi3 = np.broadcast_to(np.asarray(lo, F32), (3,)), np.broadcast_to(np.asarray(hi, F32), (3,))
        for ax in range(3):      # on the two faces of this level's box, and an ulp to either side of them
            for v in (lo3[ax], hi3[ax]):
                for w in (v, np.nextafter(v, F32(-np.inf)), np.nextafter(v, F32(np.inf))):
                    p = (lo3 + (hi3 - lo3) * rs.rand(6, 3)).astype(F32)
                    p[:, ax] = w
                    pts.append(p)
        pts.append(np.stack([lo3, hi3, np.nextafter(lo3, F32(-np.inf)), np.nextafter(hi3, F32(-np.inf))]))
    pts.append((rs.rand(60, 3) * 8 - 4).astype(F32))        # anywhere: inside several boxes, one, none
    pts.append((rs.rand(40, 3) * 1.2 - 0.6).astype(F32))     # inside every box of the scene cascade
    odd = (rs.rand(12, 3) - 0.5).astype(F32)
    for i, v in enumerate((np.nan, np.inf, -np.inf, 3e38)):
        for ax in range(3):
            odd[i * 3 + ax, ax] = v
    pts.append(odd)
    return np.concatenate(pts, 0)


def test_restatement_equals_a_brute_force_loop():
    rs = np.random.RandomState(4)
    levels, _ = RC.scene_cascade()
    apart = [(rs.rand(3, 4, 5) < 0.5, np.array([0.0, 0.0, 0.0], F32), np.array([1.0, 2.0, 3.0], F32)),      # overlapping, not nested
             (rs.rand(4, 4, 4) < 0.5, np.array([0.5, -1.0, 1.0], F32), np.array([2.5, 1.0, 4.0], F32)),
             (rs.rand(2, 2, 2) < 0.5, F32(-9.0), F32(-8.0))]                                                  # disjoint from both
    for lv in (levels, levels[::-1], apart, levels[:1]):
        pts = special_points(lv, rs)
        assert 200 < pts.shape[0] < 1000
        who = RC.decided_by(lv, pts)
        for outside in (False, True):
            got = RC.query(lv, outside, pts)
            ref = np.array([brute(lv, outside, p) for p in pts])
            assert np.array_equal(got, ref), pts[got != ref][:5]
        assert bool((who[~np.isfinite(pts).all(-1)] == -1).all())      # every non-finite point ends in 'no level'
        if lv is levels or lv is apart:
            assert set(np.unique(who).tolist()) == {-1, 0, 1, 2}
    assert set(np.unique(RC.decided_by(levels[::-1], special_points(levels, rs))).tolist()) == {-1, 0}      # the outer box first hides the rest
    pts = special_points(levels, rs)
    both = RC.inside(levels[0], pts) & RC.inside(levels[1], pts) & RC.inside(levels[2], pts)
    assert both.sum() >= 40 and bool((RC.decided_by(levels, pts)[both] == 0).all())       # inside several boxes: the first decides
    assert bool((RC.decided_by(levels[::-1], pts)[both] == 0).all())                      # ... whichever grid that is
    one = levels[:1]
    for outside in (False, True):      # a cascade of one level is the single grid
        assert np.array_equal(RC.query(one, outside, pts), R.query(one[0][0], one[0][1], one[0][2], outside, pts))


def test_only_the_cascades_outside_flag_is_read():
    levels, _ = RC.scene_cascade()
    far = np.array([[7.0, 0.0, 0.0], [np.nan, 0.0, 0.0]], F32)
    between = np.array([[1.9, 0.0, 0.0]], F32)       # outside levels 0 and 1, inside level 2, on its occupied side
    assert RC.query(levels, True, far).all() and not RC.query(levels, False, far).any()
    assert RC.decided_by(levels, between).tolist() == [2] and RC.query(levels, False, between).all()


# ---- the file format ---------------------------------------------------------------------------------------------------------
def pack(mask):
    flat = np.zeros((mask.size + 31) // 32 * 32, np.uint32)
    flat[:mask.size] = mask.reshape(-1)
    return (flat.reshape(-1, 32) << np.arange(32, dtype=np.uint32)).sum(1).astype(np.uint32)


def test_npz_layout_round_trips_with_numpy_alone(tmp_path):
    levels, oo = RC.scene_cascade()
    fields = dict(levels=np.asarray(len(levels), np.int64), outside_occupied=np.asarray(oo))
    for i, (m, lo, hi) in enumerate(levels):
        fields.update({'l%d_words' % i: pack(m), 'l%d_shape' % i: np.asarray(m.shape, np.int64),
                       'l%d_lo' % i: np.broadcast_to(np.asarray(lo, F32), (3,)).copy(), 'l%d_hi' % i: np.broadcast_to(np.asarray(hi, F32), (3,)).copy(),
                       'l%d_outside_occupied' % i: np.asarray(True)})
    p = str(tmp_path / 'c.npz')
    with open(p, 'wb') as fh:
        np.savez(fh, **fields)
    with np.load(p) as f:
        assert int(f['levels']) == 3 and 'words' not in f.files
        for i, (m, lo, hi) in enumerate(levels):
            assert np.array_equal(R.words_to_mask(f['l%d_words' % i], f['l%d_shape' % i]), m)
    import fastnerf
    doc = fastnerf.occupancy.OccupancyCascade.save.__doc__
    assert 'l{i}_' in doc and 'levels' in doc and 'outside_occupied' in doc
    with pytest.raises(ValueError, match='cascade'):      # never level 0 silently
        fastnerf.occupancy.OccupancyGrid.load(p, device='cpu')
    single = str(tmp_path / 'g.npz')
    with open(single, 'wb') as fh:
        np.savez(fh, words=pack(levels[0][0]), shape=np.asarray(levels[0][0].shape, np.int64), lo=np.zeros(3, F32), hi=np.ones(3, F32),
                 outside_occupied=np.asarray(True))
    with pytest.raises(ValueError, match='single'):
        fastnerf.occupancy.OccupancyCascade.load(single, device='cpu')


# ---- header, library, binding ------------------------------------------------------------------------------------------------
def test_new_symbols_and_struct_in_header_library_and_binding():
    from fastnerf import _lib
    src = open(os.path.join(ROOT, 'include', 'fastnerf.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(fastnerf_\w+)\s*\(', src))
    lib = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(lib, s) and s in _lib.SIGNATURES, s
    m = re.search(r'typedef struct fn_occ_cascade \{(.*?)\} fn_occ_cascade;', src, re.S)
    assert m and re.sub(r'\s+', ' ', m.group(1)).strip() == 'int32_t levels; int32_t reserved; fn_occ_grid level[FN_OCC_MAX_LEVELS];'
    assert re.search(r'#define FN_OCC_MAX_LEVELS 8\b', src) and _lib.OCC_MAX_LEVELS == 8
    # the header's layout: two int32, then 8 fn_occ_grid of 48 bytes (8-byte aligned: they start with a pointer)
    assert ctypes.sizeof(_lib.OccGrid) == 48                      # unchanged
    assert ctypes.sizeof(_lib.OccCascade) == 8 + 8 * 48
    assert (_lib.OccCascade.levels.offset, _lib.OccCascade.reserved.offset, _lib.OccCascade.level.offset) == (0, 4, 8)
    assert [f[0] for f in _lib.OccCascade._fields_] == ['levels', 'reserved', 'level']
    assert lib.fastnerf_step_args_size() == ctypes.sizeof(_lib.StepArgs)      # unchanged: the cascade is not in fn_step_args
    assert [f[0] for f in _lib.StepArgs._fields_][-2:] == ['occ', 'occ_counts']
    for name, i in (('fastnerf_occ_query_cascade', 0), ('fastnerf_occ_classify_cascade', 0), ('fastnerf_render_rays_fwd_occ_cascade', 17)):
        assert _lib.SIGNATURES[name][1][i] == ctypes.POINTER(_lib.OccCascade)
        single = name[:-len('_cascade')]
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[single][1])      # the same arguments
        assert _lib.SIGNATURES[name][1][:i] + _lib.SIGNATURES[name][1][i + 1:] == _lib.SIGNATURES[single][1][:i] + _lib.SIGNATURES[single][1][i + 1:]


def good_cascade(levels=3):
    """A cascade whose descriptors pass every check; its `words` are not device memory: nothing may be launched with it."""
    from fastnerf import _lib
    c = _lib.OccCascade()
    c.levels = levels
    for l in range(min(levels, 8)):
        g = c.level[l]
        g.words = 0x1000
        for a in range(3):
            g.lo[a], g.inv[a], g.n[a] = -1.0, 4.0, 8
    return c


def faulty_cascades():
    zero, nine, inv, words, nan = good_cascade(0), good_cascade(9), good_cascade(), good_cascade(), good_cascade(2)
    inv.level[1].inv[2] = 0.0
    words.level[2].words = None
    nan.level[0].lo[1] = float('nan')
    neg = good_cascade()
    neg.level[0].inv[0] = -1.0
    cells = good_cascade()
    cells.level[1].n[0] = 0
    return {'levels = 0': zero, 'levels = 9': nine, 'inv == 0': inv, 'inv < 0': neg, 'null words': words, 'NaN lo': nan, 'n == 0': cells}


@pytest.mark.parametrize('case', ['levels = 0', 'levels = 9', 'inv == 0', 'inv < 0', 'null words', 'NaN lo', 'n == 0'])
def test_argument_errors_name_the_function(case):
    from fastnerf import _lib
    lib = _lib.lib()
    c = faulty_cascades()[case]
    p = 0x1000      # never dereferenced: the argument check comes before any launch
    assert lib.fastnerf_occ_query_cascade(c, 4, p, p, None) != 0
    assert lib.fastnerf_last_error().startswith(b'fastnerf_occ_query_cascade: bad argument')
    assert lib.fastnerf_occ_classify_cascade(c, 4, 8, p, p, p, p, p, p, None) != 0
    assert lib.fastnerf_last_error().startswith(b'fastnerf_occ_classify_cascade: bad argument')
    rc = lib.fastnerf_render_rays_fwd_occ_cascade(0, 4, 8, 8, p, 0, 0, 1, 0, None, None, 0, 0, p, p, p, p, c, p, p, *([p] * 16), 0, None)
    assert rc != 0 and lib.fastnerf_last_error().startswith(b'fastnerf_render_rays_fwd_occ_cascade: bad argument'), lib.fastnerf_last_error()


def test_other_argument_errors_of_the_new_entry_points():
    from fastnerf import _lib
    lib = _lib.lib()
    c, p = good_cascade(), 0x1000
    assert lib.fastnerf_occ_query_cascade(None, 4, p, p, None) != 0 and b'fastnerf_occ_query_cascade' in lib.fastnerf_last_error()
    assert lib.fastnerf_occ_query_cascade(c, -1, p, p, None) != 0 and b'fastnerf_occ_query_cascade' in lib.fastnerf_last_error()
    assert lib.fastnerf_occ_query_cascade(c, 4, None, p, None) != 0 and b'fastnerf_occ_query_cascade' in lib.fastnerf_last_error()
    assert lib.fastnerf_occ_query_cascade(c, 0, None, None, None) == 0      # nothing to do, as fastnerf_occ_query
    assert lib.fastnerf_occ_classify_cascade(c, 0, 8, p, p, p, p, p, p, None) != 0 and b'fastnerf_occ_classify_cascade' in lib.fastnerf_last_error()
    assert lib.fastnerf_occ_classify_cascade(c, 1 << 20, 1 << 11, p, p, p, p, p, p, None) != 0      # n * S >= 2^31
    assert lib.fastnerf_occ_classify_cascade(c, 4, 8, p, p, p, p, p, None, None) != 0 and b'fastnerf_occ_classify_cascade' in lib.fastnerf_last_error()
    tail = [p] * 16 + [0, None]
    assert lib.fastnerf_render_rays_fwd_occ_cascade(3, 4, 8, 8, p, 0, 0, 1, 0, None, None, 0, 0, p, p, p, p, c, p, p, *tail) != 0
    assert lib.fastnerf_last_error().startswith(b'fastnerf_render_rays_fwd_occ_cascade:')
    assert lib.fastnerf_render_rays_fwd_occ_cascade(0, 4, 8, 8, p, 0, 0, 1, 0, None, None, 0, 0, p, p, p, p, None, p, p, *tail) != 0
    assert lib.fastnerf_last_error().startswith(b'fastnerf_render_rays_fwd_occ_cascade: null pointer')
    # the single-grid function keeps its own name in its texts
    assert lib.fastnerf_render_rays_fwd_occ(3, 4, 8, 8, p, 0, 0, 1, 0, None, None, 0, 0, p, p, p, p, None, p, p, *tail) != 0
    assert lib.fastnerf_last_error().startswith(b'fastnerf_render_rays_fwd_occ: bad argument')


# ---- the surface -------------------------------------------------------------------------------------------------------------
def test_surface_refuses_cpu_tensors_without_a_gpu():
    import inspect
    import fastnerf
    occ = fastnerf.occupancy
    assert hasattr(occ, 'OccupancyCascade')
    with pytest.raises(RuntimeError):      # the levels are OccupancyGrids: no host grid exists to make a cascade of
        occ.OccupancyCascade([occ.OccupancyGrid.from_mask(torch.ones(4, 4, 4, dtype=torch.bool), -1.0, 1.0)])
    with pytest.raises(ValueError):
        occ.OccupancyCascade([])
    with pytest.raises(TypeError):
        occ.OccupancyCascade([object()])
    with pytest.raises(ValueError):
        occ.OccupancyCascade.from_network({}, levels=9)
    with pytest.raises(ValueError):
        occ.OccupancyCascade.from_network({}, levels=3, N=[8, 8])
    sig = inspect.signature(occ.OccupancyCascade.from_network).parameters
    assert [sig[k].default for k in ('levels', 'N', 'bound', 'growth', 'threshold', 'dilate', 'which', 'outside_occupied')] == \
        [3, 256, 1.2, 2.0, 0., 1, 'both', True]
    assert inspect.signature(occ.OccupancyCascade.__init__).parameters['outside_occupied'].default is None
    for name in ('query', 'classify', 'decided_by', 'occupied_fraction', 'save', 'load', 'levels'):
        assert hasattr(occ.OccupancyCascade, name), name
    c = good_cascade()
    with pytest.raises(RuntimeError):
        fastnerf.ops.occ_query(c, torch.zeros(1, 3))
    with pytest.raises(RuntimeError):
        fastnerf.ops.occ_classify(c, torch.zeros(2, 11), torch.zeros(2, 4))
    # ops dispatches on the descriptor's type and takes nothing else
    assert fastnerf.ops._occ_entry(c, 'fastnerf_occ_query')[1] == 'fastnerf_occ_query_cascade'
    assert fastnerf.ops._occ_entry(c.level[0], 'fastnerf_occ_query')[1] == 'fastnerf_occ_query'
    with pytest.raises(TypeError):
        fastnerf.ops._occ_entry(object(), 'fastnerf_occ_query')


# ---- the scene of the GPU tests ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('white_bkgd', [False, True])
@pytest.mark.parametrize('perturb', [0, 1])
def test_the_gpu_tests_cascade_puts_every_level_in_play(white_bkgd, perturb):
    """The cascade, networks and seeds test_gpu_occupancy_cascade.py fixes, on the CPU oracle alone: in each pass every level and
    the 'no level' outcome decide at least 2 % of the samples, between 0.2 and 0.9 of the samples are masked, and the masked image
    differs from the plain one by more than 1e-2 somewhere."""
    rays = R.scene_rays(O)
    sdc, sdf = R.scene_networks(O)
    tr, u = R.scene_randoms(rays.shape[0], 64, 128, perturb)
    tr, u = (None if t is None else torch.from_numpy(t) for t in (tr, u))
    levels, oo = RC.scene_cascade()
    plain = RC.render_rays_masked(O, rays, sdc, sdf, None, True, 64, 128, white_bkgd, tr, u)
    r = RC.render_rays_masked(O, rays, sdc, sdf, levels, oo, 64, 128, white_bkgd, tr, u)
    for who, b in ((r['who0'], r['bits0']), (r['who1'], r['bits1'])):
        sh = RC.shares(who, len(levels))
        print('decided per level, none:', [round(s, 4) for s in sh], 'masked %.4f' % (1.0 - b.mean()))
        assert min(sh) >= 0.02, sh
        assert 0.2 < 1.0 - b.mean() < 0.9
    assert float((r['rgb_map'] - plain['rgb_map']).abs().max()) > 1e-2
    assert ((r['raw0'] == 0).all(-1).numpy() == ~r['bits0']).all()
    # leaving a level out, or reading another level's flag, changes the bits: the GPU comparison cannot pass without every level
    z = O.coarse_z(torch.as_tensor(rays)[:, 6:7], torch.as_tensor(rays)[:, 7:8], 64, False, tr).numpy()
    for drop in range(3):
        assert not np.array_equal(RC.classify(levels[:drop] + levels[drop + 1:], oo, rays, z), r['bits0'])
    assert not np.array_equal(RC.classify(levels, not oo, rays, z), r['bits0'])
