"""What training through an occupancy grid promises without a GPU: the ctypes mirror of fn_step_args ends with the two new
fields, the step refuses a grid it cannot honour before anything is enqueued, and the new entry points
validate their arguments."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


@pytest.fixture(scope='module')
def lib():
    import fastnerf
    return fastnerf._lib


def test_step_args_end_with_the_grid(lib):
    S = lib.StepArgs
    names = [f[0] for f in S._fields_]
    assert names[-2:] == ['occ', 'occ_counts'] and names[-3] == 'adam_t'
    assert lib.lib().fastnerf_step_args_size() == C.sizeof(S)
    assert S.occ.offset % 8 == 0 and S.occ_counts.offset == S.occ.offset + 8 and C.sizeof(S) == S.occ_counts.offset + 8
    a = S()
    assert not a.occ and not a.occ_counts      # a zeroed struct is the step without a grid


def test_the_step_refuses_before_it_enqueues(lib):
    l = lib.lib()
    a = lib.StepArgs()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    a.n, a.N_samples, a.N_importance, a.math_mode, a.net_floats = 4, 8, 0, 2, 16
    a.params = a.grads = a.packed_fwd_c = a.packed_bwd_c = p
    grid = lib.OccGrid(p, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_int32 * 3)(2, 2, 2), 0)
    a.occ = C.addressof(grid)
    a.live = 0
    assert l.fastnerf_train_step(C.byref(a), 1, None) == -1
    assert b'compacted step' in l.fastnerf_last_error() and b'no list' in l.fastnerf_last_error()
    a.live = 1
    a.noise0 = p
    assert l.fastnerf_train_step(C.byref(a), 1, None) == -1
    assert b'sigma noise' in l.fastnerf_last_error() and b'before the relu' in l.fastnerf_last_error()
    a.noise0 = None
    assert l.fastnerf_train_step(C.byref(a), 1, None) == -1 and b'live_ws' in l.fastnerf_last_error()


def test_entry_points_validate(lib):
    l = lib.lib()
    grid = lib.OccGrid(None, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_int32 * 3)(2, 3, 4), 0)
    assert l.fastnerf_occ_cell_points(grid, 0, 0, 0, None, None) == 0          # no cells: nothing to do, the bits are not needed
    assert l.fastnerf_occ_cell_points(grid, 24, 1, 0, None, None) == -1        # past the last cell
    assert l.fastnerf_occ_cell_points(grid, -1, 1, 0, None, None) == -1
    assert l.fastnerf_occ_cell_points(grid, 0, 1, 0, None, None) == -1         # no output buffer
    bad = lib.OccGrid(None, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 0, 1), (C.c_int32 * 3)(2, 3, 4), 0)
    assert l.fastnerf_occ_cell_points(bad, 0, 0, 0, None, None) == -1          # inv must be > 0
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert l.fastnerf_occ_update(None, None, 0, 1, 2, 3, 4, 0.9, 0.0, 0, p, p, None, None) == -1      # cells without logits
    assert l.fastnerf_occ_update(p, None, 20, 5, 2, 3, 4, 0.9, 0.0, 0, p, p, None, None) == -1        # past the last cell
    assert l.fastnerf_occ_update(p, None, 0, 1, 2, 3, 4, 1.5, 0.0, 0, p, p, None, None) == -1         # decay in [0, 1]
    assert l.fastnerf_occ_update(p, None, 0, 1, 2, 3, 4, 0.9, float('nan'), 0, p, p, None, None) == -1
    assert l.fastnerf_occ_update(p, None, 0, 1, 2, 3, 4, 0.9, 0.0, 1, p, p, None, None) == -1         # dilation needs scratch
    assert l.fastnerf_occ_update(p, None, 0, 1, 0, 3, 4, 0.9, 0.0, 0, p, p, None, None) == -1
