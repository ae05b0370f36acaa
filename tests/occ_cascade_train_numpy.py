"""numpy restatement of what training through an occupancy cascade adds (include/fastnerf.h, "cascade, trained"): the own cells
of a level, the concatenation of the levels' own lists, and the cursor that rotates over it.

A level here is (shape, lo, hi): (nx, ny, nz), float32 bounds -- what tests/occ_cascade_numpy.py takes with a mask in front.

Covered rule, in float64 from each level's fp32 lo, its fp32 inv (occ_numpy.inv_of: what fn_occ_grid carries) and its n:
w = 1 / (double)inv, hi = lo + n * w, every product and sum rounded on its own (numpy does not contract).  Cell (i0, i1, i2) of level l
is covered when there is ONE level j < l with, on every axis a and m = dilate + 1,
    lo_l[a] + (i_a - m) * w_l[a] >= lo_j[a] + w_j[a]     and     lo_l[a] + (i_a + 1 + m) * w_l[a] <= hi_j[a] - w_j[a]."""
import numpy as np

import occ_numpy as R

F32 = np.float32
MAX_TRAIN_N = 4096


def geometry(level):
    """(lo, w, hi) float64 [3] of a level, from its fp32 lo and inv."""
    shape, lo, hi = level
    lo64 = np.broadcast_to(np.asarray(lo, F32), (3,)).astype(np.float64)
    w = 1.0 / R.inv_of(shape, F32(lo), F32(hi)).astype(np.float64)
    return lo64, w, lo64 + np.asarray(shape, np.float64) * w


def covered(levels, l, dilate):
    """bool [nx, ny, nz] of level l: the cells a lookup never reads (and dilation never needs)."""
    shape = tuple(int(s) for s in levels[l][0])
    lo_l, w_l, _ = geometry(levels[l])
    m = int(dilate) + 1
    out = np.zeros(shape, bool)
    for j in range(l):
        lo_j, w_j, hi_j = geometry(levels[j])
        per_axis = []
        for a in range(3):
            i = np.arange(shape[a], dtype=np.float64)
            left = lo_l[a] + (i - m) * w_l[a]
            right = lo_l[a] + (i + 1 + m) * w_l[a]
            per_axis.append((left >= lo_j[a] + w_j[a]) & (right <= hi_j[a] - w_j[a]))
        out |= per_axis[0][:, None, None] & per_axis[1][None, :, None] & per_axis[2][None, None, :]
    return out


def own_cells(levels, l, dilate):
    """Ascending int32 linear indices c = (i*ny + j)*nz + k of level l's own cells."""
    return np.nonzero(~covered(levels, l, dilate).reshape(-1))[0].astype(np.int32)


def concatenation(levels, dilate):
    """(own int32 [total], offsets int64 [levels + 1]): the levels' own lists, level 0 first."""
    lists = [own_cells(levels, l, dilate) for l in range(len(levels))]
    return np.concatenate(lists), np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.int64)


def refresh_slice(cursor, primed, total, cells_per_call):
    """(positions int64 [..] in the order they are refreshed, next cursor) of one update() call: everything on the first call or
    without a budget, else cells_per_call positions from the cursor on, wrapping round."""
    if cells_per_call is None or not primed or cells_per_call >= total:
        return np.arange(total, dtype=np.int64), cursor
    k = max(1, int(cells_per_call))
    return (cursor + np.arange(k, dtype=np.int64)) % total, (cursor + k) % total


def level_of(offsets, positions):
    """(level, index into that level's own list) of positions of the concatenation."""
    l = np.searchsorted(offsets, positions, side='right') - 1
    return l, positions - offsets[l]


# ---- the scenes of the tests ---------------------------------------------------------------------------------------------------------
def cube(n, bound):
    return ((n,) * 3 if np.ndim(n) == 0 else tuple(n)), np.full(3, -bound, F32), np.full(3, bound, F32)


def scenes():
    """name -> levels.  concentric: OccupancyCascade.for_training(levels=3, N=16, bound=1.2, growth=2); noncubic: the same boxes cut
    into (6, 5, 7) / (5, 5, 4) / (4, 6, 3); offset: two boxes that overlap without nesting; buried: the middle level lies wholly
    inside the inner one (its own list may be empty), the outer one around both."""
    return {
        'concentric': [cube(16, 1.2 * 2.0 ** l) for l in range(3)],
        'noncubic': [cube(s, 1.2 * 2.0 ** l) for l, s in enumerate([(6, 5, 7), (5, 5, 4), (4, 6, 3)])],
        'offset': [((8, 9, 10), np.array([0.0, 0.0, 0.0], F32), np.array([1.0, 2.0, 3.0], F32)),
                   ((12, 12, 12), np.array([0.5, -1.0, 1.0], F32), np.array([2.5, 1.0, 4.0], F32))],
        'buried': [cube(16, 1.0), ((4, 4, 4), np.full(3, -0.25, F32), np.full(3, 0.5, F32)), cube(20, 1.5)],
    }


def points(levels, count, seed):
    """float32 [count, 3]: half uniform over a box a little larger than all levels, half with one coordinate snapped onto a cell or box
    face of some level (as fp32 can name it) or a nextafter neighbour of it."""
    rs = np.random.RandomState(seed)
    lo = np.min([np.broadcast_to(L[1], (3,)) for L in levels], 0).astype(np.float64)
    hi = np.max([np.broadcast_to(L[2], (3,)) for L in levels], 0).astype(np.float64)
    span = hi - lo
    pts = (lo - 0.1 * span + 1.2 * span * rs.rand(count, 3)).astype(F32)
    faces = []
    for shape, l_lo, l_hi in levels:
        for a in range(3):
            lo_a, hi_a = np.float64(np.broadcast_to(l_lo, (3,))[a]), np.float64(np.broadcast_to(l_hi, (3,))[a])
            f = (lo_a + (hi_a - lo_a) * np.arange(shape[a] + 1) / shape[a]).astype(F32)
            faces.append((a, np.concatenate([f, np.nextafter(f, F32(-np.inf)), np.nextafter(f, F32(np.inf))])))
    half = count // 2
    pick = rs.randint(0, len(faces), half)
    for q in range(len(faces)):
        rows = np.nonzero(pick == q)[0]
        a, vals = faces[q]
        pts[rows, a] = vals[rs.randint(0, vals.size, rows.size)]
    return pts
