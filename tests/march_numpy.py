"""fp32 numpy restatement of the marched render of include/fastnerf.h ("marched render": fastnerf_occ_march, fastnerf_march_list), on top of
the lookups of tests/occ_numpy.py and tests/occ_cascade_numpy.py: the test oracle of csrc/march.hip and render_rays(..., march=K).

Two layers, kept apart so that one checks the other (tests/test_march_cpu.py):
  the contract   lattice -> live bits -> `sequence` (runs, each with its closing entry) -> `packed_row` (cap, overflow, padding)
  the kernel     `march_round`: one round of occ_march_kernel, operation for operation, with its per-ray state

A grid is ('grid', mask, lo, hi, outside_occupied) or ('cascade', levels, outside_occupied)."""
import numpy as np

import occ_cascade_numpy as RC
import occ_numpy as R

F32 = np.float32
GROUP = 4      # MARCH_GROUP of csrc/march.hip: lattice points looked up per batch


# ---- the lattice ---------------------------------------------------------------------------------------------------------------
def lin01(i, S):
    """lin01 of csrc/depths.h: torch.linspace(0, 1, S) in fp32, evaluated from the nearer end."""
    i = np.asarray(i)
    step = F32(1) / F32(S - 1)
    lo = (step * i.astype(F32)).astype(F32)
    hi = (F32(1) - (step * (S - 1 - i).astype(F32)).astype(F32)).astype(F32)
    return np.where(i < S // 2, lo, hi).astype(F32)


def lattice(rays11, K, lindisp=False):
    """float32 [n, K + 1]: z_0 .. z_{K-1} = coarse_depth(near, far, k, K, lindisp), and z_K = z_{K-1} + (z_{K-1} - z_{K-2})."""
    r = np.asarray(rays11, F32)
    near, far = r[:, 6:7], r[:, 7:8]
    t = lin01(np.arange(K), K)[None, :]
    with np.errstate(all='ignore'):
        omt = (F32(1) - t).astype(F32)
        if not lindisp:
            z = ((near * omt).astype(F32) + (far * t).astype(F32)).astype(F32)
        else:
            a = ((F32(1) / near).astype(F32) * omt).astype(F32)
            b = ((F32(1) / far).astype(F32) * t).astype(F32)
            z = (F32(1) / (a + b).astype(F32)).astype(F32)
        zK = (z[:, K - 1] + (z[:, K - 1] - z[:, K - 2]).astype(F32)).astype(F32)
    return np.concatenate([z, zK[:, None]], -1).astype(F32)


def live_bits(grid, rays11, z):
    """bool [n, S]: the dense classify of the depths z [n, S] (occ_numpy.classify / occ_cascade_numpy.classify)."""
    if grid[0] == 'grid':
        return np.asarray(R.classify(grid[1], grid[2], grid[3], grid[4], rays11, z), bool)
    return np.asarray(RC.classify(grid[1], grid[2], rays11, z), bool)


# ---- the contract --------------------------------------------------------------------------------------------------------------
def runs(live_row):
    """[(a, b)]: the maximal runs a .. b of consecutive live lattice points, in depth order."""
    lv = np.concatenate([[False], np.asarray(live_row, bool), [False]]).astype(np.int8)
    d = np.diff(lv)
    return list(zip(np.nonzero(d == 1)[0].tolist(), (np.nonzero(d == -1)[0] - 1).tolist()))


def sequence(live_row, zlat_row):
    """The packed sequence of one ray: [(z, k)], per run (z_a, a) .. (z_b, b) and the closing entry (z_{b+1}, -1)."""
    seq = []
    for a, b in runs(live_row):
        seq += [(zlat_row[k], k) for k in range(a, b + 1)] + [(zlat_row[b + 1], -1)]
    return seq


def packed_row(seq, C, z0):
    """(z float32 [C], kidx int32 [C], overflow) of a sequence: its first min(L, C) entries, the last kept one without its index when
    L > C, then padding (z of the slot before, -1); an empty sequence is (z0, -1) throughout."""
    z = np.empty(C, F32)
    k = np.full(C, -1, np.int32)
    m = min(len(seq), C)
    for s in range(m):
        z[s], k[s] = seq[s]
    overflow = len(seq) > C
    if overflow:
        k[C - 1] = -1
    z[m:] = z[m - 1] if m else z0
    return z, k, overflow


def packed(live, zlat, C):
    """The packed rows of all rays from the contract: (z [n, C], kidx [n, C], overflow bool [n])."""
    rows = [packed_row(sequence(live[r], zlat[r]), C, zlat[r, 0]) for r in range(live.shape[0])]
    return np.stack([a for a, _, _ in rows]), np.stack([b for _, b, _ in rows]), np.array([c for _, _, c in rows], bool)


# ---- the kernel ----------------------------------------------------------------------------------------------------------------
Z_UNSET, K_UNSET = F32(np.nan), np.int32(-2)      # what a slot holds that no round has written (the device buffers are uninitialised there)


def march_round(live, zlat, C, s0, s1, prev=None, trans=None, eps=0.0):
    """One round [s0, s1) of occ_march_kernel for all rays.  live bool [n, K] are the answers of the lookups, zlat [n, K + 1] the
    lattice.  prev: (z, kidx, overflow, state) of the round before (None exactly when s0 == 0).  trans float32 [n] or None.
    -> (z [n, C], kidx [n, C], overflow uint8 [n], state int32 [n, 2]), new arrays."""
    n, K = live.shape
    assert (prev is None) == (s0 == 0) and 0 <= s0 < s1 <= C
    if prev is None:
        z, kidx = np.full((n, C), Z_UNSET, F32), np.full((n, C), K_UNSET, np.int32)
        overflow, state = np.zeros(n, np.uint8), np.zeros((n, 2), np.int32)
    else:
        z, kidx, overflow, state = (np.array(a) for a in prev)
    eps = F32(eps)
    for r in range(n):
        lv_r, zl = live[r], zlat[r]

        def group(k):
            return sum(1 << j for j in range(GROUP) if k + j < K and lv_r[k + j])

        k, st = (0, 0) if s0 == 0 else (int(state[r, 0]), int(state[r, 1]))
        k = min(max(k, 0), K)
        pend = bool(st & 1)
        nv = min((st >> 4) & 3, K - k)
        m = (st >> 1) & ((1 << nv) - 1)
        s = s0
        zlast = z[r, s0 - 1] if s0 > 0 else zl[0]
        ovf = False
        with np.errstate(invalid='ignore'):
            cut = trans is not None and not (F32(trans[r]) > eps)
        if cut:
            if pend:
                zlast = zl[k]
                z[r, s], kidx[r, s] = zlast, -1
                s += 1
                pend = False
        else:
            while s < s1:
                if nv == 0:
                    if k >= K:
                        break
                    m = group(k)
                    nv = min(GROUP, K - k)
                if m == 0 and not pend:      # (the kernel consumes these one by one, without a store: the same state)
                    k += nv
                    nv = 0
                    continue
                lv = bool(m & 1)
                m >>= 1
                nv -= 1
                if lv or pend:
                    last = s == C - 1
                    zlast = zl[k]
                    z[r, s] = zlast
                    kidx[r, s] = k if (lv and not last) else -1
                    ovf = ovf or (lv and last)
                    s += 1
                    pend = lv and not last
                k += 1
            if s < s1 and pend:
                zlast = zl[K]
                z[r, s], kidx[r, s] = zlast, -1
                s += 1
                pend = False
            if s == C:
                while not ovf:
                    if nv == 0:
                        if k >= K:
                            break
                        m = group(k)
                        nv = min(GROUP, K - k)
                    ovf = m != 0
                    k += nv
                    nv = 0
                    m = 0
                k, nv, m = K, 0, 0
        z[r, s:s1] = zlast
        kidx[r, s:s1] = -1
        if s1 < C:
            z[r, s1] = zl[k] if pend else zlast
        state[r] = (k, int(pend) | (m << 1) | (nv << 4))
        if s0 == 0:
            overflow[r] = 1 if ovf else 0
        elif ovf:
            overflow[r] = 1
    return z, kidx, overflow, state


def march(live, zlat, C, B=None, trans_of=None, eps=0.0):
    """All rounds: segments of B slots (None: one round).  trans_of(j, z, kidx) -> float32 [n] or None: the transmittance that round
    j >= 1 sees.  -> (z, kidx, overflow, state) after the last round."""
    B = C if B is None else min(int(B), C)
    cur = None
    for j, s0 in enumerate(range(0, C, B)):
        tr = trans_of(j, cur[0], cur[1]) if (trans_of is not None and j > 0) else None
        cur = march_round(live, zlat, C, s0, min(s0 + B, C), cur, tr, eps)
    return cur


def live_list(kidx, s0, s1):
    """int64: the ascending indices ray * C + slot of the live slots of the segment [s0, s1)."""
    r, c = np.nonzero(np.asarray(kidx)[:, s0:s1] >= 0)
    return r * kidx.shape[1] + s0 + c


# ---- compositing in float64 ----------------------------------------------------------------------------------------------------
def composite64(raw, z, rays11):
    """dict of float64 maps of render.py:149-192 for one row layout (dense or packed): rgb [n, 3], acc, depth, disp, weights.  The
    1e-10 that raw2outputs adds to 1 - alpha is left out: it is below fp32 resolution beside 1 (the kernels' factor of an empty sample
    is exactly 1), while in float64 it would make the transmittance depend on the NUMBER of empty samples, K 1e-10 -- a property of the
    guard, not of where the samples lie."""
    raw = np.asarray(raw, F32).astype(np.float64)
    z = np.asarray(z, F32).astype(np.float64)
    d = np.asarray(rays11, F32)[:, 3:6].astype(np.float64)
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((z.shape[0], 1), 1e10)], -1) * np.linalg.norm(d, axis=-1)[:, None]
    with np.errstate(over='ignore', invalid='ignore'):
        alpha = 1.0 - np.exp(-np.maximum(raw[..., 3], 0.0) * dist)
    T = np.concatenate([np.ones((z.shape[0], 1)), np.cumprod(1.0 - alpha, -1)[:, :-1]], -1)
    w = alpha * T
    rgb = (w[..., None] / (1.0 + np.exp(-raw[..., :3]))).sum(-2)
    acc, depth = w.sum(-1), (w * z).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        disp = 1.0 / np.maximum(1e-10, depth / acc)
    return dict(rgb=rgb, acc=acc, depth=depth, disp=disp, weights=w)


def pack_raw(raw_dense, kidx):
    """raw [n, C, 4] of packed rows: the dense logits raw_dense [n, K, 4] at the live slots, zeros elsewhere."""
    kidx = np.asarray(kidx)
    out = np.take_along_axis(np.asarray(raw_dense), np.maximum(kidx, 0)[..., None], 1)
    return np.where((kidx >= 0)[..., None], out, 0).astype(np.asarray(raw_dense).dtype)


# ---- the scenes ----------------------------------------------------------------------------------------------------------------
def two_shells():
    """('grid', mask, lo, hi, False): two concentric occupied shells, 0.6 < r < 0.8 and 1.05 < r < 1.3, in a 32^3 box over +-1.5: a ray
    through the middle has four runs (outer, inner, inner, outer), one that misses the inner shell two."""
    c = (np.arange(32) + 0.5) / 32 * 3.0 - 1.5
    X, Y, Z = np.meshgrid(c, c, c, indexing='ij')
    r = np.sqrt(X * X + Y * Y + Z * Z)
    return ('grid', ((r > 0.6) & (r < 0.8)) | ((r > 1.05) & (r < 1.3)), F32(-1.5), F32(1.5), False)


def cascade2(outside_occupied=False):
    """('cascade', levels, outside_occupied): the first two levels of occ_cascade_numpy.scene_cascade.  With outside_occupied=False
    the far end of the test rays is empty; with True lattice point K - 1 of every test ray is live."""
    return ('cascade', RC.scene_cascade()[0][:2], bool(outside_occupied))


def scene_grids():
    """name -> grid of the march tests: ball and random of occ_numpy.scene_grids, two_shells, and the two-level cascade."""
    g = R.scene_grids()
    return {'ball': ('grid',) + tuple(g['ball']), 'random': ('grid',) + tuple(g['random']), 'two_shells': two_shells(),
            'cascade': cascade2(False)}
