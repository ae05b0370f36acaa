"""Vectorised numpy restatement of the marching-cubes contract of include/fastnerf.h (fastnerf_mc_*), the test oracle of
csrc/mesh.hip, plus the mesh checks the tests share (closedness, orientation, Euler characteristic, components, volume).

The triangle table is read from the library (fastnerf_mc_tables: a host call, no GPU); the classic corner / edge
numbering is restated here."""
import numpy as np

CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], np.int64)
EDGE_LO = np.array([0, 1, 3, 0, 4, 5, 7, 4, 0, 1, 2, 3], np.int64)
EDGE_AXIS = np.array([0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2], np.int64)


def tables():
    import fastnerf
    return fastnerf.ops.mc_tables()


def marching_cubes(vol, thr, tri_table=None):
    """-> (verts [V,3] float32 in index coordinates, tris [T,3] int64), in the contract's order."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    thr = np.float32(thr)
    if tri_table is None:
        tri_table = tables()[0]
    nx, ny, nz = vol.shape
    stride = np.array([ny * nz, nz, 1], np.int64)
    ins = vol > thr
    cross = np.zeros(vol.shape + (3,), bool)
    cross[:-1, :, :, 0] = ins[:-1] != ins[1:]
    cross[:, :-1, :, 1] = ins[:, :-1] != ins[:, 1:]
    cross[:, :, :-1, 2] = ins[:, :, :-1] != ins[:, :, 1:]
    flat = cross.reshape(-1, 3)
    cnt = flat.sum(1)
    vbase = np.zeros(flat.shape[0], np.int64)
    np.cumsum(cnt[:-1], out=vbase[1:])
    pidx, ax = np.nonzero(flat)                      # row-major: by point, then axis
    v = vol.reshape(-1)
    a, b = v[pidx], v[pidx + stride[ax]]
    t = (thr - a) / (b - a)                          # float32 throughout
    verts = np.stack(np.unravel_index(pidx, vol.shape), 1).astype(np.float32)
    verts[np.arange(pidx.size), ax] += t
    # triangles: cells with a non-empty case, in cell order, then table order
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for n, (ci, cj, ck) in enumerate(CORNERS):
        case |= ins[ci:nx - 1 + ci, cj:ny - 1 + cj, ck:nz - 1 + ck].astype(np.int64) << n
    ntri = (tri_table >= 0).sum(1) // 3
    cells = np.nonzero(ntri[case.reshape(-1)])[0]
    cc = case.reshape(-1)[cells]
    ci, cj, ck = np.unravel_index(cells, case.shape)
    p = (ci * ny + cj) * nz + ck                     # the cell's lower corner point
    rows = tri_table[cc][:, :15].astype(np.int64).reshape(-1, 5, 3)
    valid = rows[..., 0] >= 0
    e = rows[valid]                                  # [T, 3], cell-major then slot order
    pp = np.repeat(p, valid.sum(1))[:, None]
    q = pp + CORNERS[EDGE_LO[e]] @ stride
    axis = EDGE_AXIS[e]
    rank = flat[q, 0].astype(np.int64) * (axis > 0) + flat[q, 1].astype(np.int64) * (axis > 1)   # a count, not a bool sum
    tris = vbase[q] + rank
    return verts, tris.astype(np.int64)


# ---- mesh checks ---------------------------------------------------------------------------------------------------
def edge_stats(tris, V):
    """(every undirected edge in exactly 2 triangles, every directed edge once, number of undirected edges)."""
    t = np.asarray(tris, np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], 0)
    directed = d[:, 0] * V + d[:, 1]
    und = np.minimum(d[:, 0], d[:, 1]) * V + np.maximum(d[:, 0], d[:, 1])
    _, counts = np.unique(und, return_counts=True)
    return bool(np.all(counts == 2)), np.unique(directed).size == directed.size, counts.size


def euler(verts, tris):
    return len(verts) - edge_stats(tris, len(verts))[2] + len(tris)


def components(tris, V):
    """Connected components of the vertices that triangles use (label propagation with pointer jumping)."""
    t = np.asarray(tris, np.int64)
    u = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    w = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    lab = np.arange(V)
    while True:
        m = np.minimum(lab[u], lab[w])
        new = lab.copy()
        np.minimum.at(new, u, m)
        np.minimum.at(new, w, m)
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    return np.unique(lab[np.unique(u)]).size


def signed_volume(verts, tris):
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris, np.int64)
    return float(np.einsum('ij,ij->i', v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)


def sphere(n, c, r0):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing='ij'), -1)
    return (r0 - np.linalg.norm(g - np.asarray(c), axis=-1)).astype(np.float32)


def torus(n, c, R, r):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing='ij'), -1) - np.asarray(c)
    q = np.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2) - R
    return (r - np.sqrt(q ** 2 + g[..., 2] ** 2)).astype(np.float32)


def two_blobs(n):
    a = sphere(n, (n * 0.3 + 0.21, n * 0.5 + 0.13, n * 0.5 - 0.31), n * 0.18)
    b = sphere(n, (n * 0.7 - 0.17, n * 0.45 + 0.29, n * 0.55 + 0.07), n * 0.15)
    return np.maximum(a, b)


def white_noise(n, seed=0):
    v = np.random.default_rng(seed).standard_normal((n, n, n)).astype(np.float32)
    v[0], v[-1], v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1] = -1, -1, -1, -1, -1, -1   # border below the threshold 0
    return v


def check_sphere(verts, tris, c, r0):
    """Asserts of the analytic sphere checks; vertices in index coordinates."""
    V = len(verts)
    two, once, _ = edge_stats(tris, V)
    assert two and once, 'mesh not closed / not consistently oriented'
    assert euler(verts, tris) == 2
    assert components(tris, V) == 1
    vol = signed_volume(verts, tris)
    ref = 4.0 / 3.0 * np.pi * r0 ** 3
    assert vol > 0 and abs(vol - ref) < 0.01 * ref, (vol, ref)
    r = np.linalg.norm(np.asarray(verts, np.float64) - np.asarray(c), axis=1)
    assert np.abs(r - r0).max() < 0.05, np.abs(r - r0).max()


def read_ply(path):
    """Parser of the binary little-endian PLY export_ply writes -> (verts [V,3] float32, tris [T,3] int64)."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    head = data[:end].decode('ascii').split('\n')
    assert head[0] == 'ply' and head[1] == 'format binary_little_endian 1.0'
    V = int([h for h in head if h.startswith('element vertex')][0].split()[-1])
    T = int([h for h in head if h.startswith('element face')][0].split()[-1])
    assert 'property list uchar int vertex_indices' in head
    verts = np.frombuffer(data, '<f4', V * 3, end).reshape(V, 3)
    faces = np.frombuffer(data, [('n', 'u1'), ('i', '<i4', (3,))], T, end + 12 * V)
    assert np.all(faces['n'] == 3) and len(data) == end + 12 * V + 13 * T
    return verts.copy(), faces['i'].astype(np.int64)
