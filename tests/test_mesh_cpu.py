"""The marching-cubes oracle (tests/mc_numpy.py) and, through it, the library's table (fastnerf_mc_tables, a host call) on
analytic fields, without a GPU: closed and consistently oriented meshes, Euler characteristic, components, volume and
vertex radius; and the PLY writer against a numpy parser."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M   # noqa: E402


@pytest.fixture(scope='module')
def tri_table():
    return M.tables()[0]


def test_table_shape_and_edge_masks(tri_table):
    tri, edge = M.tables()
    assert tri.shape == (256, 16) and edge.shape == (256,)
    assert edge[0] == 0 and edge[255] == 0 and edge[1] == 0x109
    for c in range(256):
        row = tri[c]
        n = int((row >= 0).sum())
        assert n % 3 == 0 and n <= 15 and np.all(row[n:] == -1)
        used = set(int(e) for e in row[:n])
        assert used == {e for e in range(12) if (int(edge[c]) >> e) & 1}, c   # exactly the crossing edges


@pytest.mark.parametrize('n,c,r0', [(64, (31.3, 32.7, 30.6), 20.5), (128, (63.4, 64.1, 62.7), 45.3)])
def test_sphere(tri_table, n, c, r0):
    verts, tris = M.marching_cubes(M.sphere(n, c, r0), 0.0, tri_table)
    M.check_sphere(verts, tris, c, r0)


def test_torus_has_euler_characteristic_zero(tri_table):
    verts, tris = M.marching_cubes(M.torus(64, (31.6, 32.2, 31.9), 18.3, 7.1), 0.0, tri_table)
    two, once, _ = M.edge_stats(tris, len(verts))
    assert two and once
    assert M.euler(verts, tris) == 0 and M.components(tris, len(verts)) == 1


def test_two_blobs(tri_table):
    verts, tris = M.marching_cubes(M.two_blobs(64), 0.0, tri_table)
    two, once, _ = M.edge_stats(tris, len(verts))
    assert two and once
    assert M.components(tris, len(verts)) == 2 and M.euler(verts, tris) == 4
    assert M.signed_volume(verts, tris) > 0


@pytest.mark.parametrize('seed', range(4))
def test_white_noise_is_closed_and_oriented(tri_table, seed):
    """Every ambiguous face configuration occurs here; the table's face rule (ambiguous faces separate the inside corners)
    keeps the mesh closed."""
    verts, tris = M.marching_cubes(M.white_noise(24, seed), 0.0, tri_table)
    assert len(tris) > 1000
    two, once, _ = M.edge_stats(tris, len(verts))
    assert two and once


def test_vertex_order_and_positions(tri_table):
    """The contract's vertex order (lower endpoint, then axis) and position rule on a hand-checked 2 x 2 x 2 volume."""
    vol = np.zeros((2, 2, 2), np.float32)
    vol[0, 0, 0] = 1.0
    vol[1, 0, 0], vol[0, 1, 0], vol[0, 0, 1] = -1.0, -3.0, -0.25
    verts, tris = M.marching_cubes(vol, 0.0, tri_table)
    np.testing.assert_array_equal(verts, np.array([[0.5, 0, 0], [0, 0.25, 0], [0, 0, 0.8]], np.float32))
    assert tris.tolist() == [[0, 1, 2]]   # normal (+,+,+): from the inside corner outwards


def test_ply_round_trip(tmp_path):
    from fastnerf import mesh
    rng = np.random.default_rng(0)
    verts = rng.standard_normal((57, 3)).astype(np.float32)
    tris = rng.integers(0, 57, (101, 3))
    path = str(tmp_path / 'm.ply')
    mesh.export_ply(path, verts, tris)
    v2, t2 = M.read_ply(path)
    np.testing.assert_array_equal(v2, verts)
    np.testing.assert_array_equal(t2, tris)
    mesh.export_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    v3, t3 = M.read_ply(path)
    assert v3.shape == (0, 3) and t3.shape == (0, 3)


def test_marching_cubes_refuses_cpu_tensors():
    import torch
    from fastnerf import mesh
    with pytest.raises(RuntimeError):
        mesh.marching_cubes(torch.zeros(4, 4, 4), 0.0)
