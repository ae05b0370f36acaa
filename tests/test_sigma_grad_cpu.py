"""The density-gradient feature without a GPU: the two C-ABI symbols and their ctypes signatures, the argument checks of
fastnerf_mlp_sigma_grad (made before anything touches a device), the PLY writer with and without normals, and the struct
sizes that the feature must leave alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fastnerf import _lib, mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_declared_exported_and_bound():
    src = open(os.path.join(ROOT, 'include', 'fastnerf.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    lib = _lib.lib()
    for name in ('fastnerf_mlp_sigma_grad_ws_floats', 'fastnerf_mlp_sigma_grad'):
        assert re.search(r'\b%s\s*\(' % name, src), name + ' is not declared in fastnerf.h'
        assert hasattr(lib, name), name + ' is not exported'
        assert name in _lib.SIGNATURES
    I, L, P = C.c_int, C.c_int64, C.c_void_p
    assert _lib.SIGNATURES['fastnerf_mlp_sigma_grad_ws_floats'] == (L, [I, L])
    # math_mode, kind, n, S, rays11, z, params, packed_fwd, packed_bwd, ws, sigma, grad, stream
    assert _lib.SIGNATURES['fastnerf_mlp_sigma_grad'] == (I, [I, I, L, I] + [P] * 9)


def test_workspace_is_about_20_kb_per_point():
    lib = _lib.lib()
    for mode in (0, 1, 2):
        a, b = lib.fastnerf_mlp_sigma_grad_ws_floats(mode, 65536), lib.fastnerf_mlp_sigma_grad_ws_floats(mode, 2 * 65536)
        per_point = (b - a) / 65536 * 4
        assert 19000 < per_point < 21500, (mode, per_point)     # saved activations + pre-activation gradients + 2 x [P,4]
        assert lib.fastnerf_mlp_sigma_grad_ws_floats(mode, 1) > 0
    assert lib.fastnerf_mlp_sigma_grad_ws_floats(3, 64) == -1
    assert lib.fastnerf_last_error()


# a fake non-NULL address for every buffer: a call that passed its checks would enqueue work on it, so these cases also show that
# the checks come first (no device is present when this file runs)
X = 0x1000


@pytest.mark.parametrize('what,args,needle', [
    ('kind 1', dict(kind=1), 'kind 0'),
    ('kind 2', dict(kind=2), 'kind 0'),
    ('math_mode 3', dict(math_mode=3), 'math_mode'),
    ('n = 0', dict(n=0), 'n>0'),
    ('S = 0', dict(S=0), 'S>=1'),
    ('null grad', dict(grad=None), 'null'),
    ('null ws', dict(ws=None), 'null'),
])
def test_bad_arguments_are_refused_before_the_device(what, args, needle):
    a = dict(math_mode=2, kind=0, n=4, S=3, rays11=X, z=X, params=X, packed_fwd=X, packed_bwd=X, ws=X, sigma=None, grad=X)
    a.update(args)
    lib = _lib.lib()
    rc = lib.fastnerf_mlp_sigma_grad(a['math_mode'], a['kind'], a['n'], a['S'], a['rays11'], a['z'], a['params'], a['packed_fwd'],
                                     a['packed_bwd'], a['ws'], a['sigma'], a['grad'], None)
    assert rc == -1, what
    msg = lib.fastnerf_last_error().decode()
    assert msg.startswith('fastnerf_mlp_sigma_grad') and needle in msg, (what, msg)


def todays_export_ply(path, vertices, triangles):
    """mesh.export_ply as it was before normals existed, kept here: without normals the bytes must not change."""
    v = np.ascontiguousarray(np.asarray(vertices), dtype='<f4').reshape(-1, 3)
    f = np.asarray(triangles).reshape(-1, 3)
    faces = np.empty(f.shape[0], dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    faces['n'] = 3
    faces['i'] = f
    head = ('ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n'
            'element face %d\nproperty list uchar int vertex_indices\nend_header\n' % (v.shape[0], f.shape[0]))
    with open(path, 'wb') as fh:
        fh.write(head.encode('ascii'))
        fh.write(v.tobytes())
        fh.write(faces.tobytes())


def some_mesh(V=7, T=5):
    rng = np.random.default_rng(11)
    v = rng.standard_normal((V, 3)).astype(np.float32)
    n = rng.standard_normal((V, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[2] = 0
    t = rng.integers(0, V, (T, 3)).astype(np.int64)
    return v, t, n


def read_ply_with_normals(path):
    """(header lines, vertex block [V, floats per vertex], faces [T,3])"""
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    lines = raw[:end].decode('ascii').split('\n')[:-1]
    V = int([l for l in lines if l.startswith('element vertex')][0].split()[-1])
    T = int([l for l in lines if l.startswith('element face')][0].split()[-1])
    props = [l.split()[-1] for l in lines[lines.index('element vertex %d' % V) + 1: lines.index('element face %d' % T)]]
    stride = 4 * len(props)
    vb = np.frombuffer(raw, '<f4', V * len(props), end).reshape(V, len(props))
    fb = np.frombuffer(raw, np.dtype([('n', 'u1'), ('i', '<i4', (3,))]), T, end + V * stride)
    assert end + V * stride + T * 13 == len(raw)
    assert (fb['n'] == 3).all()
    return lines, props, vb, fb['i']


def test_export_ply_with_normals(tmp_path):
    v, t, n = some_mesh()
    path = str(tmp_path / 'n.ply')
    mesh.export_ply(path, v, t, normals=n)
    lines, props, vb, faces = read_ply_with_normals(path)
    assert lines == ['ply', 'format binary_little_endian 1.0', 'element vertex 7', 'property float x', 'property float y',
                     'property float z', 'property float nx', 'property float ny', 'property float nz', 'element face 5',
                     'property list uchar int vertex_indices', 'end_header']
    assert props == ['x', 'y', 'z', 'nx', 'ny', 'nz'] and vb.strides[0] == 24
    assert np.array_equal(vb[:, :3], v) and np.array_equal(vb[:, 3:], n) and np.array_equal(faces, t)
    with pytest.raises(ValueError):
        mesh.export_ply(path, v, t, normals=n[:-1])


def test_export_ply_without_normals_writes_todays_bytes(tmp_path):
    v, t, _ = some_mesh()
    a, b, c = str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply'), str(tmp_path / 'c.ply')
    todays_export_ply(a, v, t)
    mesh.export_ply(b, v, t)
    mesh.export_ply(c, v, t, normals=None)
    want = open(a, 'rb').read()
    assert open(b, 'rb').read() == want and open(c, 'rb').read() == want
    todays_export_ply(a, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    mesh.export_ply(b, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    assert open(b, 'rb').read() == open(a, 'rb').read()


def test_struct_sizes_are_what_they_were():
    """The feature adds entry points of its own: fn_step_args (512 bytes) and fn_occ_grid (pointer + 6 floats + 4 int32) keep the
    sizes that tests/test_occupancy_cascade_cpu.py pins."""
    assert _lib.lib().fastnerf_step_args_size() == C.sizeof(_lib.StepArgs) == 512
    assert C.sizeof(_lib.OccGrid) == 48
