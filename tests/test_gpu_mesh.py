"""Mesh extraction on the GPU (csrc/mesh.hip, fastnerf.mesh, tools/extract_mesh.py): marching cubes against the numpy
restatement of its contract (tests/mc_numpy.py) at the scan's block and level boundaries and at 257^3, empty / full
volumes, determinism, the analytic mesh checks on the kernel's output, both routes of the density query against the
reference's loop, and the command-line tool on a freshly saved checkpoint."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_numpy as M   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return fastnerf


@pytest.fixture(scope='module')
def tri_table():
    return M.tables()[0]


def gpu_mc(fn, vol, thr):
    v, t = fn.mesh.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol)).cuda(), thr)
    return v.cpu().numpy(), t.cpu().numpy()


def smooth_field(shape, seed):
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing='ij')
    f = sum(np.sin(g[a] * rng.uniform(0.2, 0.9) + rng.uniform(0, 6)) for a in range(3) for _ in range(2))
    return f.astype(np.float32)


# points per shape: 8; odd; 255 / 256 / 258 (one scan group of blocks minus / at / past MC_BLOCK points); 65535 / 65536 / 65538
# (256 blocks of 256 points: the second scan level starts); 274625 (two scan levels below the totals)
SHAPES = [(2, 2, 2), (17, 33, 9), (3, 5, 17), (4, 8, 8), (2, 3, 43), (15, 17, 257), (16, 64, 64), (2, 3, 10923), (65, 65, 65)]


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('kind', ['random', 'smooth'])
def test_gpu_equals_oracle(fn, tri_table, shape, kind):
    seed = 2 * SHAPES.index(shape) + (kind == 'smooth')
    vol = np.random.default_rng(seed).standard_normal(shape).astype(np.float32) if kind == 'random' else smooth_field(shape, seed)
    thr = 0.1
    v_ref, t_ref = M.marching_cubes(vol, thr, tri_table)
    v, t = gpu_mc(fn, vol, thr)
    assert t.shape == t_ref.shape and np.array_equal(t, t_ref)
    assert v.shape == v_ref.shape and np.abs(v - v_ref).max(initial=0) <= 1e-6
    assert np.array_equal(v, v_ref), 'bit-identical expected (-ffp-contract=off, correctly rounded division)'
    if kind == 'random':
        assert len(t) > 0


def test_gpu_equals_oracle_257(fn, tri_table):
    """257^3 points = 16.97 M: 66 307 blocks, three scan levels below the totals."""
    c, r0 = (128.3, 127.6, 128.9), 100.2
    vol = M.sphere(257, c, r0)
    vol += np.random.default_rng(7).standard_normal(vol.shape).astype(np.float32) * 0.3
    v_ref, t_ref = M.marching_cubes(vol, 0.0, tri_table)
    v, t = gpu_mc(fn, vol, 0.0)
    assert np.array_equal(t, t_ref) and np.array_equal(v, v_ref)
    two, once, _ = M.edge_stats(t, len(v))
    assert two and once


def test_empty_and_full_volumes(fn):
    for vol, thr in ((np.zeros((9, 7, 5), np.float32), 1.0), (np.ones((9, 7, 5), np.float32), 0.0),
                     (np.zeros((2, 2, 2), np.float32), 0.0)):     # value == threshold is outside: empty too
        v, t = gpu_mc(fn, vol, thr)
        assert v.shape == (0, 3) and t.shape == (0, 3)


def test_two_runs_are_bit_identical(fn):
    vol = torch.randn(70, 61, 83, device='cuda')
    v1, t1 = fn.mesh.marching_cubes(vol, 0.2)
    v2, t2 = fn.mesh.marching_cubes(vol, 0.2)
    assert torch.equal(t1, t2) and torch.equal(v1.view(torch.int32), v2.view(torch.int32))
    assert t1.dtype == torch.int64 and v1.dtype == torch.float32 and t1.is_cuda and v1.is_cuda


def test_bad_input(fn):
    with pytest.raises(ValueError):
        fn.mesh.marching_cubes(torch.zeros(1, 4, 4, device='cuda'), 0.0)
    with pytest.raises(ValueError):
        fn.mesh.marching_cubes(torch.zeros(4, 4, device='cuda'), 0.0)
    bad = torch.zeros(4, 4, 4, device='cuda')
    bad[1, 2, 3] = float('nan')
    with pytest.raises(ValueError):
        fn.mesh.marching_cubes(bad, 0.0)
    v, t = fn.mesh.marching_cubes(torch.zeros(5, 5, 5, dtype=torch.float64, device='cuda')[::1, :, 1:], -1.0)   # cast + copy
    assert len(v) == 0


def test_analytic_meshes_on_gpu(fn):
    for n, c, r0 in ((64, (31.3, 32.7, 30.6), 20.5), (128, (63.4, 64.1, 62.7), 45.3)):
        v, t = gpu_mc(fn, M.sphere(n, c, r0), 0.0)
        M.check_sphere(v, t, c, r0)
    v, t = gpu_mc(fn, M.torus(64, (31.6, 32.2, 31.9), 18.3, 7.1), 0.0)
    assert M.edge_stats(t, len(v))[:2] == (True, True) and M.euler(v, t) == 0 and M.components(t, len(v)) == 1
    v, t = gpu_mc(fn, M.two_blobs(64), 0.0)
    assert M.edge_stats(t, len(v))[:2] == (True, True) and M.euler(v, t) == 4 and M.components(t, len(v)) == 2
    for seed in range(3):
        v, t = gpu_mc(fn, M.white_noise(32, seed), 0.0)
        assert M.edge_stats(t, len(v))[:2] == (True, True)


@pytest.mark.parametrize('viewdirs', [True, False])
def test_density_grid_fused_equals_reference_loop(fn, viewdirs):
    """extract_mesh.py:40-61 verbatim (network_query_fn on flat[i:i+chunk, None, :]) against density_grid: same forward, same
    point values, same 65 536-point tiles -> bit-identical."""
    torch.manual_seed(3)
    args = fn.run_nerf.make_args(N_importance=16, use_viewdirs=viewdirs, no_reload=True)
    _, kw, _, _, _, _ = fn.run_nerf.create_nerf(args)
    net, nqf = kw['network_fine'], kw['network_query_fn']
    N, chunk = 48, 1024 * 64
    t = torch.linspace(-1.2, 1.2, N + 1)
    flat = torch.stack(torch.meshgrid(t, t, t, indexing='ij'), -1).reshape(-1, 3).cuda()
    out = []
    with torch.no_grad():
        for i in range(0, flat.shape[0], chunk):
            vd = torch.zeros_like(flat[i:i + chunk]) if viewdirs else None
            out.append(nqf(flat[i:i + chunk, None, :], vd, net))
    ref = torch.relu(torch.cat(out, 0)[..., -1]).reshape(N + 1, N + 1, N + 1)
    vol = fn.mesh.density_grid(net, t, t, t)
    assert vol.shape == ref.shape and vol.is_cuda
    assert torch.equal(vol, ref)
    assert fn.mesh.density_grid(net, t[:0], t, t).shape == (0, N + 1, N + 1)


class RadialSigma(nn.Module):
    """sigma = k (r0 - |x|) from the first three embedding channels (the raw point: include_input); rgb 0."""

    def __init__(self, k, r0):
        super().__init__()
        self.k, self.r0 = k, r0
        self.dummy = nn.Parameter(torch.zeros(1))

    def forward(self, x):
        sig = self.k * (self.r0 - x[..., :3].norm(dim=-1, keepdim=True))
        return torch.cat([torch.zeros_like(x[..., :3]), sig], -1)


def test_extract_mesh_closure_route(fn):
    # the level set sigma = 50 sits at r0 - 0.5 = 0.5; sigma stays linear (above the relu) a cell beyond it on either side
    k, r0, thr, N, bound = 100.0, 1.0, 50.0, 96, 1.2
    embed, _ = fn.run_nerf_helpers.get_embedder(10)
    nqf = lambda pts, vd, net: fn.run_nerf.run_network(pts, vd, net, embed_fn=embed)
    kw = {'network_fn': RadialSigma(k, r0).cuda(), 'network_fine': None, 'network_query_fn': nqf, 'use_viewdirs': False}
    v, t = fn.mesh.extract_mesh(kw, N=N, bound=bound, threshold=thr)
    v, t = v.cpu().numpy(), t.cpu().numpy()
    rs = r0 - thr / k                       # the level set sigma = threshold
    cell = 2 * bound / N
    two, once, _ = M.edge_stats(t, len(v))
    assert two and once and M.euler(v, t) == 2 and M.components(t, len(v)) == 1
    vol = M.signed_volume(v, t)
    assert vol > 0 and abs(vol - 4 / 3 * np.pi * rs ** 3) < 0.01 * 4 / 3 * np.pi * rs ** 3
    assert np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - rs).max() < 0.05 * cell


def test_tool_writes_the_mesh(fn, tmp_path):
    torch.manual_seed(5)
    args = fn.run_nerf.make_args(N_importance=16, use_viewdirs=True, no_reload=True, basedir=str(tmp_path), expname='exp')
    kw_train, kw_test, _, _, _, optimizer = fn.run_nerf.create_nerf(args)
    os.makedirs(tmp_path / 'exp')
    torch.save({'global_epoch': 0, 'global_iter': 0,
                'network_fn_state_dict': fn.run_nerf.reference_state_dict(kw_train['network_fn']),
                'network_fine_state_dict': fn.run_nerf.reference_state_dict(kw_train['network_fine']),
                'optimizer_state_dict': optimizer.state_dict()}, str(tmp_path / 'exp' / '000.tar'))
    N = 32
    t = torch.linspace(-1.2, 1.2, N + 1, device='cuda')
    thr = float(fn.mesh.density_grid(kw_test['network_fine'], t, t, t).median())   # a level set the random net has
    v_ref, t_ref = fn.mesh.extract_mesh(kw_test, N=N, threshold=thr)
    assert len(t_ref) > 0
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'extract_mesh.py'), '--basedir', str(tmp_path), '--expname', 'exp',
                        '--N_importance', '16', '--use_viewdirs', '--N', str(N), '--threshold', repr(thr)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert '"V": %d' % len(v_ref) in r.stdout and 'marching_cubes_ms' in r.stdout
    v, tr = M.read_ply(str(tmp_path / 'exp' / 'lego_mesh.ply'))
    assert np.array_equal(tr, t_ref.cpu().numpy())
    assert np.array_equal(v, v_ref.cpu().numpy())
