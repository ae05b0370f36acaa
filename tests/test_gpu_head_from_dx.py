"""The rgb-head and alpha-bias gradients formed in the dX kernel's phase A (csrc/mlp_bwd_dx.hip), fp32 and bf16x6.

dWr[c][k] = sum_p draw[p][c] hv[p][k], dbr[c] = sum_p draw[p][c], dba = sum_p draw[p][3] are summed per 64-point tile by the dX
kernel, per group of tiles by head_group_kernel and per row by reduce_all (csrc/mlp_bwd_dw.hip).  FASTNERF_HEAD_FROM_DX=0 in the
environment, read at every call, sends a backward down the former route (head_grads_kernel's own pass over hv and draw);
FASTNERF_HEAD_FROM_DX=nan fills the library's per-tile workspace with NaNs ahead of the dX launch.

  * the three gradients against a float64 sum over the saved hv and the cotangent, per element within
    (64 + ntiles) 2^-24 sum_p |draw hv| -- the a-priori bound of any grouping of that many fp32 additions -- plus one ulp of the
    result for the final store;
  * every other gradient of the call bit-equal to the former route's;
  * a live list that keeps about half of the points: bit-equal to the plain backward of the gathered points;
  * two calls bit-equal; NaN-filled workspace and partial buffer: every gradient finite.

Shapes: P = 1, 63, 64 (one tile: one row, a ragged row, a full tile), 3 x 70 = 210 (a ragged fourth tile), 37 x 960 = 35 520
(555 tiles: more tiles than dX workgroups on a 256-CU part, 3 tiles per group and 185 rows, neither a multiple of 16).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = {'P=1': (1, 1), 'P=63': (63, 1), 'P=64': (64, 1), 'P=210': (3, 70), 'P=35520': (37, 960)}
MODES = ('bf16x6', 'fp32')
HEAD = 388        # the last 388 floats of a kind-0 gradient: A.b (1), R.W (3 x 128), R.b (3)
ENV = 'FASTNERF_HEAD_FROM_DX'


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


@pytest.fixture(scope='module')
def flat(golden_dir):
    from oracle import nerf_oracle as O
    g7 = np.load(os.path.join(golden_dir, 'g7_weights.npz'))
    sd = {k[2:]: torch.from_numpy(g7[k]) for k in g7.files if k.startswith('c.')}
    return torch.cat([sd[n].reshape(-1) for n, _ in O.nerf_param_shapes()]).cuda()


class env:
    """The switch for the length of one call (the library reads it at every call)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get(ENV)
        if self.value is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = self.old


def batch(fn, n, S, seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    ro = (torch.rand(n, 3, generator=gen, device='cuda') - 0.5) * 0.5 + torch.tensor([0.0, 0.0, 4.0], device='cuda')
    rd = torch.randn(n, 3, generator=gen, device='cuda') * 0.2 - torch.tensor([0.0, 0.0, 1.0], device='cuda')
    rays = fn.ops.pack_rays(ro, rd, 2.0, 6.0)
    z = torch.sort(torch.rand(n, S, generator=gen, device='cuda') * 4 + 2, -1).values
    cot = torch.randn(n, S, 4, generator=gen, device='cuda')
    cot[torch.rand(n, S, generator=gen, device='cuda') < 0.45] = 0.0
    return rays, z, cot


def backward(fn, mode, rays, z, cot, flat, switch=None, nan_partial=False):
    """-> (gradient, hv [P, 128]) of the saving forward + backward under `mode` with the switch set to `switch`."""
    n, S = z.shape
    P = n * S
    old = fn.ops.get_math()
    fn.ops.set_math(mode)
    try:
        pf, pb = fn.ops.mlp_pack(flat)
        act = torch.empty(fn.ops.act_floats(P), device='cuda')
        fn.ops.mlp_fwd(rays, z, flat, pf, act=act)
        dact = torch.empty(fn.ops.dact_floats(P), device='cuda')
        partial = torch.full((fn.ops.mlp_bwd_partial_floats(),), float('nan') if nan_partial else 0.0, device='cuda')
        g = torch.full((fn.ops.NET_PARAMS,), float('nan'), device='cuda')
        with env(switch):
            fn.ops.mlp_bwd(cot, act, flat, pb, dact, partial, g)
        torch.cuda.synchronize()
        o = P * (64 + 2048 + 256 + 32)   # act_hv (csrc/mlp_layout.h), 64-channel encoding
        return g, act[o:o + P * 128].view(P, 128).clone()
    finally:
        fn.ops.set_math(old)


def head_of(g):
    """(dWr [3, 128], dbr [3], dba [1]) of a kind-0 gradient"""
    N = g.numel()
    return g[N - 387:N - 3].view(3, 128), g[N - 3:], g[N - HEAD:N - 387]


RUNS = {}


def runs(fn, flat, case, mode):
    """The calls of one (case, mode), made once: the new route twice, the former route, the new route over NaN-filled buffers."""
    key = (case, mode)
    if key not in RUNS:
        n, S = CASES[case]
        rays, z, cot = batch(fn, n, S, seed=n * S)
        g, hv = backward(fn, mode, rays, z, cot, flat)
        g2, _ = backward(fn, mode, rays, z, cot, flat)
        g_old, _ = backward(fn, mode, rays, z, cot, flat, switch='0')
        g_nan, _ = backward(fn, mode, rays, z, cot, flat, switch='nan', nan_partial=True)
        RUNS[key] = dict(cot=cot, hv=hv, g=g, g2=g2, g_old=g_old, g_nan=g_nan)
    return RUNS[key]


def ulp32(x64):
    return torch.from_numpy(np.spacing(x64.abs().cpu().numpy().astype(np.float32)).astype(np.float64)).to(x64.device)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', list(CASES))
def test_head_gradients_vs_fp64(fn, flat, case, mode):
    r = runs(fn, flat, case, mode)
    P = r['hv'].shape[0]
    ntiles = (P + 63) // 64
    d = r['cot'].reshape(P, 4).double()
    hv = r['hv'].double()
    ref = (d[:, :3].t() @ hv, d[:, :3].sum(0), d[:, 3:].sum(0))
    A = (d[:, :3].abs().t() @ hv.abs(), d[:, :3].abs().sum(0), d[:, 3:].abs().sum(0))
    for name, got, want, a in zip(('dWr', 'dbr', 'dba'), head_of(r['g']), ref, A):
        bound = (64 + ntiles) * 2.0 ** -24 * a + ulp32(want)
        err = (got.double() - want).abs()
        print('%s %s %s: max |g - g64| = %.3e, max of err / bound = %.3f' % (case, mode, name, float(err.max()), float((err / bound).max())))
        assert torch.isfinite(got).all(), (case, mode, name)
        assert (err <= bound).all(), (case, mode, name, float((err / bound).max()))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', list(CASES))
def test_other_gradients_equal_the_former_route(fn, flat, case, mode):
    r = runs(fn, flat, case, mode)
    N = r['g'].numel()
    assert torch.isfinite(r['g_old']).all(), (case, mode)
    assert torch.equal(r['g'][:N - HEAD], r['g_old'][:N - HEAD]), (case, mode)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', list(CASES))
def test_two_calls_are_bit_equal(fn, flat, case, mode):
    r = runs(fn, flat, case, mode)
    assert torch.equal(r['g'], r['g2']), (case, mode)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', list(CASES))
def test_nan_filled_buffers_leave_no_trace(fn, flat, case, mode):
    r = runs(fn, flat, case, mode)
    assert torch.isfinite(r['g_nan']).all(), (case, mode)
    assert torch.equal(r['g_nan'], r['g']), (case, mode)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', ['P=210', 'P=35520'])
def test_live_list_equals_plain_backward_of_the_live_points(fn, flat, case, mode):
    n, S = CASES[case]
    P = n * S
    rays, z, _ = batch(fn, n, S, seed=P + 1)
    gen = torch.Generator(device='cuda').manual_seed(P)
    alive = torch.rand(P, generator=gen, device='cuda') < 0.5
    cot = (torch.randn(n, S, 4, generator=gen, device='cuda') * alive.view(n, S, 1)).contiguous()
    live = int(alive.sum())
    old = fn.ops.get_math()
    fn.ops.set_math(mode)
    try:
        pf, pb = fn.ops.mlp_pack(flat)
        idx, cnt = fn.ops.compact_live(cot)
        assert cnt.tolist() == [live, P]
        act = torch.empty(fn.ops.act_floats(P), device='cuda')
        dact = torch.empty(fn.ops.dact_floats(P), device='cuda')
        partial = torch.full((fn.ops.mlp_bwd_partial_floats(),), float('nan'), device='cuda')
        fn.ops.mlp_fwd_live(rays, z, flat, pf, act, idx, cnt)
        g_live = torch.full((fn.ops.NET_PARAMS,), float('nan'), device='cuda')
        with env('nan'):
            fn.ops.mlp_bwd_live(cot, act, flat, pb, dact, partial, g_live, idx, cnt)
        torch.cuda.synchronize()
    finally:
        fn.ops.set_math(old)
    sel = idx[:live].long()
    g, _ = backward(fn, mode, rays[sel // S].contiguous(), z.reshape(-1)[sel].reshape(-1, 1).contiguous(),
                    cot.reshape(P, 4)[sel].reshape(-1, 1, 4).contiguous(), flat)
    assert torch.isfinite(g_live).all(), (case, mode)
    assert torch.equal(g_live, g), (case, mode, 'the live-list backward differs from the plain backward of the live points')
