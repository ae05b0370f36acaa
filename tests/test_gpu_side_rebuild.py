"""The view-layer dW job of the bf16x6 backward that rebuilds dYv on chip (csrc/mlp_bwd_dw.hip dw6_body RBV, csrc/dw_pair.h SideRb).

In the backward passes of a fused step (bf16x6, plain backward) the view job forms dYv = (drgb . Wr) [hv > 0] from hv, d(loss)/d(raw) and
the rgb weights in the lane that splits it, and dX does not store dYv.  The expression is dX's own (csrc/mlp_common.h dyv_value), so every
rebuilt value equals the stored one bit for bit, and so does every gradient: all comparisons here are torch.equal, on the whole flat
gradient of both nets after each step and on the parameters after two steps, between the default route and FASTNERF_SIDE_REBUILD=0
(the reading route with the store on; the variable is read at every call).

Shapes (rays x (N_samples + N_importance)):
    3 x (64 + 128)     P = 192 and 576: a handful of k-steps of 16 points, most workgroups without a point
    37 x (20 + 12)     P = 740 and 1184: 740 is no multiple of 16 or 64 (a ragged last k-step, rows clamped and zeroed); S = 20 is no multiple
                       of 8, ray boundaries fall inside a lane's 8-point group
    130 x (64 + 128)   P = 8320 and 24 960: 520 and 1560 k-steps, more than one per workgroup, split unevenly over the workgroups
FASTNERF_SIDE_REBUILD=nan fills dact_yv with NaNs ahead of the backward's first kernel: a reader would carry them into the gradient.
Ray gradients (render_rays with rays that require a gradient; fastnerf_ray_grad reads dact_yv) and the compacted step never take the
rebuilding route: the store stays on and their results do not depend on the variable.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENV = 'FASTNERF_SIDE_REBUILD'
CASES = {'3x(64+128)': (3, 64, 128), '37x(20+12)': (37, 20, 12), '130x(64+128)': (130, 64, 128)}


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


@pytest.fixture(autouse=True)
def bf16x6(fn):
    old_math, old_compact = fn.ops.get_math(), fn.render.get_compact()
    fn.ops.set_math('bf16x6')
    fn.render.set_compact('0')
    yield
    fn.ops.set_math(old_math)
    fn.render.set_compact(old_compact)


class env:
    """The switch for the length of a block (the library reads it at every call)."""

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


def rebuild_passes(fn):
    return int(fn._lib.lib().fastnerf_side_rebuild_passes())


def _trainer(fn, golden_dir, Ns, Ni):
    torch.manual_seed(3)
    args = fn.run_nerf.make_args(N_importance=Ni, N_samples=Ns, perturb=1.0, white_bkgd=True, no_reload=True, lrate=5e-4, lrate_decay=500)
    ktr = fn.run_nerf.create_nerf(args)[0]
    wts = np.load(os.path.join(golden_dir, 'g7_weights.npz'))
    for net, pre in ((ktr['network_fn'], 'c.'), (ktr['network_fine'], 'f.')):
        net.load_state_dict({k[2:]: torch.from_numpy(np.ascontiguousarray(wts[k])) for k in wts.files if k.startswith(pre)})
    K = np.array([[1111.1, 0, 400.0], [0, 1111.1, 400.0], [0, 0, 1]])
    tr = fn.run_nerf.Trainer(ktr, 800, 800, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500)
    assert tr.fused and tr.world == 1
    return tr


def _batches(fn, n, steps=2):
    gen = torch.Generator().manual_seed(1000 + n)
    K = np.array([[1111.1, 0, 400.0], [0, 1111.1, 400.0], [0, 0, 1]])
    poses = torch.stack([fn.synthetic.pose_spherical(-180.0 + 45.0 * k, -30.0, 4.0)[:3, :4] for k in range(8)], 0).cuda()
    out = []
    for _ in range(steps):
        pix = torch.stack([torch.randint(0, 8, (n,), generator=gen), torch.randint(0, 800, (n,), generator=gen),
                           torch.randint(0, 800, (n,), generator=gen)], 1).int().cuda()
        ro, rd = fn.ops.gen_rays_pixels(pix, poses, K)
        out.append((ro.contiguous(), rd.contiguous(), torch.rand(n, 3, generator=gen).cuda()))
    return out


def two_steps(fn, golden_dir, case, switch, compact='0'):
    """-> (gradient after step 1, gradient after step 2, parameters after step 2, losses, rebuilding passes counted) of two fused steps."""
    n, Ns, Ni = CASES[case]
    fn.render.set_compact(compact)
    tr = _trainer(fn, golden_dir, Ns, Ni)
    torch.manual_seed(5)            # the device-side Philox streams are keyed from torch's CPU generator
    grads, losses = [], []
    before = rebuild_passes(fn)
    with env(switch):
        for b in _batches(fn, n):
            loss2, _ = tr.step(*b, decay=False)
            torch.cuda.synchronize()
            grads.append(tr.grad.clone())
            losses.append(loss2.clone())
    assert tr.adam_t == 2 and tr.last_step_live == (compact == '1')
    return grads[0], grads[1], tr.flat.clone(), torch.stack(losses), rebuild_passes(fn) - before


RUNS = {}


def runs(fn, golden_dir, case):
    """The reference (reading route) and the default route of a case, made once and left unchanged."""
    if case not in RUNS:
        RUNS[case] = (two_steps(fn, golden_dir, case, '0'), two_steps(fn, golden_dir, case, None))
    return RUNS[case]


def assert_same(got, ref, what):
    for name, x, y in zip(('gradient, step 1', 'gradient, step 2', 'parameters after two steps', 'losses'), got, ref):
        assert torch.isfinite(x).all(), (what, name)
        assert torch.equal(x, y), (what, name, int((x != y).sum()), float((x - y).abs().max()))


@pytest.mark.parametrize('case', list(CASES))
def test_rebuilding_route_equals_reading_route(fn, golden_dir, case):
    ref, got = runs(fn, golden_dir, case)
    assert ref[4] == 0, 'FASTNERF_SIDE_REBUILD=0 must select the reading route'
    assert got[4] == 4, ('two steps of two passes each rebuild', got[4])
    assert float(ref[0].abs().max()) > 0 and float(ref[1].abs().max()) > 0
    N = ref[0].numel() // 2
    assert float(ref[0][:N].abs().max()) > 0 and float(ref[0][N:].abs().max()) > 0      # both nets
    assert_same(got, ref, case)


def test_nan_filled_regions_leave_no_trace(fn, golden_dir):
    case = '37x(20+12)'
    ref, _ = runs(fn, golden_dir, case)
    got = two_steps(fn, golden_dir, case, 'nan')
    assert got[4] == 4
    assert_same(got, ref, case + ' nan')


def test_live_list_step_keeps_the_reading_route(fn, golden_dir):
    case = '37x(20+12)'
    a = two_steps(fn, golden_dir, case, None, compact='1')
    b = two_steps(fn, golden_dir, case, '0', compact='1')
    assert a[4] == 0 and b[4] == 0
    assert_same(a, b, case + ' live list')


def test_ray_gradients_keep_the_stores(fn, golden_dir):
    """render_rays with rays that require a gradient: forward, backward and fastnerf_ray_grad in one autograd call.  ray_grad reads dact_yv,
    so this route must store it whatever the variable says: same ray and network gradients with and without it, no rebuilding pass."""
    n, Ns, Ni = CASES['37x(20+12)']
    res = []
    before = rebuild_passes(fn)
    for switch in (None, '0'):
        tr = _trainer(fn, golden_dir, Ns, Ni)
        ro, rd, tgt = _batches(fn, n, steps=1)[0]
        rb = fn.ops.pack_rays(ro, rd, 2.0, 6.0).clone().requires_grad_(True)
        nets = (tr.net_c, tr.net_f)
        for net in nets:
            for p in net.parameters():
                p.grad = None
        with env(switch):
            out = fn.render.render_rays(rb, tr.net_c, None, Ns, N_importance=Ni, network_fine=tr.net_f, perturb=0., white_bkgd=True)
            (((out['rgb_map'] - tgt) ** 2).mean() + ((out['rgb0'] - tgt) ** 2).mean()).backward()
            torch.cuda.synchronize()
        res.append((rb.grad.clone(), torch.cat([p.grad.reshape(-1) for net in nets for p in net.parameters()])))
    assert rebuild_passes(fn) == before
    for x, y in zip(*res):
        assert torch.isfinite(x).all() and float(x.abs().max()) > 0
        assert torch.equal(x, y)
