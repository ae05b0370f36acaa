"""The paired dW trunk launch of the bf16x6 backward (csrc/mlp_bwd_dw.hip mlp_bwd_dw6_trunk_pair_kernel, csrc/render.cpp rr_bwd): one call
that runs both passes of a two-net step on the saving route multiplies the seven 256 x 256 dW jobs of BOTH passes in one launch.  Nothing
inside a job changes -- chunk counts, k-step ranges, partial regions, the order of the reduction -- so every gradient must equal, bit for
bit, what the unpaired route of the same build gives: the backward pass by pass (raw2outputs_bwd + mlp_bwd per pass), or the fused step
issued phase by phase.

Shapes (unit = ncu / 8 chunks per B = 16 * 256 * unit points, dw_trunk_chunks):
    3 rays x (5 + 7)         P = 15 and 36: ragged k-step tails, almost every chunk empty
    64 rays x (16 + 32)      one eighth of the chip for each pass, equal chunk counts
    1024 rays x (B/1024 + 1) P = B -> one eighth, P = B + 1024 -> two eighths (128 + 1 samples, P = 131 072 and 132 096, on a 256-CU part):
                             unequal chunk counts, where a wrong (pass, job, chunk) decode of the flat grid shows
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

QMAX = 256               # DW_QMAX, csrc/mlp_bwd_dw.hip


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


@pytest.fixture(scope='module')
def ncu(fn):
    n = int(fn._lib.lib().fastnerf_device_cus())
    assert n > 0
    return n


@pytest.fixture(autouse=True)
def plain_backward(fn):
    """The saving route: no point compaction."""
    old = fn.render.get_compact()
    fn.render.set_compact('0')
    yield
    fn.render.set_compact(old)


def trunk_chunks(P, ncu):
    """dw_trunk_chunks (csrc/mlp_bwd_dw.hip), restated."""
    unit = max(1, ncu // 8)
    nq = (P + 15) // 16
    k = (nq + unit * QMAX - 1) // (unit * QMAX)
    return unit * min(8, max(1, k))


def shapes(ncu):
    B = 16 * QMAX * max(1, ncu // 8)
    assert B % 1024 == 0
    return {'ragged': (3, 5, 7), 'equal': (64, 16, 32), 'unequal': (1024, B // 1024, 1)}


def _nets(fn, golden_dir, Ns, Ni):
    args = fn.run_nerf.make_args(N_importance=Ni, N_samples=Ns, perturb=0.0, white_bkgd=True, no_reload=True)
    ktr = fn.run_nerf.create_nerf(args)[0]
    wts = np.load(os.path.join(golden_dir, 'g7_weights.npz'))
    for net, pre in ((ktr['network_fn'], 'c.'), (ktr['network_fine'], 'f.')):
        net.load_state_dict({k[2:]: torch.from_numpy(np.ascontiguousarray(wts[k])) for k in wts.files if k.startswith(pre)})
    return ktr['network_fn'], ktr['network_fine']


def pair_launches(fn):
    """Paired trunk launches this process has enqueued (fastnerf_x6_pair_launches): which route a backward took."""
    return int(fn._lib.lib().fastnerf_x6_pair_launches())


def both_routes(fn, golden_dir, mode, n, Ns, Ni):
    """-> ((grads_c, grads_f) of the one call, (grads_c, grads_f) pass by pass) for one saving forward under `mode`.  Asserts the routes:
    the one call makes exactly one paired trunk launch in bf16x6 and none in the other modes, the pass-by-pass backward never makes one."""
    old = fn.ops.get_math()
    fn.ops.set_math(mode)
    try:
        net_c, net_f = _nets(fn, golden_dir, Ns, Ni)
        gen = torch.Generator().manual_seed(n * 1000 + Ns)
        K = np.array([[1111.1, 0, 400.0], [0, 1111.1, 400.0], [0, 0, 1]])
        poses = torch.stack([fn.synthetic.pose_spherical(-180.0 + 45.0 * k, -30.0, 4.0)[:3, :4] for k in range(8)], 0).cuda()
        pix = torch.stack([torch.randint(0, 8, (n,), generator=gen), torch.randint(0, 800, (n,), generator=gen),
                           torch.randint(0, 800, (n,), generator=gen)], 1).int().cuda()
        ro, rd = fn.ops.gen_rays_pixels(pix, poses, K)
        rays11 = fn.ops.pack_rays(ro, rd, 2.0, 6.0)
        tgt = torch.rand(n, 3, generator=gen).cuda()
        out, saved = fn.render._forward_core(rays11, net_c, net_f, Ns, Ni, False, 0.0, True, None, None, None, None, save=True)
        _, g1, g0 = fn.ops.mse_leafmax(out['rgb_map'], out['rgb0'], tgt)
        res = []
        for route in (fn.render._backward_core, fn.render._backward_passes):
            gc = torch.full_like(net_c.flat, float('nan'))
            gf = torch.full_like(net_f.flat, float('nan'))
            before = pair_launches(fn)
            route(saved, g1, g0, gc, gf)
            torch.cuda.synchronize()
            want = 1 if (route is fn.render._backward_core and mode == 'bf16x6') else 0
            assert pair_launches(fn) - before == want, (mode, route.__name__, pair_launches(fn) - before)
            res.append((gc, gf))
        return res
    finally:
        fn.ops.set_math(old)


def test_shapes_hit_the_chunk_counts(ncu):
    unit = max(1, ncu // 8)
    sh = shapes(ncu)
    eighths = {k: (trunk_chunks(n * Ns, ncu) // unit, trunk_chunks(n * (Ns + Ni), ncu) // unit) for k, (n, Ns, Ni) in sh.items()}
    assert eighths == {'ragged': (1, 1), 'equal': (1, 1), 'unequal': (1, 2)}, eighths


@pytest.mark.parametrize('case', ['ragged', 'equal', 'unequal'])
def test_one_call_equals_pass_by_pass_bf16x6(fn, golden_dir, ncu, case):
    n, Ns, Ni = shapes(ncu)[case]
    (gc, gf), (rc, rf) = both_routes(fn, golden_dir, 'bf16x6', n, Ns, Ni)
    assert torch.isfinite(gc).all() and torch.isfinite(gf).all()
    assert float(gf.abs().max()) > 0 and float(gc.abs().max()) > 0
    assert torch.equal(gf, rf), ('fine net', case, int((gf != rf).sum()))
    assert torch.equal(gc, rc), ('coarse net', case, int((gc != rc).sum()))


@pytest.mark.parametrize('mode', ['fp32', 'bf16x3'])
def test_other_modes_are_untouched(fn, golden_dir, mode):
    """fp32 and bf16x3 have no trunk launch: the one call is the two passes in a row there, as before."""
    (gc, gf), (rc, rf) = both_routes(fn, golden_dir, mode, 64, 16, 32)
    assert torch.isfinite(gc).all() and torch.isfinite(gf).all()
    assert torch.equal(gf, rf) and torch.equal(gc, rc)


def test_side_workspace_regrowth(fn, golden_dir):
    """The coarse pass's second dact / partial set grows on demand: small, larger, small again."""
    first = both_routes(fn, golden_dir, 'bf16x6', 64, 16, 32)[0]
    (gc, gf), (rc, rf) = both_routes(fn, golden_dir, 'bf16x6', 256, 48, 16)
    assert torch.equal(gf, rf) and torch.equal(gc, rc)
    third = both_routes(fn, golden_dir, 'bf16x6', 64, 16, 32)[0]
    assert torch.equal(first[0], third[0]) and torch.equal(first[1], third[1])


def test_two_streams_own_their_workspaces(fn, golden_dir):
    """The library-owned workspaces (head tiles, side dact, side partials: csrc/host_state.h fn::stream_ws) are kept per (device, stream):
    a stream's first call allocates its own, a larger call on one stream regrows that stream's only, and every stream computes what the
    default stream computes.  One call at a time, each followed by a synchronize: the keys are under test, not concurrency."""
    small, large = (64, 16, 32), (256, 48, 16)
    A, B = torch.cuda.Stream(), torch.cuda.Stream()

    def one_call(stream, shape):
        before = pair_launches(fn)
        if stream is None:
            res = both_routes(fn, golden_dir, 'bf16x6', *shape)[0]
        else:
            with torch.cuda.stream(stream):
                res = both_routes(fn, golden_dir, 'bf16x6', *shape)[0]
        torch.cuda.synchronize()
        assert pair_launches(fn) - before == 1      # (both_routes has checked that it was the one call's)
        return res

    ref_small = one_call(None, small)
    got = [(one_call(A, large), large), (one_call(B, small), small), (one_call(A, small), small)]
    ref = {small: ref_small, large: one_call(None, large)}      # (the default stream's own regrowth comes last: the order above is the test)
    for k, ((gc, gf), shape) in enumerate(got):
        assert torch.isfinite(gc).all() and torch.isfinite(gf).all() and float(gf.abs().max()) > 0 and float(gc.abs().max()) > 0
        assert torch.equal(gc, ref[shape][0]) and torch.equal(gf, ref[shape][1]), ('call', k + 2, shape)


def _trainer(fn):
    torch.manual_seed(3)
    args = fn.run_nerf.make_args(N_importance=32, N_samples=16, perturb=1.0, white_bkgd=True, no_reload=True, lrate=5e-4, lrate_decay=500)
    ktr = fn.run_nerf.create_nerf(args)[0]
    K = np.array([[40.0, 0, 16.0], [0, 40.0, 16.0], [0, 0, 1]])
    tr = fn.run_nerf.Trainer(ktr, 32, 32, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500)
    assert tr.fused and tr.world == 1
    return tr


def _phased_step(fn, tr, ro, rd, tgt):
    """Trainer.step's fused route with every phase in a call of its own (what the data-parallel step does around its all-reduce)."""
    L = fn._lib
    tr.adam_t += 1
    a, out, loss2, live = tr._fused_prepare(ro, rd, tgt, None, None, 0, None, None, None)
    a.lr, a.adam_t = float(tr.lr), int(tr.adam_t)
    for phase in (L.STEP_FORWARD, L.STEP_BWD_FINE, L.STEP_BWD_COARSE, L.STEP_UPDATE):
        tr._fused_call(a, phase)
    tr._after_backward(live)
    assert not live
    return loss2, out


def test_fused_step_equals_phase_by_phase(fn):
    old = fn.ops.get_math()
    fn.ops.set_math('bf16x6')
    try:
        g = torch.Generator().manual_seed(11)
        c2w = fn.synthetic.pose_spherical(20.0, -30.0, 4.0)[:3, :4]
        K = np.array([[40.0, 0, 16.0], [0, 40.0, 16.0], [0, 0, 1]])
        ro, rd = fn.run_nerf_helpers.get_rays(32, 32, K, c2w)
        ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
        batches = []
        for _ in range(2):
            sel = torch.randint(0, 1024, (64,), generator=g).cuda()
            batches.append((ro[sel].contiguous(), rd[sel].contiguous(), torch.rand(64, 3, generator=g).cuda()))
        res = []
        for phased in (False, True):
            tr = _trainer(fn)
            torch.manual_seed(5)            # the device-side Philox streams are keyed from torch's CPU generator
            losses = []
            before = pair_launches(fn)
            for b in batches:
                loss2, _ = _phased_step(fn, tr, *b) if phased else tr.step(*b, decay=False)
                losses.append(loss2.clone())
            assert not tr.last_step_live and tr.adam_t == 2
            assert pair_launches(fn) - before == (0 if phased else 2)     # the fused call pairs, the phase-split calls cannot
            res.append((torch.stack(losses), tr.flat.clone(), tr.m.clone(), tr.v.clone(), tr.grad.clone()))
        for x, y in zip(*res):
            assert torch.equal(x, y)
        assert float(res[0][4].abs().max()) > 0
    finally:
        fn.ops.set_math(old)
