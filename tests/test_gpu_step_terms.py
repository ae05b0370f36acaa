"""The training step with ALL its optional terms on at once -- depth / opacity supervision, per-ray background colours, the distortion loss --
which is the one case in which every tail of the step's block (run_nerf._term_regions: base | aux | bkgd | dist) is there:

  1. the fused step in one call = the phase-split step = the call-by-call route, bit for bit, on the plain and on the compacted backward;
  2. the marched step (background + distortion: it has no depth / opacity terms) in one call = forward + backward, then update;
  3. a step on an empty batch leaves the host RNG where the step on rays leaves it, on every route;
  4. (no GPU) the layout of the block for every subset of the terms.

Everything draws its own seeds (perturb = 1, bkgd = 'random', nothing injected), so the comparisons cover the order of the draws too."""
import itertools
import math

import numpy as np
import pytest
import torch

CAM = np.array([[14.0, 0, 4.0], [0, 14.0, 4.0], [0, 0, 1]])
N = 64
LAMBDAS = dict(lambda_depth=0.3, lambda_acc=0.2, lambda_dist=0.5)


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


@pytest.fixture
def math3(fn):
    old = fn.ops.get_math()
    yield fn.ops.set_math
    fn.ops.set_math(old)


@pytest.fixture
def compact(fn):
    old = fn.render.get_compact()
    yield fn.render.set_compact
    fn.render.set_compact(old)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def moments(tr):
    g = torch.Generator().manual_seed(5)      # moments that an update has to read
    tr.m.copy_(torch.rand(tr.m.numel(), generator=g) * 2e-3 - 1e-3)
    tr.v.copy_(torch.rand(tr.v.numel(), generator=g) * 1e-6)
    return tr


def dense_trainer(fn, fused=True):
    """8 + 8 samples, two networks lifted so that most samples are live, every term on."""
    args = fn.run_nerf.make_args(N_importance=8, N_samples=8, perturb=1.0, white_bkgd=False, use_viewdirs=True, no_reload=True)
    torch.manual_seed(3)
    ktr = fn.run_nerf.create_nerf(args)[0]
    with torch.no_grad():
        for net in (ktr['network_fn'], ktr['network_fine']):
            net.alpha_linear.bias.add_(0.3)
    tr = fn.run_nerf.Trainer(ktr, 8, 8, CAM, 2.0, 6.0, bkgd='random', **LAMBDAS)
    assert tr.fused
    tr.fused = fused
    return moments(tr)


def march_trainer(fn):
    import march_numpy as M
    import test_gpu_march_train as MT
    tr, _, _ = MT.new_trainer(fn, MT.device_grid(fn, M.two_shells()), N_samples=8, N_importance=8, perturb=1.0, white_bkgd=False, march=32,
                              march_cap=16, bkgd='random', lambda_dist=LAMBDAS['lambda_dist'])
    return moments(tr)


@pytest.fixture(scope='module')
def dense_batch(fn):
    """The 64 rays of the 8 x 8 camera, a target with its alpha, and depth / opacity targets some of whose weights are zero."""
    g = torch.Generator().manual_seed(11)
    ro, rd = fn.run_nerf_helpers.get_rays(8, 8, CAM, fn.synthetic.pose_spherical(20.0, -30.0, 4.0)[:3, :4])
    depth, dw = 2 + 4 * torch.rand(N, generator=g), (torch.rand(N, generator=g) > 0.3).float()
    depth[dw == 0] = float('nan')      # sparse depth: NaN where unknown, weight 0
    aw = (torch.rand(N, generator=g) > 0.2).float()
    assert 0 < int(dw.sum()) < N and 0 < int(aw.sum()) < N
    rays = (ro.reshape(-1, 3).contiguous().cuda(), rd.reshape(-1, 3).contiguous().cuda(), torch.rand(N, 3, generator=g).cuda())
    kw = dict(alpha=torch.rand(N, generator=g).cuda(), depth=depth.cuda(), depth_weight=dw.cuda(), acc=torch.rand(N, generator=g).cuda(),
              acc_weight=aw.cuda())
    return rays, kw


@pytest.fixture(scope='module')
def march_batch(fn):
    import test_gpu_march_train as MT
    return MT.batch(N, 3), dict(alpha=torch.rand(N, generator=torch.Generator().manual_seed(12)).cuda())


def result(tr, loss2, out):
    """Everything a step leaves behind, and where it leaves the host RNG."""
    torch.cuda.synchronize()
    res = dict(loss2=loss2, aux_losses=tr.aux_losses, dist_losses=tr.dist_losses, grad=tr.grad, flat=tr.flat, m=tr.m, v=tr.v)
    res = {k: t.clone() for k, t in res.items()}
    res['out'] = {k: out[k].clone() for k in out.keys()}
    res['rng'] = torch.get_rng_state()
    return res


def assert_same(got, want, what):
    for k in ('loss2', 'aux_losses', 'dist_losses', 'grad', 'flat', 'm', 'v'):
        assert torch.equal(bits(got[k]), bits(want[k])), (what, k)
    for k, t in want['out'].items():      # every key of the one-call step's out
        assert k in got['out'] and torch.equal(bits(got['out'][k]), bits(t)), (what, 'out', k)
    assert torch.equal(got['rng'], want['rng']), (what, 'host RNG')


# ---- 1. the fused step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['bf16x6', 'fp32'])
@pytest.mark.parametrize('backward', ['plain', 'compacted'])
def test_fused_step_with_every_term(fn, math3, compact, dense_batch, mode, backward):
    math3(mode)
    compact('0' if backward == 'plain' else '1')
    rays, kw = dense_batch
    L = fn._lib
    # one call
    tr = dense_trainer(fn)
    torch.manual_seed(7)
    start = torch.get_rng_state()
    loss2, out = tr.step(*rays, decay=False, **kw)
    one = result(tr, loss2, out)
    assert tr.last_step_live == (backward == 'compacted')
    assert tr._aux is not None and tr._bk is not None and tr._dist is not None, 'all three tails of the block'
    assert {'bkgd', 'dist_map', 'dist0', 'rgb_map', 'rgb0', 'weights', 'weights0'} <= set(out.keys())
    assert torch.isfinite(one['grad']).all() and float(one['grad'].abs().max()) > 0
    assert (one['aux_losses'] > 0).all() and (one['dist_losses'] > 0).all() and (one['loss2'] > 0).all(), 'every term is on'
    assert not torch.equal(one['rng'], start), 'the step draws its seeds'
    # the phases as the data-parallel step splits them
    ts = dense_trainer(fn)
    torch.manual_seed(7)
    ts.adam_t += 1
    a, outs, loss2s, live = ts._fused_prepare(*rays, None, None, 0, None, None, None, kw['alpha'], None, kw['depth'], kw['depth_weight'], kw['acc'],
                                              kw['acc_weight'])
    a.lr, a.adam_t = float(ts.lr), int(ts.adam_t)
    for phases in (L.STEP_FORWARD | L.STEP_BWD_FINE, L.STEP_BWD_COARSE, L.STEP_UPDATE):
        ts._fused_call(a, phases)
    ts._after_backward(live)
    assert_same(result(ts, loss2s, outs), one, 'phase split')
    # the call-by-call route
    tc = dense_trainer(fn, fused=False)
    torch.manual_seed(7)
    loss2c, outc = tc.step(*rays, decay=False, **kw)
    assert_same(result(tc, loss2c, outc), one, 'call by call')


# ---- 2. the marched step -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['bf16x6', 'fp32'])
def test_marched_step_with_its_terms(fn, math3, compact, march_batch, mode):
    math3(mode)
    compact('1')
    rays, kw = march_batch
    L = fn._lib
    tr = march_trainer(fn)
    torch.manual_seed(7)
    start = torch.get_rng_state()
    loss2, out = tr.step(*rays, decay=False, **kw)
    one = result(tr, loss2, out)
    assert tr._aux is None and tr._bk is not None and tr._dist is not None
    assert {'bkgd', 'dist_map', 'march_overflow', 'march_k'} <= set(out.keys()) and out['march_overflow'].dtype == torch.bool
    assert float(one['grad'].abs().max()) > 0 and float(one['dist_losses'][0]) > 0 and int(bits(one['aux_losses']).abs().max()) == 0
    assert not torch.equal(one['rng'], start), 'the step draws its seeds'
    t2 = march_trainer(fn)
    torch.manual_seed(7)
    t2.adam_t += 1
    a, x, out2, loss2b = t2._march_prepare(32, 16, *rays, None, None, 0, None, None, kw['alpha'], None)
    a.lr, a.adam_t = float(t2.lr), int(t2.adam_t)
    t2._march_call(a, x, L.STEP_FORWARD | L.STEP_BWD_FINE | L.STEP_BWD_COARSE)
    t2._march_call(a, x, L.STEP_UPDATE)
    out2['march_overflow'] = out2['march_overflow'].bool()      # (as step() hands it out)
    assert_same(result(t2, loss2b, out2), one, 'forward + backward, then update')


# ---- 3. the empty batch --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('route', ['fused', 'call_by_call', 'marched'])
def test_empty_batch_draws_what_the_step_draws(fn, compact, dense_batch, march_batch, route):
    compact('1')
    rays, kw = march_batch if route == 'marched' else dense_batch
    new = (lambda: march_trainer(fn)) if route == 'marched' else (lambda: dense_trainer(fn, fused=route == 'fused'))      # noqa: E731
    tr = new()
    torch.manual_seed(7)
    start = torch.get_rng_state()
    tr.step(*rays, **kw)
    torch.cuda.synchronize()
    after = torch.get_rng_state()
    assert not torch.equal(after, start)
    te = new()
    torch.manual_seed(7)
    loss2, out = te.step(*[t[:0] for t in rays], **{k: t[:0] for k, t in kw.items()})
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), after), 'an empty step leaves the host RNG where the step on rays leaves it'
    assert out == {} and loss2.tolist() == [0.0, 0.0] and te.aux_losses.tolist() == [0.0] * 4 and te.dist_losses.tolist() == [0.0] * 2


# ---- 4. the layout (no GPU) ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 63, 64, 65])
@pytest.mark.parametrize('S0,Ni', [(8, 0), (8, 8)])
def test_block_layout_for_every_subset_of_the_terms(n, S0, Ni):
    from fastnerf import run_nerf
    r = lambda k: (k + 63) // 64 * 64      # noqa: E731
    base, size = run_nerf._step_regions(n, S0, Ni)
    frozen = dict(base)
    # what each term appends: 4 rows + loss4 | colours, blended target, 2 rows | 2 per-ray rows, the weight-gradient rows of each pass, loss2d
    tails = dict(aux=4 * r(n) + 64, bkgd=2 * r(3 * n) + 2 * r(n), dist=2 * r(n) + r(n * (S0 + Ni)) + (r(n * S0) if Ni else 0) + 64)
    for on in itertools.product([False, True], repeat=3):
        terms = dict(zip(('aux', 'bkgd', 'dist'), on))
        regions, total = run_nerf._term_regions(base, size, n, S0, Ni, **terms)
        assert base == frozen, 'the cached base table is not written to'
        spans = sorted((off, off + math.prod(shape), name) for name, (off, shape) in regions.items())
        for off, end, name in spans:
            assert off % 64 == 0 and off < end <= total, name
        for (_, end, name), (off, _, other) in zip(spans, spans[1:]):
            assert end <= off, (name, other)
        for name, region in frozen.items():
            assert regions[name] == region, name
        # base | aux | bkgd | dist: a term starts where the terms before it end
        at = size
        for term in ('aux', 'bkgd', 'dist'):
            mine = [off for name, (off, _) in regions.items() if name.startswith(term + '.')]
            assert bool(mine) == terms[term], term
            if mine:
                assert min(mine) == at, term
                at += tails[term]
        assert total == at
