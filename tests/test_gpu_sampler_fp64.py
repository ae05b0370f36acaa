"""sample_pdf_merge_kernel through its four entry points (ops.sample_pdf, ops.pp_sample_pdf, ops.sample_pdf_merge,
ops.pp_sample_pdf_merge) against the float64 reference with per-sample conditioning of tests/sampler_ref.py: every sample within
the float32 bound of an allowed candidate, on the injected-u and the det route (the Philox route: test_gpu_seeded_draws.py), from
one weight and one sample up to S = 512 and Ni = 1024, past the first trip of the grid-stride loop, and with tied depths."""
import pytest
import torch

import sampler_ref as R

pytestmark = pytest.mark.gpu

GRID_ROWS = 16384      # grid_waves caps the launch at 4096 blocks of 4 waves: ray 16384 is the first of a wave's second trip


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return fastnerf


def full_weights(w, gen):
    """[n,S] weights whose inner S-2 columns are w; the merge ops must not read the outer two."""
    n = w.shape[0]
    return torch.cat([torch.rand(n, 1, generator=gen), w, torch.rand(n, 1, generator=gen)], -1).contiguous()


def run_ops(fn, variant, z, w, u, det):
    """name -> (samples, z_out or None, z_std or None) of the two entry points of one variant, on the CPU."""
    n, Ni = u.shape
    kw = dict(det=True) if det else dict(u=u.cuda())
    gen = torch.Generator().manual_seed(z.shape[1])
    bins_op, merge_op = ((fn.ops.sample_pdf, fn.ops.sample_pdf_merge), (fn.ops.pp_sample_pdf, fn.ops.pp_sample_pdf_merge))[variant]
    out = {bins_op.__name__: (bins_op(R.mid(z).cuda(), w.cuda(), Ni, **kw).cpu(), None, None)}
    res = merge_op(z.cuda(), full_weights(w, gen).cuda(), Ni, **kw)
    out[merge_op.__name__] = (res[1].cpu(), res[0].cpu(), res[2].cpu() if len(res) > 2 else None)
    return out


def check_case(fn, tag, variant, z, w, u, det, stats, tail=None):
    bins = R.mid(z)
    for name, (smp, z_out, z_std) in run_ops(fn, variant, z, w, u, det).items():
        assert smp.shape == u.shape and torch.isfinite(smp).all(), (name, tag)
        v = R.judge(smp.numpy(), bins.numpy(), w.numpy(), u.numpy(), variant)
        worst, excl = stats.get(name, (0.0, 0.0))
        stats[name] = (max(worst, v.worst), max(excl, v.excluded))
        assert v.violations == 0, (name, tag, v)
        assert v.excluded <= 0.005, (name, tag, v)
        if tail is not None:
            vt = R.judge(smp[tail:].numpy(), bins[tail:].numpy(), w[tail:].numpy(), u[tail:].numpy(), variant)
            assert vt.violations == 0 and vt.excluded < 1, (name, tag, 'rows >= %d' % tail, vt)
        if z_out is not None:
            both = torch.sort(torch.cat([z, smp], -1), -1).values
            assert torch.equal(z_out.view(torch.int32), both.view(torch.int32)), (name, tag)
            assert (z_out[:, 1:] >= z_out[:, :-1]).all(), (name, tag)
        if z_std is not None:
            ref = smp.double().std(-1, unbiased=False)
            assert ((z_std.double() - ref).abs() <= 2e-5 + 1e-5 * ref).all(), (name, tag, float((z_std.double() - ref).abs().max()))


def report(stats, tag):
    for name, (worst, excl) in sorted(stats.items()):
        print('SAMPLER_FP64 %s %-20s worst error/bound %.3f  excluded at most %.4f %%' % (tag, name, worst, 100 * excl))


@pytest.mark.parametrize('S,Ni', R.SHAPES)
def test_samplers_against_float64(fn, S, Ni):
    stats = {}
    for kind, variant, route, z, w, u in R.cases(S, Ni):
        check_case(fn, (S, Ni, kind, route), variant, z, w, u, route == 'det', stats)
    report(stats, 'S=%d Ni=%d' % (S, Ni))


def test_second_trip_of_the_grid_stride_loop(fn):
    """n = 16384 + 3: the last three rays are taken by waves on their second trip, over LDS they have already used."""
    stats = {}
    for kind, variant, route, z, w, u in R.cases(4, 5, n=GRID_ROWS + 3, kinds=('random',)):
        check_case(fn, (kind, route), variant, z, w, u, route == 'det', stats, tail=GRID_ROWS)
    report(stats, 'n=%d S=4 Ni=5' % (GRID_ROWS + 3))


def test_tied_depths(fn, S=66, Ni=65):
    """z[:, k+1] = z[:, k] for a seeded third of the k: zero-width bins, and equal keys in the merge."""
    stats = {}
    for kind, variant, route, z, w, u in R.cases(S, Ni, ties=True):
        assert (z[:, 1:] == z[:, :-1]).any()
        check_case(fn, (S, Ni, kind, route, 'ties'), variant, z, w, u, route == 'det', stats)
    report(stats, 'ties S=%d Ni=%d' % (S, Ni))
