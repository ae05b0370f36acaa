"""tests/sampler_ref.py judged on the CPU: it accepts the two float32 torch oracles over every shape, weight kind and route the
GPU test (test_gpu_sampler_fp64.py) uses, and it rejects samplers that are wrong in the ways a kernel could be."""
import numpy as np
import pytest
import torch

import sampler_ref as R
from oracle import nerf_oracle as O
from oracle import nerfpp_oracle as PP

ORACLES = (O.sample_pdf, PP.sample_pdf)


def cdf32(weights, variant):
    """The cdf as the float32 oracles form it (torch's float32 cumsum)."""
    w = weights + R.EPS[variant]
    pdf = w / w.sum(-1, keepdim=True)
    return torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)


@pytest.mark.parametrize('S,Ni', R.SHAPES)
def test_reference_accepts_the_float32_oracles(S, Ni):
    """0 violations, at most 0.5 % excluded, worst error / bound at most 0.5, over every shape, kind and route of the GPU test.

    The reference's premise is a cdf within E = 4 * 2^-24 of float64.  sample_pdf_merge_kernel keeps it by construction (it sums
    the float32 pdf in float64 and rounds once per entry) and is judged with E on every row.  torch's float32 cumsum adds
    sequentially in float32 and leaves it on some rows: up to 1.8 E at S = 64 and 2.2 E at S = 512 with `twohot` weights, 1.25 E on
    every row of `zero` at S = 512.  Where u lies in a run of empty bins (cdf steps of 3.3e-7 in variant 1) such a cdf moves the
    index by two bins.  The same happens past a `surface` bump whose far weights underflow to 0.  The reference has nothing to
    say about such a row, so the three bars are asserted on the rows where the oracle's own cdf (never its samples) is within E
    of float64; the others are judged too, and their count and violations printed."""
    for kind, variant, route, z, w, u in R.cases(S, Ni):
        bins = R.mid(z)
        err = np.abs(cdf32(w, variant).numpy().astype(np.float64) - R.pdf_cdf(w.numpy(), variant)[1]).max(-1)
        got, within = ORACLES[variant](bins, w, Ni, u).numpy(), err <= R.E
        sel = lambda rows, *ts: [np.asarray(t)[rows] for t in ts]      # noqa: E731
        line = 'S=%d Ni=%d %-8s variant %d %-8s rows beyond E %d (max %.2f E)' % (S, Ni, kind, variant, route, int((~within).sum()), err.max() / R.E)
        if within.any():
            v = R.judge(*sel(within, got, bins, w, u), variant)
            line += ' excluded %.4f%% worst %.3f' % (100 * v.excluded, v.worst)
            assert v.violations == 0, (line, v)
            assert v.excluded <= 0.005, (line, v)      # the reference alone stays at or under 0.13 %
            assert v.worst <= 0.5, (line, v)           # measured 0.38
        if not within.all():       # reported, not asserted
            v = R.judge(*sel(~within, got, bins, w, u), variant)
            line += ' | rows beyond E: %d violations, excluded %.4f%%' % (v.violations, 100 * v.excluded)
        print(line)


def sampler32(bins, weights, u, variant, eps=None, right=True, above_max=None, lower=None):
    """The float32 sampler of either variant with the places a kernel can get wrong as knobs (all defaults = the oracle):
    eps, the side of the search, the clamp of `above`, and a mask of samples whose index is taken one too low."""
    eps = R.EPS[variant] if eps is None else eps
    w = weights + eps
    pdf = w / w.sum(-1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)
    M = cdf.shape[-1]
    knots = (cdf[:, :M - 1] if variant else cdf)[:, None, :]
    inds = ((u[..., None] >= knots) if right else (u[..., None] > knots)).sum(-1)
    if lower is not None:
        inds = inds - lower.long()
    below = (inds - 1).clamp(min=0)
    above = inds.clamp(max=M - 1 if above_max is None else above_max)
    c0, c1, b0, b1 = cdf.gather(-1, below), cdf.gather(-1, above), bins.gather(-1, below), bins.gather(-1, above)
    denom = c1 - c0
    denom = torch.where(denom < eps, torch.ones_like(denom), denom)
    return b0 + (u - c0) / denom * (b1 - b0 + (eps if variant else 0.0))


def _case(S, Ni, kind, route):
    for k, variant, r, z, w, u in R.cases(S, Ni, kinds=(kind,)):
        if r == route:
            yield variant, R.mid(z), w, u


def _verdict(got, bins, w, u, variant):
    return R.judge(got.numpy(), bins.numpy(), w.numpy(), u.numpy(), variant)


def test_knobs_at_rest_are_the_oracles():
    for variant, bins, w, u in _case(64, 128, 'random', 'u'):
        assert torch.equal(sampler32(bins, w, u, variant), ORACLES[variant](bins, w, 128, u))


def test_mutant_eps_of_the_other_variant():
    for variant, bins, w, u in _case(64, 128, 'random', 'u'):
        v = _verdict(sampler32(bins, w, u, variant, eps=R.EPS[1 - variant]), bins, w, u, variant)
        assert v.violations > 0.2 * u.numel(), (variant, v)


def test_mutant_index_one_too_low_on_two_percent():
    for variant, bins, w, u in _case(64, 128, 'random', 'u'):
        lower = torch.rand(u.shape, generator=torch.Generator().manual_seed(11)) < 0.02
        v = _verdict(sampler32(bins, w, u, variant, lower=lower), bins, w, u, variant)
        assert v.violations >= 0.8 * int(lower.sum()), (variant, int(lower.sum()), v)


def test_mutant_above_clamped_one_bin_too_low():
    for variant, bins, w, u in _case(64, 128, 'random', 'u'):
        v = _verdict(sampler32(bins, w, u, variant, above_max=bins.shape[-1] - 2), bins, w, u, variant)
        assert v.violations > 0, (variant, v)


def test_mutant_row_shift():
    for kind in ('random', 'surface', 'twohot'):
        for variant, bins, w, u in _case(64, 128, kind, 'u'):
            v = _verdict(sampler32(bins, torch.roll(w, 1, 0), u, variant), bins, w, u, variant)
            assert v.violations > 0.2 * u.numel(), (kind, variant, v)


def test_search_side_at_a_knot_is_not_observable():
    """`right=False` in place of `right=True` on the `zero` kind at S = 65, Ni = 64, det, where the knots are the linspace values
    and the samples sit on them.  The inverse cdf is continuous at its knots: the bin below gives b0 + 1 * (b1 - b0), the bin above
    gives b1 + 0, so this mutant returns the oracle's samples bit for bit there and no judge of sample values can reject it (a
    kernel that searched with lower_bound would be as right as one that searches with upper_bound).  What is asserted is that
    the premise holds (the samples do sit on knots, so both sides are reached) and that the reference accepts both sides."""
    for variant, bins, w, u in _case(65, 64, 'zero', 'det'):
        knots = R.pdf_cdf(w.numpy(), variant)[1][:, None, :]
        on_knot = (np.abs(u.numpy().astype(np.float64)[..., None] - knots) <= R.E).any(-1)
        assert on_knot.mean() > 0.95
        mutant, oracle = sampler32(bins, w, u, variant, right=False), ORACLES[variant](bins, w, 64, u)
        inds = lambda right: ((u[..., None] >= cdf32(w, variant)[:, None, :]) if right else (u[..., None] > cdf32(w, variant)[:, None, :])).sum(-1)  # noqa: E731
        assert (inds(True) != inds(False)).any(-1).all()                 # the two searches do pick different bins, on every ray
        assert (mutant - oracle).abs().max() <= 4 * R.U * 6.0            # and return the same depth (z <= 6)
        for got in (mutant, oracle):
            v = _verdict(got, bins, w, u, variant)
            assert v.violations == 0 and v.excluded == 0, (variant, v)
