"""float64 reference of the two inverse-CDF samplers, with per-sample conditioning (numpy, no GPU).

variant 0 = NeRF (run_nerf_helpers.sample_pdf): eps 1e-5, index = searchsorted(cdf, u, right=True) over all M cdf entries.
variant 1 = NeRF++ (ddp_train_nerf.sample_pdf): eps 1e-6, index = #(u >= cdf[:M-1]), bin width + 1e-6.

A float32 sampler is a discontinuous function of its own rounding: a `u` that lies within the float32 error of a cdf knot may
fall into either neighbouring bin, and a bin whose cdf step lies within that error of eps may or may not take the `denom -> 1`
branch.  So the reference does not return one value per sample but a short list of candidates, each with the error a correct
float32 evaluation may have against it, and `judge` accepts a sample that is within the bound of any allowed candidate.

E = 4 * 2^-24 is the allowed |cdf32 - cdf64|: (w + eps), the sum and the quotient round once each (3 * 2^-24 relative, cdf <= 1)
and the cdf entry itself rounds once more (2^-25).  A sample b0 + (u - c0) / d * width then moves by at most width * 3E / d
(c0, c1 and the quotient), plus the roundings of the bins and of the result, 4 * 2^-24 * max(|b0|, |b1|)."""
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24
E = 4 * U
EPS = (1e-5, 1e-6)
SHAPES = ((3, 1), (3, 2), (4, 5), (64, 128), (65, 64), (66, 65), (130, 200), (257, 513), (512, 1024))     # (S, Ni)
KINDS = ('random', 'zero', 'twohot', 'surface')

Candidate = namedtuple('Candidate', 'value bound switch_ambiguous allowed')
Verdict = namedtuple('Verdict', 'excluded violations worst')


def _take(a, i):
    return np.take_along_axis(a, i, -1)


def pdf_cdf(weights, variant):
    """float64 (pdf [n,M-1], cdf [n,M]) of float32 weights."""
    w = np.asarray(weights, np.float32).astype(np.float64) + EPS[variant]
    pdf = w / w.sum(-1, keepdims=True)
    return pdf, np.concatenate([np.zeros_like(pdf[:, :1]), np.cumsum(pdf, -1)], -1)


def ref(bins, weights, u, variant):
    """bins [n,M], weights [n,M-1], u [n,Ni] (float32) -> [nominal, one lower, one higher] Candidates of [n,Ni] arrays."""
    eps = EPS[variant]
    b = np.asarray(bins, np.float32).astype(np.float64)
    u = np.asarray(u, np.float32).astype(np.float64)
    _, cdf = pdf_cdf(weights, variant)
    M = cdf.shape[1]
    K = M - 1 if variant else M          # number of knots searched
    knots = cdf[:, :K]
    idx = (u[:, :, None] >= knots[:, None, :]).sum(-1)       # >= 1: knot 0 is exactly 0

    def at(i, allowed):
        below, above = np.maximum(i - 1, 0), np.minimum(i, M - 1)
        c0, c1, b0, b1 = _take(cdf, below), _take(cdf, above), _take(b, below), _take(b, above)
        denom = c1 - c0
        d = np.where(denom < eps, 1.0, denom)
        width = (b1 - b0) + (eps if variant else 0.0)
        value = b0 + (u - c0) / d * width
        bound = np.abs(width) * 3 * E / d + 4 * U * np.maximum(np.abs(b0), np.abs(b1))
        return Candidate(value, bound, np.abs(denom - eps) <= 2 * E, allowed)

    # the knot that one index lower / higher would put on the other side of u; knot 0 is 0 in every precision: never crossed
    lower = (idx >= 2) & (np.abs(u - _take(knots, np.clip(idx - 1, 0, K - 1))) <= E)
    higher = (idx <= K - 1) & (np.abs(u - _take(knots, np.clip(idx, 0, K - 1))) <= E)
    return [at(idx, np.ones(idx.shape, bool)), at(np.maximum(idx - 1, 1), lower), at(np.minimum(idx + 1, K), higher)]


def judge(got, bins, weights, u, variant):
    """Verdict(excluded share, number of violations, worst error / bound among the judged samples) of samples `got` [n,Ni]."""
    got = np.asarray(got).astype(np.float64)
    ratio = np.full(got.shape, np.inf)
    excluded = np.zeros(got.shape, bool)
    for c in ref(bins, weights, u, variant):
        ratio = np.minimum(ratio, np.where(c.allowed, np.abs(got - c.value) / c.bound, np.inf))
        excluded |= c.allowed & c.switch_ambiguous
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    judged = ~excluded
    return Verdict(float(excluded.mean()), int(((ratio > 1) & judged).sum()), float(ratio[judged].max()) if judged.any() else 0.0)


def make_z(n, S, gen, ties=False):
    """Sorted depths [n,S] in [2, 6]; ties: z[:, k+1] = z[:, k] for a seeded third of the k."""
    z = torch.sort(torch.rand(n, S, generator=gen) * 4 + 2, -1).values
    if ties:
        for k in torch.nonzero(torch.rand(S - 1, generator=gen) < 1 / 3).flatten().tolist():
            z[:, k + 1] = z[:, k]
    return z.contiguous()


def mid(z):
    return (0.5 * (z[:, 1:] + z[:, :-1])).contiguous()


def make_weights(kind, n, NW, gen):
    """float32 weights [n,NW] of one kind."""
    if kind == 'random':
        return torch.rand(n, NW, generator=gen) ** 4
    if kind == 'zero':
        return torch.zeros(n, NW)
    if kind == 'twohot':          # two weights of 1.5; with fewer than 3 weights there is no empty bin to keep: all 0
        w = torch.zeros(n, NW)
        if NW >= 3:
            w.scatter_(1, torch.stack([torch.randperm(NW, generator=gen)[:2] for _ in range(n)]), 1.5)
        return w
    if kind == 'surface':
        centre = NW * torch.rand(n, 1, generator=gen)
        return torch.exp(-0.5 * ((torch.arange(NW)[None] - centre) / 1.5) ** 2)
    raise ValueError(kind)


def linspace_u(n, Ni):
    return torch.linspace(0.0, 1.0, Ni).expand(n, Ni).contiguous()


def twohot_u(weights, Ni, variant, gen):
    """u [n,Ni] inside the empty bins of `twohot` weights: float32(cdf64[k] + f * pdf64[k]), f in [0.2, 0.8], k a seeded
    empty bin.  None when the weights have no empty bin."""
    w = weights.numpy()
    n, NW = w.shape
    if NW < 3 or not ((w != 0).sum(-1) == 2).all():
        return None
    pdf, cdf = pdf_cdf(w, variant)
    score = torch.rand(n, NW, generator=gen).numpy() + (w != 0)                # empty bins sort first
    empty = np.argsort(score, -1)[:, :NW - 2]
    k = _take(empty, torch.randint(0, NW - 2, (n, Ni), generator=gen).numpy())
    f = 0.2 + 0.6 * torch.rand(n, Ni, generator=gen).double().numpy()
    return torch.from_numpy((_take(cdf, k) + f * _take(pdf, k)).astype(np.float32))


def cases(S, Ni, n=24, kinds=KINDS, ties=False):
    """(kind, variant, route, z [n,S], weights [n,S-2], u [n,Ni]) of one shape: route 'u' = injected uniforms, 'det' = the
    linspace a det=True call uses, 'twohot_u' = injected uniforms inside the empty bins.  bins = mid(z)."""
    gen = torch.Generator().manual_seed(S * 7 + Ni + (1000 if ties else 0))
    z = make_z(n, S, gen, ties)
    u = torch.rand(n, Ni, generator=gen)
    for kind in kinds:
        w = make_weights(kind, n, S - 2, gen)
        for variant in (0, 1):
            yield kind, variant, 'u', z, w, u
            yield kind, variant, 'det', z, w, linspace_u(n, Ni)
            if kind == 'twohot':
                ut = twohot_u(w, Ni, variant, gen)
                if ut is not None:
                    yield kind, variant, 'twohot_u', z, w, ut
