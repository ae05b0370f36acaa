"""References for the exposure table (csrc/exposure.hip; include/fastnerf.h, "exposure table"); no GPU needed.

Row i of ab [n_img,2] is (a_i, shift_i), scale_i = |a_i| + 0.5.  For ray r of image i = img[r], pass p, channel c:
    e_p[r,c] = (rgb_p[r,c] - shift_i) / scale_i
    g_p[r,c] = G_p[r,c] / scale_i                                   G_p = dL/de_p
    d_shift_i = -sum g,   d_scale_i = -sum g e                      over the rays of image i, both passes, three channels
    d_ab[i,0] = sign(a_i) (d_scale_i + lam gs cnt_i/n sign(scale_i - 1)),   d_ab[i,1] = d_shift_i + lam gs cnt_i/n sign(shift_i)
    loss_reg  = sum_i cnt_i/n (|scale_i - 1| + |shift_i|)
A ray whose img is outside [0, n_img) is left untouched and belongs to no image.

ref64          float64 autograd of these formulas written with torch.abs (the gradient kernel takes e and G as fp32 inputs: the
               reference rebuilds rgb = e scale + shift in float64, so that its e equals the input to 1e-16), and B: the same sums with
               every factor replaced by its absolute value
restate_*      numpy float32, operation by operation: the bits of e and of the in-place g; d_ab and loss_reg in ONE summation order (rays
               in batch order), which the kernel's tree does not share: they are compared through the bound
bound          |d_ab - ref64| <= (6 m_i + 32) 2^-24 B_i, m_i the rays of image i.  A row is a sum of at most 6 m_i terms g e (or g) of at
               most 3 roundings each (scale, the division, the product), so ANY order of adding them is within (6 m_i + 2) u B_i to first
               order; the penalty line adds 4 roundings of a term that B holds too.  A derived cap, not a measurement.
exact_case     integers for which every term is a multiple of 0.5 of magnitude <= 24 and every partial sum stays below 2^23 for
               n <= 2^15: any fp32 summation order gives the int64 sum."""
import numpy as np
import torch

U = 2.0 ** -24
F = np.float32


def bound_factor(m):
    return (6.0 * m + 32.0) * U


def in_range(img, n_img):
    return (img >= 0) & (img < n_img)


# ---- float64 ----------------------------------------------------------------------------------------------------------------------
def ref64(img, ab, lam, gs, e1, G1, e0=None, G0=None):
    """-> dict(d_ab [n_img,2], B [n_img,2], g1, g0, counts [n_img], loss_reg), float64 (counts int64).  img int [n]; ab [n_img,2];
    e*, G* [n,3]; all torch CPU tensors of any float dtype (taken as exact)."""
    n, n_img = img.shape[0], ab.shape[0]
    ab = ab.double().clone().requires_grad_(True)
    ok = in_range(img, n_img)
    idx = img.long().clamp(0, n_img - 1)
    scale, shift = torch.abs(ab[:, 0]) + 0.5, ab[:, 1]
    loss = torch.zeros((), dtype=torch.float64)
    gs_out = []
    Bs, Bsc = torch.zeros(n_img, dtype=torch.float64), torch.zeros(n_img, dtype=torch.float64)
    for e, G in ((e1, G1), (e0, G0)):
        if e is None:
            gs_out.append(None)
            continue
        e, G = e.double(), G.double()
        sc, sh = scale[idx][:, None], shift[idx][:, None]
        rgb = (e * sc + sh).detach()
        e_ = torch.where(ok[:, None], (rgb - sh) / sc, rgb)
        loss = loss + (G * e_).sum()
        g = torch.where(ok[:, None], G / sc.detach(), G)
        gs_out.append(g)
        Bs.index_add_(0, idx[ok], g.abs().sum(-1)[ok])
        Bsc.index_add_(0, idx[ok], (g.abs() * e.abs()).sum(-1)[ok])
    counts = torch.bincount(idx[ok], minlength=n_img)
    pull = torch.abs(scale - 1.0) + torch.abs(shift)
    frac = counts.double() / max(n, 1)
    loss_reg = (frac * pull).sum()
    loss = loss + lam * gs * loss_reg
    d_ab = torch.autograd.grad(loss, ab, allow_unused=True)[0]
    d_ab = torch.zeros_like(ab) if d_ab is None else d_ab
    pen = lam * gs * frac
    sgn = lambda x: torch.sign(x).abs()      # noqa: E731
    sc_d, sh_d = scale.detach(), shift.detach()
    a_d = ab.detach()[:, 0]
    B = torch.stack([sgn(a_d) * (Bsc + pen * sgn(sc_d - 1.0)), Bs + pen * sgn(sh_d)], 1)
    return dict(d_ab=d_ab.detach(), B=B, g1=gs_out[0], g0=gs_out[1], counts=counts, loss_reg=loss_reg.detach())


# ---- numpy float32, operation by operation ---------------------------------------------------------------------------------------
def scale_of(ab):
    return (np.abs(ab[:, 0]) + F(0.5)).astype(F)


def restate_apply(img, ab, rgb):
    """e [n,3] float32 with the kernel's bits: one fsub, one IEEE division; rgb's bits for a ray outside the table."""
    img, ab, rgb = np.asarray(img), np.asarray(ab, F), np.asarray(rgb, F)
    ok = in_range(img, ab.shape[0])
    idx = np.clip(img, 0, ab.shape[0] - 1)
    e = ((rgb - ab[idx, 1][:, None]).astype(F) / scale_of(ab)[idx][:, None]).astype(F)
    return np.where(ok[:, None], e, rgb)


def restate_grad(img, ab, lam, gs, e1, G1, e0=None, G0=None):
    """-> dict(g1, g0: the bits of the in-place gradient; d_ab, counts, loss_reg: in batch order)."""
    img, ab = np.asarray(img), np.asarray(ab, F)
    n, n_img = img.shape[0], ab.shape[0]
    ok = in_range(img, n_img)
    idx = np.clip(img, 0, n_img - 1)
    scale = scale_of(ab)
    g = [None if G is None else np.where(ok[:, None], (np.asarray(G, F) / scale[idx][:, None]).astype(F), np.asarray(G, F)) for G in (G1, G0)]
    es = [None if e is None else np.asarray(e, F) for e in (e1, e0)]
    d_ab, counts = np.zeros((n_img, 2), F), np.zeros(n_img, np.int32)
    reg = F(0.0)
    sign = lambda x: F((x > 0) - F(x < 0))      # noqa: E731
    for i in range(n_img):
        rows = np.nonzero(ok & (img == i))[0]
        m = counts[i] = rows.shape[0]
        if m == 0:
            continue
        # a ray's terms: the image pass's three channels, then the coarse pass's
        tg = np.concatenate([x[rows] for x in g if x is not None], 1).reshape(-1)
        tge = np.concatenate([(x[rows] * e[rows]).astype(F) for x, e in zip(g, es) if x is not None], 1).reshape(-1)
        s_g, s_ge = np.cumsum(tg, dtype=F)[-1], np.cumsum(tge, dtype=F)[-1]
        frac = F(F(m) / F(n))
        pen = F(F(F(lam) * F(gs)) * frac)
        a, shift = ab[i]
        d_ab[i, 0] = F(sign(a) * F(-s_ge + F(pen * sign(F(scale[i] - F(1.0))))))
        d_ab[i, 1] = F(-s_g + F(pen * sign(shift)))
        pull = F(np.abs(F(scale[i] - F(1.0))) + np.abs(shift))
        reg = F(reg + F(frac * pull))
    return dict(g1=g[0], g0=g[1], d_ab=d_ab, counts=counts, loss_reg=reg)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def image_list(n, n_img, gen, empty=None, outside=False):
    """img int32 [n] over the images of the table; `empty`: an image that gets no ray; outside: every 13th ray names no image (-1 or
    n_img, in turn)."""
    img = torch.randint(0, n_img, (n,), generator=gen)
    if empty is not None and n_img > 1:
        img[img == empty] = (empty + 1) % n_img
    if outside:
        img[5::26] = -1
        img[18::26] = n_img
    return img.int()


def float_case(n, n_img, two, seed, empty=None, outside=True):
    """a in +-[0.3, 1.5], shift in +-0.1, colours in [0, 1), G ~ N(0, 1) / n."""
    gen = torch.Generator().manual_seed(seed)
    a = (0.3 + 1.2 * torch.rand(n_img, generator=gen)) * (torch.randint(0, 2, (n_img,), generator=gen) * 2 - 1)
    ab = torch.stack([a, (torch.rand(n_img, generator=gen) - 0.5) * 0.2], 1).float()
    img = image_list(n, n_img, gen, empty, outside)
    new = lambda: torch.rand(n, 3, generator=gen)      # noqa: E731
    grad = lambda: torch.randn(n, 3, generator=gen) / max(n, 1)      # noqa: E731
    return dict(img=img, ab=ab, rgb1=new(), G1=grad(), rgb0=new() if two else None, G0=grad() if two else None)


def exact_case(n, n_img, two, seed, empty=None):
    """a in {0, 0.5, 1.5, -1.5} (scale in {0.5, 1, 2}), integer shift in [-2, 2], integer colours in [-4, 4], G = scale * k with integer k
    in [-2, 2]; lam = 0.  -> the case and `want`: d_ab [n_img,2] and counts as exact integers' floats (float64)."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.tensor([0.0, 0.5, 1.5, -1.5])[torch.randint(0, 4, (n_img,), generator=gen)]
    shift = torch.randint(-2, 3, (n_img,), generator=gen).float()
    ab = torch.stack([a, shift], 1)
    img = image_list(n, n_img, gen, empty)
    scale = a.abs() + 0.5
    idx = img.long()
    case = dict(img=img, ab=ab)
    want = torch.zeros(n_img, 2, dtype=torch.float64)
    for p in ((1, 0) if two else (1,)):
        rgb = torch.randint(-4, 5, (n, 3), generator=gen).float()
        k = torch.randint(-2, 3, (n, 3), generator=gen)
        case['rgb%d' % p], case['G%d' % p] = rgb, k.float() * scale[idx][:, None]
        # twice e, an integer: 2 (rgb - shift) / scale with 2 / scale in {4, 2, 1}
        e2 = (rgb.long() - shift.long()[idx][:, None]) * (2.0 / scale).long()[idx][:, None]
        want[:, 1].index_add_(0, idx, -k.sum(-1).double())
        want[:, 0].index_add_(0, idx, -(k * e2).sum(-1).double() / 2.0)
    if not two:
        case['rgb0'] = case['G0'] = None
    want[:, 0] *= torch.sign(a).double()
    return case, want, torch.bincount(idx, minlength=n_img)
