"""The NeRF++ compositing rule (ddp_model.py:97-135, oracle/nerfpp_oracle.nerfnet_forward with the networks taken out) as a plain
torch function, and the inputs that make it hard.  It runs in the dtype of `raw`: float64 is the reference, float32 on the CPU is
the yardstick of what float32 arithmetic itself loses."""
import torch

EPS = 1e-6            # TINY_NUMBER
HUGE = 1e10           # HUGE_NUMBER
KINDS = ('random', 'saturate', 'thin', 'opaque', 'zero_sigma')
SIZES = (2, 3, 63, 64, 65, 129, 512)


def composite(raw, z, dnorm, fg_far, part):
    """raw [n,S,4] in consumption order (part 1: far -> near, as the background MLP writes it), z [n,S] as stored (near -> far),
    dnorm [n] = |d|, fg_far [n] (part 0) -> rgb [n,3], weights [n,S] (consumption order), depth [n], lambda [n]
    (depth and weights before the multiplication by lambda; lambda = the product of every 1 - alpha + 1e-6)."""
    z, dnorm = z.to(raw.dtype), dnorm.to(raw.dtype)
    sigma, colour = raw[..., 3].abs(), torch.sigmoid(raw[..., :3])
    if part == 0:
        zc = z
        dists = dnorm[:, None] * torch.cat((z[:, 1:] - z[:, :-1], fg_far.to(raw.dtype)[:, None] - z[:, -1:]), -1)
    else:
        zc = torch.flip(z, dims=[-1])
        dists = torch.cat((zc[:, :-1] - zc[:, 1:], HUGE * torch.ones_like(zc[:, :1])), -1)
    alpha = 1.0 - torch.exp(-sigma * dists)
    T = torch.cumprod(1.0 - alpha + EPS, dim=-1)
    lam = T[:, -1]
    T = torch.cat((torch.ones_like(T[:, :1]), T[:, :-1]), -1)
    weights = alpha * T
    return (weights[..., None] * colour).sum(-2), weights, (weights * zc).sum(-1), lam


def grad(raw, z, dnorm, fg_far, part, g_rgb, g_lambda, dtype=torch.float64):
    """d(sum(rgb * g_rgb) + sum(lambda * g_lambda)) / d raw by autograd in `dtype` (either cotangent may be None)."""
    x = raw.to(dtype).requires_grad_(True)
    rgb, _, _, lam = composite(x, z, dnorm, fg_far, part)
    loss = 0.0
    if g_rgb is not None:
        loss = loss + (rgb * g_rgb.to(dtype)).sum()
    if g_lambda is not None:
        loss = loss + (lam * g_lambda.to(dtype)).sum()
    return torch.autograd.grad(loss, x)[0]


def make_case(kind, n, S, part, seed):
    """float32 (raw [n,S,4], z [n,S], rays_o [n,3], rays_d [n,3], fg_far [n] or None, g_rgb [n,3], g_lambda [n]).  As make_case of
    test_gpu_raw2outputs_grad.py, the per-sample optical depth x is chosen and sigma = +-x / dist, so that the alphas are well
    conditioned in float32 where the gradient lives.  |d| in [0.5, 2]; part 0: z in [1e-3, 1.5], fg_far = z_last + [0.05, 0.25];
    part 1: z in [0.01, 0.99]."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=gen)       # noqa: E731
    rd = rn(n, 3)
    rd = (rd / rd.norm(dim=-1, keepdim=True) * (0.5 + 1.5 * ru(n, 1))).float()
    dnorm = rd.double().norm(dim=-1)
    if part == 0:
        z = torch.sort(ru(n, S) * 1.5 + 1e-3, -1).values
        far = z[:, -1] + 0.05 + 0.2 * ru(n)
        dist = torch.cat((z[:, 1:] - z[:, :-1], (far - z[:, -1])[:, None]), -1).double() * dnorm[:, None]
    else:
        z = torch.sort(ru(n, S) * 0.98 + 0.01, -1).values
        far = None
        zc = torch.flip(z, [-1])
        dist = torch.cat((zc[:, :-1] - zc[:, 1:], torch.ones(n, 1)), -1).double()     # (the 1e10 interval: x / 1 is saturated anyway)
    dist = dist.clamp(min=1e-30)
    sign = lambda: torch.sign(rn(n, S))                 # noqa: E731
    if kind in ('random', 'zero_sigma'):
        x = 0.3 * (rn(n, S) + 0.5)
    elif kind == 'saturate':
        x = (1.5 + ru(n, S)) * sign()
    elif kind == 'thin':
        x = (0.5 / S) * ru(n, S) * sign()
    elif kind == 'opaque':
        x = 30.0 * ru(n, S) * sign()
    else:
        raise ValueError(kind)
    if kind == 'zero_sigma':
        x[ru(n, S) < 0.25] = 0.0
    raw = torch.cat((2.0 * rn(n, S, 3), (x.double() / dist).float()[..., None]), -1).float().contiguous()
    assert torch.isfinite(raw).all()
    ro = 0.1 * rn(n, 3)
    return raw, z.float().contiguous(), ro, rd.contiguous(), None if far is None else far.float(), rn(n, 3), rn(n)
