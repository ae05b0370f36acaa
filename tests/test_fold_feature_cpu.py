"""The algebra of the folded view layer (csrc/mlp_pack.hip fold_kernel, csrc/mlp_bwd_dw.hip unfold_kernel) in torch float64, without a GPU.

The feature layer (256 -> 256, no activation) feeds the first 256 input columns of the view layer (-> 128, ReLU) and nothing else, so
    zv = Wv_a (Wf h7 + bf) + Wv_b vpe + bv = M h7 + Wv_b vpe + b',     M = Wv_a Wf,  b' = bv + Wv_a bf,
and with G = dL/dM = sum_p dzv_p h7_p^T the gradients of the two layers are
    dWf = Wv_a^T G,   dbf = Wv_a^T dbv,   dWv_a = G Wf^T + dbv bf^T.
Checked against autograd of the two-stage network to 1e-12 relative, with random masks, and for the identity feature layer of the
use_viewdirs=False emulation (M == Wv_a exactly)."""
import pytest
import torch

REL = 1e-12


def head(gen, identity=False):
    d = torch.float64
    W = {'Wf': torch.randn(256, 256, generator=gen, dtype=d) / 16, 'bf': torch.randn(256, generator=gen, dtype=d) * 0.1,
         'Wv': torch.randn(128, 283, generator=gen, dtype=d) / 16, 'bv': torch.randn(128, generator=gen, dtype=d) * 0.1,
         'Wr': torch.randn(3, 128, generator=gen, dtype=d) / 11}
    if identity:
        W['Wf'] = torch.eye(256, dtype=d)
        W['bf'] = torch.zeros(256, dtype=d)
    return W


def two_stage(W, h7, vpe):
    feat = h7 @ W['Wf'].t() + W['bf']
    return torch.cat([feat, vpe], 1) @ W['Wv'].t() + W['bv']


def fold(W):
    Wva = W['Wv'][:, :256]
    return Wva @ W['Wf'], W['bv'] + Wva @ W['bf']


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


@pytest.mark.parametrize('identity', [False, True])
def test_fold_and_unfold_equal_the_two_stage_network(identity):
    gen = torch.Generator().manual_seed(5 + identity)
    W = {k: v.requires_grad_(True) for k, v in head(gen, identity).items()}
    P = 64
    h7 = (torch.randn(P, 256, generator=gen, dtype=torch.float64) * (torch.rand(P, 256, generator=gen) < 0.5)).requires_grad_(True)   # post-ReLU
    vpe = torch.randn(P, 27, generator=gen, dtype=torch.float64)
    cot = torch.randn(P, 3, generator=gen, dtype=torch.float64)
    # two-stage forward and autograd
    zv = two_stage(W, h7, vpe)
    mask = (zv > 0).double().detach()
    rgb = (zv * mask) @ W['Wr'].t()
    (rgb * cot).sum().backward()
    # folded forward
    with torch.no_grad():
        M, b1 = fold(W)
        if identity:
            assert torch.equal(M, W['Wv'][:, :256]) and torch.equal(b1, W['bv'])
        zf = h7 @ M.t() + vpe @ W['Wv'][:, 256:].t() + b1
        assert rel(zf, zv) <= REL
        # folded backward: dzv, G, dbv, then the unfold
        dzv = (cot @ W['Wr']) * mask
        G, dbv = dzv.t() @ h7, dzv.sum(0)
        Wva = W['Wv'][:, :256]
        assert rel(Wva.t() @ G, W['Wf'].grad) <= REL
        assert rel(Wva.t() @ dbv, W['bf'].grad) <= REL
        assert rel(G @ W['Wf'].t() + torch.outer(dbv, W['bf']), W['Wv'].grad[:, :256]) <= REL
        assert rel(dzv.t() @ vpe, W['Wv'].grad[:, 256:]) <= REL
        assert rel(dbv, W['bv'].grad) <= REL
        assert rel(dzv @ M, h7.grad) <= REL          # dX: one K = 128 product
