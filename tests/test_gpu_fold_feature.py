"""The folded view layer of the fp32 / bf16x6 kernels (feature layer multiplied into the view layer: csrc/mlp_pack.hip fold_kernel,
csrc/mlp_fwd.hip, csrc/mlp_bwd_dx.hip, csrc/mlp_bwd_dw.hip unfold_kernel) against float64 at small point counts.

Cases: kind 0 at P = 17, 64, 65, 1000 (below one 64-point tile, one tile, tile + 1, tails of the dW k-steps), kinds 1 and 2 at P = 65.
  * logits within 2e-5 max(1, |raw64|) of an fp64 evaluation of the UNFOLDED network (the bound of tests/test_gpu_mlp_fp64.py);
  * F.W, F.b, V.W, V.b, A.W, A.b against fp64 autograd with the kernel's ReLU masks, metric e_T of tests/test_gpu_mlp_fp64.py:
    e_T(bf16x6) <= 2 e_T(fp32) + 2^-24 and both <= 2^-14;
  * saving and non-saving forward agree bit for bit; the live-list backward over a full list equals the plain backward bit for bit;
  * after an Adam step and a repack, M^T in the packed backward buffer is the fp64 product Wv[:, :256] Wf of the NEW weights rounded to
    fp32 (bf16x6: its three planes sum back to it bit for bit);
  * the feat / dfeat regions of act / dact are holes: a NaN pattern written before the calls is still there, and every gradient is finite.

The forward's part of the fold lives in the packed forward buffer itself (csrc/mlp_layout.h PFM | PFB | PFR), kinds 0 and 2 at P = 65 (one
64-point tile plus one point; kind 2 shifts every offset), both modes:
  * a clone of a packed forward buffer gives the same logits bit for bit, saving and non-saving, through the C entry points;
  * a pack call writes every word of the packed forward buffer, and what was there before does not reach the logits;
  * the plain floats at PFR / PFB and the decoded PFM block are the fp64 M = Wv[:, :256] Wf and b' = bv + Wv[:, :256] bf rounded once to fp32
    ([M | Wv[:, 256:] | 0]; bf16x6: the three planes sum back bit for bit).
"""
import os

import numpy as np
import pytest
import torch

import test_gpu_mlp_fp64 as F
from oracle import nerfpp_oracle as PP

pytestmark = pytest.mark.gpu

TENSORS = ['F.W', 'F.b', 'V.W', 'V.b', 'A.W', 'A.b']
PATTERN = 0x7FC12345            # a quiet NaN with a payload
MODES = ('fp32', 'bf16x6')


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


def nan_filled(n):
    return torch.full((n,), PATTERN, dtype=torch.int32, device='cuda').view(torch.float32)


def net_and_batch(fn, golden_dir, kind, P):
    if kind == 0:
        g7 = np.load(os.path.join(golden_dir, 'g7_weights.npz'))
        flat = F.flat_kind0({k[2:]: torch.from_numpy(g7[k]) for k in g7.files if k.startswith('c.')}).cuda()
    else:
        w = np.load(os.path.join(golden_dir, 'g10_pp_weights.npz'))
        pre = 'l0.fg_net.' if kind == 1 else 'l0.bg_net.'
        flat = F.flat_pp({k[len(pre):]: torch.from_numpy(w[k]) for k in w.files if k.startswith(pre)}, 63 if kind == 1 else 84).cuda()
    gen = torch.Generator(device='cuda').manual_seed(100 * kind + P)
    if kind == 2:   # ray origins inside the unit sphere, depths = inverse radii in (0, 1)
        ro = (torch.rand(P, 3, generator=gen, device='cuda') - 0.5) * 0.8
        rd = torch.randn(P, 3, generator=gen, device='cuda')
        rays = fn.ops.pack_rays(ro, rd, 0.0, 0.0)
        z = torch.rand(P, 1, generator=gen, device='cuda') * 0.98 + 0.01
    else:
        rays, z, _ = F.kind0_batch(fn, golden_dir, P, 1, seed=P + kind)
    cot = torch.randn(P, 1, 4, generator=gen, device='cuda')      # every row non-zero: the live list is the full list
    return flat, rays, z, cot


def run(fn, mode, flat, rays, z, cot, kind):
    """-> dict of the saving forward + plain backward, the non-saving forward and the live-list route over the full list."""
    P = z.numel()
    fn.ops.set_math(mode)
    pf, pb = fn.ops.mlp_pack(flat, kind=kind)
    out = {'pf': pf, 'pb': pb}
    act, dact = nan_filled(fn.ops.act_floats(P, kind)), nan_filled(fn.ops.dact_floats(P, kind))
    partial = torch.empty(fn.ops.mlp_bwd_partial_floats(), device='cuda')
    out['raw'] = fn.ops.mlp_fwd(rays, z, flat, pf, act=act, kind=kind)
    out['raw_nosave'] = fn.ops.mlp_fwd(rays, z, flat, pf, kind=kind)
    g = torch.full((fn.ops.net_floats(kind, 0),), float('nan'), device='cuda')
    fn.ops.mlp_bwd(cot, act, flat, pb, dact, partial, g, kind=kind)
    out.update(g=g, act=act, dact=dact)
    idx, cnt = fn.ops.compact_live(cot)
    assert cnt.tolist() == [P, P]
    act2, dact2 = nan_filled(act.numel()), nan_filled(dact.numel())
    fn.ops.mlp_fwd_live(rays, z, flat, pf, act2, idx, cnt, kind=kind)
    g2 = torch.full_like(g, float('nan'))
    fn.ops.mlp_bwd_live(cot, act2, flat, pb, dact2, partial, g2, idx, cnt, kind=kind)
    out['g_live'] = g2
    torch.cuda.synchronize()
    return out


def packed_mt(fn, pb, kind, mode):
    """M [128][256] (float64) decoded from the M^T block of the packed backward buffer."""
    off = int(fn._lib.lib().fastnerf_mlp_fold_offset(kind, 3))
    if mode == 'fp32':      # [(jt*KS + ks)*64 + l][t] = M[ks*8 + (l>>5)*4 + t][jt*32 + (l&31)], KS = 16
        blk = pb[off:off + 128 * 256].cpu().numpy().reshape(8, 16, 2, 32, 4)            # [jt][ks][half][c][t]
        return blk.transpose(1, 2, 4, 0, 3).reshape(128, 256).astype(np.float64), None
    u16 = pb.cpu().numpy().view(np.uint16)
    u0 = off * 3 // 8       # uint4 units: [tile][ks][plane][lane][8] = M[ks*32 + (l>>4)*8 + e][tile*16 + (l&15)]
    blk = u16[u0 * 8:(u0 + 16 * 4 * 3 * 64) * 8].reshape(16, 4, 3, 4, 16, 8)            # [tile][ks][plane][kc][c][e]
    planes = (blk.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    tot = planes[:, :, 0] + planes[:, :, 1] + planes[:, :, 2]                            # [tile][ks][kc][c][e]
    return tot.transpose(1, 2, 4, 0, 3).reshape(128, 256), planes


@pytest.mark.parametrize('kind,P', [(0, 17), (0, 64), (0, 65), (0, 1000), (1, 65), (2, 65)])
def test_folded_view_layer_vs_fp64(fn, golden_dir, kind, P):
    flat, rays, z, cot = net_and_batch(fn, golden_dir, kind, P)
    W = F.split_flat(flat, kind)
    pep = 96 if kind == 2 else 64
    old = fn.ops.get_math()
    e = {}
    try:
        for mode in MODES:
            r = run(fn, mode, flat, rays, z, cot, kind)
            case = 'kind %d P=%d %s' % (kind, P, mode)
            # holes: nothing wrote feat / dfeat, so nothing may have read them
            feat = r['act'][P * (pep + 2048):P * (pep + 2048 + 256)].view(torch.int32)
            dfeat = r['dact'][8 * P * 256:9 * P * 256].view(torch.int32)
            assert bool((feat == PATTERN).all()) and bool((dfeat == PATTERN).all()), (case, 'feat / dfeat regions were written')
            assert torch.isfinite(r['g']).all() and torch.isfinite(r['raw']).all(), case
            # routes
            assert torch.equal(r['raw'], r['raw_nosave']), (case, 'saving and non-saving forward differ')
            assert torch.equal(r['g'], r['g_live']), (case, 'live-list backward over the full list differs from the plain backward')
            # fp64
            raw64, ref, _ = F.reference(W, kind, mode, rays, z, cot, (r['act'], r['dact']))
            assert ref.flips[1] == 0, (case, ref.flips)
            d = (r['raw'].reshape(-1, 4).double() - raw64).abs() / raw64.abs().clamp(min=1.0)
            print('\n%s: max |raw - raw64| / max(1, |raw64|) = %.2e' % (case, float(d.max())))
            assert float(d.max()) <= 2e-5, (case, float(d.max()))
            e[mode] = F.e_of(r['g'], ref, kind)
    finally:
        fn.ops.set_math(old)
    for k in TENSORS:
        print('kind %d P=%d  e_T(%s): fp32 %.2e  bf16x6 %.2e' % (kind, P, k, e['fp32'][k], e['bf16x6'][k]))
    for k in TENSORS:
        assert e['bf16x6'][k] <= 2 * e['fp32'][k] + 2.0 ** -24, (kind, P, k, e['bf16x6'][k], e['fp32'][k])
        assert max(e['fp32'][k], e['bf16x6'][k]) <= 2.0 ** -14, (kind, P, k, e['fp32'][k], e['bf16x6'][k])


@pytest.mark.parametrize('mode', MODES)
def test_repack_after_adam_refolds(fn, golden_dir, mode):
    flat, rays, z, cot = net_and_batch(fn, golden_dir, 0, 65)
    old = fn.ops.get_math()
    try:
        r = run(fn, mode, flat, rays, z, cot, 0)
        flat2 = flat.clone()
        m, v = torch.zeros_like(flat), torch.zeros_like(flat)
        fn.ops.adam_step(flat2, r['g'], m, v, 5e-4, 1)
        assert not torch.equal(flat2, flat)
        fn.ops.mlp_pack(flat2, r['pf'], r['pb'], kind=0)
        torch.cuda.synchronize()
        got, planes = packed_mt(fn, r['pb'], 0, mode)
        W = F.split_flat(flat2.double(), 0)
        want = (W['V.W'][:, :256] @ W['F.W']).float().cpu().numpy()
        assert np.array_equal(got.astype(np.float32), want), 'M in the packed buffer is not the fp64 product of the new weights rounded to fp32'
        if planes is not None:
            assert np.array_equal(got, want.astype(np.float64)), 'the three bf16 planes do not sum back to M bit for bit'
        # and the forward runs on the refolded layer: logits of the new weights against fp64
        raw = fn.ops.mlp_fwd(rays, z, flat2, r['pf'])
        act = torch.empty(fn.ops.act_floats(65), device='cuda')
        fn.ops.mlp_fwd(rays, z, flat2, r['pf'], act=act)
        raw64, _, _ = F.reference(F.split_flat(flat2, 0), 0, mode, rays, z, cot, (act, nan_filled(fn.ops.dact_floats(65))))
        d = (raw.reshape(-1, 4).double() - raw64).abs() / raw64.abs().clamp(min=1.0)
        assert float(d.max()) <= 2e-5, float(d.max())
    finally:
        fn.ops.set_math(old)


# ---- the forward's part of the fold is part of the packed forward buffer ----------------------------------------------------------
IN_BUFFER_CASES = [(0, 65), (2, 65)]


def c_fwd(fn, rays, z, flat, pf, kind, save):
    """Logits from the current mode's forward entry point of the C ABI, called on `pf` as it is (ops.mlp_fwd refuses a packed buffer
    that ops.mlp_pack did not hand out)."""
    P = z.numel()
    raw = torch.full((P, 1, 4), float('nan'), device='cuda')
    act = nan_filled(fn.ops.act_floats(P, kind)) if save else None
    f, name = fn.ops._mlp('fwd', kind)
    flags = (0,) if name == 'fastnerf_mlp_x6_fwd' else ()
    fn.ops.check(f(kind, P, 1, fn.ops.ptr(rays), fn.ops.ptr(z), fn.ops.ptr(flat), fn.ops.ptr(pf), fn.ops.ptr(raw), fn.ops.ptr(act),
                   *flags, fn.ops.stream()), name)
    torch.cuda.synchronize()
    return raw


def fold_offsets(fn, kind, mode):
    """(PFM in units of the fp32 packing, float offsets of the plain b' and M) in a packed forward buffer of this mode."""
    pfm, pfb, pfr = (int(fn._lib.lib().fastnerf_mlp_fold_offset(kind, w)) for w in range(3))
    x = 3 if mode == 'bf16x6' else 2
    return pfm, pfb * x // 2, pfr * x // 2


def packed_pfm(pf, pfm, mode):
    """[128][288] (float64) decoded from the PFM block of the packed forward buffer, and the bf16x6 planes (None under fp32)."""
    if mode == 'fp32':      # [(nt*KS + ks)*64 + l][t] = W'[nt*32 + (l&31)][ks*8 + (l>>5)*4 + t], KS = 36
        blk = pf[pfm:pfm + 128 * 288].cpu().numpy().reshape(4, 36, 2, 32, 4)             # [nt][ks][half][n][t]
        return blk.transpose(0, 3, 1, 2, 4).reshape(128, 288).astype(np.float64), None
    u16 = pf.cpu().numpy().view(np.uint16)
    u0 = pfm * 3 // 8       # uint4 units: [tile][ks][plane][lane][8] = W'[tile*16 + (l&15)][ks*32 + (l>>4)*8 + e]
    blk = u16[u0 * 8:(u0 + 8 * 9 * 3 * 64) * 8].reshape(8, 9, 3, 4, 16, 8)               # [tile][ks][plane][kc][n][e]
    planes = (blk.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    tot = planes[:, :, 0] + planes[:, :, 1] + planes[:, :, 2]                            # [tile][ks][kc][n][e]
    return tot.transpose(0, 3, 1, 2, 4).reshape(128, 288), planes


@pytest.mark.parametrize('kind,P', IN_BUFFER_CASES)
@pytest.mark.parametrize('mode', MODES)
def test_copy_of_packed_fwd_is_the_buffer(fn, golden_dir, mode, kind, P):
    flat, rays, z, _ = net_and_batch(fn, golden_dir, kind, P)
    old = fn.ops.get_math()
    try:
        fn.ops.set_math(mode)
        pf, _ = fn.ops.mlp_pack(flat, kind=kind)
        pf2 = pf.clone()
        for save in (False, True):
            want, got = c_fwd(fn, rays, z, flat, pf, kind, save), c_fwd(fn, rays, z, flat, pf2, kind, save)
            assert torch.isfinite(want).all(), (mode, kind, save)
            assert torch.equal(got, want), (mode, kind, save, 'logits from a clone of packed_fwd differ')
    finally:
        fn.ops.set_math(old)


@pytest.mark.parametrize('kind,P', IN_BUFFER_CASES)
@pytest.mark.parametrize('mode', MODES)
def test_pack_writes_all_of_packed_fwd_and_reads_nothing_else(fn, golden_dir, mode, kind, P):
    flat, rays, z, _ = net_and_batch(fn, golden_dir, kind, P)
    old = fn.ops.get_math()
    try:
        fn.ops.set_math(mode)
        n = fn.ops.packed_floats(kind, 1)
        pf_nan, _ = fn.ops.mlp_pack(flat, nan_filled(n), kind=kind)
        pf_zero, _ = fn.ops.mlp_pack(flat, torch.zeros(n, device='cuda'), kind=kind)
        torch.cuda.synchronize()
        left = int((pf_nan.view(torch.int32) == PATTERN).sum())
        assert left == 0, (mode, kind, '%d of %d words of packed_fwd were not written by the pack call' % (left, n))
        assert torch.equal(pf_nan.view(torch.int32), pf_zero.view(torch.int32))
        raw = fn.ops.mlp_fwd(rays, z, flat, pf_nan, kind=kind)
        assert torch.isfinite(raw).all(), (mode, kind)
        assert torch.equal(raw, fn.ops.mlp_fwd(rays, z, flat, pf_zero, kind=kind)), (mode, kind)
    finally:
        fn.ops.set_math(old)


@pytest.mark.parametrize('kind,P', IN_BUFFER_CASES)
@pytest.mark.parametrize('mode', MODES)
def test_fold_regions_of_packed_fwd_hold_the_fp64_fold(fn, golden_dir, mode, kind, P):
    flat, _, _, _ = net_and_batch(fn, golden_dir, kind, P)
    W = F.split_flat(flat.double(), kind)
    Wv = W['V.W']
    m_want = (Wv[:, :256] @ W['F.W']).float().cpu().numpy()                       # fp64, rounded once
    b_want = (W['V.b'] + Wv[:, :256] @ W['F.b']).float().cpu().numpy()
    block_want = np.concatenate([m_want, Wv[:, 256:].float().cpu().numpy(), np.zeros((128, 5), np.float32)], 1)
    old = fn.ops.get_math()
    try:
        fn.ops.set_math(mode)
        pf, _ = fn.ops.mlp_pack(flat, kind=kind)
        torch.cuda.synchronize()
    finally:
        fn.ops.set_math(old)
    pfm, b_off, m_off = fold_offsets(fn, kind, mode)
    assert np.array_equal(pf[m_off:m_off + 128 * 256].cpu().numpy().reshape(128, 256), m_want), (mode, kind, 'plain M')
    assert np.array_equal(pf[b_off:b_off + 128].cpu().numpy(), b_want), (mode, kind, "plain b'")
    got, planes = packed_pfm(pf, pfm, mode)
    assert np.array_equal(got.astype(np.float32), block_want), (mode, kind, 'the PFM block is not [M | Wv[:, 256:] | 0]')
    if planes is not None:
        assert np.array_equal(got, block_want.astype(np.float64)), (mode, kind, 'the three bf16 planes do not sum back bit for bit')
