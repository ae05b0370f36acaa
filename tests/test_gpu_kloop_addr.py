"""The addressing of the bf16x6 forward / dX k-loops (csrc/mlp_common.h gemm_seg16: register-held LDS addresses, scalar weight bases, the
row bursts of the saved tensors, the row copy of a partial tile) computes no value: every output is a function of the point alone.

Small point counts around the 64-point tile -- 1, 63, 64 (one full tile: the burst), 65 (a full tile and a one-row tile: burst and row
copy in one launch), 200 (three full tiles and one of 8 rows, more than one workgroup) -- on kind 0 (63-channel encoding) and kind 2
(nerf++ background: the extra 32 encoding channels, k-loops of one k-step).

  * the saving and the non-saving forward give the same logits, bit for bit;
  * position independence: the same 200 points alone and behind 37 unrelated points (every row in another tile row, another swizzle class,
    another tile) give bit-equal logits, saved rows (pe, h0..h7, vpe, hv) and, after the backward with the same cotangent rows, bit-equal
    pre-activation gradient rows (dY0..dY7, dYv);
  * a live-list forward / backward over the identity list equals the plain one: saved rows, gradient rows, parameter gradients; the list
    forward's logits (kind 0, the only kind it serves) equal the plain forward's;
  * the `feat` holes of act / dact, pre-filled with a sentinel, come back untouched, and no saved row keeps a sentinel;
  * logits and parameter gradients against the float64 reference of tests/test_gpu_mlp_fp64.py, at that file's bars.
Every bit-equality also holds for the kernels before the change (measured: profiles/kloop_addr.md).
"""
import os

import numpy as np
import pytest
import torch

import test_gpu_mlp_fp64 as F

pytestmark = pytest.mark.gpu

PS = [1, 63, 64, 65, 200]
KINDS = [0, 2]
SENTINEL = 0x7FC12345          # a NaN with a payload: no kernel output


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


_NETS, _RUNS = {}, {}


def net(golden_dir, kind):
    if kind not in _NETS:
        if kind == 0:
            g7 = np.load(os.path.join(golden_dir, 'g7_weights.npz'))
            flat = F.flat_kind0({k[2:]: torch.from_numpy(g7[k]) for k in g7.files if k.startswith('c.')}).cuda()
        else:
            w = np.load(os.path.join(golden_dir, 'g10_pp_weights.npz'))
            pre = 'l0.bg_net.'
            flat = F.flat_pp({k[len(pre):]: torch.from_numpy(w[k]) for k in w.files if k.startswith(pre)}, 84).cuda()
        _NETS[kind] = flat
    return _NETS[kind]


def batch(fn, golden_dir, kind, n, seed):
    """n points, one per ray (S = 1), and a cotangent without a zero row (so that the live list of it is the identity)."""
    gen = torch.Generator(device='cuda').manual_seed(1000 * kind + seed)
    if kind == 0:
        rays, z, _ = F.kind0_batch(fn, golden_dir, n, 1, seed=seed)
    else:   # ray origins inside the unit sphere, depths = inverse radii in (0, 1)
        ro = (torch.rand(n, 3, generator=gen, device='cuda') - 0.5) * 0.8
        rd = torch.randn(n, 3, generator=gen, device='cuda')
        rays = fn.ops.pack_rays(ro, rd, 0.0, 0.0)
        z = torch.rand(n, 1, generator=gen, device='cuda') * 0.98 + 0.01
    cot = torch.randn(n, 1, 4, generator=gen, device='cuda')
    cot[cot == 0] = 1.0
    return rays, z, cot


def regions(P, kind):
    """{name: (float offset, row width)} of the saved activations / of the pre-activation gradients (csrc/mlp_layout.h)"""
    pep = 96 if kind == 2 else 64
    act = {'pe': (0, pep), 'vpe': (P * (pep + 2048 + 256), 32), 'hv': (P * (pep + 2048 + 256 + 32), 128)}
    act.update({'h%d' % l: (P * pep + l * P * 256, 256) for l in range(8)})
    dact = {'Y%d' % l: (l * P * 256, 256) for l in range(8)}
    dact['Yv'] = (9 * P * 256, 128)
    holes = {'act': (P * (pep + 2048), P * 256), 'dact': (8 * P * 256, P * 256)}
    return act, dact, holes


def rows(buf, reg, p0, p1):
    off, w = reg
    return buf[off + p0 * w: off + p1 * w].view(torch.int32)


def sentinel_buffer(nfloats):
    return torch.full((nfloats,), SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)


def run_x6(fn, golden_dir, kind, rays, z, cot, live=False):
    """bf16x6 saving forward + backward into sentinel-filled buffers -> dict(raw, g, act, dact); live: through the identity live list"""
    flat = net(golden_dir, kind)
    P = z.numel()
    old = fn.ops.get_math()
    fn.ops.set_math('bf16x6')
    try:
        pf, pb = fn.ops.mlp_pack(flat, kind=kind)
        act = sentinel_buffer(fn.ops.act_floats(P, kind))
        dact = sentinel_buffer(fn.ops.dact_floats(P, kind))
        partial = torch.empty(fn.ops.mlp_bwd_partial_floats(), device='cuda')
        g = torch.full((fn.ops.net_floats(kind, 0),), float('nan'), device='cuda')
        out = {}
        if live:
            idx, cnt = fn.ops.compact_live(cot)
            assert cnt.tolist() == [P, P] and torch.equal(idx[:P].long(), torch.arange(P, device='cuda'))
            fn.ops.mlp_fwd_live(rays, z, flat, pf, act, idx, cnt, kind=kind)
            fn.ops.mlp_bwd_live(cot, act, flat, pb, dact, partial, g, idx, cnt, kind=kind)
            if kind == 0:
                raw = sentinel_buffer(P * 4)
                out['raw'] = fn.ops.mlp_fwd_list(rays, z, flat, pf, raw, idx, cnt).reshape(P, 4)
        else:
            out['raw'] = fn.ops.mlp_fwd(rays, z, flat, pf, act=act, kind=kind).reshape(P, 4).clone()
            out['raw_nosave'] = fn.ops.mlp_fwd(rays, z, flat, pf, kind=kind).reshape(P, 4).clone()
            fn.ops.mlp_bwd(cot, act, flat, pb, dact, partial, g, kind=kind)
        torch.cuda.synchronize()
        out.update(g=g, act=act, dact=dact)
        return out
    finally:
        fn.ops.set_math(old)


def plain_run(fn, golden_dir, kind, P):
    """one plain run per (kind, P), shared by the tests below and left unchanged"""
    if (kind, P) not in _RUNS:
        b = batch(fn, golden_dir, kind, P, seed=P)
        _RUNS[(kind, P)] = (b, run_x6(fn, golden_dir, kind, *b))
    return _RUNS[(kind, P)]


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('P', PS)
def test_saving_and_plain_forward_agree_and_holes_stay(fn, golden_dir, kind, P):
    _, r = plain_run(fn, golden_dir, kind, P)
    assert torch.isfinite(r['raw']).all() and torch.isfinite(r['g']).all()
    assert torch.equal(bits(r['raw']), bits(r['raw_nosave'])), 'saving and non-saving forward differ'
    ra, rd, holes = regions(P, kind)
    for name, buf in (('act', r['act']), ('dact', r['dact'])):
        off, n = holes[name]
        assert bool((buf[off:off + n].view(torch.int32) == SENTINEL).all()), '%s: the feat hole was written' % name
    for name, reg in ra.items():    # every saved row written, nothing of the sentinel left in it
        assert not bool((rows(r['act'], reg, 0, P) == SENTINEL).any()), name
    for name, reg in rd.items():
        assert not bool((rows(r['dact'], reg, 0, P) == SENTINEL).any()), name


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('P', PS)
def test_identity_live_list_equals_plain(fn, golden_dir, kind, P):
    b, r = plain_run(fn, golden_dir, kind, P)
    v = run_x6(fn, golden_dir, kind, *b, live=True)
    ra, rd, holes = regions(P, kind)
    for name, reg in ra.items():
        assert torch.equal(rows(v['act'], reg, 0, P), rows(r['act'], reg, 0, P)), ('saved rows', name)
    for name, reg in rd.items():
        assert torch.equal(rows(v['dact'], reg, 0, P), rows(r['dact'], reg, 0, P)), ('gradient rows', name)
    assert torch.equal(bits(v['g']), bits(r['g'])), 'parameter gradients'
    for name, buf in (('act', v['act']), ('dact', v['dact'])):
        off, n = holes[name]
        assert bool((buf[off:off + n].view(torch.int32) == SENTINEL).all()), '%s: the feat hole was written' % name
    if kind == 0:
        assert torch.equal(bits(v['raw']), bits(r['raw'])), 'list forward logits'


@pytest.mark.parametrize('kind', KINDS)
def test_position_independence(fn, golden_dir, kind):
    P, SHIFT = 200, 37
    (rays, z, cot), r = plain_run(fn, golden_dir, kind, P)
    o_rays, o_z, o_cot = batch(fn, golden_dir, kind, SHIFT, seed=7777)
    s = run_x6(fn, golden_dir, kind, torch.cat([o_rays, rays]).contiguous(), torch.cat([o_z, z]).contiguous(),
               torch.cat([o_cot, cot]).contiguous())
    assert torch.equal(bits(s['raw'][SHIFT:]), bits(r['raw'])), 'logits'
    assert torch.equal(bits(s['raw_nosave'][SHIFT:]), bits(r['raw'])), 'logits of the non-saving forward'
    ra, rd, _ = regions(P, kind)
    sa, sd, _ = regions(P + SHIFT, kind)
    for name in ra:
        assert torch.equal(rows(s['act'], sa[name], SHIFT, SHIFT + P), rows(r['act'], ra[name], 0, P)), ('saved rows', name)
    for name in rd:
        assert torch.equal(rows(s['dact'], sd[name], SHIFT, SHIFT + P), rows(r['dact'], rd[name], 0, P)), ('gradient rows', name)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('P', PS)
def test_logits_and_gradients_vs_fp64(fn, golden_dir, kind, P):
    """the bars of tests/test_gpu_mlp_fp64.py: logits within 2e-5 of max(1, |raw64|), gradients (a) and (b)"""
    flat = net(golden_dir, kind)
    W = F.split_flat(flat, kind)
    rays, z, cot = plain_run(fn, golden_dir, kind, P)[0]
    e = {}
    for mode in ('fp32', 'bf16x6'):
        raw, g, bufs = F.run_kernels(fn, mode, rays, z, cot, flat, kind)
        assert torch.isfinite(g).all(), (kind, P, mode)
        raw64, ref, _ = F.reference(W, kind, mode, rays, z, cot, bufs)
        assert ref.flips[1] == 0, ('kernel ReLU decisions that fp64 contradicts above the margin', kind, P, mode, ref.flips)
        e[mode] = F.e_of(g, ref, kind)
        rms = F.check_raw('kind %d P=%d %s' % (kind, P, mode), raw, raw64)
        print('kind %d P=%d %s: RMS logit error vs fp64 %.2e' % (kind, P, mode, rms))
    F.check_grads('kloop kind %d P=%d' % (kind, P), e, kind)
