"""The loss, the optimizer and their neighbours in csrc/train.hip against the float64 restatements of tests/train_ref.py, in every
launch regime: mse_leafmax_kernel with one workgroup (n <= 65536, up to 64 rays per thread), with up to 1024 workgroups meeting in
atomics behind a memset, and grid-striding beyond 2^20 rays; adam_kernel with its float4 body, its tail and its grid stride beyond
2,097,152 floats; leaf_sumcount_kernel and gauss_noise_kernel past their grid caps.  Every bound is a count of roundings (u = 2^-24,
derived in tests/train_ref.py and validated on the CPU in tests/test_train_ref_cpu.py) or a bit-exact equality."""
import numpy as np
import pytest
import torch

import philox_numpy as P
import train_ref as T
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

U = T.U
F32 = np.float32
B1, B2, EPS = 0.9, 0.999, 1e-8
N_IMG, MAX_LEAVES = 3, 20
LOSS_N = (1, 1023, 1025, 65536, 65537, 1048576 + 1025)
HOT = (0, 1023, 1024, 65535, 65536, 1048575, 1048576)


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return fastnerf


def tags_of(n, rs):
    tag = np.stack([rs.randint(0, N_IMG, n), rs.randint(0, MAX_LEAVES, n)], 1)
    tag[rs.randint(0, n)] = (N_IMG - 1, MAX_LEAVES - 1)      # the last slot of the table, (2, 19), is in use
    return torch.from_numpy(tag)


def run_loss(fn, rgb, rgb0, tgt, tag, grad_scale=1.0, want_grads=True):
    table = torch.zeros(N_IMG * MAX_LEAVES, dtype=torch.int32, device='cuda')
    loss2, g, g0 = fn.ops.mse_leafmax(rgb, rgb0, tgt, grad_scale=grad_scale, want_grads=want_grads, leaf_tag=tag, max_leaves=MAX_LEAVES,
                                      table=table)
    return loss2.cpu().numpy(), g, g0, table.view(torch.float32).view(N_IMG, MAX_LEAVES).cpu()


# ---- 1. the loss ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grad_scale', [1.0, 0.25])
@pytest.mark.parametrize('two', [True, False], ids=['rgb0', 'no_rgb0'])
@pytest.mark.parametrize('n', LOSS_N)
def test_loss_of_exact_terms(fn, n, two, grad_scale):
    """target is a multiple of 2^-10 in [0, 1) and rgb = target + s / 2, s in {-1, 0, 1}: every difference is 0 or +-0.5 exactly, every
    square 0.25, every partial sum a multiple of 0.25 below 2^24 * 0.25 -- exact in fp32 in any order, S = 0.25 * (number of s != 0).
    One workgroup (g = 1): loss == fl(S) * fl(1 / 3n) bit for bit.  g > 1: a block's product with inv_count rounds once and every
    atomic addition once, each relative to at most the total: within g u loss of S / 3n.  (Counting the rounding of inv_count itself
    and the first, exact, addition the strict count is g + 1; the tighter g is asserted, the measured worst is 15 of 1024.)
    The gradient is fl(2 grad_scale / 3n) * (+-0.5) or 0: a product with a power of two, bit for bit.  The leaf table is a max: exact."""
    g_blocks, _, _ = T.loss_chain(n)
    rs = np.random.RandomState(n % 9973 + (7 if two else 0))
    tgt = (rs.randint(0, 1024, (n, 3)) / 1024.0).astype(F32)
    s, s0 = (rs.randint(-1, 2, (n, 3)).astype(F32) for _ in range(2))
    rgb, rgb0 = tgt + F32(0.5) * s, tgt + F32(0.5) * s0
    tag = tags_of(n, rs)
    loss2, g, g0, table = run_loss(fn, torch.from_numpy(rgb).cuda(), torch.from_numpy(rgb0).cuda() if two else None,
                                   torch.from_numpy(tgt).cuda(), tag.int().cuda(), grad_scale)
    inv = F32(1.0 / (3.0 * n))
    for k, sk in enumerate((s, s0) if two else (s,)):
        S = 0.25 * np.count_nonzero(sk)
        if g_blocks == 1:
            assert loss2[k] == F32(S) * inv, (k, loss2[k], F32(S) * inv)
        else:
            exact = S / (3.0 * n)
            err = abs(float(loss2[k]) - exact)
            print('LOSS_EXACT n=%d pass %d: |loss - S/3n| = %.3g u loss (bound %d)' % (n, k, err / (U * exact), g_blocks))
            assert err <= g_blocks * U * exact
    if not two:
        assert loss2[1] == 0.0 and g0 is None
    gscale = F32(2.0 / (3.0 * n) * grad_scale)
    assert np.array_equal(g.cpu().numpy(), gscale * (F32(0.5) * s))
    if two:
        assert np.array_equal(g0.cpu().numpy(), gscale * (F32(0.5) * s0))
    assert torch.equal(table, O.leaf_loss_max(torch.from_numpy(tgt), torch.from_numpy(rgb), tag, N_IMG, MAX_LEAVES))
    assert n < 50 or float(table[N_IMG - 1, MAX_LEAVES - 1]) == 0.5


@pytest.mark.parametrize('n', LOSS_N)
def test_loss_of_a_single_hot_ray(fn, n):
    """rgb == rgb0 == target except one channel of one ray, off by 0.5, in one of the passes: that pass's loss is exactly
    fl(0.25 * inv_count) (zeros and one 0.25 add exactly; the product with a power of two and the atomic additions of zeros are exact
    in every regime), the other pass's is 0, one gradient entry is +-0.5 gscale, one table slot holds 0.5 (the table sees the image
    pass only).  The hot ray sits on every round, block and stride boundary that exists at n: a dropped or doubled ray shows."""
    rs = np.random.RandomState(n % 9973)
    tgt = torch.from_numpy((rs.randint(0, 1024, (n, 3)) / 1024.0).astype(F32)).cuda()
    rgb, rgb0 = tgt.clone(), tgt.clone()
    tag = tags_of(n, rs)
    tag_d = tag.int().cuda()
    want = F32(0.25) * F32(1.0 / (3.0 * n))
    gscale = F32(2.0 / (3.0 * n))
    hots = sorted({h for h in HOT + (n - 1,) if 0 <= h < n})
    assert hots
    for j, h in enumerate(hots):
        c, sign = j % 3, (-1.0 if j % 2 else 1.0)
        for hot_pass, x in enumerate((rgb, rgb0)):
            x[h, c] += sign * 0.5
            loss2, g, g0, table = run_loss(fn, rgb, rgb0, tgt, tag_d)
            assert loss2[hot_pass] == want and loss2[1 - hot_pass] == 0.0, (h, hot_pass, loss2, want)
            gh, gz = (g, g0) if hot_pass == 0 else (g0, g)
            assert int(torch.count_nonzero(gh)) == 1 and float(gh[h, c]) == float(gscale * F32(sign * 0.5)) and int(torch.count_nonzero(gz)) == 0
            hit = torch.zeros(N_IMG, MAX_LEAVES)
            if hot_pass == 0:
                hit[int(tag[h, 0]), int(tag[h, 1])] = 0.5
            assert torch.equal(table, hit), (h, hot_pass)
            x[h, c] = tgt[h, c]


@pytest.mark.parametrize('n', LOSS_N)
def test_loss_of_random_data_against_float64(fn, n, capsys):
    """Uniform inputs: each loss within k u of mse64, relative (k = train_ref.loss_chain(n)[2], the roundings on the longest path of
    one loss: all terms are non-negative), each gradient within 3u |g64| (gscale, the difference, the product).  want_grads=False
    returns no gradients and the same loss (bit for bit up to 65536 rays, where one workgroup reduces in a fixed order; within the
    atomics' g u loss beyond).  Up to 65536 rays two calls are torch.equal: the documented bit-reproducibility."""
    g_blocks, rounds, k = T.loss_chain(n)
    rs = np.random.RandomState(n % 9973 + 1)
    rgb, rgb0, tgt = (rs.rand(n, 3).astype(F32) for _ in range(3))
    tag = tags_of(n, rs)
    dev = [torch.from_numpy(x).cuda() for x in (rgb, rgb0, tgt)] + [tag.int().cuda()]
    worst_l, worst_g = 0.0, 0.0
    for grad_scale in (1.0, 0.25):
        loss2, g, g0, table = run_loss(fn, *dev, grad_scale=grad_scale)
        l1, l0, r1, r0 = T.mse64(rgb, rgb0, tgt, grad_scale)
        for got, ref in ((loss2[0], l1), (loss2[1], l0)):
            worst_l = max(worst_l, abs(float(got) - ref) / (U * ref))
        for got, ref in ((g, r1), (g0, r0)):
            e = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            worst_g = max(worst_g, float((e / (U * np.maximum(np.abs(ref), 1e-300))).max()))
            assert (e <= T.GRAD_ROUNDINGS * U * np.abs(ref)).all()
        assert torch.equal(table, O.leaf_loss_max(torch.from_numpy(tgt), torch.from_numpy(rgb), tag, N_IMG, MAX_LEAVES))
    with capsys.disabled():
        print('\nLOSS_RANDOM n=%d (g=%d, rounds=%d): worst |loss - loss64| = %.2f u loss (bound k = %d); worst |g - g64| = %.2f u |g64| (bound 3)'
              % (n, g_blocks, rounds, worst_l, k, worst_g))
    assert worst_l <= k
    lossB, gB, g0B, tableB = run_loss(fn, *dev, grad_scale=0.25)
    lossN, gN, g0N, tableN = run_loss(fn, *dev, grad_scale=0.25, want_grads=False)
    assert gN is None and g0N is None and torch.equal(tableN, table)
    if g_blocks == 1:
        assert np.array_equal(lossB, loss2) and np.array_equal(lossN, loss2) and torch.equal(gB, g) and torch.equal(g0B, g0)
    else:
        assert (np.abs(lossN.astype(np.float64) - loss2) <= g_blocks * U * loss2).all()
    one, g1, none0, _ = run_loss(fn, dev[0], None, dev[2], dev[3], grad_scale=0.25)
    assert none0 is None and one[1] == 0.0 and torch.equal(g1, g)
    assert abs(float(one[0]) - l1) <= k * U * l1


def test_direct_call_clears_the_losses_before_the_atomics(fn):
    """fastnerf_mse_leafmax called the way ops.mse_leafmax calls it, on a loss2 pre-filled with NaN, at n = 65537 (65 workgroups):
    the memset in front of the atomics is the library's.  ops.mse_leafmax hands in torch.empty, which as a rule is recycled zeros or
    an old loss -- a lost memset would show there as a loss that is off, here as a NaN.  Two orders of the same 65 block results
    are each within g u loss of their exact sum."""
    n = 65537
    g_blocks = T.loss_chain(n)[0]
    assert g_blocks == 65
    rs = np.random.RandomState(5)
    rgb, rgb0, tgt = (torch.from_numpy(rs.rand(n, 3).astype(F32)).cuda() for _ in range(3))
    L, ptr = fn._lib.lib(), fn._lib.ptr
    loss2 = torch.full((2,), float('nan'), device='cuda')
    fn._lib.check(L.fastnerf_mse_leafmax(n, ptr(rgb), ptr(rgb0), ptr(tgt), 1.0, None, None, ptr(loss2), None, 0, None, fn._lib.stream()),
                  'fastnerf_mse_leafmax')
    ref, _, _ = fn.ops.mse_leafmax(rgb, rgb0, tgt, want_grads=False)
    got, ref = loss2.cpu().numpy().astype(np.float64), ref.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and (got > 0.1).all()
    assert (np.abs(got - ref) <= g_blocks * U * ref).all(), (got, ref)
    l1, l0, _, _ = T.mse64(rgb.cpu().numpy(), rgb0.cpu().numpy(), tgt.cpu().numpy(), 1.0)
    assert abs(got[0] - l1) <= T.loss_chain(n)[2] * U * l1 and abs(got[1] - l0) <= T.loss_chain(n)[2] * U * l0


# ---- 2. Adam --------------------------------------------------------------------------------------------------------------------------
GUARD = 64
ADAM_SMALL = (1, 2, 3, 4, 5, 7, 1003, 4096, 4097, 4098, 4099)
ADAM_STRIDE = 2097152 + 7 * 1024 + 3      # 2048 workgroups x 256 threads x float4 = 2,097,152: 7168 floats in a second trip, a tail of 3


def guarded(x):
    """x as the view [64 : 64 + n] of a NaN-filled device buffer of n + 128 floats (16-byte aligned like the buffer)."""
    buf = torch.full((x.size + 2 * GUARD,), float('nan'), device='cuda')
    view = buf[GUARD:GUARD + x.size]
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 0
    return buf, view


def adam_once(fn, n, seed, lr, t):
    """One kernel step from train_ref.adam_state(n, seed) inside guard regions -> the worst ratios (p, m, v) against their bounds."""
    p, g, m, v, zero = T.adam_state(n, seed)
    bufs, views = zip(*[guarded(x) for x in (p, g, m, v)])
    fn.ops.adam_step(*views, lr, t, B1, B2, EPS)
    p1, g1, m1, v1 = (x.cpu().numpy() for x in views)
    for b in bufs:
        assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[GUARD + n:]).all()), 'nothing outside the n floats is written'
    assert np.array_equal(g1, g), 'the gradient is read only'
    p64, m64, v64, bp, bm, bv = T.adam_bounds(p, g, m, v, lr, B1, B2, EPS, t)
    r = T.adam_ratios(p1, m1, v1, p, g, m, v, lr, B1, B2, EPS, t)
    assert (np.abs(m1.astype(np.float64) - m64) <= bm).all(), ('m', n, t, lr, r)
    assert (np.abs(v1.astype(np.float64) - v64) <= bv).all(), ('v', n, t, lr, r)
    assert (np.abs(p1.astype(np.float64) - p64) <= bp).all(), ('p', n, t, lr, r)
    assert np.array_equal(p1[zero], p[zero]) and not m1[zero].any() and not v1[zero].any(), 'g = m = v = 0: nothing moves, bit for bit'
    return r


@pytest.mark.parametrize('lr', T.ADAM_LR)
@pytest.mark.parametrize('t', T.ADAM_T)
def test_adam_one_step_tails_and_small_sizes(fn, t, lr, capsys):
    """|m' - m64| <= 3u (|b1 m| + |(1 - b1) g|), |v' - v64| <= 4u v64, |p' - p64| <= u |p64| + 12u A (train_ref's derivation) at every
    size around the float4 body: no body at all (n < 4), body and tails of 0..3."""
    worst = np.zeros(3)
    for n in ADAM_SMALL:
        worst = np.maximum(worst, adam_once(fn, n, 100 + n, lr, t))
    with capsys.disabled():
        print('\nADAM_SMALL t=%d lr=%g: worst ratios p %.2f (bound %d)  m %.2f (%d)  v %.2f (%d)' % (
            t, lr, worst[0], T.P_ROUNDINGS, worst[1], T.M_ROUNDINGS, worst[2], T.V_ROUNDINGS))


@pytest.mark.parametrize('t,lr', [(1, 5e-4), (2, 5e-5), (3, 5e-4), (10, 5e-5), (1000, 5e-4), (200000, 5e-5), (200000, 5e-4), (1, 5e-5)])
def test_adam_one_step_grid_stride(fn, t, lr, capsys):
    """n = 2,097,152 + 7 * 1024 + 3: the first 1792 threads take a second float4, the tail is 3 floats behind it."""
    r = adam_once(fn, ADAM_STRIDE, 7 + t, lr, t)
    with capsys.disabled():
        print('\nADAM_STRIDE t=%d lr=%g: worst ratios p %.2f (bound %d)  m %.2f (%d)  v %.2f (%d)' % (
            t, lr, r[0], T.P_ROUNDINGS, r[1], T.M_ROUNDINGS, r[2], T.V_ROUNDINGS))


def test_adam_on_the_trainers_slice(fn):
    """The Trainer updates one network as flat[N:2N], N = ops.NET_PARAMS: the slice starts at a multiple of four floats (16-byte
    aligned, what the float4 reads need) and the first N floats are not touched.  Without view directions a single-pass network has
    a multiple of four parameters too; the two-pass count (output_ch = 5) is odd, 527,237 -- that Trainer is not on the fused step
    and updates its [coarse | fine] buffer whole, from its aligned start (Trainer._host_update), never a network's slice."""
    N = fn.ops.NET_PARAMS
    assert N % 4 == 0 and fn.ops.net_floats(1) % 4 == 0 and fn.ops.net_floats(2) % 4 == 0
    assert fn.model.noview_slices(4)[1] % 4 == 0 and fn.model.noview_slices(5)[1] == 527237
    p, g, m, v, _ = T.adam_state(2 * N, 11)
    dev = [torch.from_numpy(x).cuda() for x in (p, g, m, v)]
    assert all(x[N:].data_ptr() % 16 == 0 for x in dev)
    fn.ops.adam_step(*[x[N:2 * N] for x in dev], 5e-4, 3, B1, B2, EPS)
    for x, x0 in zip(dev, (p, g, m, v)):
        assert np.array_equal(x[:N].cpu().numpy(), x0[:N])
    p64, m64, v64, bp, bm, bv = T.adam_bounds(p[N:], g[N:], m[N:], v[N:], 5e-4, B1, B2, EPS, 3)
    assert (np.abs(dev[0][N:].cpu().numpy().astype(np.float64) - p64) <= bp).all()
    assert (np.abs(dev[2][N:].cpu().numpy().astype(np.float64) - m64) <= bm).all()
    assert (np.abs(dev[3][N:].cpu().numpy().astype(np.float64) - v64) <= bv).all()


def test_adam_two_pass_trainer_without_view_directions_updates_its_buffer_whole(fn, golden_dir):
    """The odd parameter count above, on the product route: one Trainer.step of two networks without view directions (the G19 nets
    and batch, where both passes have a gradient) goes through fastnerf_adam_step and its alignment check over the whole buffer and
    moves both networks."""
    import os
    from conftest import noview_state_dicts
    g19 = np.load(os.path.join(golden_dir, 'g19_noview.npz'))
    args = fn.run_nerf.make_args(N_importance=32, N_samples=32, perturb=1.0, white_bkgd=True, no_reload=True, use_viewdirs=False)
    ktr = fn.run_nerf.create_nerf(args, device='cuda')[0]
    for key, sd in zip(('network_fn', 'network_fine'), noview_state_dicts(golden_dir)):
        ktr[key].load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    tr = fn.run_nerf.Trainer(ktr, 800, 800, g19['K'], 2.0, 6.0)
    N = fn.model.noview_slices(5)[1]
    assert not tr.fused and tr.flat.numel() == 2 * N and tr.flat.data_ptr() % 16 == 0 and tr.flat[N:].data_ptr() % 16 != 0
    before = tr.flat.clone()
    tr.step(torch.from_numpy(g19['ro']).cuda(), torch.from_numpy(g19['rd']).cuda(), torch.from_numpy(g19['target']).cuda())
    moved = tr.flat != before
    assert bool(moved[:N].any()) and bool(moved[N:].any()) and bool(torch.isfinite(tr.flat).all())


def test_adam_sequence_of_steps(fn, capsys):
    """20 consecutive steps with fresh gradients from m = v = 0, lr on O.lr_schedule (decaying tenfold over the 20 steps): every step
    is held to adam_step64 of the kernel's OWN previous state, so the bounds do not loosen along the trajectory."""
    n = 4099
    rs = np.random.RandomState(3)
    scale = (10.0 ** rs.uniform(-6.0, 0.0, n))
    p = torch.from_numpy(rs.randn(n).astype(F32)).cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    worst = np.zeros(3)
    for it in range(20):
        lr = O.lr_schedule(5e-4, 0.02, it)
        g = (rs.randn(n) * scale).astype(F32)
        prev = [x.cpu().numpy() for x in (p, m, v)]
        fn.ops.adam_step(p, torch.from_numpy(g).cuda(), m, v, lr, it + 1, B1, B2, EPS)
        got = [x.cpu().numpy() for x in (p, m, v)]
        p64, m64, v64, bp, bm, bv = T.adam_bounds(prev[0], g, prev[1], prev[2], lr, B1, B2, EPS, it + 1)
        assert (np.abs(got[0].astype(np.float64) - p64) <= bp).all(), it
        assert (np.abs(got[1].astype(np.float64) - m64) <= bm).all(), it
        assert (np.abs(got[2].astype(np.float64) - v64) <= bv).all(), it
        worst = np.maximum(worst, T.adam_ratios(got[0], got[1], got[2], prev[0], g, prev[1], prev[2], lr, B1, B2, EPS, it + 1))
    assert abs(O.lr_schedule(5e-4, 0.02, 20) - 5e-5) < 1e-12
    with capsys.disabled():
        print('\nADAM_SEQUENCE 20 steps: worst ratios p %.2f (bound %d)  m %.2f (%d)  v %.2f (%d)' % (
            worst[0], T.P_ROUNDINGS, worst[1], T.M_ROUNDINGS, worst[2], T.V_ROUNDINGS))


# ---- 3. the alignment check -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', [0, 1, 2, 3], ids=['params', 'grads', 'm', 'v'])
def test_adam_refuses_a_misaligned_array(fn, which):
    """adam_kernel reads the four arrays as float4: fastnerf_adam_step returns an error for one that is not 16-byte aligned (flat[1:])
    and launches nothing -- every array keeps its bits."""
    n = 1003
    p, g, m, v, _ = T.adam_state(n + 1, 5)
    full = [torch.from_numpy(x).cuda() for x in (p, g, m, v)]
    args = [x[1:] if k == which else x[:n] for k, x in enumerate(full)]
    assert args[which].data_ptr() % 16 == 4
    keep = [x.clone() for x in full]
    L, ptr = fn._lib.lib(), fn._lib.ptr
    rc = L.fastnerf_adam_step(n, ptr(args[0]), ptr(args[1]), ptr(args[2]), ptr(args[3]), 5e-4, B1, B2, EPS, 1, fn._lib.stream())
    assert rc < 0 and b'16-byte aligned' in L.fastnerf_last_error()
    with pytest.raises(RuntimeError, match='16-byte aligned'):
        fn.ops.adam_step(*args, 5e-4, 1, B1, B2, EPS)
    torch.cuda.synchronize()
    for x, k in zip(full, keep):
        assert torch.equal(x, k)
    fn.ops.adam_step(*[x[:n] for x in full], 5e-4, 1, B1, B2, EPS)      # the aligned call goes through
    assert not torch.equal(full[0], keep[0])


# ---- 4. leaf_sumcount past its grid cap ----------------------------------------------------------------------------------------------
def test_leaf_sumcount_past_the_grid_cap(fn):
    """600,001 rays over 2048 x 256 = 524,288 threads: 75,713 threads take a second ray.  A ray's term is a multiple of 2^-30, the
    fp64 atomics are exact: sums and counts equal the oracle's bit for bit and do not depend on the order of the rays."""
    n, ni, ml = 600001, 5, 16
    gen = torch.Generator().manual_seed(3)
    pred, gt = torch.rand(n, 3, generator=gen), torch.rand(n, 3, generator=gen)
    tag = torch.stack([torch.randint(0, ni, (n,), generator=gen), torch.randint(0, ml, (n,), generator=gen)], 1).int()
    tag[n - 1] = torch.tensor([ni - 1, ml - 1])

    def tables(idx):
        s = torch.zeros(ni * ml, device='cuda', dtype=torch.float64)
        c = torch.zeros(ni * ml, device='cuda', dtype=torch.int32)
        fn.ops.leaf_sumcount(pred[idx].cuda(), gt[idx].cuda(), tag[idx].cuda().contiguous(), ml, s, c)
        return s, c
    s0, c0 = tables(torch.arange(n))
    so, co = O.leaf_loss_sumcount(gt, pred, tag.long(), ni, ml)
    assert int(c0.sum()) == n and torch.equal(c0.cpu(), co) and torch.equal(s0.cpu(), so)
    s1, c1 = tables(torch.randperm(n, generator=gen))
    assert torch.equal(s0, s1) and torch.equal(c0, c1)


# ---- 5. sigma noise past its grid cap ------------------------------------------------------------------------------------------------
def test_sigma_noise_past_the_grid_cap(fn, capsys):
    """4,194,304 + 1203 values: 4096 x 256 threads x 4 values is the whole grid, the first 301 threads take a second float4 and the
    last of them writes 3 of its 4 values.  The bar and its argument are those of
    test_gpu_seeded_draws.py::test_sigma_noise_is_box_muller_on_the_nois_stream: within 1e-5 * std of the float64 Box-Muller of the
    same Philox words (three times the few-ulp error of logf / sqrtf / sincosf on r <= 5.9, five orders below a wrong word, counter
    or pairing).  Compared: the last 4096 values (the second trip and the partial float4) and every 1021st one; the host reference is
    evaluated on those counters only."""
    S0, S1, seed = 4194304, 1203, (1 << 40) + 12345
    total = S0 + S1
    pick = np.unique(np.concatenate([np.arange(0, total, 1021), np.arange(total - 4096, total)]))
    worst = 0.0
    for std in (1.0, 0.25):
        n0, n1 = fn.ops.sigma_noise(1, S0, S1, std, seed, 'cuda')
        assert n0.shape == (1, S0) and n1.shape == (1, S1)
        got = torch.cat([n0.reshape(-1), n1.reshape(-1)])
        assert bool(torch.isfinite(got).all())
        got = got[torch.from_numpy(pick).cuda()].cpu().numpy().astype(np.float64)
        ref = P.box_muller(P.stream_words(P.NOIS, (pick // 4).astype(np.uint64), seed), std)[np.arange(pick.size), pick % 4]
        worst = max(worst, float(np.abs(got - ref).max()) / std)
    with capsys.disabled():
        print('\nSIGMA_NOISE %d values: max |device - float64 Box-Muller| = %.3g * std over %d picked values' % (total, worst, pick.size))
    assert worst <= 1e-5
