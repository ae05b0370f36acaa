"""cp_scan_kernel (csrc/train.hip) beyond its first round.  The exclusive scan of the per-block counts is ONE 1024-thread workgroup
that walks the block counts 1024 at a time and carries the running total in LDS; a block holds 1024 entries, so the second round
begins past 1,048,576 entries -- where a default render chunk through an occupancy grid (32768 rays x 64..256 samples), an ERT
segment of 32768 rays x 32 samples and a 4096 x 256 training batch all are.  Every user of the scan is taken there: compact_live,
the classify of a grid and of a cascade, ert_classify, march_list, and render() through a grid in one chunk against many.  All
comparisons are exact (lists of indices, counts, bit patterns)."""
import numpy as np
import pytest
import torch

import ert_numpy as E
import march_numpy as M
import occ_cascade_numpy as RC
import occ_numpy as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

ROUND = 1024 * 1024      # entries per round of the scan: 1024 block counts of 1024 entries
# P, blocks: one full round; a second round of one block with one entry; two full rounds; a third round of two blocks
SCAN_P = [(ROUND, 1024), (ROUND + 1, 1025), (2 * ROUND, 2048), (2 * ROUND + 1025, 2050)]


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


def same_bits(a, b):
    """torch.equal on the bit patterns (disp_map is 0 / 0 = NaN on a ray without any weight)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- compact_live -----------------------------------------------------------------------------------------------------------------
def draw_of(P, pattern):
    if pattern == 'random':      # 45 % live, negative zeros, points kept alive by a single tiny component (test_gpu_compact.py)
        gen = torch.Generator().manual_seed(P % 100003)
        draw = torch.randn(P, 4, generator=gen)
        dead = torch.rand(P, generator=gen) >= 0.45
        draw[dead] = 0.0
        draw[dead & (torch.rand(P, generator=gen) < 0.3)] = -0.0
        one = (~dead) & (torch.rand(P, generator=gen) < 0.2)
        draw[one] = 0.0
        draw[one, 3] = 1e-30
        return draw.cuda()
    if pattern == 'all live':      # the carry grows by 1,048,576 per round
        return torch.ones(P, 4, device='cuda')
    draw = torch.zeros(P, 4, device='cuda')
    at = {'all dead': None, 'last': P - 1, 'first of round 2': ROUND, 'last of round 1': ROUND - 1}[pattern]
    if at is not None and at < P:
        draw[at, 2] = -1.0
    return draw


@pytest.mark.parametrize('pattern', ['random', 'all live', 'all dead', 'last', 'first of round 2', 'last of round 1'])
@pytest.mark.parametrize('P,nb', SCAN_P)
def test_compact_live_past_one_round(fn, P, nb, pattern):
    assert int(fn._lib.lib().fastnerf_compact_ws_ints(P)) == nb
    draw = draw_of(P, pattern)
    idx, cnt = fn.ops.compact_live(draw)
    want = torch.nonzero((draw != 0).any(1)).reshape(-1).int()
    c = cnt.cpu().tolist()
    assert c == [want.numel(), P], (c, want.numel())
    assert torch.equal(idx[:c[0]], want)
    if pattern == 'first of round 2':
        assert c[0] == (1 if P > ROUND else 0)
    if pattern in ('last', 'last of round 1'):
        assert c[0] == 1


# ---- classify of a grid and of a cascade --------------------------------------------------------------------------------------------
def rays_and_depths(n, S, seed):
    side = int(np.ceil(np.sqrt(n)))
    rays = R.scene_rays(O, side=side, focal=14.0 * side / 8)[:n]
    assert rays.shape[0] == n
    z = np.sort(2.0 + 4.0 * np.random.RandomState(seed).rand(n, S).astype(np.float32), -1)
    return rays, z


@pytest.fixture(scope='module')
def classify_inputs():
    """(rays, z, rays on the device, z on the device) of the two sizes, made once: 5462 x 192 = 1,048,704 samples (1025 blocks) and
    16384 x 192 = 3,145,728 (3072 blocks: three full rounds)."""
    out = {}
    for n in (5462, 16384):
        rays, z = rays_and_depths(n, 192, n)
        out[n] = (rays, z, torch.from_numpy(rays).cuda(), torch.from_numpy(z).cuda())
    return out


def check_classify(obj, bits, rays_t, z_t, name):
    n, S = z_t.shape
    raw = torch.full((n, S, 4), 7.0, device='cuda')
    idx, cnt = obj.classify(rays_t, z_t, raw)
    live = torch.from_numpy(np.nonzero(bits.reshape(-1))[0].astype(np.int32)).cuda()
    assert cnt.tolist() == [live.numel(), bits.size], name
    assert torch.equal(idx[:live.numel()], live), name
    bits_t = torch.from_numpy(bits).cuda()
    assert torch.equal((raw == 0).all(-1), ~bits_t), 'the masked rows are zeroed: ' + name
    assert bool((raw[bits_t] == 7.0).all()), 'nothing else is written: ' + name
    return live.numel()


@pytest.mark.parametrize('grid', ['ball', 'outside only'])
@pytest.mark.parametrize('n', [5462, 16384])
def test_grid_classify_past_one_round(fn, classify_inputs, n, grid):
    rays, z, rays_t, z_t = classify_inputs[n]
    m, lo, hi, oo = R.scene_grids()['ball'] if grid == 'ball' else (np.zeros((4, 4, 4), bool), np.float32(-0.5), np.float32(0.5), True)
    g = fn.occupancy.OccupancyGrid.from_mask(torch.from_numpy(m).cuda(), lo, hi, oo)
    live = check_classify(g, R.classify(m, lo, hi, oo, rays, z), rays_t, z_t, grid)
    assert 0 < live < n * 192


@pytest.mark.parametrize('cascade', ['scene', 'outside only'])
@pytest.mark.parametrize('n', [5462, 16384])
def test_cascade_classify_past_one_round(fn, classify_inputs, n, cascade):
    rays, z, rays_t, z_t = classify_inputs[n]
    if cascade == 'scene':
        levels, oo = RC.scene_cascade()
    else:
        levels, oo = [(np.zeros((4, 4, 4), bool), np.float32(-0.5), np.float32(0.5)), (np.zeros((2, 2, 2), bool), np.float32(-0.7), np.float32(0.7))], True
    G = fn.occupancy
    c = G.OccupancyCascade([G.OccupancyGrid.from_mask(torch.from_numpy(m).cuda(), lo, hi, not oo) for m, lo, hi in levels], outside_occupied=oo)
    live = check_classify(c, RC.classify(levels, oo, rays, z), rays_t, z_t, cascade)
    assert 0 < live < n * 192


# ---- one segment of more than 1,048,576 entries: ert_classify and march_list ----------------------------------------------------------
def test_ert_classify_past_one_round(fn):
    """16385 rays x a 64-sample segment = 1,048,640 entries (1025 blocks), through the ball grid, a third of the rays passing."""
    n, S, s0, s1 = 16385, 96, 32, 96
    rays, z = rays_and_depths(n, S, 1)
    rs = np.random.RandomState(2)
    eps = np.float32(1e-2)
    trans = (rs.rand(n) * 0.03).astype(np.float32)
    trans[:6] = [eps, np.nextafter(eps, np.float32(1)), np.nextafter(eps, np.float32(0)), 0.0, 1.0, np.nan]
    trans = trans[rs.permutation(n)]
    m, lo, hi, oo = R.scene_grids()['ball']
    g = fn.occupancy.OccupancyGrid.from_mask(torch.from_numpy(m).cuda(), lo, hi, oo)
    keep = E.classify(trans, eps, S, s0, s1, R.classify(m, lo, hi, oo, rays, z))
    live = torch.from_numpy(E.live_list(keep, S, s0).astype(np.int32)).cuda()
    raw = torch.full((n, S, 4), 7.0, device='cuda')
    idx, cnt = fn.ops.ert_classify(torch.from_numpy(rays).cuda(), torch.from_numpy(z).cuda(), s0, s1, torch.from_numpy(trans).cuda(),
                                   float(eps), g._c, raw)
    assert n * (s1 - s0) > ROUND and cnt.tolist() == [live.numel(), n * (s1 - s0)] and 0 < live.numel() < n * (s1 - s0)
    assert torch.equal(idx[:live.numel()], live)
    want = torch.zeros(n, S, dtype=torch.bool, device='cuda')
    want[:, s0:s1] = ~torch.from_numpy(keep).cuda()
    assert torch.equal((raw == 0).all(-1), want) and bool((raw[~want] == 7.0).all())


def test_march_list_past_one_round(fn):
    """Packed rows of 16385 rays x 96 slots with live runs of random length (a live slot holds its lattice index, the others -1):
    the segment [32, 96) is 1,048,640 entries."""
    n, C, s0, s1 = 16385, 96, 32, 96
    rs = np.random.RandomState(4)
    used = rs.randint(0, C + 1, n)
    used[:3] = (0, C, s0)
    kidx = np.where(np.arange(C)[None, :] < used[:, None], np.cumsum(rs.randint(1, 4, (n, C)), 1), -1).astype(np.int32)
    raw = torch.full((n, C, 4), 7.0, device='cuda')
    idx, cnt = fn.ops.march_list(torch.from_numpy(kidx).cuda(), s0, s1, raw)
    live = torch.from_numpy(M.live_list(kidx, s0, s1).astype(np.int32)).cuda()
    assert n * (s1 - s0) > ROUND and cnt.tolist() == [live.numel(), n * (s1 - s0)] and 0 < live.numel() < n * (s1 - s0)
    assert torch.equal(idx[:live.numel()], live)
    want = torch.zeros(n, C, dtype=torch.bool, device='cuda')
    want[:, s0:s1] = torch.from_numpy(kidx[:, s0:s1] < 0).cuda()
    assert torch.equal((raw == 0).all(-1), want) and bool((raw[~want] == 7.0).all())


# ---- render() through the grid: one chunk of several rounds against chunks of one -------------------------------------------------------
NS, NI = 64, 128


def networks(fn, opaque):
    """create_nerf's render kwargs with the random-init parameters of the occupancy tests (occ_numpy.scene_networks), or the opaque
    ones of the ERT and march tests (ert_numpy.scene_networks: rays do saturate), loaded into both networks."""
    kw = dict(N_importance=NI, N_samples=NS, perturb=0., white_bkgd=False, use_viewdirs=True, no_reload=True)
    _, kte, _, _, _, _ = fn.run_nerf.create_nerf(fn.run_nerf.make_args(**kw))
    sdc, sdf = (E if opaque else R).scene_networks(O)
    kte['network_fn'].load_state_dict(sdc)
    kte['network_fine'].load_state_dict(sdf)
    return kte


# H = W = 96: 9216 rays.  One chunk: the fine pass classifies 9216 x 192 samples = 1728 blocks, an ERT segment of 128 samples is 1152
# blocks, the marched rows of 128 slots are 1152 blocks; chunks of 1024 rays stay within one round everywhere.
@pytest.mark.parametrize('mode,extra', [('grid', {}), ('ert', dict(ert=1e-2, ert_block=128)), ('march', dict(march=256, march_cap=128)),
                                        ('march+ert', dict(march=256, march_cap=128, ert=1e-2, ert_block=16))])
@pytest.mark.parametrize('opaque', [False, True], ids=['scene nets', 'opaque nets'])
def test_render_in_one_chunk_is_the_render_in_many(fn, opaque, mode, extra):
    kte = networks(fn, opaque)
    m, lo, hi, oo = R.scene_grids()['ball']
    g = fn.occupancy.OccupancyGrid.from_mask(torch.from_numpy(m).cuda(), lo, hi, oo)
    H = W = 96
    K = np.array([[14.0 * H / 8, 0, 0.5 * W], [0, 14.0 * H / 8, 0.5 * H], [0, 0, 1]])
    c2w = fn.synthetic.pose_spherical(30.0, -30.0, 4.0)[:3, :4].cuda()
    kw = dict(kte, near=2.0, far=6.0, occupancy=g, **extra)
    kw.pop('ndc', None)
    with torch.no_grad():
        whole = fn.render.render(H, W, K, chunk=H * W, c2w=c2w, ndc=False, **kw)
        parts = fn.render.render(H, W, K, chunk=1024, c2w=c2w, ndc=False, **kw)
    for name, a, b in zip(('rgb', 'disp', 'acc'), whole[:3], parts[:3]):
        assert a.shape[:2] == (H, W) and same_bits(a, b), (mode, name)
    acc = whole[2]
    assert float(acc.max()) > 0 and float(acc.min()) == 0, 'rays through the ball, and rays that miss it'
    if opaque:
        assert float(acc.max()) > 0.99, 'rays saturate: early termination has something to stop'
