"""The seeded random draws that training runs (perturb=1: every sampler keyed by render._next_seed(), no injected numbers) against the
host restatement of Philox4x32-10 and of the stream table in tests/philox_numpy.py (itself pinned to Random123's known answers by
tests/test_philox_cpu.py).  The seeded and the injected branch of every sampler share all arithmetic after the uniform number is
obtained, and the injected branch is tied to the oracle by the parity tests, so `op(seed=s) == op(u = host stream of s)` bit for
bit carries that parity over to the configuration that trains.  Exact comparisons throughout; the one tolerance is the Gaussian's
(its derivation is at test_sigma_noise_is_box_muller_on_the_nois_stream)."""
import os

import numpy as np
import pytest
import torch

import occ_numpy as R
import philox_numpy as P

pytestmark = pytest.mark.gpu

F32 = np.float32
SEEDS = [1, 2 ** 32, 2 ** 62 - 1]          # (2^32: the low key word is zero)


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_u(stream, shape, seed):
    return dev(P.stream_u(stream, shape, seed))


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def rays_for(fn, n, gen):
    """n rays with per-ray near / far (so that a jitter row applied to the wrong ray shows)."""
    r = fn.ops.pack_rays(torch.randn(n, 3, generator=gen).cuda(), torch.randn(n, 3, generator=gen).cuda(), 2.0, 6.0)
    r[:, 6] = dev(2.0 + torch.rand(n, generator=gen).numpy())
    r[:, 7] = dev(5.0 + torch.rand(n, generator=gen).numpy())
    return r


# ---- a. seeded == injected, per kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('n,S', [(1, 1), (5, 3), (300, 65), (8200, 64)])      # 8200 x 64: one past the 2048 x 256 grid (grid-stride loop)
def test_sample_coarse_seeded_equals_injected(fn, n, S, seed):
    rays = rays_for(fn, n, torch.Generator().manual_seed(n + S))
    t = host_u(P.COAR, (n, S), seed)
    for lindisp in (False, True):
        got = fn.ops.sample_coarse(rays, S, lindisp=lindisp, perturb=True, seed=seed)
        assert same(got, fn.ops.sample_coarse(rays, S, lindisp=lindisp, t_rand=t)), (n, S, lindisp)
        if S > 2:
            assert not same(got, fn.ops.sample_coarse(rays, S, lindisp=lindisp)), 'the jitter moved nothing'


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('n,S', [(7, 2), (300, 65)])
def test_pp_fg_depths_seeded_equals_injected(fn, n, S, seed):
    gen = torch.Generator().manual_seed(n + S)
    fg_far = (0.5 + torch.rand(n, generator=gen)).cuda()
    got = fn.ops.pp_fg_depths(fg_far, S, perturb=True, seed=seed)
    assert same(got, fn.ops.pp_fg_depths(fg_far, S, t_rand=host_u(P.FGDP, (n, S), seed)))
    if S > 2:
        assert not same(got, fn.ops.pp_fg_depths(fg_far, S, perturb=False))


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('n,S', [(1, 1), (300, 65)])
def test_pp_perturb_samples_seeded_equals_injected(fn, n, S, seed):
    gen = torch.Generator().manual_seed(n + S)
    z = torch.sort(torch.rand(n, S, generator=gen), -1).values.cuda()
    got = fn.ops.pp_perturb_samples(z, seed=seed)
    assert same(got, fn.ops.pp_perturb_samples(z, t_rand=host_u(P.PRTB, (n, S), seed)))
    if S > 2:
        assert not same(got, z)


def pdf_inputs(n, S, gen):
    """Sorted depths and non-degenerate weights (rand^4: a few dominant bins, like test_sample_pdf_merge_vs_oracle)."""
    z = torch.sort(torch.rand(n, S, generator=gen) * 4 + 2, -1).values
    return z.cuda(), (torch.rand(n, S, generator=gen) ** 4).cuda()


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('n,S,Ni', [(3, 3, 1), (50, 64, 128), (50, 100, 130), (4, 512, 1024), (16400, 8, 5)])
def test_sample_pdf_merge_seeded_equals_injected(fn, n, S, Ni, seed):
    """(50, 100, 130): NP = 256 differs from Ni; (4, 512, 1024): the LDS maximum; (16400, 8, 5): past the 4096 x 4 wave cap."""
    z, w = pdf_inputs(n, S, torch.Generator().manual_seed(S + Ni))
    u = host_u(P.PDFS, (n, Ni), seed)
    got = fn.ops.sample_pdf_merge(z, w, Ni, det=False, seed=seed)
    want = fn.ops.sample_pdf_merge(z, w, Ni, u=u)
    for name, a, b in zip(('z_out', 'z_samples', 'z_std'), got, want):
        assert same(a, b), (name, n, S, Ni)
    gpp = fn.ops.pp_sample_pdf_merge(z, w, Ni, det=False, seed=seed)
    wpp = fn.ops.pp_sample_pdf_merge(z, w, Ni, u=u)
    for name, a, b in zip(('z_out', 'z_samples'), gpp, wpp):
        assert same(a, b), ('pp', name, n, S, Ni)
    if Ni > 1:
        assert not same(got[1], fn.ops.sample_pdf_merge(z, w, Ni, det=True)[1]), 'the seeded branch took the deterministic positions'


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('n,M,Ni', [(50, 63, 128), (3, 2, 1)])
def test_sample_pdf_bins_mode_seeded_equals_injected(fn, n, M, Ni, seed):
    gen = torch.Generator().manual_seed(M + Ni)
    bins = torch.sort(torch.rand(n, M, generator=gen) * 4 + 2, -1).values.cuda()
    w = (torch.rand(n, M - 1, generator=gen) ** 4).cuda()
    u = host_u(P.PDFS, (n, Ni), seed)
    assert same(fn.ops.sample_pdf(bins, w, Ni, det=False, seed=seed), fn.ops.sample_pdf(bins, w, Ni, u=u))
    assert same(fn.ops.pp_sample_pdf(bins, w, Ni, det=False, seed=seed), fn.ops.pp_sample_pdf(bins, w, Ni, u=u))


# ---- b. the streams do not collide ----------------------------------------------------------------------------------------
def test_streams_do_not_collide(fn):
    n = S = 64
    seed = SEEDS[2]
    us = {name: P.stream_u(st, (n, S), seed) for name, st in (('coar', P.COAR), ('fgdp', P.FGDP), ('prtb', P.PRTB), ('pdfs', P.PDFS))}
    us['nois'] = np.stack(P.stream_words(P.NOIS, np.arange(n * S // 4, dtype=np.uint64), seed), 1).reshape(n, S)
    us['nois'] = P.u01(us['nois'])          # the first 4096 uniform words behind the Gaussian
    names = sorted(us)
    for i, a in enumerate(names):
        assert len({us[a][r].tobytes() for r in range(n)}) == n, (a, 'two rays share a row of draws')
        for b in names[i + 1:]:
            assert not np.array_equal(us[a], us[b]), (a, b)
            assert float((us[a] == us[b]).mean()) < 0.01, (a, b)
    # the device's side of it: on identical rays the jitter alone tells the rows apart, and every consumer has its own numbers
    rays = fn.ops.pack_rays(torch.zeros(n, 3).cuda(), torch.ones(n, 3).cuda(), 2.0, 6.0)
    zc = fn.ops.sample_coarse(rays, S, perturb=True, seed=seed)
    assert torch.unique(zc, dim=0).shape[0] == n
    lin = torch.linspace(0.1, 0.9, S).expand(n, S).contiguous().cuda()
    zp = fn.ops.pp_perturb_samples(lin, seed=seed)
    zf = fn.ops.pp_fg_depths(torch.ones(n).cuda(), S, perturb=True, seed=seed)
    assert torch.unique(zp, dim=0).shape[0] == n and torch.unique(zf, dim=0).shape[0] == n
    for name, z, st in (('coar', zc, P.COAR), ('prtb', zp, P.PRTB), ('fgdp', zf, P.FGDP)):
        for other in (P.COAR, P.PRTB, P.FGDP, P.PDFS):
            t = host_u(other, (n, S), seed)
            inj = {'coar': lambda: fn.ops.sample_coarse(rays, S, t_rand=t), 'prtb': lambda: fn.ops.pp_perturb_samples(lin, t_rand=t),
                   'fgdp': lambda: fn.ops.pp_fg_depths(torch.ones(n).cuda(), S, t_rand=t)}[name]()
            assert same(z, inj) == (other == st), (name, hex(other))


# ---- c. sigma noise ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('n,S0,S1', [(3, 5, 7), (64, 64, 192), (4, 8, 0)])
def test_sigma_noise_is_box_muller_on_the_nois_stream(fn, n, S0, S1, seed, capsys):
    """Element e of the flat buffer (coarse view, padding to a multiple of 4, fine view) is slot e % 4 of block e // 4.
    Tolerance 1e-5 * std: u2 is exact in fp32 and ln(u1) is taken of the exact u1 (its 25 bits do not fit fp32 above 1/2: the kernel's
    log_u1 goes through 1 - u1 there; rounding u1 itself cost 1.4e-5 * std at (64, 64, 192), seed 2^62 - 1); r <= sqrt(-2 ln 2^-25) = 5.9; logf, sqrtf and sincosf are good to a few ulp
    (1.2e-7 relative) on an angle below 2 pi, so the device is within about 3e-6 * std of the float64 value.  1e-5 is three times
    that, and five orders below the O(std) error of a wrong word, counter or pairing."""
    worst = 0.0
    for std in (1.0, 0.25):
        n0, n1 = fn.ops.sigma_noise(n, S0, S1, std, seed, 'cuda')
        tot0 = (n * S0 + 3) // 4 * 4
        ref = P.gauss_noise(tot0 + n * S1, std, seed)
        assert n0.shape == (n, S0) and (n1 is None if S1 == 0 else n1.shape == (n, S1))
        err = np.abs(n0.cpu().numpy().astype(np.float64).reshape(-1) - ref[:n * S0]).max()
        if S1 > 0:
            err = max(err, np.abs(n1.cpu().numpy().astype(np.float64).reshape(-1) - ref[tot0:]).max())
        worst = max(worst, err / std)
    with capsys.disabled():
        print('\nSIGMA_NOISE n=%d S0=%d S1=%d seed=%d: max |device - float64 Box-Muller| = %.3g * std' % (n, S0, S1, seed, worst))
    assert worst <= 1e-5


# ---- d. epoch rows ----------------------------------------------------------------------------------------------------------
def refined_manager(fn, sharp=None):
    """3 views of 64 x 48, depth 2, two adjust rounds with a random error table: leaves of two sizes
    (the fixture of tests/test_gpu_epoch_rays.py)."""
    n, H, W = 3, 64, 48
    gen = torch.Generator().manual_seed(0)
    imgs = torch.rand(n, H, W, 3, generator=gen)
    poses = torch.stack([fn.synthetic.pose_spherical(40.0 * i, -30.0, 4.0)[:3, :4] for i in range(n)], 0)
    K = np.array([[50.0, 0, W / 2], [0, 50.0, H / 2], [0, 0, 1]])
    mgr = fn.tree.QuadTreeManager(H, W, K, imgs, poses, 0.0, 2, sharp_imgs=sharp)
    gen = torch.Generator().manual_seed(5)
    for _ in range(2):
        mgr.adjust_tree_from_table(torch.rand(mgr.n_images, mgr.max_leaves(), generator=gen), thres=0.5)
    return mgr


def plan_of(mgr):
    plan, N = mgr.epoch_plan(down_scale=1)
    offs = np.zeros(plan.shape[0] + 1, dtype=np.int64)
    np.cumsum(plan[:, 2], out=offs[1:])
    assert N == offs[-1] and N > 1000 and len(set(plan[:, 2].tolist())) > 1      # several blocks of rows, leaves of two sizes
    return plan, offs, N


def check_rows(mgr, plan, want, rows=None):
    src, leaf_row, pix = want
    sel = slice(None) if rows is None else rows
    assert np.array_equal(mgr.result_pix.cpu().numpy().astype(np.int64), pix[sel])
    assert np.array_equal(mgr.result_leaf_tag.cpu().numpy().astype(np.int64), plan[leaf_row[sel], 0:2].astype(np.int64))


@pytest.mark.parametrize('seed', SEEDS)
def test_epoch_rows_uniform_picks(fn, seed):
    from fastnerf import parallel
    mgr = refined_manager(fn)
    plan, offs, N = plan_of(mgr)
    for shuffle in (True, False):
        mgr.gen_rays_device(down_scale=1, seed=seed, shuffle=shuffle, want_pix=True)
        want = P.epoch_rows(plan, offs, N, seed, shuffle, 64, 48)
        assert np.array_equal(np.sort(want[0]), np.arange(N))
        check_rows(mgr, plan, want)
    want = P.epoch_rows(plan, offs, N, seed, True, 64, 48)
    mgr.gen_rays_device(down_scale=1, seed=seed, want_pix=True, shard=(3, 8, 5))
    check_rows(mgr, plan, want, parallel.shard_global_rows(N, 5, 3, 8))


@pytest.mark.parametrize('seed', SEEDS)
def test_epoch_rows_weighted_picks(fn, seed):
    from fastnerf import parallel
    rng = np.random.RandomState(2)
    sharp = [np.abs(rng.randn(64, 48)) ** 2 * 0.05 for _ in range(3)]          # variance maps as an input fixture
    mgr = refined_manager(fn, sharp)
    plan, offs, N = plan_of(mgr)
    tabs = {k: v.cpu().numpy() for k, v in mgr._weighted_tables(False).items()}
    nw = np.floor(plan[:, 2].astype(np.float64) * (1.0 - 0.5)).astype(np.int64)
    nw[tabs['npix'] == 0] = 0
    assert 0 < nw.sum() < N
    wt = dict(n_weighted=nw, seg_beg=tabs['seg_beg'], seg_end=tabs['seg_end'], order=tabs['order'], cum=tabs['cum'])
    for shuffle in (True, False):
        mgr.gen_rays_device(down_scale=1, prob=True, rand=0.5, seed=seed, shuffle=shuffle, want_pix=True)
        want = P.epoch_rows(plan, offs, N, seed, shuffle, 64, 48, weighted=wt)
        uni = P.epoch_rows(plan, offs, N, seed, shuffle, 64, 48)
        assert float((want[2] != uni[2]).any(1).mean()) > 0.3          # (the weighted picks are a different set of pixels)
        check_rows(mgr, plan, want)
    want = P.epoch_rows(plan, offs, N, seed, True, 64, 48, weighted=wt)
    mgr.gen_rays_device(down_scale=1, prob=True, rand=0.5, seed=seed, want_pix=True, shard=(3, 8, 5))
    check_rows(mgr, plan, want, parallel.shard_global_rows(N, 5, 3, 8))


# ---- e. occupancy cell points -------------------------------------------------------------------------------------------------
OCC_SHAPE, OCC_LO, OCC_HI = (5, 6, 7), np.array([0.3, -1.1, 2.0], F32), np.array([1.7, 0.4, 3.3], F32)


def occ_host_points(seed):
    """(points float32 [ncells, 3], inside bool [ncells, 3]): lo + (index + u) / inv, every operation rounded to fp32, u = words 0..2
    of block `cell` of the occg stream; `inside` = the point falls into its own cell under floor((x - lo) * inv)."""
    ncells = int(np.prod(OCC_SHAPE))
    ijk = np.stack(np.meshgrid(*[np.arange(s) for s in OCC_SHAPE], indexing='ij'), -1).reshape(-1, 3).astype(F32)
    w = P.stream_words(P.OCCG, np.arange(ncells, dtype=np.uint64), seed)
    u = np.stack([P.u01(w[a]) for a in range(3)], 1)
    inv = R.inv_of(OCC_SHAPE, OCC_LO, OCC_HI)
    x = (OCC_LO + ((ijk + u).astype(F32) / inv).astype(F32)).astype(F32)
    return x, R.cell_index(x, OCC_SHAPE, OCC_LO, OCC_HI) == ijk, ijk


@pytest.mark.parametrize('seed', SEEDS)
def test_occ_cell_points_are_keyed_by_the_cell(fn, seed):
    ncells = int(np.prod(OCC_SHAPE))
    g = fn.occupancy.OccupancyGrid.from_mask(torch.ones(OCC_SHAPE, dtype=torch.bool).cuda(), OCC_LO, OCC_HI, outside_occupied=False)
    cut = 97                                  # two calls: the second one's local index 0 is cell 97
    a, b = torch.empty(cut, 11, device='cuda'), torch.empty(ncells - cut, 11, device='cuda')
    fn.ops.occ_cell_points(g._c, 0, a, seed)
    fn.ops.occ_cell_points(g._c, cut, b, seed)
    got = torch.cat([a, b], 0)[:, 0:3].cpu().numpy()
    x, inside, ijk = occ_host_points(seed)
    clamped = ~inside.all(1)
    assert clamped.sum() <= ncells // 100, int(clamped.sum())
    assert np.array_equal(got[inside], x[inside])
    assert np.array_equal(R.cell_index(got, OCC_SHAPE, OCC_LO, OCC_HI), ijk)      # (the clamped ones too)
    c = torch.empty(ncells, 11, device='cuda')
    fn.ops.occ_cell_points(g._c, 0, c, 0)
    centre = (OCC_LO + ((ijk + F32(0.5)) / R.inv_of(OCC_SHAPE, OCC_LO, OCC_HI)).astype(F32)).astype(F32)
    assert np.array_equal(c[:, 0:3].cpu().numpy(), centre)


# ---- f. the fused routes use the seeds they draw ------------------------------------------------------------------------------
NS, NI, NRAYS = 64, 64, 40


def g7_networks(fn, golden_dir, raw_noise_std=0.):
    args = fn.run_nerf.make_args(N_importance=NI, N_samples=NS, perturb=1.0, white_bkgd=True, use_viewdirs=True, no_reload=True,
                                 raw_noise_std=raw_noise_std)
    ktr = fn.run_nerf.create_nerf(args)[0]
    wts = np.load(os.path.join(golden_dir, 'g7_weights.npz'))
    for net, pre in ((ktr['network_fn'], 'c.'), (ktr['network_fine'], 'f.')):
        net.load_state_dict({k[2:]: torch.from_numpy(np.ascontiguousarray(wts[k])) for k in wts.files if k.startswith(pre)})
    return ktr


def g8_rays(golden_dir):
    g8 = np.load(os.path.join(golden_dir, 'g8_train_step.npz'))
    return torch.from_numpy(g8['ro'][:NRAYS]).cuda(), torch.from_numpy(g8['rd'][:NRAYS]).cuda()


def test_forward_core_hands_its_seeds_to_the_streams(fn, golden_dir, math_mode):
    ktr = g7_networks(fn, golden_dir)
    net_c, net_f = ktr['network_fn'], ktr['network_fine']
    ro, rd = g8_rays(golden_dir)
    rays11 = fn.ops.pack_rays(ro, rd, 2.0, 6.0)
    torch.manual_seed(11)
    s0, s1 = fn.render._next_seed(), fn.render._next_seed()
    torch.manual_seed(11)
    got, _ = fn.render._forward_core(rays11, net_c, net_f, NS, NI, False, 1.0, True, None, None, None, None, save=True)
    want, _ = fn.render._forward_core(rays11, net_c, net_f, NS, NI, False, 1.0, True, host_u(P.COAR, (NRAYS, NS), s0),
                                      host_u(P.PDFS, (NRAYS, NI), s1), None, None, save=True)
    for k in ('z0', 'z_vals', 'rgb0', 'rgb_map'):
        assert same(got[k], want[k]), k
    swapped, _ = fn.render._forward_core(rays11, net_c, net_f, NS, NI, False, 1.0, True, host_u(P.COAR, (NRAYS, NS), s1),
                                         host_u(P.PDFS, (NRAYS, NI), s0), None, None, save=True)
    assert not same(got['z0'], swapped['z0']) and not same(got['z_vals'], swapped['z_vals'])


@pytest.mark.parametrize('route', ['step', 'forward_backward'])
@pytest.mark.parametrize('noise', [0.0, 1.0])
def test_trainer_hands_its_seeds_to_the_streams(fn, golden_dir, math_mode, route, noise):
    """The noise seed (raw_noise_std > 0) is drawn before the coarse and the fine seed; with the same noise on both sides the
    depths of both passes are those of the injected run."""
    ro, rd = g8_rays(golden_dir)
    tgt = torch.rand(NRAYS, 3, generator=torch.Generator().manual_seed(1)).cuda()
    K = np.array([[1111.1, 0, 400.0], [0, 1111.1, 400.0], [0, 0, 1]])
    torch.manual_seed(12)
    if noise > 0.:
        fn.render._next_seed()
    s0, s1 = fn.render._next_seed(), fn.render._next_seed()
    outs = []
    for inject in (False, True):
        tr = fn.run_nerf.Trainer(g7_networks(fn, golden_dir, noise), 800, 800, K, 2.0, 6.0)
        assert tr.raw_noise_std == noise and tr.perturb and tr.fused
        kw = dict(t_rand=host_u(P.COAR, (NRAYS, NS), s0), u=host_u(P.PDFS, (NRAYS, NI), s1)) if inject else {}
        torch.manual_seed(12)
        _, out = getattr(tr, route)(ro, rd, tgt, **kw)
        outs.append({k: out[k].clone() for k in ('z0', 'z_vals')})
    assert same(outs[0]['z0'], outs[1]['z0']) and same(outs[0]['z_vals'], outs[1]['z_vals'])
    assert same(outs[0]['z0'], fn.ops.sample_coarse(fn.ops.pack_rays(ro, rd, 2.0, 6.0), NS, t_rand=host_u(P.COAR, (NRAYS, NS), s0)))


def test_cascade_trainer_hands_its_seeds_to_the_streams(fn, golden_dir, math_mode):
    S0, S1, N = 8, 5, 24
    w = np.load(os.path.join(golden_dir, 'g10_pp_weights.npz'))
    nets = []
    for m in range(2):
        net = fn.nerfpp.NerfNetWithAutoExpo(None)
        net.nerf_net.load_state_dict({k[len(f'l{m}.'):]: torch.from_numpy(np.asarray(w[k])).clone() for k in w.files
                                      if k.startswith((f'l{m}.fg_net.', f'l{m}.bg_net.'))})
        nets.append(net)
    gen = torch.Generator().manual_seed(S0 * 131 + S1)
    ro = ((torch.rand(N, 3, generator=gen) - 0.5) * 0.9).cuda()
    rd = torch.randn(N, 3, generator=gen).cuda()
    tgt = torch.rand(N, 3, generator=gen).cuda()
    tr = fn.nerfpp.CascadeTrainer(nets, cascade_samples=(S0, S1), lrate=5e-4)
    torch.manual_seed(13)
    s = [fn.render._next_seed() for _ in range(4)]          # the step's order: fg jitter, bg jitter, fg u, bg u
    torch.manual_seed(13)
    tr.step(ro, rd, tgt, update=False)
    got = [(a.clone(), b.clone()) for a, b in tr.last_depths]
    rand = [{'fg_t': host_u(P.FGDP, (N, S0), s[0]), 'bg_t': host_u(P.COAR, (N, S0), s[1])},
            {'fg_u': host_u(P.PDFS, (N, S1), s[2]), 'bg_u': host_u(P.PDFS, (N, S1), s[3])}]
    tr.step(ro, rd, tgt, rand=rand, update=False)
    for m in range(2):
        assert got[m][0].shape == (N, S0 if m == 0 else S0 + S1)
        assert same(got[m][0], tr.last_depths[m][0]) and same(got[m][1], tr.last_depths[m][1]), m
    assert not same(got[0][0], got[0][1]) and not same(got[1][0], got[1][1])
