"""Occupancy grid on the GPU against the restatement of tests/occ_numpy.py: build / query / classify bit for bit, the masked
render against the CPU oracle at the GPU's own depths, the exactness the contract promises, and the public surface."""
import numpy as np
import pytest
import torch

import occ_numpy as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

TOL_RGB = 1e-4      # test_gpu_render.TOL_RGB, the north star's bound
TOL_ACC = 3e-4      # test_gpu_render.test_properties_at_baseline_size
NS, NI = 64, 128


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


def G(fn):
    return fn.occupancy.OccupancyGrid


def same_bits(a, b):
    """torch.equal on the bit patterns: disp_map is 0 / 0 = NaN on a ray without any weight, in the plain render too."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def grid_of(fn, name):
    m, lo, hi, oo = R.scene_grids()[name]
    return G(fn).from_mask(torch.from_numpy(m).cuda(), lo, hi, oo), (m, lo, hi, oo)


def networks(fn, **over):
    """create_nerf's render kwargs with the scene's random-init parameters loaded into both networks."""
    kw = dict(N_importance=NI, N_samples=NS, perturb=0., white_bkgd=False, use_viewdirs=True, no_reload=True)
    kw.update(over)
    ktr, kte, _, _, _, _ = fn.run_nerf.create_nerf(fn.run_nerf.make_args(**kw))
    sdc, sdf = R.scene_networks(O)
    kte['network_fn'].load_state_dict(sdc)
    kte['network_fine'].load_state_dict(sdf)
    return kte, sdc, sdf


# ---- 1. build --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(33, 20, 47), (2, 2, 2), (65, 65, 65), (5, 70, 3)])
@pytest.mark.parametrize('dilate', [0, 1, 3])
def test_build_equals_the_restatement(fn, shape, dilate):
    rs = np.random.RandomState(sum(shape) + dilate)
    c = [np.linspace(-1, 1, s) for s in shape]
    X, Y, Z = np.meshgrid(*c, indexing='ij')
    smooth = (np.exp(-4 * ((X - 0.2) ** 2 + Y ** 2 + (Z + 0.3) ** 2)) + 0.5 * np.exp(-30 * ((X + 0.5) ** 2 + (Y - 0.5) ** 2 + Z ** 2))).astype(np.float32)
    sparse = (rs.rand(*shape) * (rs.rand(*shape) < 0.02)).astype(np.float32)
    for vol, thrs in ((smooth, (0.3, 0.0, 2.0, -1.0)), (sparse, (0.0, 0.5, 1.0, -0.5)),
                      (np.full(shape, 0.25, np.float32), (0.25, float(np.nextafter(np.float32(0.25), np.float32(0)))))):
        for thr in thrs:
            g = G(fn).from_density(torch.from_numpy(vol).cuda(), -1.0, 1.0, threshold=thr, dilate=dilate)
            ref = R.build(vol, thr, dilate)
            assert g.shape == ref.shape and np.array_equal(g.to_mask().cpu().numpy(), ref), (shape, dilate, thr)
            assert abs(g.occupied_fraction() - ref.mean()) < 1e-6
    assert not R.build(smooth, 2.0, dilate).any() and R.build(smooth, -1.0, dilate).all()      # the empty and the full grid were among them
    assert not R.build(np.full(shape, 0.25, np.float32), 0.25, dilate).any()                  # equal to the threshold: not occupied


@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 5, 7), (32, 32, 32), (31, 33, 65)])
def test_from_mask_round_trips_and_saves(fn, shape, tmp_path):
    m = np.random.RandomState(5).rand(*shape) < 0.37
    lo, hi = np.array([-1.0, -2.0, 0.5], np.float32), np.array([1.0, 0.25, 3.0], np.float32)
    g = G(fn).from_mask(torch.from_numpy(m).cuda(), lo, hi, outside_occupied=False)
    assert torch.equal(g.to_mask(), torch.from_numpy(m).cuda())
    p = str(tmp_path / 'grid.npz')
    g.save(p)
    with np.load(p) as f:
        assert np.array_equal(R.words_to_mask(f['words'], f['shape']), m)
    h = G(fn).load(p)
    assert torch.equal(h.words, g.words) and h.shape == g.shape and h.outside_occupied is False
    assert np.array_equal(h.lo, lo) and np.array_equal(h.hi, hi) and np.array_equal(h.inv, R.inv_of(shape, lo, hi))


# ---- 2. query and classify -------------------------------------------------------------------------------------------
def special_points(shape, lo, hi, rs):
    lo3, hi3 = np.broadcast_to(np.asarray(lo, np.float32), (3,)), np.broadcast_to(np.asarray(hi, np.float32), (3,))
    pts = [(lo3 + (hi3 - lo3) * rs.rand(4000, 3) * 1.3 - 0.15 * (hi3 - lo3)).astype(np.float32)]      # random, some outside
    faces = []
    for ax in range(3):      # exactly on cell faces (as fp32 can name them), on lo and on hi, and an ulp to either side
        f = (lo3[ax].astype(np.float64) + (hi3[ax].astype(np.float64) - lo3[ax]) * np.arange(shape[ax] + 1) / shape[ax]).astype(np.float32)
        for v in (f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
            p = (lo3 + (hi3 - lo3) * rs.rand(v.size, 3)).astype(np.float32)
            p[:, ax] = v
            faces.append(p)
    pts += faces
    odd = (lo3 + (hi3 - lo3) * rs.rand(12, 3)).astype(np.float32)
    for i, v in enumerate((np.nan, np.inf, -np.inf, 3e38)):
        for ax in range(3):
            odd[i * 3 + ax, ax] = v
    pts.append(odd)
    pts.append(np.stack([lo3, hi3, np.nextafter(lo3, np.float32(-np.inf)), np.nextafter(hi3, np.float32(-np.inf))]))
    return np.concatenate(pts, 0)


@pytest.mark.parametrize('outside', [False, True])
def test_query_equals_the_restatement(fn, outside):
    rs = np.random.RandomState(11)
    seen_any, seen_all = False, True
    for shape, lo, hi in (((16, 16, 16), -1.0, 1.0), ((7, 33, 12), np.array([-1.5, 0.1, -3.0], np.float32), np.array([2.0, 0.7, 5.0], np.float32)),
                          ((1, 1, 1), 0.0, 1.0), ((129, 3, 65), -0.3, 0.9)):
        m = rs.rand(*shape) < 0.5
        g = G(fn).from_mask(torch.from_numpy(m).cuda(), lo, hi, outside_occupied=outside)
        pts = special_points(shape, lo, hi, rs)
        got = g.query(torch.from_numpy(pts).cuda()).cpu().numpy()
        ref = R.query(m, lo, hi, outside, pts)
        assert np.array_equal(got, ref), (shape, np.nonzero(got != ref)[0][:5], pts[got != ref][:5])
        seen_any, seen_all = seen_any or bool(got.any()), seen_all and bool(got.all())
    assert seen_any and not seen_all
    assert g.query(torch.from_numpy(pts).cuda().reshape(-1, 1, 3)).shape == (pts.shape[0], 1)


# 169 rays: 169 * 64 and 169 * 192 are no multiples of the 1024-point block.  The tails: 37 x 13 = 481 points, one partial block, and
# a thread's four consecutive samples straddle two rays (13 is no multiple of 4); 300 x 7 = 2100 points, three blocks, the last one
# partial, so the scanned block offsets are used
@pytest.mark.parametrize('n,S', [pytest.param(169, 64, id='64'), pytest.param(169, 192, id='192'), pytest.param(37, 13, id='37x13'),
                                 pytest.param(300, 7, id='300x7')])
def test_classify_equals_the_restatement(fn, n, S):
    rs = np.random.RandomState(S)
    rays = R.scene_rays(O, side=13 if n <= 169 else 18)
    rays = rays[np.round(np.linspace(0, rays.shape[0] - 1, n)).astype(int)]      # n rays spread over the image (all 169 of them)
    assert rays.shape[0] == n
    z = np.sort(2.0 + 4.0 * rs.rand(rays.shape[0], S).astype(np.float32), -1)
    rays_t, z_t = torch.from_numpy(rays).cuda(), torch.from_numpy(z).cuda()
    cases = dict(R.scene_grids())
    cases['empty'] = (np.zeros((8, 8, 8), bool), np.float32(-8), np.float32(8), False)
    cases['full'] = (np.ones((8, 8, 8), bool), np.float32(-8), np.float32(8), False)
    cases['outside only'] = (np.zeros((4, 4, 4), bool), np.float32(-0.5), np.float32(0.5), True)
    for name, (m, lo, hi, oo) in cases.items():
        g = G(fn).from_mask(torch.from_numpy(m).cuda(), lo, hi, oo)
        raw = torch.full((rays.shape[0], S, 4), 7.0, device='cuda')
        idx, cnt = g.classify(rays_t, z_t, raw)
        bits = R.classify(m, lo, hi, oo, rays, z)
        live = np.nonzero(bits.reshape(-1))[0]
        assert cnt.tolist() == [live.size, bits.size], name
        assert np.array_equal(idx[:live.size].cpu().numpy(), live), name
        dead = (raw == 0).all(-1).cpu().numpy()
        assert np.array_equal(dead, ~bits) and bool((raw[torch.from_numpy(bits).cuda()] == 7.0).all()), name
        idx2, cnt2 = g.classify(rays_t, z_t)      # raw is optional; two calls agree
        assert torch.equal(cnt, cnt2) and torch.equal(idx[:live.size], idx2[:live.size])
        if name == 'empty':
            assert live.size == 0
        if name == 'full':
            assert live.size == bits.size


# ---- 3. the masked render is the contract ------------------------------------------------------------------------------
def restate(fn, sdc, sdf, rays, out, gm, white_bkgd):
    """The contract at the GPU's own depths: bits of o + d * z for the returned z0 / z1, the oracle's MLP at every point,
    zeros where the bit is clear, compositing."""
    m, lo, hi, oo = gm
    res = {}
    for tag, sd, zk, rk, ck, ak in (('0', sdc, 'z0', 'raw0', 'rgb0', 'acc0'), ('1', sdf, 'z_vals', 'raw', 'rgb_map', 'acc_map')):
        z = out[zk].cpu().numpy()
        bits = R.classify(m, lo, hi, oo, rays, z)
        raw, rgb, acc, _ = R.composite_at(O, sd, rays, z, bits, white_bkgd)
        got = out[rk].cpu()
        zero = (got == 0).all(-1).numpy()
        print('pass %s: masked %.4f of %d samples, max|raw - ref| / max(1, |ref|) = %.3g, max|rgb - ref| = %.3g, max|acc - ref| = %.3g' % (
            tag, 1 - bits.mean(), bits.size, float(((got - raw).abs() / raw.abs().clamp(min=1.0)).max()),
            float((out[ck].cpu() - rgb).abs().max()), float((out[ak].cpu() - acc).abs().max())))
        assert np.array_equal(zero, ~bits), 'the pattern of exact zeros is the restated mask'
        assert ((got - raw).abs() <= 2e-5 * raw.abs().clamp(min=1.0)).all()
        assert float((out[ck].cpu() - rgb).abs().max()) < TOL_RGB
        assert float((out[ak].cpu() - acc).abs().max()) < TOL_ACC
        assert 0.2 < 1.0 - bits.mean() < 0.9
        res[tag] = bits
    return res


@pytest.mark.parametrize('grid', ['ball', 'random', 'half'])
@pytest.mark.parametrize('perturb', [0, 1])
@pytest.mark.parametrize('white_bkgd', [False, True])
def test_masked_render_is_the_contract(fn, math_mode, grid, perturb, white_bkgd):
    kte, sdc, sdf = networks(fn)
    g, gm = grid_of(fn, grid)
    rays = R.scene_rays(O)
    rays_t = torch.from_numpy(rays).cuda()
    tr, u = R.scene_randoms(rays.shape[0], NS, NI, perturb)
    tr, u = (None if t is None else torch.from_numpy(t).cuda() for t in (tr, u))
    with torch.no_grad():
        out = fn.render._forward_occ(rays_t, kte['network_fn'], kte['network_fine'], NS, NI, False, float(perturb), white_bkgd, tr, u, g)
        plain, _ = fn.render._forward_core(rays_t, kte['network_fn'], kte['network_fine'], NS, NI, False, float(perturb), white_bkgd,
                                           tr, u, None, None, False)
    bits = restate(fn, sdc, sdf, rays, out, gm, white_bkgd)
    assert out['counts'].tolist() == [int(bits['0'].sum()), bits['0'].size, int(bits['1'].sum()), bits['1'].size]
    assert float((out['rgb_map'] - plain['rgb_map']).abs().max()) > 1e-2, 'the grid changes the image: the test is not empty'


# ---- 4. exactness ----------------------------------------------------------------------------------------------------
def render_rays(fn, kte, rays_t, **kw):
    args = {k: kte[k] for k in ('network_fn', 'network_fine', 'network_query_fn', 'N_samples', 'N_importance', 'white_bkgd')}
    args.update(kw)
    with torch.no_grad():
        return fn.render.render_rays(rays_t, **args)


def test_a_full_grid_is_the_plain_render_bit_for_bit(fn, math_mode):
    kte, _, _ = networks(fn, white_bkgd=True)
    rays_t = torch.from_numpy(R.scene_rays(O, side=13)).cuda()
    full = G(fn).from_mask(torch.ones(4, 5, 6, dtype=torch.bool, device='cuda'), -8.0, 8.0, outside_occupied=False)
    also = G(fn).from_mask(torch.zeros(2, 2, 2, dtype=torch.bool, device='cuda'), 50.0, 51.0, outside_occupied=True)
    for retraw in (True, False):
        a = render_rays(fn, kte, rays_t, retraw=retraw)
        for g in (full, also):
            b = render_rays(fn, kte, rays_t, retraw=retraw, occupancy=g)
            assert sorted(a) == sorted(b)
            for k in a:
                assert same_bits(a[k], b[k]), (k, retraw)


@pytest.mark.parametrize('grid', ['ball', 'random', 'half'])
def test_occupied_coarse_logits_are_the_plain_ones_bit_for_bit(fn, math_mode, grid):
    kte, _, _ = networks(fn)
    g, gm = grid_of(fn, grid)
    rays = R.scene_rays(O, side=13)
    rays_t = torch.from_numpy(rays).cuda()
    with torch.no_grad():
        out = fn.render._forward_occ(rays_t, kte['network_fn'], kte['network_fine'], NS, NI, False, 0., False, None, None, g)
        plain, _ = fn.render._forward_core(rays_t, kte['network_fn'], kte['network_fine'], NS, NI, False, 0., False, None, None, None,
                                           None, False)
        again = fn.render._forward_occ(rays_t, kte['network_fn'], kte['network_fine'], NS, NI, False, 0., False, None, None, g)
    assert torch.equal(out['z0'], plain['z0'])
    bits = torch.from_numpy(R.classify(*gm, rays, out['z0'].cpu().numpy())).cuda()
    assert 0 < int(bits.sum()) < bits.numel()
    raw0_plain = fn.ops.mlp_fwd(rays_t, plain['z0'], kte['network_fn'].flat, kte['network_fn'].packed()[0])
    assert torch.equal(out['raw0'][bits], raw0_plain[bits])
    assert bool((out['raw0'][~bits] == 0).all())
    for k in out:      # (d) two calls give bit-identical results 
        assert same_bits(out[k], again[k]), k


@pytest.mark.parametrize('white_bkgd', [False, True])
def test_an_empty_grid_renders_the_background_without_running_the_network(fn, math_mode, white_bkgd):
    kte, _, _ = networks(fn, white_bkgd=white_bkgd)
    rays_t = torch.from_numpy(R.scene_rays(O)).cuda()
    empty = G(fn).from_mask(torch.zeros(8, 8, 8, dtype=torch.bool, device='cuda'), -1.0, 1.0, outside_occupied=False)
    with torch.no_grad():
        out = fn.render._forward_occ(rays_t, kte['network_fn'], kte['network_fine'], NS, NI, False, 0., white_bkgd, None, None, empty)
    n = rays_t.shape[0]
    assert out['counts'].tolist() == [0, n * NS, 0, n * (NS + NI)]      # list length 0 on the device: no MLP row ran
    assert bool((out['rgb_map'] == (1.0 if white_bkgd else 0.0)).all()) and bool((out['acc_map'] == 0).all())
    assert bool((out['rgb0'] == (1.0 if white_bkgd else 0.0)).all()) and bool((out['raw'] == 0).all()) and bool((out['raw0'] == 0).all())
    ret = render_rays(fn, kte, rays_t, occupancy=empty)
    assert torch.equal(ret['rgb_map'], out['rgb_map']) and torch.equal(ret['acc_map'], out['acc_map'])


def test_list_forward_writes_only_the_listed_rows(fn, math_mode):
    kte, _, _ = networks(fn)
    net = kte['network_fn']
    rays = R.scene_rays(O, side=13)
    rays_t = torch.from_numpy(rays).cuda()
    z = fn.ops.sample_coarse(rays_t, NS)
    P = z.numel()
    plain = fn.ops.mlp_fwd(rays_t, z, net.flat, net.packed()[0])
    pick = torch.from_numpy(np.sort(np.random.RandomState(0).choice(P, 777, replace=False)).astype(np.int32)).cuda()
    idx = torch.full((P,), 2 ** 30, device='cuda', dtype=torch.int32)      # entries past the count are never read as rows
    idx[:777] = pick
    cnt = torch.tensor([777, P], device='cuda', dtype=torch.int32)
    raw = torch.full((rays.shape[0], NS, 4), -3.0, device='cuda')
    fn.ops.mlp_fwd_list(rays_t, z, net.flat, net.packed()[0], raw, idx, cnt)
    sel = torch.zeros(P, dtype=torch.bool, device='cuda')
    sel[pick.long()] = True
    assert bool((raw.reshape(P, 4)[~sel] == -3.0).all())
    # rows of the matrix products do not see each other and the VALU heads are per row too: a row's logits do not depend on which
    # tile, or which row of it, the point lands in -- bit for bit, for a list whose tiles are composed unlike the plain batch's
    got, ref = raw.reshape(P, 4)[sel], plain.reshape(P, 4)[sel]
    print('list forward vs plain forward on 777 scattered rows (%s): max |difference| = %.3g' % (math_mode, float((got - ref).abs().max())))
    assert torch.equal(got, ref)
    with pytest.raises(RuntimeError):
        fn._lib.check(fn._lib.lib().fastnerf_mlp_fwd_list_ex(2, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, None), 'list forward of another kind')


# ---- 5. the surface --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chunk', [25, 50, 40, 64, 1000])      # 100 rays: 25 and 50 divide the image, 40 and 64 do not
def test_render_and_render_path_pass_the_grid_through(fn, chunk):
    kte, _, _ = networks(fn, white_bkgd=True)
    g, _ = grid_of(fn, 'ball')
    H = W = 10
    K = np.array([[17.0, 0, 5.0], [0, 17.0, 5.0], [0, 0, 1]])
    c2w = fn.synthetic.pose_spherical(30.0, -30.0, 4.0)[:3, :4]
    kw = dict(kte, near=2.0, far=6.0, occupancy=g)
    kw.pop('ndc', None)
    with torch.no_grad():
        rgb, disp, acc, _ = fn.render.render(H, W, K, chunk=chunk, c2w=c2w.cuda(), ndc=False, **kw)
        ro, rd = fn.run_nerf_helpers.get_rays(H, W, K, c2w.cuda())
        rays11 = fn.ops.pack_rays(ro, rd, 2.0, 6.0)
        parts = [render_rays(fn, kte, rays11[i:i + chunk], occupancy=g) for i in range(0, H * W, chunk)]
        plain, _, _, _ = fn.render.render(H, W, K, chunk=chunk, c2w=c2w.cuda(), ndc=False, **{k: v for k, v in kw.items() if k != 'occupancy'})
    assert torch.equal(rgb.reshape(-1, 3), torch.cat([p['rgb_map'] for p in parts], 0))
    assert torch.equal(acc.reshape(-1), torch.cat([p['acc_map'] for p in parts], 0))
    assert float((rgb - plain).abs().max()) > 1e-2
    rgbs, _ = fn.render.render_path([c2w.numpy()], (H, W, 17.0), K, chunk, dict(kw, ndc=False))
    assert np.array_equal(rgbs[0], rgb.cpu().numpy())


class TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(3)
        self.a, self.b = torch.nn.Linear(3, 48), torch.nn.Linear(48, 4)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * 1.5)

    def forward(self, x):
        return self.b(torch.sin(self.a(x)))


@pytest.mark.parametrize('grid', ['ball', 'half'])
@pytest.mark.parametrize('white_bkgd', [False, True])
def test_closure_route_meets_the_contract(fn, grid, white_bkgd):
    """Any torch network: the samples are classified on the device, network_query_fn sees exactly the occupied points, and the
    result is the contract restated with the same network evaluated by torch on the CPU, at the GPU's own depths."""
    coarse, fine = TinyNet(), TinyNet()
    with torch.no_grad():
        fine.b.bias.add_(0.3)
    cpu = {id(m): m for m in (coarse, fine)}
    import copy
    gc, gf = copy.deepcopy(coarse).cuda(), copy.deepcopy(fine).cuda()
    g, gm = grid_of(fn, grid)
    rays = R.scene_rays(O)
    rays_t = torch.from_numpy(rays).cuda()
    seen = []

    def query(pts, viewdirs, net):
        assert pts.dim() == 3 and pts.shape[1:] == (1, 3) and viewdirs.shape == (pts.shape[0], 3)
        seen.append(pts.shape[0])
        return net(pts)
    kw = dict(network_fn=gc, network_fine=gf, network_query_fn=query, N_samples=NS, N_importance=NI, white_bkgd=white_bkgd, retraw=True)
    with torch.no_grad():
        ret = fn.render.render_rays(rays_t, occupancy=g, **kw)
        n_plain = []
        plain = fn.render.render_rays(rays_t, **dict(kw, network_query_fn=lambda p, v, net: (n_plain.append(p.shape[0]), net(p))[1]))
        # the same kernels step by step give the depths the route used (deterministic: perturb = 0)
        z0 = fn.ops.sample_coarse(rays_t, NS)
        raw0 = fn.render._query_occupied(lambda p, v, net: net(p), gc, rays_t, z0, rays_t[:, 8:11], g)
        rgb0, _, acc0, w0, _ = fn.ops.raw2outputs_fwd(raw0.contiguous(), z0, rays_t, None, white_bkgd)
        z1, _, _ = fn.ops.sample_pdf_merge(z0, w0, NI, det=True)
        c0, c1 = g.classify(rays_t, z0)[1], g.classify(rays_t, z1)[1]
    assert seen == [int(c0[0]), int(c1[0])] and n_plain == [rays.shape[0]] * 2      # exactly as many points as the list is long
    assert torch.equal(ret['rgb0'], rgb0)
    out = {'z0': z0, 'z_vals': z1, 'raw0': raw0, 'raw': ret['raw'], 'rgb0': ret['rgb0'], 'acc0': ret['acc0'], 'rgb_map': ret['rgb_map'],
           'acc_map': ret['acc_map']}
    m, lo, hi, oo = gm
    for sd_net, zk, rk, ck, ak in ((coarse, 'z0', 'raw0', 'rgb0', 'acc0'), (fine, 'z_vals', 'raw', 'rgb_map', 'acc_map')):
        z = out[zk].cpu().numpy()
        bits = R.classify(m, lo, hi, oo, rays, z)
        with torch.no_grad():
            raw, rgb, acc, _ = R.composite_at(O, None, rays, z, bits, white_bkgd, query_fn=sd_net)
        got = out[rk].cpu()
        assert np.array_equal((got == 0).all(-1).numpy(), ~bits)
        assert ((got - raw).abs() <= 2e-5 * raw.abs().clamp(min=1.0)).all()
        assert float((out[ck].cpu() - rgb).abs().max()) < TOL_RGB and float((out[ak].cpu() - acc).abs().max()) < TOL_ACC
        assert 0.2 < 1.0 - bits.mean() < 0.9
    assert float((ret['rgb_map'] - plain['rgb_map']).abs().max()) > 1e-2


@pytest.mark.parametrize('white_bkgd', [False, True])
def test_closure_route_with_an_empty_list(fn, white_bkgd):
    """A chunk whose rays all miss the occupied cells is an ordinary input: the background comes out, and network_query_fn is
    handed 0 points (it is still asked: its answer's last dimension is the channel count of raw)."""
    gc, gf = TinyNet().cuda(), TinyNet().cuda()
    rays_t = torch.from_numpy(R.scene_rays(O)).cuda()
    empty = G(fn).from_mask(torch.zeros(8, 8, 8, dtype=torch.bool, device='cuda'), -1.0, 1.0, outside_occupied=False)
    seen = []

    def query(pts, viewdirs, net):
        seen.append(pts.shape[0])
        assert pts.shape[1:] == (1, 3) and viewdirs.shape == (pts.shape[0], 3)
        return net(pts)
    with torch.no_grad():
        ret = fn.render.render_rays(rays_t, gc, query, NS, retraw=True, N_importance=NI, network_fine=gf, white_bkgd=white_bkgd,
                                    occupancy=empty)
    assert seen == [0, 0]
    bg = 1.0 if white_bkgd else 0.0
    assert bool((ret['rgb_map'] == bg).all()) and bool((ret['acc_map'] == 0).all()) and bool((ret['rgb0'] == bg).all())
    assert ret['raw'].shape == (rays_t.shape[0], NS + NI, 4) and bool((ret['raw'] == 0).all())
    # a grid that some rays of the batch miss entirely and others hit: nothing special either
    g, _ = grid_of(fn, 'ball')
    far = rays_t.clone()
    far[:32, 0:3] += 50.0
    with torch.no_grad():
        part = fn.render.render_rays(far, gc, query, NS, N_importance=NI, network_fine=gf, white_bkgd=white_bkgd, occupancy=g)
        near = fn.render.render_rays(rays_t, gc, query, NS, N_importance=NI, network_fine=gf, white_bkgd=white_bkgd, occupancy=g)
    assert bool((part['rgb_map'][:32] == bg).all()) and torch.equal(part['rgb_map'][32:], near['rgb_map'][32:])


def test_ray_batches_without_view_directions(fn, math_mode):
    args = fn.run_nerf.make_args(N_importance=NI, N_samples=NS, perturb=0., white_bkgd=True, use_viewdirs=False, no_reload=True)
    torch.manual_seed(0)
    _, kte, _, _, _, _ = fn.run_nerf.create_nerf(args)
    rays = R.scene_rays(O)[:, :8].copy()
    rays_t = torch.from_numpy(rays).cuda()
    full = G(fn).from_mask(torch.ones(2, 2, 2, dtype=torch.bool, device='cuda'), -8.0, 8.0)
    g, gm = grid_of(fn, 'ball')
    a = render_rays(fn, kte, rays_t, retraw=True)
    b = render_rays(fn, kte, rays_t, retraw=True, occupancy=full)
    for k in a:
        assert same_bits(a[k], b[k]), k
    c = render_rays(fn, kte, rays_t, retraw=True, occupancy=g)
    assert c['raw'].shape == a['raw'].shape and torch.isfinite(c['rgb_map']).all()
    dead = (c['raw'][..., :4] == 0).all(-1)
    assert 0.2 < float(dead.float().mean()) < 0.9


def test_errors(fn):
    kte, _, _ = networks(fn)
    g, _ = grid_of(fn, 'ball')
    rays_t = torch.from_numpy(R.scene_rays(O)).cuda()
    args = {k: kte[k] for k in ('network_fn', 'network_fine', 'network_query_fn', 'N_samples', 'N_importance')}
    with torch.no_grad():
        with pytest.raises(ValueError):
            fn.render.render_rays(rays_t, raw_noise_std=1.0, occupancy=g, **args)
    assert any(p.requires_grad for p in kte['network_fn'].parameters())
    with pytest.raises(ValueError):
        fn.render.render_rays(rays_t, occupancy=g, **args)      # grad mode on, parameters require grad
    tiny = TinyNet().cuda()
    with pytest.raises(ValueError):
        fn.render.render_rays(rays_t, tiny, lambda p, v, n: n(p), NS, occupancy=g)
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            fn.render.render_rays(rays_t.cpu(), occupancy=g, **args)
    with pytest.raises(RuntimeError):
        G(fn).from_mask(torch.ones(2, 2, 2, dtype=torch.bool), -1.0, 1.0)
    with pytest.raises(RuntimeError):
        G(fn).from_density(torch.ones(3, 3, 3), -1.0, 1.0)
    with pytest.raises(RuntimeError):
        g.query(torch.zeros(4, 3))
    with pytest.raises(ValueError):
        G(fn).from_mask(torch.ones(2, 2, 2, dtype=torch.bool, device='cuda'), 1.0, 1.0)
    with pytest.raises(ValueError):
        G(fn).from_density(torch.ones(3, 3, 3, device='cuda'), -1.0, 1.0, dilate=-1)


def test_from_network_takes_the_maximum_of_both_networks(fn):
    kte, _, _ = networks(fn)
    N, bound = 24, 1.2
    t = torch.linspace(-bound, bound, N + 1, device='cuda')
    vc = fn.mesh.density_grid(kte['network_fn'], t, t, t)
    vf = fn.mesh.density_grid(kte['network_fine'], t, t, t)
    for which, vol in (('both', torch.maximum(vc, vf)), ('fine', vf), ('coarse', vc)):
        g = G(fn).from_network(kte, N=N, bound=bound, threshold=0.05, dilate=1, which=which)
        assert g.shape == (N, N, N) and np.array_equal(g.to_mask().cpu().numpy(), R.build(vol.cpu().numpy(), 0.05, 1)), which
        assert np.array_equal(g.lo, np.full(3, -bound, np.float32)) and g.outside_occupied
