"""The per-ray and per-sample kernels of csrc/rays.hip against tests/rays_ref.py, through the C ABI: gen_rays, gen_rays_pixels,
ndc_rays, pack_rays, sample_coarse, posenc, pp_gen_rays, pp_intersect_sphere, pp_fg_depths, pp_perturb_samples.

Every kernel runs at a tail size (1 and 257 elements) and one trip past grid_for's 2048 x 256 threads, where every element is
compared.  The output buffers are 256 elements longer than the kernel may write and pre-filled with a NaN canary that must
survive.  The bounds: |got - v| <= e of the running-error evaluation (validated on these very inputs by
tests/test_rays_ref_cpu.py) wherever e is finite, and equality, bit for bit, with the numpy-float32 evaluation of the same formula.
posenc is held to float64 sin / cos of its exact argument, pp_gen_rays to the float64 product rounded once.  Measured figures:
profiles/ray_side_fp64.md."""
import numpy as np
import pytest
import torch

import rays_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
PAD = 256
CANARY = 0x7fc0beef                 # a quiet NaN with a payload
RAY_SIZES = (1, 257, R.N_RAYS_BIG)
# posenc: the largest |got - float64 sin / cos| measured on the MI355X over all six input sets is 1.171 u (profiles/ray_side_fp64.md);
# the assertion is twice that, far below the 2e-6 = 33.6 u of test_posenc_g3
POSENC_MEASURED_U = 1.171
POSENC_TOL = 2.0 * POSENC_MEASURED_U * R.U
assert POSENC_TOL <= 2e-6


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return fastnerf


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def padded(numel):
    """An output buffer of numel floats plus PAD canaries."""
    return torch.full((numel + PAD,), CANARY, dtype=torch.int32, device='cuda').view(torch.float32)


def taken(buf, *shape):
    """The first prod(shape) floats of a padded buffer as numpy, after checking that the canaries behind them are untouched."""
    numel = int(np.prod(shape))
    assert buf.numel() == numel + PAD
    assert bool((buf.view(torch.int32)[numel:] == CANARY).all()), 'the kernel wrote beyond its output'
    out = buf[:numel].cpu().numpy().reshape(shape)
    assert not (out.view(np.uint32) == CANARY).any(), 'an output element was not written'
    return out


def call(fn, name, *args):
    fn.ops.check(getattr(fn.ops.lib(), name)(*args, fn.ops.stream()), name)


def p(t):
    assert t is None or t.is_contiguous()
    return None if t is None else t.data_ptr()


def bit_equal(got, emu):
    """Equal bit for bit, NaN matching NaN."""
    got, emu = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(emu, dtype=F32)
    return got.shape == emu.shape and bool(((got.view(np.uint32) == emu.view(np.uint32)) | (np.isnan(got) & np.isnan(emu))).all())


def hold(name, got, re_, emu):
    """|got - v| <= e wherever e is finite; the NaN pattern and every bit as in the fp32 evaluation."""
    r, fin = R.ratio(got, re_)
    print('RATIO %s: max |got - v| / e = %.3f over %d elements, %.4f %% without a finite bound, bit-equal to the emulation: %s' % (
        name, float(r.max()), got.size, 100.0 * (1.0 - fin.mean()), bit_equal(got, emu)))
    assert float(r.max()) <= 1.0, name
    assert np.array_equal(np.isnan(got), np.isnan(emu)), name
    assert bit_equal(got, emu), name


def grid(H, W):
    i = np.arange(H * W)
    return i // W, i % W


# ---- gen_rays, gen_rays_pixels -----------------------------------------------------------------------------------------------------
def run_gen_rays_pixels(fn, pix, poses):
    n, cam = len(pix), R.CAMERA
    ro, rd = padded(n * 3), padded(n * 3)
    pix_t, poses_t = G(pix), G(poses)      # (named: a temporary is freed, and its block handed to the next one, before the launch)
    assert pix_t.dtype == torch.int32 and poses_t.dtype == torch.float32 and int(pix_t[:, 0].max()) < poses_t.shape[0]
    call(fn, 'fastnerf_gen_rays_pixels', n, p(pix_t), p(poses_t), cam['fx'], cam['fy'], cam['cx'], cam['cy'], p(ro), p(rd))
    return taken(ro, n, 3), taken(rd, n, 3)


@pytest.mark.parametrize('case', R.gen_rays_inputs(), ids=lambda c: '%dx%d' % c[:2])
def test_gen_rays(fn, case):
    H, W, c2w = case
    cam = R.CAMERA
    host = np.ascontiguousarray(c2w, dtype=F32)
    ro, rd = padded(H * W * 3), padded(H * W * 3)
    call(fn, 'fastnerf_gen_rays', H, W, cam['fx'], cam['fy'], cam['cx'], cam['cy'], host.ctypes.data, p(ro), p(rd))
    o, d = taken(ro, H * W, 3), taken(rd, H * W, 3)
    row, col = grid(H, W)
    re_, emu = R.both(R.pixel_ray, row, col, cam['fx'], cam['fy'], cam['cx'], cam['cy'], c2w.reshape(12))
    hold('gen_rays %dx%d' % (H, W), d, re_, emu)
    assert bit_equal(o, np.broadcast_to(c2w[:, 3], (H * W, 3)))
    # the pixel-list kernel at the same pixels: the same bits
    pix = np.stack([np.zeros(H * W), row, col], 1).astype(np.int32)
    o2, d2 = run_gen_rays_pixels(fn, pix, c2w[None])
    assert bit_equal(d2, d) and bit_equal(o2, o)


@pytest.mark.parametrize('n', RAY_SIZES)
def test_gen_rays_pixels(fn, n):
    pix, poses = R.gen_rays_pixels_inputs(n)
    assert pix[:, 1:].max() == 4031
    o, d = run_gen_rays_pixels(fn, pix, poses)
    cam = R.CAMERA
    c = poses.reshape(-1, 12)[pix[:, 0]]
    re_, emu = R.both(R.pixel_ray, pix[:, 1], pix[:, 2], cam['fx'], cam['fy'], cam['cx'], cam['cy'], c)
    hold('gen_rays_pixels n=%d' % n, d, re_, emu)
    assert bit_equal(o, c[:, [3, 7, 11]])


# ---- ndc_rays, pack_rays -----------------------------------------------------------------------------------------------------------
def run_ndc(fn, ro, rd, near):
    n = len(ro)
    H, W, focal = R.NDC_CAM
    oo, od = padded(n * 3), padded(n * 3)
    ro_t, rd_t = G(ro), G(rd)
    call(fn, 'fastnerf_ndc_rays', n, H, W, focal, near, p(ro_t), p(rd_t), p(oo), p(od))
    return np.concatenate([taken(oo, n, 3), taken(od, n, 3)], 1)


def run_pack(fn, ro, rd, near, far, ndc):
    n = len(ro)
    H, W, focal = R.NDC_CAM
    out = padded(n * 11)
    ro_t, rd_t = G(ro), G(rd)
    call(fn, 'fastnerf_pack_rays', n, p(ro_t), p(rd_t), near, far, int(ndc), H, W, focal, p(out))
    return taken(out, n, 11)


@pytest.mark.parametrize('near', R.NDC_NEARS)
@pytest.mark.parametrize('n', RAY_SIZES)
def test_ndc_rays(fn, n, near):
    ro, rd = R.ndc_inputs(n)
    H, W, focal = R.NDC_CAM
    got = run_ndc(fn, ro, rd, near)
    re_, emu = R.both(R.ndc_one, R.ndc_scale(W, focal), R.ndc_scale(H, focal), near, ro, rd)
    hold('ndc_rays n=%d near=%g' % (n, near), got, re_, emu)


@pytest.mark.parametrize('ndc', [False, True], ids=['plain', 'ndc'])
@pytest.mark.parametrize('n', RAY_SIZES)
def test_pack_rays(fn, n, ndc):
    H, W, focal = R.NDC_CAM
    ro, rd = R.ndc_inputs(n) if ndc else R.pack_inputs(n)
    near, far = (0.0, 1.0) if ndc else (2.0, 6.0)
    got = run_pack(fn, ro, rd, near, far, ndc)
    re_, emu = R.both(R.pack_rays, ro, rd, near, far, ndc, R.ndc_scale(W, focal), R.ndc_scale(H, focal))
    hold('pack_rays n=%d ndc=%d' % (n, ndc), got, re_, emu)
    assert bit_equal(got[:, 6], np.full(n, near, dtype=F32)) and bit_equal(got[:, 7], np.full(n, far, dtype=F32))
    if ndc:
        assert bit_equal(got[:, :6], run_ndc(fn, ro, rd, 1.0))
    else:
        assert bit_equal(got[:, :3], ro) and bit_equal(got[:, 3:6], rd)
    # columns 8-10: the direction before NDC over its norm -- a unit vector to the accuracy of its own bound
    v = got[:, 8:].astype(np.float64)
    assert (np.abs((v * v).sum(1) - 1.0) <= 2.0 * (np.abs(v) * re_.e[:, 8:]).sum(1) + (re_.e[:, 8:] ** 2).sum(1)).all()


# ---- sample_coarse -----------------------------------------------------------------------------------------------------------------
def coarse_n(S):
    return (R.N_SAMPLE_RAYS,) if S != 64 else (1, 257, R.N_SAMPLE_RAYS)


@pytest.mark.parametrize('lindisp', [False, True], ids=['lin', 'lindisp'])
@pytest.mark.parametrize('S', R.COARSE_S)
def test_sample_coarse(fn, S, lindisp):
    for n in coarse_n(S):
        near, far, u = R.coarse_inputs(n, S)
        assert (near > 0).all() and (u == 0).any() and (n * S < 20 or (u == R.ONE_BELOW).any()) and (u < 1).all()
        rays = G(R.rays11_of(near, far))
        for t in (None, u):
            z, t_t = padded(n * S), None if t is None else G(t)
            call(fn, 'fastnerf_sample_coarse', n, S, p(rays), int(lindisp), int(t is not None), p(t_t), 0, p(z))
            got = taken(z, n, S)
            re_, emu = R.both(R.sample_coarse, near, far, S, lindisp, t)
            hold('sample_coarse n=%d S=%d lindisp=%d jitter=%d' % (n, S, lindisp, t is not None), got, re_, emu)
            assert (np.diff(got, axis=1) >= 0).all()
            assert (got >= near[:, None]).all() and (got <= far[:, None]).all()


# ---- pp_intersect_sphere -----------------------------------------------------------------------------------------------------------
def run_sphere(fn, rays):
    n = len(rays)
    far = padded(n)
    cnt = torch.full((1 + PAD,), 12345, dtype=torch.int32, device='cuda')       # the library zeroes the counter itself
    rays_t = G(rays)
    call(fn, 'fastnerf_pp_intersect_sphere', n, p(rays_t), p(far), cnt.data_ptr())
    assert bool((cnt[1:] == 12345).all())
    return taken(far, n), int(cnt[0].item())


@pytest.mark.parametrize('n', RAY_SIZES)
def test_pp_intersect_sphere_inside(fn, n):
    rays, _ = R.sphere_inputs(n)
    (far_re, pn2_re), (far_emu, pn2_emu) = R.both(R.intersect_sphere, rays)
    assert (pn2_emu < 1).all() and (n < 1000 or pn2_re.v.max() > 1 - 1e-5)
    got, count = run_sphere(fn, rays)
    hold('pp_intersect_sphere inside n=%d' % n, got, far_re, far_emu)
    assert count == 0 and np.isfinite(got).all()


@pytest.mark.parametrize('n', RAY_SIZES[1:])
def test_pp_intersect_sphere_counts_rays_on_and_beyond_the_sphere(fn, n):
    """`planted` rays have pn2 >= 1 in the fp32 evaluation, among them o = (1,0,0), d = (0,1,0) with pn2 == 1.0f exactly (counted,
    and fg_far finite: sqrt(0)); at the large size they sit in 513 different blocks of both trips of the grid-stride loop."""
    rays, planted = R.sphere_inputs(n, outside=True)
    (far_re, _), (far_emu, pn2) = R.both(R.intersect_sphere, rays)
    assert int((pn2 >= 1).sum()) == planted and int((pn2 == 1).sum()) >= 3 and planted >= 9
    assert np.array_equal(rays[5, :6], np.array([1, 0, 0, 0, 1, 0], dtype=F32)) and pn2[5] == 1.0
    got, count = run_sphere(fn, rays)
    hold('pp_intersect_sphere outside n=%d' % n, got, far_re, far_emu)
    assert count == planted
    assert np.array_equal(np.isnan(got), pn2 > 1)
    with pytest.raises(Exception, match='unit sphere'):
        fn.ops.pp_intersect_sphere(G(rays))
    assert fn.ops.pp_intersect_sphere(G(rays), check_inside=False).shape == (n,)


# ---- pp_fg_depths, pp_perturb_samples ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', R.FG_S)
def test_pp_fg_depths(fn, S):
    for n in coarse_n(S):
        far, u = R.fg_inputs(n, S)
        for t in (None, u):
            z, far_t, t_t = padded(n * S), G(far), None if t is None else G(t)
            call(fn, 'fastnerf_pp_fg_depths', n, S, R.FG_NEAR, p(far_t), int(t is not None), p(t_t), 0, p(z))
            got = taken(z, n, S)
            re_, emu = R.both(R.fg_depths, far, R.FG_NEAR, S, t)
            hold('pp_fg_depths n=%d S=%d jitter=%d' % (n, S, t is not None), got, re_, emu)
            assert (got[:, 0] >= F32(R.FG_NEAR)).all() and (np.diff(got, axis=1) >= 0).all()


@pytest.mark.parametrize('S', (1,) + R.FG_S)
def test_pp_perturb_samples(fn, S):
    for n in coarse_n(S):
        zin, u = R.perturb_inputs(n, S)
        z, zin_t, u_t = padded(n * S), G(zin), G(u)
        call(fn, 'fastnerf_pp_perturb_samples', n, S, p(zin_t), p(u_t), 0, p(z))
        got = taken(z, n, S)
        re_, emu = R.both(R.perturb_samples, zin, u)
        hold('pp_perturb_samples n=%d S=%d' % (n, S), got, re_, emu)
        assert (got[:, 0] >= zin[:, 0]).all() and (np.diff(got, axis=1) >= 0).all()
        if S == 1:
            assert bit_equal(got, zin)


# ---- posenc ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', sorted(R.POSENC_BIG))
def test_posenc(fn, L):
    C = 3 + 6 * L
    for n in (1, 257, R.POSENC_BIG[L]):
        x = R.posenc_inputs(n)
        out, x_t = padded(n * C), G(x)
        call(fn, 'fastnerf_posenc', n, L, p(x_t), p(out))
        got = taken(out, n, C)
        ref = R.posenc_ref(x, L)
        assert bit_equal(got[:, :3], x)
        err = np.abs(got[:, 3:] - ref[:, 3:])
        print('POSENC L=%d n=%d: max |got - float64 sin / cos| = %.3f u over %d channels' % (L, n, float(err.max()) / R.U, err.size))
        assert float(err.max()) <= POSENC_TOL


# ---- pp_gen_rays -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(6, 8), R.IMG_BIG], ids=lambda s: '%dx%d' % s)
def test_pp_gen_rays(fn, size):
    H, W = size
    K, M = R.pp_camera()
    K, M = np.ascontiguousarray(K), np.ascontiguousarray(M)
    ro, rd = padded(H * W * 3), padded(H * W * 3)
    call(fn, 'fastnerf_pp_gen_rays', H, W, K.ctypes.data, M.ctypes.data, p(ro), p(rd))
    o, d = taken(ro, H * W, 3), taken(rd, H * W, 3)
    v, bound, origin = R.pp_gen_rays_ref(H, W, K, M)
    worst = float((np.abs(d - v) / bound).max())
    print('RATIO pp_gen_rays %dx%d: max |got - v| / bound = %.3f, bit-equal to the fp64 route rounded once: %s' % (
        H, W, worst, bit_equal(d, R.pp_gen_rays_emu(H, W, K, M))))
    assert worst <= 1.0
    assert bit_equal(o, np.broadcast_to(origin, (H * W, 3)))


# ---- the wrappers refuse what the library would misread ----------------------------------------------------------------------------
def wrapper_calls(fn):
    n, S = 7, 5
    rays = torch.zeros(n, 11, device='cuda')
    rays[:, 3:6], rays[:, 6], rays[:, 7] = 1.0, 2.0, 6.0
    far = torch.ones(n, device='cuda')
    z = torch.linspace(2, 6, S, device='cuda').expand(n, S).contiguous()
    raw = torch.zeros(n, S, 4, device='cuda')
    ops = fn.ops
    return {
        'sample_coarse': (lambda rays11=rays: ops.sample_coarse(rays11, S), dict(rays11=((n, 11), (n, 12)))),
        'pp_intersect_sphere': (lambda rays11=rays * 0.1: ops.pp_intersect_sphere(rays11), dict(rays11=((n, 11), (n, 12)))),
        'pp_fg_depths': (lambda fg_far=far: ops.pp_fg_depths(fg_far, S, perturb=False), dict(fg_far=((n,), (n, 1)))),
        'raw2outputs_fwd': (lambda raw=raw, z=z, rays11=rays: ops.raw2outputs_fwd(raw, z, rays11),
                            dict(raw=((n, S, 4), (n, S, 5)), z=((n, S), (n, S - 1)), rays11=((n, 11), (n, 12)))),
    }


@pytest.mark.parametrize('name', ['sample_coarse', 'pp_intersect_sphere', 'pp_fg_depths', 'raw2outputs_fwd'])
def test_wrappers_refuse_float64_and_wrong_shapes(fn, name):
    """A float64 tensor of the right shape (twice the bytes the kernel would read) and an fp32 tensor with a wrong trailing size
    (chosen so that nothing could be read beyond a buffer) raise in Python, before any launch."""
    f, args = wrapper_calls(fn)[name]
    f()                                                              # the good call passes
    for arg, (shape, wrong_shape) in args.items():
        with pytest.raises(TypeError, match=arg):
            f(**{arg: torch.ones(*shape, device='cuda', dtype=torch.float64)})
        with pytest.raises(ValueError):
            f(**{arg: torch.ones(*wrong_shape, device='cuda')})


def test_wrappers_keep_converted_inputs_alive(fn):
    """Two inputs that both need a conversion to fp32: each conversion is a new tensor, and the second must not land in the block
    of the first (ops._f32).  float64 inputs give the bits of their fp32 roundings."""
    gen = torch.Generator().manual_seed(3)
    n, S = 33, 16
    ro = ((torch.rand(n, 3, generator=gen) - 0.5) * 0.8).cuda()
    rd = torch.randn(n, 3, generator=gen).cuda()
    dep = torch.sort(torch.rand(n, S, generator=gen) * 0.98 + 0.01, -1).values.cuda()
    want = fn.ops.pp_depth2pts_outside(ro, rd, dep)
    got = fn.ops.pp_depth2pts_outside(ro.double(), rd.double(), dep)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    bins = torch.sort(torch.rand(n, S, generator=gen), -1).values.cuda()
    w = (torch.rand(n, S - 1, generator=gen) + 0.1).cuda()
    u = torch.rand(n, 24, generator=gen).cuda()
    for f in (fn.ops.pp_sample_pdf, fn.ops.sample_pdf):
        assert torch.equal(f(bins.double(), w.double(), 24, u=u), f(bins, w, 24, u=u))
