"""Training with a pose table: Trainer(poses=table).step(None, None, target, pix=pix) in the math modes fp32 and bf16x6.

Setting: a 24 x 24 synthetic set (synthetic.make_dataset), 67 rays over 3 images of which image 1 has none, N_samples = N_importance
= 16, perturb = 0, two freshly initialised networks with the density head lifted (tests/test_gpu_ray_grad.py: most samples live).
(i)   the network gradients, the parameters after the step, the loss and the maps are bit-identical to a trainer without poses=
      stepping call by call (FASTNERF_FUSED_STEP=0, FASTNERF_COMPACT=0) on the rays the table's poses generate;
(ii)  trainer.pose_grad against float64 autograd of the step's loss with respect to xi -- torch.matrix_exp on the base pose, the
      oracle's rays and render_rays -- by the rule of tests/test_gpu_ray_grad.py::test_render_pose_gradient: relative L2 error of the
      omega and the tau block <= FACTOR x the error of the same oracle in float32 (poses and rays are float32 in both, as there);
(iii) xi after the step is ops.adam_step applied by hand to zeros and trainer.pose_grad, bit for bit; the image without rays has a
      zero gradient and keeps xi = 0;
(iv)  every refusal, with the trainer's state untouched;
(v)   behaviour: a field fitted to 24 views for 500 steps, then frozen (lrate = 0); all poses perturbed by 1 degree / 0.02; after 100 pose steps
      the gauge-free rotation and translation errors are below their starting values (printed; recorded in profiles/pose_train.md).
      A sign or index error in any of the three kernels makes them grow;
(vi)  a checkpoint round trip restores xi and its moments; a checkpoint without a table leaves the table alone."""
import os

import numpy as np
import pytest
import torch

import pose_ref as P
import test_gpu_ray_grad as RG
import test_ray_grad_cpu as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

H = W = 24
N_S = N_I = 16
N_RAYS = 67


@pytest.fixture(scope='module')
def fn():
    import fastnerf
    return fastnerf


@pytest.fixture(params=['fp32', 'bf16x6'])
def mode(request, fn):
    old = fn.ops.get_math()
    fn.ops.set_math(request.param)
    yield request.param
    fn.ops.set_math(old)


_DATA = {}


def data(fn, n_images=3):
    if n_images not in _DATA:
        images, poses, focal = fn.synthetic.make_dataset(n_images=n_images, H=H, W=W)
        K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
        _DATA[n_images] = (images.float().cuda(), poses.float().cuda(), K)
    return _DATA[n_images]


def batch(fn):
    """67 pixels of images 0 and 2 and their colours."""
    images, poses, K = data(fn)
    gen = torch.Generator().manual_seed(4)
    pix = torch.stack([torch.randint(0, 2, (N_RAYS,), generator=gen) * 2, torch.randint(0, H, (N_RAYS,), generator=gen),
                       torch.randint(0, W, (N_RAYS,), generator=gen)], 1).int().cuda()
    p = pix.long()
    return pix, images[p[:, 0], p[:, 1], p[:, 2]].contiguous()


def new_trainer(fn, poses=None, lift=True, **kw):
    """Two networks from seed 0 (the same parameters in every trainer), density head lifted by 0.3."""
    images, base, K = data(fn)
    args = fn.run_nerf.make_args(N_importance=N_I, N_samples=N_S, perturb=0., white_bkgd=True, no_reload=True)
    torch.manual_seed(0)
    ktr = fn.run_nerf.create_nerf(args, device='cuda')[0]
    if lift:
        with torch.no_grad():
            ktr['network_fn'].alpha_linear.bias.add_(0.3)
            ktr['network_fine'].alpha_linear.bias.add_(0.3)
    kw.setdefault('kw_update', {})
    ktr.update(kw.pop('kw_update'))
    table = None
    if poses is not None:
        table = fn.poses.PoseTable(poses).cuda()
    return fn.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, poses=table, **kw), ktr


@pytest.fixture
def call_by_call(fn, monkeypatch):
    monkeypatch.setenv('FASTNERF_FUSED_STEP', '0')
    old = fn.render.get_compact()
    fn.render.set_compact('0')
    yield
    fn.render.set_compact(old)


def oracle_pose_grad(sd_c, sd_f, base, pix, K, target, dtype):
    """d(mse(fine) + mse(coarse))/d(xi) at xi = 0; the poses and the rays are float32 (the rays the kernels see), the rendering `dtype`."""
    xi = torch.zeros(base.shape[0], 6, requires_grad=True)
    poses = torch.cat([torch.matrix_exp(P.hat(xi[:, :3])) @ base[:, :, :3], base[:, :, 3:] + xi[:, 3:, None]], -1)
    dirs = P.dirs_of(pix, K, torch.float32)
    c2w = poses[pix[:, 0].long()]
    rd = torch.sum(dirs[:, None, :] * c2w[:, :, :3], -1)
    rb = O.make_ray_batch(c2w[:, :, 3], rd, 2.0, 6.0).to(dtype)
    ret = O.render_rays(rb, sd_c, sd_f, N_S, N_I, white_bkgd=True)
    loss = O.img2mse(ret['rgb_map'], target.to(dtype)) + O.img2mse(ret['rgb0'], target.to(dtype))
    return torch.autograd.grad(loss, xi)[0]


_ORACLE = {}


def test_pose_step_gradients(fn, mode, call_by_call):
    """(i), (ii), (iii) on one step."""
    images, base, K = data(fn)
    pix, target = batch(fn)
    a, ktr = new_trainer(fn, poses=base, pose_lrate=1e-3)
    b, _ = new_trainer(fn)
    assert not b.fused and torch.equal(a.flat, b.flat)
    if 'ref' not in _ORACLE:
        sds = [[RG.state(ktr[k], dt) for k in ('network_fn', 'network_fine')] for dt in (torch.float64, torch.float32)]
        _ORACLE['ref'] = [oracle_pose_grad(sd[0], sd[1], base.cpu(), pix.cpu(), K, target.cpu(), dt).double()
                          for sd, dt in zip(sds, (torch.float64, torch.float32))]
    ref64, ref32 = _ORACLE['ref']
    poses = a.poses.poses()
    assert np.array_equal(poses.cpu().numpy().view(np.uint32), base.cpu().numpy().view(np.uint32))
    ro, rd = fn.ops.gen_rays_pixels(pix, poses, K)
    loss_a, out_a = a.step(None, None, target, pix=pix)
    loss_b, out_b = b.step(ro, rd, target)
    # (i)
    assert torch.equal(loss_a, loss_b)
    for k in out_b:
        if torch.is_tensor(out_b[k]):
            assert torch.equal(out_a[k], out_b[k]), k
    assert torch.equal(a.grad, b.grad) and float(a.grad.abs().max()) > 0
    assert torch.equal(a.flat, b.flat) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    assert out_a['d_rays'].shape == (N_RAYS, 11) and (out_a['d_rays'][:, 6:8] == 0).all()
    # (ii)
    got = a.pose_grad.cpu().double()
    assert got.shape == (3, 6) and torch.isfinite(got).all() and (got[1] == 0).all() and (ref64[1] == 0).all()
    for name, sl in (('omega', slice(0, 3)), ('tau', slice(3, 6))):
        err, e32 = R.rel_l2(got[:, sl], ref64[:, sl]), R.rel_l2(ref32[:, sl], ref64[:, sl])
        print('\npose step %-6s %-5s err %.3e  E32 %.3e  bound %.3e' % (mode, name, err, e32, RG.FACTOR * e32))
        assert err <= RG.FACTOR * e32, (name, err, e32)
    # (iii)
    xi, m, v = torch.zeros(3, 6, device='cuda'), torch.zeros(3, 6, device='cuda'), torch.zeros(3, 6, device='cuda')
    fn.ops.adam_step(xi, a.pose_grad, m, v, 1e-3, 1, a.beta1, a.beta2, a.eps)
    assert torch.equal(a.poses.xi.data, xi) and torch.equal(a.pose_m, m) and torch.equal(a.pose_v, v)
    assert (a.poses.xi.data[1] == 0).all() and float(a.poses.xi.data[[0, 2]].abs().min()) > 0
    assert a.adam_t == 1 and a.global_iter == 1


def test_pose_step_takes_the_other_terms(fn, mode, call_by_call):
    """Depth / opacity, background, distortion, the leaf table and a batch of one image alone pass through: the networks' gradients
    stay those of the call-by-call step with the same keywords."""
    images, base, K = data(fn)
    pix, target = batch(fn)
    kw = dict(lambda_depth=0.1, lambda_acc=0.1, lambda_dist=0.01, bkgd=(0.2, 0.4, 0.6), kw_update={'white_bkgd': False})
    a, _ = new_trainer(fn, poses=base, **dict(kw, kw_update=dict(kw['kw_update'])))
    b, _ = new_trainer(fn, **dict(kw, kw_update=dict(kw['kw_update'])))
    gen = torch.Generator().manual_seed(6)
    step_kw = dict(depth=(torch.rand(N_RAYS, generator=gen) * 4 + 2).cuda(), acc=torch.rand(N_RAYS, generator=gen).cuda(),
                   alpha=torch.rand(N_RAYS, generator=gen).cuda(), leaf_tag=torch.stack([pix[:, 0], pix[:, 1] % 4], 1).int().contiguous(),
                   max_leaves=4)
    ta, tb = torch.zeros(12, device='cuda', dtype=torch.int32), torch.zeros(12, device='cuda', dtype=torch.int32)
    ro, rd = fn.ops.gen_rays_pixels(pix, base, K)
    a.step(None, None, target, pix=pix, table=ta, **step_kw)
    b.step(ro, rd, target, table=tb, **step_kw)
    assert torch.equal(a.grad, b.grad) and torch.equal(ta, tb) and torch.equal(a.aux_losses, b.aux_losses)
    assert torch.equal(a.dist_losses, b.dist_losses) and torch.isfinite(a.pose_grad).all() and float(a.pose_grad.abs().max()) > 0


def test_refusals(fn, monkeypatch):
    images, base, K = data(fn)
    pix, target = batch(fn)
    ro, rd = fn.ops.gen_rays_pixels(pix, base, K)
    a, ktr = new_trainer(fn, poses=base)
    b, _ = new_trainer(fn)
    with pytest.raises(ValueError, match='poses='):
        b.step(None, None, target, pix=pix)
    with pytest.raises(ValueError, match='pix='):
        a.step(ro, rd, target)
    with pytest.raises(ValueError, match='not both'):
        a.step(ro, rd, target, pix=pix)
    with pytest.raises(ValueError, match='integer'):
        a.step(None, None, target, pix=pix.float())
    grid = fn.occupancy.OccupancyGrid.for_training(N=16, bound=1.5, outside_occupied=False, device='cuda')
    for bad in (dict(occupancy=grid), dict(occupancy=grid, tighten=True), dict(tighten=True), dict(occupancy=grid, march=16)):
        with pytest.raises(ValueError, match='occupancy'):
            new_trainer(fn, poses=base, **bad)
    with pytest.raises(NotImplementedError, match='ndc'):
        new_trainer(fn, poses=base, kw_update={'ndc': True})
    old = fn.ops.get_math()
    try:
        fn.ops.set_math('bf16x3')
        with pytest.raises(NotImplementedError, match='bf16x3'):
            new_trainer(fn, poses=base)
        with pytest.raises(NotImplementedError, match='bf16x3'):
            a.step(None, None, target, pix=pix)
    finally:
        fn.ops.set_math(old)
    monkeypatch.setattr(fn.parallel, 'world_size', lambda: 2)
    with pytest.raises(ValueError, match='data parallel'):
        new_trainer(fn, poses=base)
    monkeypatch.undo()
    # nothing was stepped
    assert a.adam_t == 0 and b.adam_t == 0 and (a.poses.xi.data == 0).all() and a.pose_grad is None


def test_pose_steps_pull_perturbed_poses_back(fn, mode):
    """(v).  The field is fitted with the true poses and then frozen; the table starts 1 degree / 0.02 off in every image.
    At 24 x 24 pixels (focal length 33 pixels, cameras 4 from the scene) these perturbations are 0.6 and 0.17 of a pixel: the field has
    to place its surfaces to a fraction of a pixel for the poses to come back, which is what the choices left to this test are for --
    24 views (13824 pixels; with 8 the geometry between the views is too loose and the pair distances stall), 500 fitting steps of
    4096 rays with the rate falling tenfold so that the fit settles, and 2048 rays per pose step (85 per image).  Measured on an MI355X
    (fp32 / bf16x6): rotation 1.356 -> 0.661 / 0.699 degrees, pair distances 0.0135 -> 0.0104 / 0.0104; in the runs that chose this
    set-up both errors fell at every 25th step, and other perturbation seeds, all pixels per step and an annealed rate gave the same
    picture (profiles/pose_train.md)."""
    n_img, n_fit, fit_rays, n_pose, n_rays = 24, 500, 4096, 100, 2048
    images, truth, K = data(fn, n_img)
    gen = torch.Generator().manual_seed(11)

    def draw(n):
        pix = torch.stack([torch.randint(0, n_img, (n,), generator=gen), torch.randint(0, H, (n,), generator=gen),
                           torch.randint(0, W, (n,), generator=gen)], 1).int().cuda()
        p = pix.long()
        return pix, images[p[:, 0], p[:, 1], p[:, 2]].contiguous()
    args = fn.run_nerf.make_args(N_importance=N_I, N_samples=N_S, perturb=1., white_bkgd=True, no_reload=True)
    torch.manual_seed(0)
    ktr = fn.run_nerf.create_nerf(args, device='cuda')[0]
    fit = fn.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, lrate=1e-3, lrate_decay=n_fit / 1000.0)
    for _ in range(n_fit):
        pix, tgt = draw(fit_rays)
        loss2, _ = fit.step(*fn.ops.gen_rays_pixels(pix, truth, K), tgt)
    table = fn.poses.PoseTable(fn.poses.perturbed(truth, 1.0, 0.02, seed=3)).cuda()
    start = fn.poses.gauge_free_errors(table.poses(), truth)
    tr = fn.run_nerf.Trainer(ktr, H, W, K, 2.0, 6.0, lrate=0., poses=table, pose_lrate=1e-3)
    flat = tr.flat.clone()
    for _ in range(n_pose):
        pix, tgt = draw(n_rays)
        tr.step(None, None, tgt, pix=pix)
    end = fn.poses.gauge_free_errors(table.poses(), truth)
    print('\npose refinement %-6s fit mse %.4f | rotation %.3f -> %.3f degrees, translation %.4f -> %.4f'
          % (mode, float(loss2[0]), start[0], end[0], start[1], end[1]))
    assert torch.equal(tr.flat, flat)      # lrate = 0: the field stayed frozen
    assert end[0] < start[0] and end[1] < start[1], (start, end)


@pytest.mark.parametrize('compat_rng', [False, True], ids=['device_rays', 'host_rays'])
def test_train_driver_refines_poses(fn, monkeypatch, tmp_path, compat_rng):
    """run_nerf.train(args.refine_poses): the warm-up and every epoch step on the rows' own pixels instead of rays, the table is
    trainer.poses, the return value is what it was, and the checkpoint carries the table."""
    imgs, poses, focal = fn.synthetic.make_dataset(n_images=3, H=32, W=32)
    seen = []
    step = fn.run_nerf.Trainer.step

    def spy(self, rays_o, rays_d, target, *a, **kw):
        seen.append((rays_o, rays_d, target.clone(), kw['pix'].clone()))
        return step(self, rays_o, rays_d, target, *a, **kw)
    monkeypatch.setattr(fn.run_nerf.Trainer, 'step', spy)
    torch.manual_seed(0)
    np.random.seed(0)
    args = fn.run_nerf.make_args(N_importance=16, N_samples=16, perturb=1.0, white_bkgd=True, no_reload=True, N_rand=256, n_epoch=2,
                                 init_level=2, subdivide_every=1, subdivide_thres=0.05, lrate=5e-4, lrate_decay=500, refine_poses=True,
                                 pose_lrate=2e-3, save_ckpt=True, basedir=str(tmp_path), expname='refine')
    ret = fn.run_nerf.train(imgs, poses, 32, 32, focal, args, log=lambda s: None, compat_rng=compat_rng, max_iters_per_epoch=3)
    torch.cuda.synchronize()
    assert len(ret) == 5
    trainer, hist = ret[2], ret[4]
    table = trainer.poses
    assert isinstance(table, fn.poses.PoseTable) and trainer.pose_lrate == 2e-3 and torch.equal(table.base.cpu(), poses.float())
    assert len(hist) == 2 and all(np.isfinite(h[2]) for h in hist) and len(seen) >= 7
    images = imgs.float().cuda()
    for rays_o, rays_d, target, pix in seen:
        assert rays_o is None and rays_d is None and pix.dtype == torch.int32 and pix.shape == (target.shape[0], 3)
        p = pix.long()
        assert torch.equal(target, images[p[:, 0], p[:, 1], p[:, 2]]), 'the colours of the rows\' own pixels'
    assert torch.isfinite(table.xi).all() and float(table.xi.data.abs().max()) > 0 and trainer.pose_grad.shape == (3, 6)
    ckpt = torch.load(os.path.join(str(tmp_path), 'refine', '002.tar'), map_location='cuda', weights_only=False)
    assert torch.equal(ckpt['pose_xi'], table.xi.data) and torch.equal(ckpt['pose_m'], trainer.pose_m)


class _NoTrees:
    def save_trees(self, path):
        pass


def test_checkpoint_round_trip(fn, tmp_path):
    images, base, K = data(fn)
    pix, target = batch(fn)
    a, ktr = new_trainer(fn, poses=base)
    for _ in range(2):
        a.step(None, None, target, pix=pix)
    args = fn.run_nerf.make_args(basedir=str(tmp_path), expname='pose')
    path = fn.run_nerf.save_checkpoint(args, 1, a, ktr, _NoTrees())
    ckpt = torch.load(path, map_location='cuda', weights_only=False)
    assert torch.equal(ckpt['pose_xi'], a.poses.xi.data) and torch.equal(ckpt['pose_base'], base)
    c, _ = new_trainer(fn, poses=base)
    assert c.load_pose_checkpoint(path)
    assert torch.equal(c.poses.xi.data, a.poses.xi.data) and torch.equal(c.pose_m, a.pose_m) and torch.equal(c.pose_v, a.pose_v)
    assert float(c.pose_m.abs().max()) > 0
    # the trainer's own state: moments of the networks and of the table
    d, _ = new_trainer(fn, poses=base)
    sd = a.state_dict()
    assert 'pose_m' in sd and 'pose_v' in sd
    d.load_state_dict(sd)
    assert torch.equal(d.pose_m, a.pose_m) and torch.equal(d.pose_v, a.pose_v) and torch.equal(d.m, a.m)
    # a checkpoint without a table loads with the table untouched; one for other base poses is refused
    b, kb = new_trainer(fn)
    assert 'pose_m' not in b.state_dict()
    plain = fn.run_nerf.save_checkpoint(fn.run_nerf.make_args(basedir=str(tmp_path), expname='plain'), 1, b, kb, _NoTrees())
    assert 'pose_xi' not in torch.load(plain, map_location='cuda', weights_only=False)
    xi = c.poses.xi.data.clone()
    assert not c.load_pose_checkpoint(plain) and torch.equal(c.poses.xi.data, xi)
    e, _ = new_trainer(fn, poses=fn.poses.perturbed(base, 1.0, 0.02))
    with pytest.raises(ValueError, match='base poses'):
        e.load_pose_checkpoint(path)
