"""The N>1 path of bench.py end to end on the GPU: two ranks under the contract's launcher command (torch.distributed.run, 127.0.0.1
rendezvous) AND from the bare `python bench.py --gpus N` (which re-executes itself under that launcher), sharded rays, gradient all-reduce, barrier-bracketed timing, rank-0 JSON.  On a 1-GPU box the two
ranks share the device and the collective backend is gloo (FASTNERF_DIST_BACKEND); on a multi-GPU box this is RCCL."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(backend, port, scaling, full_out, launcher=True):
    """launcher=True: under torch.distributed.run, the contract's N>1 command; False: the BARE `python bench.py --gpus 2 ...` (the way the
    N=1 command is started) -- bench.py must re-execute itself under the launcher instead of asserting on WORLD_SIZE."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    if backend:
        env['FASTNERF_DIST_BACKEND'] = backend
    args = ['--gpus', '2', '--steps', '3', '--warmup', '1', '--full', '--sustained-steps', '5', '--scaling', scaling, '--full-out', full_out]
    if launcher:
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
               '--master-port', str(port), os.path.join(ROOT, 'bench.py')] + args
    else:
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py')] + args
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)


def _headline(stdout):
    """Exactly ONE JSON line on stdout, from rank 0, and it is the LAST line (<= 4 KB).  (Over gloo -- 1-GPU boxes only -- every rank's
    transport prints a '[Gloo] Rank r is connected to ...' line on stdout when the group forms: before the headline, not JSON.)"""
    lines = [l for l in stdout.splitlines() if l.strip()]
    assert sum(l.lstrip().startswith('{') for l in lines) == 1 and lines[-1].startswith('{"metric"'), stdout[-2000:]
    # (eight ranks write those lines in pieces into one pipe: the pieces interleave, so the check is on the vocabulary, not on line starts)
    import re
    rest = re.sub(r'\[Gloo\]|Rank|is|connected|to|peer|ranks|Expected|number|of|[\d\s.:]', '', ' '.join(lines[:-1]))
    assert rest == '', lines[:-1]
    assert len(lines[-1]) <= 4096
    return json.loads(lines[-1])


@pytest.mark.parametrize('scaling,launcher', [('weak', True), ('strong', True), ('weak', False)])
def test_bench_two_ranks(scaling, launcher, tmp_path):
    # two or more GPUs: the collective MUST be RCCL over xGMI -- a failure there is a failure (no gloo retry);
    # a 1-GPU box can only exercise the plumbing (both ranks on one device, gloo)
    port = 29533 if scaling == 'weak' else 29535
    full_out = str(tmp_path / 'full.json')
    out = _run(None if torch.cuda.device_count() >= 2 else 'gloo', port, scaling, full_out, launcher)
    assert out.returncode == 0, out.stderr[-2000:]
    j = _headline(out.stdout)
    full = json.load(open(full_out))
    assert full['value'] == j['value'] and full['sustained']['steps'] == 5 and j['sustained_ms_per_step'] > 0
    assert j['n_gpus'] == 2 and j['steps'] == 3 and j['scaling'] == scaling and j['value'] > 0 and j['dtype'] == 'f32'
    per_gpu = 4096 if scaling == 'weak' else 2048        # weak: per-GPU work fixed; strong: 4096 rays per step split over the ranks
    assert j['config']['parallelism'] == 'dp2' and j['config']['rays_per_gpu_per_step'] == per_gpu and j['cpu_baseline'] is None
    assert abs(j['value'] - 2 * per_gpu * 3 / (j['ms_per_step'] * 3e-3)) < 1e-6 * j['value']
    assert all(abs(x) < 1.0 for x in j['final_loss'])
    assert len(j['per_rank_ms_per_step']) == 2 and all(x > 0 for x in j['per_rank_ms_per_step'])
    ar = j['allreduce_ms']
    assert ar['fine_half'] > 0 and ar['coarse_half'] > 0 and ar['whole_buffer'] > 0 and ar['overlapped_with_coarse_backward'] is True
    assert j['roofline']['frac'] > 0 and j['roofline']['bound'] == 'mfma'
    assert j['psnr'] is None and j['siblings'] is None and full['psnr_vs_cpu'] is None and full['drop_in_route'] is None  # 1-GPU legs


@pytest.mark.parametrize('scaling', ['strong', 'both'])
def test_bench_eight_ranks_on_what_the_box_has(scaling, tmp_path):
    """Multi-GPU readiness: the BARE `python bench.py --gpus 8 ...` (no launcher: bench.py re-executes itself under
    torch.distributed.run; a harness that starts N=8 the way it starts N=1 must not die on an assert).  Needs 8 GPUs: eight ranks
    on fewer devices, plus this process, are more processes on one GPU than a shared box allows, so the test skips there.  (If the
    ranks did share devices, the collectives would run over gloo and FASTNERF_COLLECTIVE=cabi would have to fall back LOUDLY, since
    RCCL cannot put two ranks of a communicator on one device: the `shared` branch below states that contract, unreached while the test
    needs 8 GPUs.)  No scaling number is claimed from this."""
    if torch.cuda.device_count() < 8:
        pytest.skip('needs 8 GPUs, found %d' % torch.cuda.device_count())
    env = dict(os.environ, FASTNERF_COLLECTIVE='cabi')
    shared = torch.cuda.device_count() < 8
    if torch.cuda.is_initialized():
        torch.cuda.empty_cache()       # eight ranks of 4096 rays need ~20 GB each on the shared device: give back this process's cached blocks
    if shared:
        env['FASTNERF_DIST_BACKEND'] = 'gloo'
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    # 'both' is what the bare driver command gets with --full (--scaling auto -> both on several GPUs): `value` is the weak leg, both curves'
    # points ride along
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '8', '--steps', '2', '--warmup', '1', '--full', '--sustained-steps', '0',
           '--full-out', os.path.join(str(tmp_path), 'full.json')] + (['--scaling', scaling] if scaling != 'both' else [])
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    j = _headline(out.stdout)
    per_gpu = 512 if scaling == 'strong' else 4096
    assert j['n_gpus'] == 8 and j['scaling'] == ('strong' if scaling == 'strong' else 'weak') and j['config']['parallelism'] == 'dp8'
    if scaling == 'both':
        w, st = j['scaling_weak'], j['scaling_strong']
        assert w['value'] == j['value'] and w['rays_per_gpu_per_step'] == 4096 and w['rays_per_step'] == 8 * 4096
        assert st['rays_per_gpu_per_step'] == 512 and st['rays_per_step'] == 4096 and st['value'] > 0
        assert abs(st['value'] - 4096 * 2 / (st['ms_per_step'] * 2e-3)) < 1e-6 * st['value']
    else:
        assert 'scaling_weak' not in j and 'scaling_strong' not in j
    assert j['config']['rays_per_gpu_per_step'] == per_gpu and j['config']['rays_per_step'] == 8 * per_gpu
    assert len(j['per_rank_ms_per_step']) == 8 and all(x > 0 for x in j['per_rank_ms_per_step'])
    assert abs(j['value'] - 8 * per_gpu * 2 / (j['ms_per_step'] * 2e-3)) < 1e-6 * j['value']
    assert j['ms_per_step'] >= max(j['per_rank_ms_per_step']) * 0.999          # MAX over ranks
    ar = j['allreduce_ms']
    assert ar['fine_half'] > 0 and ar['coarse_half'] > 0 and ar['whole_buffer'] > 0
    assert all(abs(x) < 1.0 for x in j['final_loss']) and j['cpu_baseline'] is None
    if shared:
        assert 'NOT honoured' in j['collective'] and 'share' in j['collective'] and j['collective'].startswith('torch.distributed/gloo')
        assert out.stderr.count('FASTNERF_COLLECTIVE=cabi requested but') == 8      # every rank said so
    else:
        assert j['collective'].startswith('cabi')


_SHARD_WORKER = r"""
import os, sys, json
import numpy as np, torch
sys.path.insert(0, %(root)r)
import fastnerf
from fastnerf import parallel
rank, world, local = parallel.init_from_env('cuda')
torch.cuda.set_device(0 if torch.cuda.device_count() < world else local)
torch.manual_seed(0)
if rank == 1 and os.environ.get('COMPACT_RANK1'):          # ranks that DISAGREE on compacted / plain backward
    fastnerf.render.set_compact(os.environ['COMPACT_RANK1'])
args = fastnerf.run_nerf.make_args(N_importance=32, N_samples=32, perturb=1.0, white_bkgd=True, no_reload=True, lrate=5e-4, lrate_decay=500)
ktr, _, _, _, _, _ = fastnerf.run_nerf.create_nerf(args, device='cuda')
imgs, poses, focal = fastnerf.synthetic.make_dataset(n_images=2, H=32, W=32)
K = np.array([[focal, 0, 16.0], [0, focal, 16.0], [0, 0, 1]])
tr = fastnerf.run_nerf.Trainer(ktr, 32, 32, K, 2.0, 6.0, lrate=5e-4, lrate_decay=500)
gen = torch.Generator().manual_seed(5)          # the same global batches on every rank
rays = [fastnerf.run_nerf_helpers.get_rays(32, 32, K, poses[i]) for i in range(2)]
ro = torch.cat([r[0].reshape(-1, 3) for r in rays], 0); rd = torch.cat([r[1].reshape(-1, 3) for r in rays], 0)
tgt = imgs.reshape(-1, 3).cuda()
ml = 16
table = torch.zeros(2 * ml, device='cuda', dtype=torch.int32)
losses, lives = [], []
for it in range(4):
    N = (512, 512, 511, 1)[it]                  # a batch that does not divide evenly, then one whose shard is EMPTY on rank 1
    sel = torch.randint(0, ro.shape[0], (N,), generator=gen)
    t_rand, u = torch.rand(N, 32, generator=gen).cuda(), torch.rand(N, 32, generator=gen).cuda()
    tag = torch.stack([sel // 1024, ((sel %% 1024) // 32 // 8) * 4 + (sel %% 32) // 8], 1).int().cuda()
    sl = slice(rank, N, world)
    selc = sel.cuda()
    loss2, _ = tr.step(ro[selc][sl].contiguous(), rd[selc][sl].contiguous(), tgt[selc][sl].contiguous(), leaf_tag=tag[sl].contiguous(),
                       table=table, max_leaves=ml, t_rand=t_rand[sl].contiguous(), u=u[sl].contiguous(),
                       n_global=N if world > 1 else None)
    losses.append(loss2.cpu().tolist())
    lives.append(bool(tr.last_step_live))
    if it == 0:
        grad0 = tr.grad.clone()                 # after the all-reduce: the global-batch mean gradient of step 1
        table0 = table.clone()
        parallel.all_reduce_max_int(table0)     # the table of step 1: same weights on 1 and 2 ranks
parallel.all_reduce_max_int(table)
torch.cuda.synchronize()
if rank == 0:
    torch.save({'flat': tr.flat.cpu(), 'grad0': grad0.cpu(), 'table0': table0.cpu(), 'table': table.cpu(), 'losses': losses, 'lr': tr.lr, 'adam_t': tr.adam_t}, %(out)r %% world)
if world > 1:
    torch.save({'flat': tr.flat.cpu(), 'm': tr.m.cpu(), 'v': tr.v.cpu(), 'grad0': grad0.cpu(), 'live': lives, 'overlap': tr.overlap_allreduce},
               (%(out)r %% world) + '.rank%%d' %% rank)
if world > 1:
    parallel.barrier(); torch.distributed.destroy_process_group()
"""


@pytest.mark.parametrize('compact', ['0', '1'])
def test_sharded_trainer_equals_single_rank_on_the_union(tmp_path, compact):
    """Two ranks (gloo on a 1-GPU box, RCCL otherwise) each run Trainer.step on rows r::2 of the same global batches with
    n_global; after 3 steps the flat parameters match the 1-rank run on the union and the leaf table is bit-equal."""
    script = str(tmp_path / 'worker.py')
    out = str(tmp_path / 'res_%d.pt')
    with open(script, 'w') as f:
        f.write(_SHARD_WORKER % {'root': ROOT, 'out': out})
    env = dict(os.environ, FASTNERF_COMPACT=compact)
    r1 = subprocess.run([sys.executable, script], env=env, capture_output=True, text=True, timeout=600)
    assert r1.returncode == 0, r1.stderr[-3000:]
    env2 = dict(env)
    if torch.cuda.device_count() < 2:
        env2['FASTNERF_DIST_BACKEND'] = 'gloo'
    r2 = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
                         '127.0.0.1', '--master-port', '29541', script], env=env2, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr[-3000:]
    a, b = torch.load(out % 1), torch.load(out % 2)
    # leaf-error table of the first step (identical weights): MAX over float bit patterns is exact and order independent
    assert torch.equal(a['table0'], b['table0']) and int((a['table0'] != 0).sum()) > 8
    # after three steps the weights differ in their last bits (fp32 summation order of the gradients), the errors with them
    ta, tb = a['table'].view(torch.float32), b['table'].view(torch.float32)
    assert torch.equal(ta != 0, tb != 0) and (ta - tb).abs().max().item() < 1e-5
    assert a['adam_t'] == b['adam_t'] == 4 and a['lr'] == b['lr']   # the rank with the empty shard stepped too
    # step 1's all-reduced gradient == the single rank's gradient on the union batch (only fp32 summation order differs)
    relg = (a['grad0'] - b['grad0']).abs().max().item() / a['grad0'].abs().max().item()
    assert relg < 2e-6, relg
    # parameters after 3 Adam steps: lr * g / (|g| + 1e-8) turns 1e-9-level summation noise on |g| ~ 1e-8 entries into
    # O(lr) differences (DESIGN section 5 iv), so the bulk is compared tightly and the rest is bounded by the 3 updates
    d = (a['flat'] - b['flat']).abs()
    scale = a['flat'].abs().max().item()
    assert float((d > 1e-6 * scale).float().mean()) < 0.10, float((d > 1e-6 * scale).float().mean())   # measured 2-4 %
    assert d.max().item() <= 4 * 5e-4 * 2.001


def _two_ranks(script, env, port):
    env = dict(env)
    if torch.cuda.device_count() < 2:
        env['FASTNERF_DIST_BACKEND'] = 'gloo'
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
                        '127.0.0.1', '--master-port', str(port), script], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def test_overlapped_allreduce_is_bit_identical_and_replicas_agree(tmp_path):
    """The fine net's gradient is all-reduced while the coarse pass's backward runs (Trainer.step, two collectives on the process
    group's stream): same bits as one all-reduce of the whole buffer after the backward, and both ranks hold identical
    parameters and Adam moments afterwards."""
    script = str(tmp_path / 'worker.py')
    res = {}
    for overlap in ('1', '0'):
        out = str(tmp_path / ('ov%s_%%d.pt' % overlap))
        with open(script, 'w') as f:
            f.write(_SHARD_WORKER % {'root': ROOT, 'out': out})
        _two_ranks(script, dict(os.environ, FASTNERF_COMPACT='0', FASTNERF_OVERLAP_ALLREDUCE=overlap), 29551)
        res[overlap] = [torch.load((out % 2) + '.rank%d' % r) for r in range(2)]
        a, b = res[overlap]
        assert a['overlap'] == (overlap == '1')
        for k in ('flat', 'm', 'v', 'grad0'):
            assert torch.equal(a[k], b[k]), k                       # replicas stay bit-identical
    for k in ('flat', 'm', 'v', 'grad0'):
        assert torch.equal(res['1'][0][k], res['0'][0][k]), k       # overlapping changes no bit


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='RCCL refuses two ranks on one device: needs two GPUs')
def test_collectives_through_the_c_abi_match_torch_distributed(tmp_path):
    """FASTNERF_COLLECTIVE=cabi (csrc/comm.cpp: fastnerf_allreduce_grads on a side stream, fastnerf_allreduce_leaf_table) against the
    default torch.distributed route: same parameters, Adam moments and first gradient, bit for bit, replicas identical."""
    script = str(tmp_path / 'worker.py')
    res = {}
    for route in ('cabi', 'torch'):
        out = str(tmp_path / ('%s_%%d.pt' % route))
        with open(script, 'w') as f:
            f.write(_SHARD_WORKER % {'root': ROOT, 'out': out})
        _two_ranks(script, dict(os.environ, FASTNERF_COMPACT='0', FASTNERF_COLLECTIVE=route), 29557)
        res[route] = [torch.load((out % 2) + '.rank%d' % r) for r in range(2)]
        a, b = res[route]
        for k in ('flat', 'm', 'v', 'grad0'):
            assert torch.equal(a[k], b[k]), (route, k)
    for k in ('flat', 'm', 'v', 'grad0'):
        assert torch.equal(res['cabi'][0][k], res['torch'][0][k]), k


def test_ranks_that_disagree_on_compaction_stay_identical(tmp_path):
    """Rank 0 runs the plain backward, rank 1 the compacted one (in production each rank's LivePolicy follows its own shard's live
    fraction): their gradient contributions differ in fp32 summation grouping, the all-reduced sum is the same tensor on
    both, so parameters and Adam moments stay bit-identical across the replicas."""
    script = str(tmp_path / 'worker.py')
    out = str(tmp_path / 'mix_%d.pt')
    with open(script, 'w') as f:
        f.write(_SHARD_WORKER % {'root': ROOT, 'out': out})
    _two_ranks(script, dict(os.environ, FASTNERF_COMPACT='0', COMPACT_RANK1='1'), 29553)
    a, b = [torch.load((out % 2) + '.rank%d' % r) for r in range(2)]
    assert a['live'] == [False] * 4 and b['live'][:3] == [True] * 3    # (the last batch leaves rank 1 without rays)
    for k in ('flat', 'm', 'v', 'grad0'):
        assert torch.equal(a[k], b[k]), k


_TRAIN_WORKER = r"""
import os, sys, hashlib
import numpy as np, torch
sys.path.insert(0, %(root)r)
import fastnerf
from fastnerf import parallel
rank, world, local = parallel.init_from_env('cuda')
torch.cuda.set_device(0 if torch.cuda.device_count() < world else local)
imgs, poses, focal = fastnerf.synthetic.make_dataset(n_images=3, H=32, W=32)
np.random.seed(7 + rank)               # ranks start from DIFFERENT numpy states (the warm-up coordinates are drawn with numpy):
                                       # train() must synchronise them itself (parallel.sync_seed)
args = fastnerf.run_nerf.make_args(N_importance=16, N_samples=16, perturb=1.0, white_bkgd=True, no_reload=True, N_rand=250,
                                   n_epoch=3, init_level=2, subdivide_every=1, subdivide_thres=0.05, lrate=5e-4, lrate_decay=500)
torch.manual_seed(0)                   # identical initial weights, as every data-parallel run needs
logs = []
_, _, trainer, mgr, hist = fastnerf.run_nerf.train(imgs, poses, 32, 32, focal, args, log=logs.append)
torch.cuda.synchronize()
digest = hashlib.sha1(trainer.flat.cpu().numpy().tobytes()).hexdigest()
leaves = [mgr.leaves(i).tolist() for i in range(3)]
torch.save({'digest': digest, 'leaves': leaves, 'hist': hist, 'adam_t': trainer.adam_t}, %(out)r %% rank)
if world > 1:
    parallel.barrier(); torch.distributed.destroy_process_group()
"""


def test_train_driver_on_two_ranks(tmp_path):
    """run_nerf.train() under two ranks: every rank builds the same epoch ray lists (seed broadcast from rank 0), takes rows
    r::2 of every global batch -- the last batch of an epoch can leave a rank without rays -- and all ranks hold bit-identical
    parameters and trees at the end."""
    script = str(tmp_path / 'train_worker.py')
    out = str(tmp_path / 'train_%d.pt')
    with open(script, 'w') as f:
        f.write(_TRAIN_WORKER % {'root': ROOT, 'out': out})
    env = dict(os.environ)
    if torch.cuda.device_count() < 2:
        env['FASTNERF_DIST_BACKEND'] = 'gloo'
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                        '--master-port', '29547', script], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    a, b = torch.load(out % 0), torch.load(out % 1)
    assert a['digest'] == b['digest'] and a['leaves'] == b['leaves'] and a['adam_t'] == b['adam_t']
    assert len(a['hist']) == 3 and all(np.isfinite(h[2]) for h in a['hist']) and a['hist'][-1][2] < 0.1
    assert [h[1] for h in a['hist']] == [h[1] for h in b['hist']]            # same number of steps on both ranks
