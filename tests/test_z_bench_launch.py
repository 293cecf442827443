"""bench.py as the driver runs it: `--gpus N` from a plain shell must start N ranks (reference:
tools/dist_train.sh:12-14 -> one process per GPU; apis/mmdet_train.py:71-80 -> DDP), and the distributed leg
(process group, DDP wrapper, bf16 compression hook, bucket views) must run on hardware for both training workloads
(BASELINE.json configs[3] and configs[4]).

(The file name sorts last on purpose: every test here starts fresh python processes that import torch and initialise HIP; on
a box that has just been leased the first such start pages the whole image in and can take minutes -- after the other GPU
tests it takes seconds.)"""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
# (--full: the records besides the headline -- roofline, config.latency, config.host_fed, sub-records -- that these tests check)
SMALL = ['--batch', '2', '--micro', '2', '--steps', '2', '--warmup', '0', '--full', '--no-cpu-baseline',
         '--latency-batches', '1', '--latency-steps', '2', '--sub-records', '']


def run_bench(argv, env_extra=None, timeout=900):
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + argv, env=env, capture_output=True, text=True, timeout=timeout)


def json_line(proc):
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, 'expected ONE json line, got %d\nstdout:\n%s\nstderr:\n%s' % (len(lines), proc.stdout[-2000:], proc.stderr[-4000:])
    return json.loads(lines[0])


def test_gpus_n_spawns_n_ranks_and_relays_exit_code():
    """No GPU needed: on a CPU-only box every spawned rank stops at bench.py's own 'needs a GPU' assertion; the
    launcher must have started two of them and must hand their failure back as its exit code.  On a GPU box the
    same command is the success case below."""
    import torch
    if torch.cuda.is_available():
        pytest.skip('covered by the gpu tests on a GPU box')
    proc = run_bench(['--gpus', '2', '--backend', 'gloo'] + SMALL)
    assert proc.returncode != 0
    assert proc.stderr.count('bench.py needs a GPU') >= 2, proc.stderr[-3000:]
    # RCCL needs a GPU per rank: refused before anything is spawned
    proc = run_bench(['--gpus', '2', '--backend', 'nccl'] + SMALL)
    assert proc.returncode != 0 and 'only 0 GPU(s) visible' in proc.stderr


@pytest.mark.gpu
@pytest.mark.parametrize('workload', ['vocc_c2f_train', 'vocc_full_train'])
def test_gpus_2_from_a_plain_shell_runs_two_ranks(workload):
    """`python bench.py --gpus 2 --backend gloo` (two ranks sharing the one GPU of this box, gradient sum over gloo):
    one JSON line, n_gpus = 2, twice the viewpoints of one rank per step."""
    proc = run_bench(['--gpus', '2', '--backend', 'gloo', '--workload', workload] + SMALL)
    assert proc.returncode == 0, proc.stderr[-4000:]
    line = json_line(proc)
    assert line['n_gpus'] == 2 and line['config']['parallelism'] == 'dp2'
    assert line['config']['global_viewpoints_per_step'] == 4
    assert line['config']['gradient_allreduce'] == 'gloo'
    assert line['value'] > 0 and line['cpu_baseline'] is None
    assert line['config']['latency'][0]['viewpoints_per_gpu_per_step'] == 1
    fed = line['config']['host_fed']                                   # PCIe-inclusive record: 2 viewpoints x 6 x 196 x 768 fp32
    assert fed['host_bytes_per_step'] == 2 * 6 * 196 * 768 * 4 and fed['viewpoints_per_s'] > 0


@pytest.mark.gpu
@pytest.mark.parametrize('workload', ['vocc_c2f_train', 'vocc_full_train'])
def test_rccl_leg_runs_on_hardware_with_one_rank(workload):
    """Under a launcher with WORLD_SIZE=1 the process group is RCCL ('nccl' backend): the communicator, DDP's bucket
    views, the bf16 compression hook and the all-reduce itself execute on the GPU (with one rank the reduce is the
    identity, the code path is the N-rank one)."""
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    env = dict(WORLD_SIZE='1', RANK='0', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
               HSA_ENABLE_IPC_MODE_LEGACY='0')
    proc = run_bench(['--gpus', '1', '--backend', 'nccl', '--workload', workload] + SMALL, env)
    assert proc.returncode == 0, proc.stderr[-4000:]
    line = json_line(proc)
    assert line['n_gpus'] == 1
    assert line['config']['gradient_allreduce'].startswith('RCCL')
    assert line['roofline'] is not None and line['roofline']['launches'] == 2 * 3


@pytest.mark.gpu
def test_default_line_carries_the_full_multitask_and_fp32_sub_records():
    """The driver's command is fixed, so BASELINE configs[4] and the fp32 form of the headline workload ride in the
    default line as `config.full_train` / `config.fp32` (measured after the headline region, never part of `value`)."""
    argv = [a for a in SMALL if a not in ('--sub-records', '')] + ['--sub-records', 'full_train:2,fp32:2', '--sub-steps', '2',
                                                                  '--host-fed-steps', '0']
    proc = run_bench(argv)
    assert proc.returncode == 0, proc.stderr[-4000:]
    cfg = json_line(proc)['config']
    ft, f32 = cfg['full_train'], cfg['fp32']
    assert ft['workload'] == 'vocc_full_train' and ft['dtype'] == 'bf16' and ft['viewpoints_per_gpu_per_step'] == 2
    assert f32['workload'] == 'vocc_c2f_train' and f32['dtype'] == 'fp32' and f32['viewpoints_per_gpu_per_step'] == 2
    assert ft['viewpoints_per_s'] > 0 and f32['viewpoints_per_s'] > 0
    assert ft['trainable_params'] > f32['trainable_params'] > 100e6        # the decoder is unfrozen in configs[4]


@pytest.mark.gpu
def test_plain_one_gpu_run_of_the_full_workload_replays_small_batches_as_graphs():
    """`python bench.py --workload vocc_full_train` on one GPU, no launcher: the headline is the eager step; the
    config.latency record at one viewpoint per step is the hipGraph replay of the head (graphed: true), and the line
    still carries the PCIe-inclusive record."""
    proc = run_bench(['--workload', 'vocc_full_train'] + SMALL)
    assert proc.returncode == 0, proc.stderr[-4000:]
    line = json_line(proc)
    assert line['n_gpus'] == 1 and line['value'] > 0
    rec = line['config']['latency'][0]
    assert rec['viewpoints_per_gpu_per_step'] == 1 and rec['graphed'] is True and rec['ms_per_step'] > 0
    assert line['config']['host_fed']['viewpoints_per_s'] > 0


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_the_last_step(tmp_path):
    """`python bench.py` without --full: the line carries the headline and none of the --full records, and
    `--dump-outputs DIR` writes the last timed step's loss, gradient norm and trained parameters.  Two runs with the same
    arguments start from the same inputs and weights: their dumps name the same arrays, of the same shapes, and agree to
    the atomics' summation order."""
    import numpy as np
    argv = ['--batch', '2', '--micro', '2', '--steps', '3', '--warmup', '1']
    dumps = []
    for run in (0, 1):
        out = tmp_path / ('dump%d' % run)
        proc = run_bench(argv + ['--dump-outputs', str(out)])
        assert proc.returncode == 0, proc.stderr[-4000:]
        line = json_line(proc)
        assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0 and line['value'] > 0
        assert line['unit'] == 'viewpoints/s' and line['higher_is_better'] is True and line['dtype'] == 'bf16'
        assert line['roofline'] is None and line['roofline_other_kernels'] is None and line['cpu_baseline'] is None
        cfg = line['config']
        assert cfg['full'] is False
        assert cfg['latency'] is None and cfg['host_fed'] is None and cfg['full_train'] is None and cfg['fp32'] is None
        files = sorted(os.listdir(out))
        assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
        dumps.append({f: np.load(out / f) for f in files})
    a, b = dumps
    assert set(a) == set(b) and {'loss.npy', 'grad_norm.npy'} <= set(a)
    assert sum(1 for f in a if f.startswith('param.')) > 50
    for f in a:
        assert a[f].dtype in (np.float32, np.float64) and a[f].shape == b[f].shape, f
        assert np.isfinite(a[f]).all(), f
    for f in ('loss.npy', 'grad_norm.npy'):
        assert abs(float(a[f][0]) - float(b[f][0])) <= 1e-3 * abs(float(a[f][0])), (f, a[f], b[f])
    worst = max(float(np.abs(a[f] - b[f]).max()) for f in a if f.startswith('param.'))
    # (6 AdamW steps of lr 1e-4 -- 2 priming, 1 warm-up, 3 timed: an element whose gradient is within rounding of zero may
    #  take a different sign in the two runs; everything else agrees to rounding)
    assert worst <= 2e-3, worst


@pytest.mark.gpu
def test_two_ranks_allreduce_the_gradients_of_the_real_step(tmp_path):
    """BASELINE configs[3], correctness of the exchange: two gloo ranks on the one GPU run ONE LiftTrainer step of the
    real HIP path (custom autograd Functions, frozen parameters, gradient_as_bucket_view buckets) at two viewpoints each,
    fp32, dropout p = 0; the gradients rank 0 holds after the all-reduce equal the MEAN of two single-process runs over
    the two ranks' viewpoints (reference: MMDistributedDataParallel, apis/mmdet_train.py:71-80)."""
    import torch
    helper = os.path.join(ROOT, 'tests', 'ddp_grad_helper.py')
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    outs = []
    for r in (0, 1):
        out = str(tmp_path / ('single%d.pt' % r))
        proc = subprocess.run([sys.executable, helper, 'single', str(r), out], env=env, capture_output=True, text=True, timeout=900)
        assert proc.returncode == 0, proc.stderr[-4000:]
        outs.append(torch.load(out))
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    out = str(tmp_path / 'ddp.pt')
    proc = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                           '--master-addr', '127.0.0.1', '--master-port', str(port), helper, 'ddp', out],
                          env=env, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-4000:]
    ddp = torch.load(out)
    assert abs(ddp['loss'] - outs[0]['loss']) <= 1e-6 * abs(outs[0]['loss'])          # rank 0's own loss
    assert set(ddp['grads']) == set(outs[0]['grads']) == set(outs[1]['grads']) and len(ddp['grads']) > 50
    worst = 0.0
    for k, g in ddp['grads'].items():
        want = 0.5 * (outs[0]['grads'][k] + outs[1]['grads'][k])
        err = float((g - want).norm() / want.norm().clamp_min(1e-30))
        worst = max(worst, err)
        assert err < 1e-5, (k, err)
        # and it is NOT just rank 0's own gradient: the exchange happened
        assert float((g - outs[0]['grads'][k]).norm()) > 1e-3 * float(want.norm()) or float(want.norm()) == 0.0, k
    print('worst relative L2 of the all-reduced gradients: %.2e' % worst)


@pytest.mark.gpu
def test_two_ranks_apply_the_same_clipped_adamw_update_on_the_bucket_views(tmp_path):
    """The rest of bench.py's N > 1 step that one GPU can check: after the all-reduce, ``optim.ClipAdamW`` reads the gradients
    where DDP left them -- views into its buckets (``gradient_as_bucket_view=True``) -- on two gloo ranks sharing the GPU.
    Both ranks must end with BIT-IDENTICAL parameters (same gradients, same deterministic norm, same arithmetic), equal to
    a single-process step on the mean of the two ranks' single-process gradients, and the clip norm each gets back is the
    norm of the all-reduced gradients (reference: OptimizerHook's clip_grad_norm_ + AdamW behind
    MMDistributedDataParallel, apis/mmdet_train.py:71-80, vocc.py:268-274)."""
    import torch
    helper = os.path.join(ROOT, 'tests', 'ddp_grad_helper.py')
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    singles = []
    for r in (0, 1):
        out = str(tmp_path / ('single%d.pt' % r))
        proc = subprocess.run([sys.executable, helper, 'single', str(r), out], env=env, capture_output=True, text=True, timeout=900)
        assert proc.returncode == 0, proc.stderr[-4000:]
        singles.append(out)
    ref_out = str(tmp_path / 'single_update.pt')
    proc = subprocess.run([sys.executable, helper, 'single_update', singles[0], singles[1], ref_out], env=env, capture_output=True,
                          text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-4000:]
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    out = str(tmp_path / 'ddp_update.pt')
    proc = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                           '--master-addr', '127.0.0.1', '--master-port', str(port), helper, 'ddp_update', out],
                          env=env, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-4000:]
    r0, r1, ref = torch.load(out + '.0'), torch.load(out + '.1'), torch.load(ref_out)
    assert r0['grad_views'] == len(r0['digest']) > 50                      # the optimizer did read bucket views
    assert r0['digest'] == r1['digest']                                    # bit-identical parameters on both ranks
    assert r0['clip_norm'] == r1['clip_norm']
    assert abs(r0['clip_norm'] - r0['grad_norm']) <= 1e-5 * r0['grad_norm']
    assert abs(r0['clip_norm'] - ref['clip_norm']) <= 1e-5 * ref['clip_norm']
    assert r0['clip_norm'] > 10 * 1e-3                                      # (the clip at 1e-3 was active)
    lr, off = 1e-4, 0
    for k, want in ref['sample'].items():
        d = (r0['sample'][k] - want).abs()
        # the first AdamW step moves every element by ~lr * sign(g): elements whose gradient is within rounding of zero may
        # differ by up to 2 lr between two evaluations of the same mean; everything else to fp32 rounding
        assert float(d.max()) <= 2.001 * lr, (k, float(d.max()))
        off += int((d > 1e-3 * lr).sum())
    total = sum(v.numel() for v in ref['sample'].values())
    assert off <= 2e-3 * total, (off, total)
    print('two-rank ClipAdamW update: clip norm %.6g, %d of %d sampled parameters more than 1e-3 lr from the single-process step'
          % (r0['clip_norm'], off, total))


@pytest.mark.gpu
def test_bf16_compressed_gradients_under_rccl_equal_the_rounded_single_process_gradients(tmp_path):
    """The gradient path bench.py uses for N > 1 -- RCCL communicator + DDP buckets + `bf16_compress_hook`
    (vln-ver_amd/ddp.py:62-69; reference: MMDistributedDataParallel, apis/mmdet_train.py:71-80) -- checked NUMERICALLY on
    the one GPU there is: with one rank the all-reduce is the identity, so every gradient after backward() must be the
    bf16 round trip of the single-process gradient (relative L2 <= 4e-3 = one bf16 rounding; the two runs differ by the
    atomics' summation order on top), and parameters with an all-zero gradient stay exactly zero."""
    import torch
    helper = os.path.join(ROOT, 'tests', 'ddp_grad_helper.py')
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    env['HSA_ENABLE_IPC_MODE_LEGACY'] = '0'
    single = str(tmp_path / 'single.pt')
    proc = subprocess.run([sys.executable, helper, 'single', '0', single], env=env, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-4000:]
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    out = str(tmp_path / 'rccl.pt')
    proc = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1',
                           '--master-addr', '127.0.0.1', '--master-port', str(port), helper, 'rccl', out],
                          env=env, capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-4000:]
    ref, got = torch.load(single), torch.load(out)
    assert abs(got['loss'] - ref['loss']) <= 1e-6 * abs(ref['loss'])
    assert set(got['grads']) == set(ref['grads']) and len(got['grads']) > 50
    worst, rounded = 0.0, 0
    for k, g in got['grads'].items():
        want = ref['grads'][k].bfloat16().float()                      # compress -> (identity reduce) -> decompress
        if float(ref['grads'][k].abs().max()) == 0.0:
            assert float(g.abs().max()) == 0.0, k
            continue
        err = float((g - want).norm() / want.norm())
        worst = max(worst, err)
        assert err <= 4e-3, (k, err)
        # the hook really ran: the values are bf16-representable (an uncompressed fp32 gradient would not be)
        rounded += int(torch.equal(g, g.bfloat16().float()))
    assert rounded == sum(1 for k in got['grads'] if float(ref['grads'][k].abs().max()) > 0.0)
    print('worst relative L2 against the rounded single-process gradients: %.2e' % worst)
