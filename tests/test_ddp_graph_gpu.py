"""The captured training steps under data parallelism (``graphs.GraphedLiftStep(exchange=)``, ``graphs.GraphedTrainStep(
exchange=)``; ``ddp.GradExchange``), on the one GPU there is: two gloo ranks share it, as in tests/test_z_bench_launch.py.  The
ranks run tests/ddp_graph_helper.py under ``python -m torch.distributed.run``; every child has a time limit, a failed or
timed-out child fails its test at once and no further child is started in this module.

Bounds: graph against eager, the project's bound for "same kernels, replayed" (tests/grad_exchange_cases.py: losses 1e-5
relative, every parameter's update 0.05 relative L2, fp32); the first step against one process on the mean of the two ranks'
gradients, the tolerance of ``test_two_ranks_apply_the_same_clipped_adamw_update_on_the_bucket_views`` (clip norm 1e-5
relative; AdamW's first step moves every element by ~lr * sign(g), so elements whose gradient is within rounding of zero may
differ by 2 lr, at most 2e-3 of the sampled elements by more than 1e-3 lr)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from util import ROOT, pkg

pytestmark = pytest.mark.gpu
HELPER = os.path.join(ROOT, 'tests', 'ddp_graph_helper.py')
LIMIT = 600                                    # seconds per child; they take well under a minute each
_failed = []


def _child(cmd):
    if _failed:
        pytest.fail('not started: an earlier child of this module failed (%s)' % _failed[0])
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    try:
        proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        _failed.append('timed out: ' + ' '.join(cmd[-3:]))
        pytest.fail(_failed[0])
    if proc.returncode != 0:
        _failed.append('exit status %d: %s' % (proc.returncode, ' '.join(cmd[-3:])))
        pytest.fail(_failed[0] + '\n' + proc.stderr[-6000:])


def _two_ranks(mode, out):
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    _child([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
            '--master-port', str(port), HELPER, mode, out])
    import torch
    return [torch.load(out + '.%d' % r) for r in (0, 1)]


@pytest.fixture(scope='module')
def lift(tmp_path_factory):
    """The two ranks' records of the lifting step (one child), computed once for the tests below."""
    return _two_ranks('lift', str(tmp_path_factory.mktemp('lift') / 'rec'))


def test_lifting_step_ranks_agree_bit_for_bit(lift):
    r0, r1 = lift
    assert (r0['rank'], r1['rank'], r0['world']) == (0, 1, 2) and r0['tensors'] > 50
    for run in ('graph', 'eager', 'first'):
        assert r0[run]['digest'] == r1[run]['digest'] and len(r0[run]['digest']) == r0['tensors'], run   # bit-identical parameters
    assert r0['graph']['clip_norm'] == r1['graph']['clip_norm'] and r0['eager']['clip_norm'] == r1['eager']['clip_norm']
    assert r0['graph']['steps'] == r1['graph']['steps'] == [3]
    assert r0['eager']['loss'] != r1['eager']['loss']                      # (different data per rank)
    assert r0['first']['own_grad_norm'] != r1['first']['own_grad_norm']


def test_lifting_step_replays_the_eager_exchanged_steps(lift):
    for r in lift:
        e, g = r['eager'], r['graph']
        for it, (a, b) in enumerate(zip(g['loss'], e['loss'][1:])):
            print('rank %d step %d: loss %.9g vs eager %.9g' % (r['rank'], it + 1, a, b))
        worst = max(r['updates'].values())
        print('rank %d: worst relative difference of a parameter update %.2e' % (r['rank'], worst))
        for a, b in zip(g['loss'], e['loss'][1:]):
            assert abs(a - b) <= 1e-5 * abs(b), (g['loss'], e['loss'])
        assert e['loss'][1] != e['loss'][2]                                # (the steps do move the loss)
        outside = {k: v for k, v in r['updates'].items() if not v < 0.05}
        assert not outside, outside
        # the norm a step returns is the norm of the gradients the exchange holds, in both runs
        for run in (e, g):
            for a, b in zip(run['clip_norm'], run['held_norm']):
                assert abs(a - b) <= 1e-5 * b, (run['clip_norm'], run['held_norm'])
        assert min(e['clip_norm']) > 10 * 1e-3                             # (the clip at 1e-3 was active)


def test_lifting_first_step_equals_one_process_on_the_mean_gradient(lift, tmp_path):
    import torch
    out = str(tmp_path / 'single.pt')
    _child([sys.executable, HELPER, 'lift_single', out])
    ref, first = torch.load(out), lift[0]['first']
    assert abs(first['clip_norm'] - ref['clip_norm']) <= 1e-5 * ref['clip_norm']
    assert abs(ref['clip_norm'] - ref['grad_norm']) <= 1e-5 * ref['grad_norm']
    lr, off = 1e-4, 0
    for k, want in ref['sample'].items():
        d = (first['sample'][k] - want).abs()
        assert float(d.max()) <= 2.001 * lr, (k, float(d.max()))
        off += int((d > 1e-3 * lr).sum())
    total = sum(v.numel() for v in ref['sample'].values())
    assert off <= 2e-3 * total, (off, total)
    print('two-rank exchanged update: clip norm %.6g, %d of %d sampled parameters more than 1e-3 lr from the single-process step'
          % (first['clip_norm'], off, total))


def test_bf16_wire_holds_the_sum_of_the_two_rounded_halves(lift):
    """One backward packed onto a bf16 wire at world size 2: the scale 1/2 is exact, every rank's half is its gradient
    rounded ONCE to bf16 (``hipops.pack_host``), and the exchange holds the bf16 sum of the two halves."""
    import torch
    hip = pkg('hipops')
    r0, r1 = lift
    checked = 0
    for k, held in r0['bf16']['held'].items():
        assert torch.equal(held.view(torch.int16), r1['bf16']['held'][k].view(torch.int16)), k
        halves = [torch.from_numpy(hip.pack_host(r['bf16']['own'][k].numpy(), 0.5, torch.bfloat16).view(np.int16)).view(torch.bfloat16)
                  for r in (r0, r1)]
        want = halves[0] + halves[1]                                       # one bf16 addition: exact sum, rounded to nearest-even
        bad = held.view(torch.int16) != want.view(torch.int16)
        bad &= ~((held == 0) & (want == 0))                                # (+0 and -0 are the same sum)
        assert not bool(bad.any()), '%s: %d of %d elements differ' % (k, int(bad.sum()), bad.numel())
        checked += held.numel()
    assert checked > 1e6 and any(bool((r0['bf16']['own'][k] != r1['bf16']['own'][k]).any()) for k in r0['bf16']['own'])


def test_multi_task_step_on_two_ranks(tmp_path):
    """``GraphedTrainStep(exchange=)`` on the vocc head, one viewpoint per rank, 4 / 0 / 6 boxes on rank 0 and 3 / 5 / 2 on rank
    1: the replays read the PRESET loss normalisers, the eager exchanged twin all-reduces its own inside ``head.loss`` --
    agreement of the losses is the check on the preset rows."""
    r0, r1 = _two_ranks('multi', str(tmp_path / 'rec'))
    assert r0['counts'] == [4, 0, 6] and r1['counts'] == [3, 5, 2]
    assert r0['digest'] == r1['digest'] and len(r0['digest']) == r0['tensors'] > 100
    assert r0['clip_norm'] == r1['clip_norm'] and r0['steps'] == r1['steps'] == [3]
    for r in (r0, r1):
        outside = []
        for it, (g, w) in enumerate(zip(r['graph'], r['eager'][1:])):
            assert sorted(g) == sorted(w) and len(w) == 14
            for k in w:
                ok = abs(g[k] - w[k]) <= 1e-5 * abs(w[k])
                print('rank %d step %d %s: %.9g vs eager %.9g%s' % (r['rank'], it + 1, k, g[k], w[k], '' if ok else '   <-- outside'))
                if not ok:
                    outside.append((it + 1, k, g[k], w[k]))
        moved = {k: v for k, v in r['updates'].items() if v != 0.0}
        print('rank %d: worst relative difference of a parameter update %.2e' % (r['rank'], max(moved.values())))
        far = {k: v for k, v in r['updates'].items() if not v < 0.05}
        assert not outside and not far, (outside, far)
        assert r['flags']['assignment'] == 0 and r['flags']['rejected_pairs'] == 0
    assert r0['graph'][0]['loss_bbox'] == 0.0 and r1['graph'][0]['loss_bbox'] > 0      # rank 0's step without boxes
    assert r0['graph'][0]['loss_cls'] > 0                                  # ... still normalised by rank 1's positives
