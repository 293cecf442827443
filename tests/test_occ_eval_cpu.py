"""Occupancy IoU / mIoU evaluation without a GPU: the torch restatement of ``head.occupancy_confusion`` against the
reference's own ``SSCMetrics`` histogram (tests/golden/post_vocc.npz), the evaluation labels with a visible mask,
``DeviceSSCMetrics`` summed over two gloo ranks, and the argument checks of ``ver_occ_confusion``."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cases
from util import golden, pkg

T = torch.from_numpy


def _head():
    pkg()
    return pkg('registry').build_head(cases.vocc_head_cfg(only_occ=True))


def test_torch_confusion_reproduces_the_reference_histogram():
    """post_vocc['hist'] is SSCMetrics(17) after add_batch(pred, gt) and add_batch(pred[::-1], gt)."""
    g = golden('post_vocc')
    h = _head()
    metrics = pkg('occupancy_metrics')
    logits, gt = cases.occupancy_loss_inputs(seed=33, n=6000)
    labels = T(gt).to(torch.uint8)[None]
    hist = h.occupancy_confusion(T(logits)[None], labels)
    assert hist.dtype == torch.int64 and hist.shape == (1, 1, 17, 17)
    hist = h.occupancy_confusion(T(logits[::-1].copy())[None], labels, hist=hist)      # accumulates
    assert np.array_equal(hist[0, 0].numpy(), g['hist'])
    m = metrics.DeviceSSCMetrics(17)
    m.add_hist(hist)
    st = m.get_stats()
    for k in ('iou', 'precision', 'recall', 'miou'):
        assert float(st[k]) == pytest.approx(float(g[k]), rel=1e-12)
    assert np.allclose(st['iou_ssc'], g['iou_ssc'], rtol=1e-12, atol=0)
    assert float(m.sample_stats(0)['miou']) == pytest.approx(float(g['miou']), rel=1e-12)
    m.reset()
    assert int(m.hist.abs().sum()) == 0


def test_thresholds_are_independent_columns():
    """T thresholds in one call = T calls with one threshold each, and each is the histogram of the sparse
    prediction of ``get_occupancy_prediction`` at that threshold."""
    h = _head()
    metrics = pkg('occupancy_metrics')
    logits, gt = cases.occupancy_loss_inputs(seed=34, n=5000)
    x, labels = T(logits), T(gt).to(torch.uint8)
    thr = (0.1, 0.25, 0.5, 0.9)
    hist = h.occupancy_confusion(x[None], labels[None], thresholds=thr)
    for t, v in enumerate(thr):
        one = h.occupancy_confusion(x[None], labels[None], thresholds=(v,))
        assert torch.equal(hist[:, t], one[:, 0])
        pairs = h.get_occupancy_prediction(dict(occupancy_preds=x[None]), v)['occupancy_preds'].numpy()
        ref = metrics.SSCMetrics(17)
        ref.add_batch(metrics.dense_labels(pairs, 5000, 16), gt)
        assert np.array_equal(hist[0, t].numpy(), ref.hist)


def test_eval_labels_with_invalid_voxels_equal_the_visible_mask():
    h = _head()
    metrics = pkg('occupancy_metrics')
    n = h.voxel_num
    rng = np.random.default_rng(3)
    logits = T((rng.standard_normal((2, n, 16)) * 2 - 2.5).astype(np.float32))
    dense = rng.integers(0, 17, size=(2, n))
    dense[rng.uniform(size=dense.shape) < 0.8] = 16
    invalid = [rng.choice(n, 30000, replace=False), None]
    pairs = [np.stack([np.nonzero(d < 16)[0], d[d < 16]], 1) for d in dense]
    labels = h.occupancy_eval_labels([[p] for p in pairs], invalid, device='cpu')
    assert labels.dtype == torch.uint8 and labels.shape == (2, n)
    assert int((labels == 255).sum()) == 30000
    hist = h.occupancy_confusion(logits, labels)
    assert hist.shape == (2, 1, 17, 17)
    for b in range(2):
        sparse = h.get_occupancy_prediction(dict(occupancy_preds=logits[b:b + 1]))['occupancy_preds'].numpy()
        ref = metrics.SSCMetrics(17)
        vis = None
        if invalid[b] is not None:
            vis = np.ones(n, dtype=np.uint8)
            vis[invalid[b]] = 0
        ref.add_batch(metrics.dense_labels(sparse, n, 16), dense[b], visible_mask=vis)
        assert np.array_equal(hist[b, 0].numpy(), ref.hist), b


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import importlib
        metrics = importlib.import_module('vln-ver_amd.occupancy_metrics')
        m = metrics.DeviceSSCMetrics(17, thresholds=(0.25, 0.5))
        m.add_hist(torch.from_numpy(_rank_hist(rank)))
        m.all_reduce()
        torch.save(dict(hist=m.hist, stats=[m.get_stats(t) for t in range(2)]), os.path.join(out, 'r%d.pt' % rank))
    finally:
        dist.destroy_process_group()


def _rank_hist(rank):
    return np.random.default_rng(10 + rank).integers(0, 1 << 40, size=(3, 2, 17, 17)).astype(np.int64)


def test_two_rank_all_reduce_sums_the_histograms(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(os.path.join(str(tmp_path), 'r%d.pt' % k), weights_only=False) for k in range(world)]
    want = _rank_hist(0).sum(0) + _rank_hist(1).sum(0)
    metrics = pkg('occupancy_metrics')
    for k in range(world):
        assert np.array_equal(r[k]['hist'].numpy(), want)
        for t in range(2):
            ref = metrics.SSCMetrics(17)
            ref.hist = want[t].astype(np.float64)
            st = ref.get_stats()
            for key in ('iou', 'precision', 'recall', 'miou'):
                assert float(r[k]['stats'][t][key]) == float(st[key])
            assert np.array_equal(r[k]['stats'][t]['iou_ssc'], st['iou_ssc'])


def test_confusion_argument_validation_without_gpu():
    """Every bad argument comes back as an error code with a message, before anything is launched."""
    hip = pkg('hipops')
    lib = hip.lib()
    buf = (ctypes.c_float * 64)()
    lab = (ctypes.c_uint8 * 64)()
    hist = (ctypes.c_int64 * (17 * 17 * 8))()
    thr = (ctypes.c_float * 9)(*([0.25] * 9))

    def call(logits=buf, dtype=0, rows=4, samples=1, C=16, labels=lab, thresholds=thr, T=1, h=hist):
        return lib.ver_occ_confusion(logits, dtype, ctypes.c_long(rows), samples, C, labels, thresholds, T, h, None)

    assert call(logits=None) == -1 and b'null' in lib.ver_last_error()
    assert call(labels=None) == -1 and b'null' in lib.ver_last_error()
    assert call(h=None) == -1 and b'null' in lib.ver_last_error()
    assert call(thresholds=None) == -1 and b'null' in lib.ver_last_error()
    assert call(C=12) == -2 and b'class count' in lib.ver_last_error()
    assert call(C=40) == -2 and b'class count' in lib.ver_last_error()
    assert call(T=0) == -2 and b'thresholds' in lib.ver_last_error()
    assert call(T=9) == -2 and b'thresholds' in lib.ver_last_error()
    assert call(dtype=2) == -1 and b'dtype' in lib.ver_last_error()
    assert call(rows=-1) == -1 and b'shape' in lib.ver_last_error()
    assert call(samples=70000) == -2 and b'grid' in lib.ver_last_error()
    assert call(rows=1 << 40) == -2 and b'grid' in lib.ver_last_error()
    # an empty batch launches nothing (no device is needed) and succeeds
    assert call(logits=None, labels=None, h=None, rows=0) == 0
    assert call(logits=None, labels=None, h=None, samples=0) == 0
    assert all(v == 0 for v in hist)
