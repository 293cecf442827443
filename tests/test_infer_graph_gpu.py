"""``graphs.GraphedInference``: ``head.infer`` as ONE hipGraph, replayed on alternating viewpoints, against the eager call.

What two EAGER calls on one input already differ by is measured here first (the encoder's shared rows are added with fp32
atomics): ``E_vol`` = the relative L2 between two eager volumes, ``E_cls`` = the number of voxels whose class differs between
two eager calls, each the larger of two measurements (one per viewpoint).  A replay is then held to
    volume   relative L2 <= max(4 E_vol, B),  B = the project's bound for "same kernels, replayed": 1e-5 fp32, 2e-3 bf16
             (tests/test_train_graph_gpu.py); B is the floor when E_vol is 0
    classes  at most 4 E_cls + 8 differing voxels of 504 000 per viewpoint (the 8 is a floor against E_cls = 0, not a measurement)
against an eager call on the same input, and its pairs equal ``occ_pairs_host`` of its OWN class bytes bit for bit -- which
also says that a replay with fewer occupied voxels than the one before leaves no stale pair inside its offsets.

Threshold: ``infer_helper.threshold`` (about half of the voxels occupied).  Measured on an MI355X (printed by the test; docs/HISTORY.md, section INFER, records them)."""
import warnings

import numpy as np
import pytest
import torch

from infer_helper import head, same_as_model, threshold, viewpoints
from util import pkg, rel_l2

warnings.filterwarnings('ignore')
pytestmark = pytest.mark.gpu


def _inputs():
    """Three single viewpoints: two synthetic ones, and the first with its features zeroed (another occupied count)."""
    a, b = viewpoints(1), viewpoints(1, first=1)
    return [a, b, (torch.zeros_like(a[0]), a[1], a[2])]


def _differing(x, y):
    return int((x.classes != y.classes).sum())


@pytest.mark.parametrize('autocast', [True, False])
def test_replays_follow_the_eager_step(autocast):
    h = head()
    graphs = pkg('graphs')
    dtype = torch.bfloat16 if autocast else None
    ins = _inputs()
    thr = threshold()
    eager = lambda k: h.infer(*ins[k], occ_threshold=thr, pair_capacity=h.voxel_num, autocast_dtype=dtype)
    ref = [eager(k) for k in range(3)]
    twins = [eager(k) for k in range(2)]
    e_vol = max(rel_l2(twins[k].volume, ref[k].volume) for k in range(2))
    e_cls = max(_differing(twins[k], ref[k]) for k in range(2))
    floor = 2e-3 if autocast else 1e-5
    vol_bound, cls_bound = max(4 * e_vol, floor), 4 * e_cls + 8
    print('autocast=%s: E_vol %.3e E_cls %d -> bounds %.3e / %d voxels' % (autocast, e_vol, e_cls, vol_bound, cls_bound))
    step = graphs.GraphedInference(h, *ins[0], autocast_dtype=dtype, occ_threshold=thr, pair_capacity=h.voxel_num)
    assert all(t.data_ptr() != s.data_ptr() for t, s in zip(step.inputs, ins[0]))
    counts, outside = [], []
    for it, k in enumerate((0, 1, 2, 0, 1)):
        outs = step(*ins[k])
        assert outs is step.outputs
        torch.cuda.synchronize()
        vol, cls = rel_l2(outs.volume, ref[k].volume), _differing(outs, ref[k])
        print('  replay %d (viewpoint %d): volume rel L2 %.3e, %d differing voxels, %d pairs' % (it, k, vol, cls, int(outs.occ_count[1])))
        if vol > vol_bound or cls > cls_bound:
            outside.append((it, k, vol, cls))
        live, offsets = same_as_model(h, outs)
        assert int(outs.occ_count[2]) == 0 and len(live) == int(outs.occ_count[1])
        counts.append(len(live))
    assert not outside, outside
    assert any(b < a for a, b in zip(counts, counts[1:])), counts        # a replay with fewer pairs than the one before it
    # the static inputs themselves: no copy, same result
    step.inputs[0].copy_(ins[1][0]); step.inputs[1].copy_(ins[1][1]); step.inputs[2].copy_(ins[1][2])
    outs = step(*step.inputs)
    assert rel_l2(outs.volume, ref[1].volume) <= vol_bound
    # results(): the one host copy, as simple_test returns it
    volume, bbox_list, occ = step.results()
    live, _ = same_as_model(h, outs)
    assert volume.shape == (900, 1, 768) and volume.is_cuda and occ['flow_preds'] is None
    assert occ['occupancy_preds'].dtype == torch.int64 and np.array_equal(occ['occupancy_preds'].numpy(), live.astype(np.int64))
    r, keep = bbox_list[0]['pts_bbox'], outs.valid[0].bool().cpu()
    assert torch.equal(r['boxes_3d'], outs.boxes[0].cpu()[keep]) and torch.equal(r['scores_3d'], outs.scores[0].cpu()[keep])
    assert r['labels_3d'].dtype == torch.int64 and torch.equal(r['labels_3d'], outs.labels[0].cpu()[keep].long())
    # refusals on host data
    two = viewpoints(2)
    with pytest.raises(ValueError, match='feats'):
        step(*two)
    with pytest.raises(ValueError, match='origin'):
        step(ins[0][0], ins[0][1], ins[0][2].to(torch.float16))
    with pytest.raises(RuntimeError, match='GPU tensors'):
        step(ins[0][0].cpu(), ins[0][1], ins[0][2])
    h.train()
    try:
        with pytest.raises(RuntimeError, match='training mode'):
            step(*ins[0])
        with pytest.raises(RuntimeError, match='training mode'):
            graphs.GraphedInference(h, *ins[0])
    finally:
        h.eval()
