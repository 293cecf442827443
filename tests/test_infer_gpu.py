"""``VoxelFormerOccupancyHead.infer`` on the GPU -- vocc.py's head, seeded weights, one and two synthetic viewpoints,
``pair_capacity = voxel_num`` per viewpoint, at a threshold that leaves about half of the voxels occupied
(``infer_helper.threshold``; with seeded weights every voxel clears the default 0.25): the fixed-shape pairs against the numpy model of ``ver_occ_pairs`` on the step's
own class bytes and against the existing routes on the SAME volume (bit for bit: one classification kernel on one input),
the boxes against ``get_bboxes_padded(fused=True)`` of a full forward, the detector's ``device_inference`` switch against the
default ``simple_test``, and the overflow report.

Bounds.  Two forwards of one input differ in the last bits of the encoder output (its shared rows are added with fp32
atomics), so boxes of two forwards are held to the project's bound for "same kernels, run again": relative L2 1e-5 in fp32,
2e-3 under bf16 autocast (tests/test_train_graph_gpu.py), on slots whose labels agree -- all of them in fp32, where the
scores of the top slots are distinct."""
import warnings

import numpy as np
import pytest
import torch

import cases
from infer_helper import DEV, flat_pairs, head, same_as_model, threshold, viewpoints
from test_detector_cpu import _metas, _sparse, _store
from util import pkg, rel_l2

warnings.filterwarnings('ignore')
pytestmark = pytest.mark.gpu


def _ctx(autocast):
    return torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast, cache_enabled=False)


@pytest.mark.parametrize('n', [1, 2])
def test_bf16_pairs_are_the_models_and_the_class_map_routes(n):
    h = head()
    outs = h.infer(*viewpoints(n), occ_threshold=threshold(), pair_capacity=n * h.voxel_num)
    assert outs.classes.dtype == torch.uint8 and outs.classes.numel() == n * h.voxel_num and outs.plan is not None
    assert outs.volume.shape == (n, 900, 768) and outs.occ_pairs.shape == (n * h.voxel_num, 2) and outs.occ_pairs.dtype == torch.int32
    live, offsets = same_as_model(h, outs)
    assert 0 < len(live) < n * h.voxel_num and int(outs.occ_count[n + 1]) == 0
    with torch.no_grad(), _ctx(True):
        want = h.get_occupancy_prediction_from_volume(outs.volume, threshold())['occupancy_preds']
    assert want.dtype == torch.int64 and torch.equal(flat_pairs(outs, h.voxel_num), want.cpu())


@pytest.mark.parametrize('n', [1, 2])
def test_fp32_pairs_are_those_of_the_logits(n):
    h = head()
    outs = h.infer(*viewpoints(n), occ_threshold=threshold(), pair_capacity=n * h.voxel_num, autocast_dtype=None)
    same_as_model(h, outs)
    with torch.no_grad():
        logits = h.occupancy_from_volume(outs.volume)
        assert logits.dtype == torch.float32 and logits.shape == (n, h.voxel_num, 16)
        want = h.get_occupancy_prediction(dict(occupancy_preds=logits), threshold())['occupancy_preds']
    assert len(want) > 0 and torch.equal(flat_pairs(outs, h.voxel_num), want.cpu())


@pytest.mark.parametrize('autocast', [False, True])
@pytest.mark.parametrize('n', [1, 2])
def test_boxes_are_those_of_a_full_forward(n, autocast):
    h = head()
    ins = viewpoints(n)
    outs = h.infer(*ins, occ_threshold=threshold(), pair_capacity=n * h.voxel_num, autocast_dtype=torch.bfloat16 if autocast else None)
    with torch.no_grad(), _ctx(autocast):
        full = h(ins[0], None, world2pixel=ins[1], origin=ins[2])
        want = h.get_bboxes_padded(full, fused=True)
    got = (outs.boxes, outs.scores, outs.labels, outs.valid)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
    tol = 2e-3 if autocast else 1e-5
    agree = (got[2] == want[2]) & (got[3] == want[3])
    print('boxes n=%d autocast=%s: %d of %d slots agree in label and valid; rel L2 boxes %.3e scores %.3e (bound %.0e)'
          % (n, autocast, int(agree.sum()), agree.numel(), rel_l2(got[0][agree], want[0][agree]), rel_l2(got[1][agree], want[1][agree]), tol))
    assert int(want[3].sum()) > 0
    if not autocast:
        assert bool(agree.all())
    assert int(agree.sum()) >= 0.9 * agree.numel()              # (bf16: slots of near-equal scores may swap between two forwards)
    assert rel_l2(got[0][agree], want[0][agree]) <= tol and rel_l2(got[1][agree], want[1][agree]) <= tol


def test_out_reuses_the_buffers_of_an_earlier_call():
    h = head()
    first = h.infer(*viewpoints(1, first=1), occ_threshold=threshold(), pair_capacity=h.voxel_num)
    ptrs = [t.data_ptr() for t in first if torch.is_tensor(t)]
    again = h.infer(*viewpoints(1), occ_threshold=threshold(), pair_capacity=h.voxel_num, out=first)
    assert [t.data_ptr() for t in again if torch.is_tensor(t)] == ptrs and again.plan is first.plan
    same_as_model(h, again)
    fresh = h.infer(*viewpoints(1), occ_threshold=threshold(), pair_capacity=h.voxel_num)
    assert rel_l2(again.volume, fresh.volume) <= 2e-3 and torch.equal(again.labels, fresh.labels)


def test_overflow_sets_the_flag_and_writes_nothing_past_the_capacity():
    h = head()
    mod = pkg('dense_heads.voxelformer_occupancy_head')
    ins = viewpoints(2)
    full = h.infer(*ins, occ_threshold=threshold(), pair_capacity=2 * h.voxel_num, autocast_dtype=None)
    total = int(full.occ_count[2])
    cap = total // 3
    assert cap > 0
    small = h.infer(*ins, occ_threshold=threshold(), pair_capacity=cap, autocast_dtype=None)
    assert small.occ_pairs.shape == (cap, 2) and small.occ_count.tolist()[2:] == [total, 1]
    assert int(small.occ_offsets[-1]) == cap and int(small.occ_offsets.max()) == cap
    guarded = torch.full((cap + 64, 2), -7, dtype=torch.int32, device=DEV)
    again = h.infer(*ins, occ_threshold=threshold(), pair_capacity=cap, autocast_dtype=None, out=small._replace(occ_pairs=guarded[:cap]))
    assert bool((guarded[cap:] == -7).all()) and int(again.occ_count[3]) == 1
    same_as_model(h, again)
    with pytest.raises(RuntimeError, match='pair capacity'):
        mod.inference_results(h, again)


def test_device_inference_switch_against_the_default_simple_test(tmp_path):
    """One viewpoint, fp32.  The encoder pass is taken ONCE and handed to both calls (as tests/test_det_decode_gpu.py reuses
    the head's outputs): two encoder passes differ in their last bits, which is not what the switch is about -- on one
    volume the pairs are the reference's bit for bit and the boxes the same wherever the scores are distinct."""
    from test_det_decode_cpu import distinct_top
    syn, reg = pkg('synthetic'), pkg('registry')
    det = reg.build_detector(dict(type='VoxelFormer', pts_bbox_head=cases.vocc_head_cfg(), train_cfg=dict(pts=cases.VOCC_TRAIN_CFG))).eval()
    assert det.device_inference is False
    h = det.pts_bbox_head
    cw = h.code_weights.detach().clone()
    syn.load_seeded(h, 7)
    h.code_weights.data.copy_(cw)
    det.to(DEV)
    names = ['scanA_vp0']
    store = _store(tmp_path, syn.vit_features(1, seed=0), names)
    dense = np.random.default_rng(9).integers(0, 17, size=(1, 504000))
    metas = _metas(tmp_path, store, names, [cases.detection_gt(seed=40, num_gt=3)], [_sparse(d) for d in dense])
    thr = threshold()
    volumes, encode = [], h.transformer.get_voxel_features

    def once(*args, **kwargs):
        if not volumes:
            volumes.append(encode(*args, **kwargs))
        return volumes[0]

    h.transformer.get_voxel_features = once
    seen = []
    hook = h.register_forward_hook(lambda mod, args, out: seen.append(out) if isinstance(out, dict) else None)
    try:
        with torch.no_grad():
            vol_w, boxes_w, occ_w = det.simple_test(metas, occ_threshold=thr)
            det.device_inference = True
            vol_g, boxes_g, occ_g = det.simple_test(metas, occ_threshold=thr)
    finally:
        hook.remove()
        del h.transformer.get_voxel_features
    assert len(volumes) == 1 and len(seen) == 1 and torch.equal(vol_g, vol_w)
    got, want = occ_g['occupancy_preds'], occ_w['occupancy_preds'].cpu()
    assert got.dtype == torch.int64 and got.device.type == 'cpu' and len(want) > 0 and torch.equal(got, want)
    assert occ_g['flow_preds'] is None and distinct_top(h.bbox_coder, seen[0])
    g, w = boxes_g[0]['pts_bbox'], boxes_w[0]['pts_bbox']
    assert g['boxes_3d'].device.type == 'cpu' and g['boxes_3d'].shape == w['boxes_3d'].shape and len(w['boxes_3d']) > 0
    assert g['labels_3d'].dtype == w['labels_3d'].dtype and torch.equal(g['labels_3d'], w['labels_3d'])
    assert rel_l2(g['boxes_3d'], w['boxes_3d']) <= 1e-5 and rel_l2(g['scores_3d'], w['scores_3d']) <= 1e-5
