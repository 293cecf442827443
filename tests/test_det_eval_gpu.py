"""Device side of the detection mAP / mAR evaluation: ``ver_box3d_overlaps`` against the float64 host model with a bound
taken from the float32 run of that model, ``ver_det_match`` against the host protocol record for record, and
``DeviceDetMetrics`` end to end on the outputs of a built vocc head."""
import math

import numpy as np
import pytest
import torch

import cases
import det_eval_helper as H
from test_det_eval_cpu import closed_form_cases
from util import pkg

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def dm():
    return pkg('detection_metrics')


def on_gpu(batch):
    return {k: T(v).cuda() for k, v in batch.items()}


def run_match(batch, thresholds, classes=cases.CLASS_NUM, npos=None):
    hip = pkg('hipops')
    d = on_gpu(batch)
    npos = torch.zeros(classes, dtype=torch.int64, device='cuda') if npos is None else npos
    iou_max, gt_index, bits = hip.det_match(d['pb'], d['pl'], d['ps'], d['pv'], d['gb'], d['gl'], d['ngt'], thresholds, npos)
    return iou_max.cpu().numpy(), gt_index.cpu().numpy(), bits.cpu().numpy(), npos.cpu().numpy()


def host_match(batch, thresholds, classes=cases.CLASS_NUM):
    iou_max, gt_index, bits, count = dm().det_match_host(batch['pb'], batch['pl'], batch['ps'], batch['pv'], batch['gb'],
                                                         batch['gl'], batch['ngt'], thresholds, classes)
    npos = np.zeros(classes, np.int64)
    for c, n in count.items():
        npos[c] = n
    return iou_max, gt_index, bits, npos


IOU_SHAPES = ((3, 1, 1), (3, 50, 12), (2, 130, 40), (1, 256, 64))
COUNTS = {(3, 1, 1): ([0, 1, 1], [1, 0, 1]), (3, 50, 12): ([0, 50, 25], [12, 12, 4]), (2, 130, 40): ([130, 77], [0, 40]),
          (1, 256, 64): ([256], [63])}                     # valid boxes per sample: none, all, and in between


@pytest.fixture(scope='module')
def iou_bound():
    """E32: the largest deviation of the float32 run of the host model from its float64 run over every pair the accuracy
    test looks at (the four shapes, the closed forms, identical boxes at 64 poses).  The kernel gets 4 x E32: another order
    of operations, FMA contraction, sinf / cosf instead of numpy's -- still 10 x under the 1e-4 screening margin."""
    m = dm()
    rng = np.random.default_rng(7)
    sets = []
    for s, ca, cb in IOU_SHAPES:
        a, b = H.random_boxes(rng, s * ca).reshape(s, ca, 7), H.random_boxes(rng, s * cb).reshape(s, cb, 7)
        k = min(ca, cb)
        near = a[:, :k] + rng.normal(0, 0.1, (s, k, 7)).astype(np.float32)
        near[..., 3:6] = np.maximum(near[..., 3:6], 0.05)
        b[:, :k] = np.where(rng.random((s, k, 1)) < 0.5, near, b[:, :k])
        na, nb = (np.array(v, np.int32) for v in COUNTS[(s, ca, cb)])
        sets.append((a, b, na, nb))
    forms = closed_form_cases()
    fa = np.array([[f[0]] for f in forms], np.float32)
    fb = np.array([[f[1]] for f in forms], np.float32)
    poses = H.random_boxes(rng, 64).reshape(64, 1, 7)
    e32 = 0.0
    refs = []
    for a, b, *_ in sets + [(fa, fb), (poses, poses)]:
        r64 = np.stack([m.box3d_overlaps_host(x, y) for x, y in zip(a, b)])
        r32 = np.stack([m.box3d_overlaps_host(x, y, dtype=np.float32) for x, y in zip(a, b)])
        e32 = max(e32, float(np.abs(r32 - r64).max()))
        refs.append(r64)
    assert 1e-8 < e32 < 2.5e-5                             # a float32 clip of room-scale boxes; 4 x E32 stays under 1e-4
    return dict(sets=sets, forms=(fa, fb, np.array([f[2] for f in forms])), poses=poses, refs=refs, e32=e32)


def test_box3d_overlaps_against_the_float64_model(iou_bound):
    hip = pkg('hipops')
    bound, worst = 4.0 * iou_bound['e32'], 0.0
    for (a, b, na, nb), ref in zip(iou_bound['sets'], iou_bound['refs']):
        got = hip.box3d_overlaps(T(a).cuda(), T(b).cuda(), T(na).cuda(), T(nb).cuda()).cpu().numpy()
        full = hip.box3d_overlaps(T(a).cuda(), T(b).cuda()).cpu().numpy()
        assert got.shape == ref.shape and got.dtype == np.float32 and np.isfinite(got).all()
        live = (np.arange(a.shape[1])[None, :, None] < na[:, None, None]) & (np.arange(b.shape[1])[None, None, :] < nb[:, None, None])
        assert not got[~live].any()                        # slots beyond the counts: written, as 0
        assert (ref > 0.05).sum() >= len(a) or a.shape[1] == 1
        err = max(float(np.abs(got - ref)[live].max()) if live.any() else 0.0, float(np.abs(full - ref).max()))
        assert (full[ref == 0] == 0).all()                 # disjoint boxes: a true zero
        worst = max(worst, err)
        print('box3d_overlaps %s: max |kernel - float64| = %.3e (E32 %.3e)' % (a.shape[:2] + b.shape[1:2], err, iou_bound['e32']))
    fa, fb, want = iou_bound['forms']
    got = hip.box3d_overlaps(T(fa).cuda(), T(fb).cuda()).cpu().numpy()[:, 0, 0]
    print('closed forms: max |kernel - value| = %.3e' % float(np.abs(got - want).max()))
    worst = max(worst, float(np.abs(got - want).max()), float(np.abs(got - iou_bound['refs'][-2][:, 0, 0]).max()))
    assert got[0] == pytest.approx(1.0, abs=bound) and got[1] == 0.0 and got[2] == 0.0 and got[-1] == 0.0
    poses = T(iou_bound['poses']).cuda()
    same = hip.box3d_overlaps(poses, poses).cpu().numpy()[:, 0, 0]
    worst = max(worst, float(np.abs(same - 1.0).max()))
    print('identical boxes at 64 poses: max |kernel - 1| = %.3e;  overall %.3e against 4 x E32 = %.3e' % (float(np.abs(same - 1.0).max()), worst, bound))
    assert worst <= bound
    # our definition for boxes the reference leaves undefined: IoU 0, not NaN
    bad = np.tile(np.array([0, 0, 0, 2, 2, 1, 0], np.float32), (1, 6, 1))
    bad[0, 0, 3], bad[0, 1, 4], bad[0, 2, 5], bad[0, 3, 0], bad[0, 4, 6] = 0.0, -1.0, 0.0, np.nan, np.inf
    got = hip.box3d_overlaps(T(bad).cuda(), T(bad).cuda()).cpu().numpy()[0]
    assert np.isfinite(got).all() and not got[:5].any() and not got[:, :5].any() and got[5, 5] == pytest.approx(1.0, abs=bound)
    assert hip.box3d_overlaps(poses[:0], poses[:0]).shape == (0, 1, 1) and hip.box3d_overlaps(poses[:, :0], poses).shape == (64, 0, 1)
    with pytest.raises(ValueError, match=r'\[S, N, 7\]'):
        hip.box3d_overlaps(poses[..., :6], poses)
    with pytest.raises(TypeError, match='float32'):
        hip.box3d_overlaps(poses.double(), poses)
    with pytest.raises(ValueError, match='one int32 per sample'):
        hip.box3d_overlaps(poses, poses, na=torch.zeros(3, dtype=torch.int32, device='cuda'))


MATCH_CASES = [(t, p) for t in (1, 4, 8) for p in (1, 50, 100, 130)]
GCAP = {1: 12, 50: 12, 100: 40, 130: 40}
SAMPLES = 10


@pytest.fixture(scope='module')
def match_batches():
    out = {}
    for i, (t, p) in enumerate(MATCH_CASES):
        thr = {1: (0.25,), 4: H.THR, 8: H.THR8}[t]
        g = GCAP[p]
        counts = [0, g] + list(np.random.default_rng(100 + i).integers(0, g + 1, SAMPLES - 2))
        out[(t, p)] = (thr,) + H.screened_batch(200 + i, SAMPLES, p, g, thr, counts)
    return out


def test_screening_redraws_few_samples(match_batches):
    redrawn = sum(v[2] for v in match_batches.values())
    print('screening: %d of %d samples redrawn' % (redrawn, SAMPLES * len(match_batches)))
    assert redrawn < 0.1 * SAMPLES * len(match_batches)


@pytest.mark.parametrize('t,p', MATCH_CASES)
def test_det_match_records_equal_the_host_protocol(match_batches, iou_bound, t, p):
    thr, batch, _ = match_batches[(t, p)]
    iou_max, gt_index, bits, npos = run_match(batch, thr)
    w_iou, w_index, w_bits, w_npos = host_match(batch, thr)
    assert gt_index.dtype == np.int32 and bits.dtype == np.uint8 and iou_max.shape == (SAMPLES, p)
    assert np.array_equal(gt_index, w_index) and np.array_equal(bits, w_bits) and np.array_equal(npos, w_npos)
    assert float(np.abs(iou_max - w_iou).max()) <= 4.0 * iou_bound['e32']
    if p > 1:
        assert (bits > 0).sum() >= 3 and (bits == 0).any() and (gt_index == -1).any() and len(np.unique(gt_index)) > 3
        taken = [(w_index[s, d] >= 0) and (w_iou[s, d] > thr[0]) and not (w_bits[s, d] & 1) for s in range(SAMPLES) for d in range(p)]
        assert any(taken)                                  # a prediction whose ground truth an earlier one had claimed


def test_det_match_edge_cases(iou_bound):
    hip = pkg('hipops')
    batch, _ = H.screened_batch(300, 4, 50, 12, H.THR, counts=[12, 12, 5, 12])
    want = host_match(batch, H.THR)
    # ngt above the capacity, and below zero: clamped
    odd = dict(batch, ngt=np.array([12, 99, 5, 12], np.int32))
    got = run_match(odd, H.THR)
    assert all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))
    neg = dict(batch, ngt=np.array([-3, 12, 5, 12], np.int32))
    w_neg = host_match(dict(batch, ngt=np.array([0, 12, 5, 12], np.int32)), H.THR)
    got = run_match(neg, H.THR)
    assert all(np.array_equal(g, w) for g, w in zip(got[1:], w_neg[1:])) and not got[2][0].any() and (got[1][0] == -1).all()
    # every prediction invalid: nothing matched, the ground truths still counted
    none = dict(batch, pv=np.zeros_like(batch['pv']))
    iou_max, gt_index, bits, npos = run_match(none, H.THR)
    assert not iou_max.any() and (gt_index == -1).all() and not bits.any() and np.array_equal(npos, want[3])
    # some invalid: the others' records are those of the batch without them
    some = dict(batch, pv=(np.arange(50)[None, :] % 3 != 0).astype(np.uint8).repeat(4, 0))
    got, w_some = run_match(some, H.THR), host_match(some, H.THR)
    assert all(np.array_equal(g, w) for g, w in zip(got[1:], w_some[1:])) and (got[1][:, ::3] == -1).all()
    # labels outside [0, num_classes): such predictions match nothing, such ground truths are neither counted nor matched
    pl, gl = batch['pl'].copy(), batch['gl'].copy()
    pl[:, 0:50:7], gl[:, 0:12:5] = 17, -1
    pl[:, 3], gl[:, 1] = -2, 40
    out = dict(batch, pl=pl, gl=gl)
    got, w_out = run_match(out, H.THR), host_match(out, H.THR)
    assert all(np.array_equal(g, w) for g, w in zip(got[1:], w_out[1:]))
    assert (got[1][:, 0:50:7] == -1).all() and int(got[3].sum()) == int(sum(min(n, 12) - len([j for j in (0, 1, 5, 10) if j < n])
                                                                            for n in batch['ngt']))
    # fewer classes than labels: the same rule, and npos has that many entries
    got, w_five = run_match(batch, H.THR, classes=5), host_match(batch, H.THR, classes=5)
    assert all(np.array_equal(g, w) for g, w in zip(got[1:], w_five[1:])) and got[3].shape == (5,)
    # no ground-truth slots at all: every valid prediction is a false positive
    empty = dict(batch, gb=np.zeros((4, 0, 7), np.float32), gl=np.zeros((4, 0), np.int32), ngt=np.zeros(4, np.int32))
    iou_max, gt_index, bits, npos = run_match(empty, H.THR)
    assert not iou_max.any() and (gt_index == -1).all() and not bits.any() and not npos.any()
    # npos is accumulated, never cleared
    npos = torch.full((17,), 5, dtype=torch.int64, device='cuda')
    assert np.array_equal(run_match(batch, H.THR, npos=npos)[3], want[3] + 5)
    assert np.array_equal(run_match(batch, H.THR, npos=npos)[3], 2 * want[3] + 5)
    d = on_gpu(batch)
    with pytest.raises(ValueError, match='thresholds'):
        hip.det_match(d['pb'], d['pl'], d['ps'], d['pv'], d['gb'], d['gl'], d['ngt'], (), npos)
    with pytest.raises(ValueError, match='P \\* G'):
        hip.det_match(*(d[k].repeat_interleave(30, 1) for k in ('pb', 'pl', 'ps', 'pv', 'gb', 'gl')), d['ngt'], H.THR, npos)
    with pytest.raises(TypeError, match='int32'):
        hip.det_match(d['pb'], d['pl'].long(), d['ps'], d['pv'], d['gb'], d['gl'], d['ngt'], H.THR, npos)
    with pytest.raises(ValueError, match='npos'):
        hip.det_match(d['pb'], d['pl'], d['ps'], d['pv'], d['gb'], d['gl'], d['ngt'], H.THR, npos.int())


def test_equal_scores_are_ordered_by_slot():
    """Three predictions on one ground truth with IoU 1, 0.6 and 1/3, all of score 0.5, in the slots 2, 0 and 1: slot 0 goes
    first and claims the ground truth at the thresholds below ITS IoU 0.6; slot 1 (1/3) gets nothing; slot 2 (IoU 1) is a
    true positive only where slot 0 was none: at 0.75.  With a higher score, slot 2 takes them all."""
    gt = np.array([[[0, 0, 0, 2, 2, 1, 0]]], np.float32)
    pb = np.array([[[0.5, 0, 0, 2, 2, 1, 0], [1, 0, 0, 2, 2, 1, 0], [0, 0, 0, 2, 2, 1, 0]]], np.float32)   # 3 / 5, 1 / 3, 1
    batch = dict(pb=pb, pl=np.full((1, 3), 4, np.int32), ps=np.full((1, 3), 0.5, np.float32), pv=np.ones((1, 3), np.uint8),
                 gb=gt, gl=np.full((1, 1), 4, np.int32), ngt=np.ones(1, np.int32))
    iou_max, gt_index, bits, npos = run_match(batch, H.THR)
    assert iou_max[0] == pytest.approx([0.6, 1.0 / 3.0, 1.0], abs=1e-6) and gt_index.tolist() == [[0, 0, 0]]
    assert bits.tolist() == [[0b0111, 0, 0b1000]] and npos[4] == 1 and npos.sum() == 1
    assert np.array_equal(bits, host_match(batch, H.THR)[2])
    batch['ps'][0, 2] = 0.51
    bits = run_match(batch, H.THR)[2]
    assert bits.tolist() == [[0, 0, 0b1111]] and np.array_equal(bits, host_match(batch, H.THR)[2])


def test_one_launch_for_a_thousand_samples(iou_bound):
    thr = H.THR
    batch, redrawn = H.screened_batch(400, 1000, 20, 6, thr)
    assert redrawn < 100
    got, want = run_match(batch, thr), host_match(batch, thr)
    assert all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))
    assert float(np.abs(got[0] - want[0]).max()) <= 4.0 * iou_bound['e32'] and int(want[3].sum()) == int(batch['ngt'].sum())


def test_device_metrics_end_to_end_on_a_built_head():
    """``DeviceDetMetrics`` over three batches of random outputs of the vocc head on the device against ``indoor_eval`` on the
    lists ``get_bboxes`` returns for the same outputs: the flags agree, and the arithmetic after them is float64 on both sides."""
    m = dm()
    head = H.build_head('cuda')
    batches = H.head_batches(head)
    want = m.indoor_eval(*H.lists_to_annos(batches), H.THR)
    metrics = m.DeviceDetMetrics(cases.CLASS_NUM, H.THR, device='cuda')
    for preds, gts, *_ in batches:
        metrics.add(head, preds, gts)
    assert metrics.npos.is_cuda and all(t.is_cuda for part in metrics._parts for t in part)
    got = metrics.get_stats()
    assert sorted(got) == sorted(want) and len(want) >= 2 * len(H.THR) * 6
    for k in want:
        assert got[k] == pytest.approx(want[k], abs=1e-12, nan_ok=True), k
    finite = [v for k, v in want.items() if '_rec_0.10' in k and not math.isnan(v)]
    assert len(finite) >= 5 and sum(finite) > 0
    # two shards counted on the device, merged on the host
    shard = m.DeviceDetMetrics(cases.CLASS_NUM, H.THR, device='cuda').add(head, *batches[0][:2])
    rest = m.DeviceDetMetrics(cases.CLASS_NUM, H.THR, device='cuda')
    for preds, gts, *_ in batches[1:]:
        rest.add(head, preds, gts)
    assert shard.merge(rest.state()).get_stats() == pytest.approx(got, abs=0, nan_ok=True)
