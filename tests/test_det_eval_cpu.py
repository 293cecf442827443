"""CPU side of the detection mAP / mAR evaluation: the two entry points' declaration, export and argument checks, the
float64 host model of the rotated box IoU against closed forms, the indoor protocol on hand-worked cases, ``DeviceDetMetrics``
on CPU tensors (the host functions in place of the kernels) and ``decode_padded`` against ``decode``."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import cases
import det_eval_helper as H
from util import ROOT, pkg


def dm():
    return pkg('detection_metrics')


def box(x=0.0, y=0.0, z=0.0, dx=2.0, dy=2.0, dz=1.0, yaw=0.0):
    return [x, y, z, dx, dy, dz, yaw]


def test_entry_points_are_declared_exported_and_the_abi_number_stays():
    text = open(os.path.join(ROOT, 'include', 'ver_ops.h')).read()
    assert re.search(r'int ver_box3d_overlaps\(const float\* a, const int32_t\* na, const float\* b, const int32_t\* nb, '
                     r'float\* iou,\s*int S, int Acap, int Bcap, void\* stream\);', text)
    assert re.search(r'int ver_det_match\(const float\* pred_boxes, const int32_t\* pred_labels, const float\* pred_scores,\s*'
                     r'const uint8_t\* pred_valid, const float\* gt_boxes, const int32_t\* gt_labels, const int32_t\* ngt,\s*'
                     r'const float\* thresholds, int num_thresholds, float\* iou_max, int32_t\* gt_index,\s*'
                     r'uint8_t\* tp_bits, int64_t\* npos, int num_classes, int S, int Pcap, int Gcap, void\* stream\);', text)
    for cited in ('mp3docc_dataset.py:304-384', 'indoor_eval.py:196', 'indoor_eval.py:102', 'indoor_eval.py:54-143'):
        assert cited in text, cited
    assert 'non-finite entry or a dimension <= 0' in text and '#define VER_ABI_VERSION 31' in text
    hip = pkg('hipops')
    pkg('csrc.build').build_hip(verbose=False)
    handle = ctypes.CDLL(hip.LIB_PATH)
    assert hasattr(handle, 'ver_box3d_overlaps') and hasattr(handle, 'ver_det_match')
    assert handle.ver_abi_version() == 31 == hip.ABI_VERSION
    ptr, i = ctypes.c_void_p, ctypes.c_int
    assert hip.PROTOTYPES['ver_box3d_overlaps'] == (i, [ptr] * 5 + [i] * 3 + [ptr])
    assert hip.PROTOTYPES['ver_det_match'] == (i, [ptr] * 8 + [i] + [ptr] * 4 + [i] * 4 + [ptr])


def test_argument_validation_without_gpu():
    """Null pointers and sizes outside the supported range come back as the documented codes, with a message, before
    anything touches a device."""
    hip = pkg('hipops')
    lib = hip.lib()
    buf = (ctypes.c_float * 64)()
    thr = (ctypes.c_float * 9)(*([0.5] * 9))

    def match(ptrs=None, nthr=4, classes=17, s=2, p=50, g=12):
        a = [buf] * 7 + [thr] + [buf] * 4 if ptrs is None else ptrs
        return lib.ver_det_match(*a[:8], nthr, *a[8:], classes, s, p, g, None)

    assert lib.ver_box3d_overlaps(None, None, None, None, None, 0, 5, 5, None) == 0          # S == 0: nothing to do
    assert lib.ver_box3d_overlaps(None, None, None, None, None, 3, 0, 5, None) == 0
    for hole in (0, 2, 4):
        a = [buf, None, buf, None, buf]
        a[hole] = None
        assert lib.ver_box3d_overlaps(*a, 2, 5, 5, None) == -1 and b'null' in lib.ver_last_error(), hole
    assert lib.ver_box3d_overlaps(buf, None, buf, None, buf, -1, 5, 5, None) == -1 and b'bad sizes' in lib.ver_last_error()
    assert lib.ver_box3d_overlaps(buf, None, buf, None, buf, 2, 5, -5, None) == -1 and b'bad sizes' in lib.ver_last_error()

    assert match([None] * 12, s=0) == 0                                                     # S == 0: nothing to do
    for hole in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11):
        a = [buf] * 7 + [thr] + [buf] * 4
        a[hole] = None
        assert match(a) == -1 and b'null' in lib.ver_last_error(), hole
    for nthr in (0, 9, -1):
        assert match(nthr=nthr) == -1 and b'num_thresholds' in lib.ver_last_error(), nthr
    for p, g in ((0, 12), (-1, 12), (50, -1)):
        assert match(p=p, g=g) == -1 and b'bad sizes' in lib.ver_last_error(), (p, g)
    assert match(classes=0) == -1 and b'bad sizes' in lib.ver_last_error()
    assert match(s=-1) == -1 and b'bad sizes' in lib.ver_last_error()
    for p, g in ((5, 3277), (16385, 1), (1025, 1), (1, 1025), (129, 128)):                  # 5 * 3277 = 16 385 pairs
        assert match(p=p, g=g) == -2 and b'16384 pairs' in lib.ver_last_error(), (p, g)
    assert (hip.DET_MATCH_MAX_BOXES, hip.DET_MATCH_MAX_PAIRS, hip.DET_MATCH_MAX_THRESHOLDS) == (1024, 16384, 8)
    with pytest.raises(RuntimeError, match='GPU'):                                          # no torch fallback inside hipops
        hip.box3d_overlaps(torch.zeros(1, 2, 7), torch.zeros(1, 3, 7))
    with pytest.raises(RuntimeError, match='GPU'):
        hip.det_match(torch.zeros(1, 2, 7), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2),
                      torch.ones(1, 2, dtype=torch.uint8), torch.zeros(1, 3, 7), torch.zeros(1, 3, dtype=torch.int32),
                      torch.zeros(1, dtype=torch.int32), (0.5,), torch.zeros(17, dtype=torch.int64))


def closed_form_cases():
    """(a, b, IoU) with the value worked out by hand."""
    r2 = math.sqrt(2.0)
    return [
        (box(1, -2, 0.5, 3, 1.5, 2, 0.7), box(1, -2, 0.5, 3, 1.5, 2, 0.7), 1.0),          # identical
        (box(), box(x=2.0), 0.0),                                                         # touching along x
        (box(), box(z=1.0), 0.0),                                                         # touching in height
        (box(), box(x=1.0), 1.0 / 3.0),                                                   # 2 x 2 x 1 shifted by 1: 2 / (4 + 4 - 2)
        (box(), box(yaw=math.pi / 4), (r2 - 1) / (2 - r2)),                               # octagon 8 (sqrt2 - 1) of two squares
        (box(), box(z=0.5), 1.0 / 3.0),                                                   # half the height: 2 / (4 + 4 - 2)
        (box(dx=4, dy=4, dz=2), box(x=0.5, y=-0.5, z=0.5, dx=1, dy=2, dz=1, yaw=math.pi / 2), 2.0 / 32.0),   # inside
        (box(), box(x=5.0, y=5.0), 0.0),                                                  # far apart
    ]


def test_host_overlaps_against_closed_forms():
    m = dm()
    for a, b, want in closed_form_cases():
        got = m.box3d_overlaps_host(np.array([a]), np.array([b]))
        assert got.shape == (1, 1) and got.dtype == np.float64
        assert got[0, 0] == pytest.approx(want, abs=1e-12), (a, b)
        assert m.box3d_overlaps_host(np.array([b]), np.array([a]))[0, 0] == pytest.approx(want, abs=1e-12)
    assert (2 - 1) / math.sqrt(2) == pytest.approx((math.sqrt(2) - 1) / (2 - math.sqrt(2)) , abs=1e-15)   # = 1 / sqrt 2
    # yaw and yaw + pi describe the same box
    rng = np.random.default_rng(5)
    a, b = H.random_boxes(rng, 20).astype(np.float64), H.random_boxes(rng, 15).astype(np.float64)
    b[:5] = a[:5] + rng.normal(0, 0.1, (5, 7))
    turned = a.copy()
    turned[:, 6] += math.pi
    ref = m.box3d_overlaps_host(a, b)
    assert ref.shape == (20, 15) and (ref > 0).sum() >= 5 and ref.max() <= 1.0
    assert np.abs(m.box3d_overlaps_host(turned, b) - ref).max() < 1e-12
    assert np.abs(np.diag(m.box3d_overlaps_host(a, a)) - 1.0).max() < 1e-12               # identical boxes at random poses
    assert np.abs(ref - m.box3d_overlaps_host(b, a).T).max() < 1e-12
    # the float32 run of the same model stays float32 and close
    r32 = m.box3d_overlaps_host(a.astype(np.float32), b.astype(np.float32), dtype=np.float32)
    assert r32.dtype == np.float32 and np.abs(r32 - m.box3d_overlaps_host(a.astype(np.float32), b.astype(np.float32))).max() < 1e-4
    # a degenerate or non-finite box overlaps nothing: 0, not NaN
    good = np.array([box()])
    for bad in (box(dx=0.0), box(dy=-1.0), box(dz=0.0), box(x=float('nan')), box(yaw=float('inf')), box(dz=float('nan'))):
        assert m.box3d_overlaps_host(good, np.array([bad]))[0, 0] == 0.0
        assert m.box3d_overlaps_host(np.array([bad]), good)[0, 0] == 0.0
        assert np.isfinite(m.box3d_overlaps_host(np.array([bad, box()]), np.array([box(), bad]))).all()
    assert m.box3d_overlaps_host(np.zeros((0, 7)), good).shape == (0, 1)


def anno(boxes, labels):
    return dict(gt_num=len(boxes), gt_boxes_upright_depth=np.array(boxes, dtype=np.float64).reshape(-1, 7), **{'class': np.array(labels, dtype=np.int64)})


def det(boxes, scores, labels):
    return dict(boxes_3d=np.array(boxes, dtype=np.float64).reshape(-1, 7), scores_3d=np.array(scores, dtype=np.float64),
                labels_3d=np.array(labels, dtype=np.int64))


def test_second_prediction_on_a_taken_ground_truth_is_a_false_positive():
    """gt0 = 2 x 2 x 1 at x = 0, gt1 the same at x = 3.  p0 = gt0 (score .9): IoU 1.  p1 at x = 1.2 (score .8) overlaps gt0
    over 0.8 m (1.6 / 6.4 = 0.25) and gt1 over 0.2 m (0.4 / 7.6 = 0.0526): its best, gt0, is taken, and it does NOT fall back
    to gt1 although 0.0526 > 0.05.  tp = [1, 0], npos = 2: recall [.5, .5], precision [1, .5], AP = .5 * 1 = .5."""
    m = dm()
    gts = [anno([box(), box(x=3.0)], [0, 0])]
    dts = [det([box(), box(x=1.2)], [0.9, 0.8], [0, 0])]
    iou = m.box3d_overlaps_host(dts[0]['boxes_3d'], gts[0]['gt_boxes_upright_depth'])
    assert iou == pytest.approx(np.array([[1.0, 0.0], [0.25, 0.4 / 7.6]]), abs=1e-12)
    res = m.indoor_eval(gts, dts, (0.05, 0.2), {0: 'chair'})
    assert res == pytest.approx({'chair_AP_0.05': 0.5, 'chair_rec_0.05': 0.5, 'mAP_0.05': 0.5, 'mAR_0.05': 0.5,
                                 'chair_AP_0.20': 0.5, 'chair_rec_0.20': 0.5, 'mAP_0.20': 0.5, 'mAR_0.20': 0.5}, abs=1e-15)
    iou_max, gt_index, bits, npos = m.det_match_host(dts[0]['boxes_3d'][None], [[0, 0]], [[0.9, 0.8]], [[1, 1]],
                                                     gts[0]['gt_boxes_upright_depth'][None], [[0, 0]], [2], (0.05, 0.2), 17)
    assert gt_index.tolist() == [[0, 0]] and bits.tolist() == [[3, 0]] and npos == {0: 2}
    assert iou_max[0] == pytest.approx([1.0, 0.25], abs=1e-12)
    # the other way round in score: p1 claims gt0 first at both thresholds, p0 (IoU 1) is the false positive
    res = m.indoor_eval(gts, [det([box(), box(x=1.2)], [0.8, 0.9], [0, 0])], (0.05, 0.2), {0: 'chair'})
    assert res['chair_AP_0.20'] == pytest.approx(0.5, abs=1e-15) and res['chair_rec_0.20'] == 0.5
    # equal scores: the earlier slot goes first
    _, _, bits, _ = m.det_match_host(dts[0]['boxes_3d'][None], [[0, 0]], [[0.5, 0.5]], [[1, 1]],
                                     gts[0]['gt_boxes_upright_depth'][None], [[0, 0]], [2], (0.2,), 17)
    assert bits.tolist() == [[1, 0]]


def test_iou_equal_to_the_threshold_is_no_true_positive():
    """A 2 x 1 x 1 box inside a 2 x 2 x 1 one: 2 / (4 + 2 - 2) = 0.5 exactly.  `iou > thr` is strict."""
    m = dm()
    gts, dts = [anno([box()], [3])], [det([box(y=0.5, dy=1.0)], [0.7], [3])]
    assert m.box3d_overlaps_host(dts[0]['boxes_3d'], gts[0]['gt_boxes_upright_depth'])[0, 0] == 0.5
    res = m.indoor_eval(gts, dts, (0.25, 0.5))
    assert res['3_AP_0.25'] == 1.0 and res['3_rec_0.25'] == 1.0 and res['3_AP_0.50'] == 0.0 and res['3_rec_0.50'] == 0.0
    assert sorted(res) == ['3_AP_0.25', '3_AP_0.50', '3_rec_0.25', '3_rec_0.50', 'mAP_0.25', 'mAP_0.50', 'mAR_0.25', 'mAR_0.50']


def test_classes_without_ground_truth_or_predictions_and_an_empty_image():
    """Image 0: gt of class 0 and class 2; predictions of class 0 (exact) and class 1 (nothing to match).  Image 1: no
    ground truth; one prediction of class 0 with the highest score: a false positive ranked first.
    Class 0: order = (img 1, .95, fp), (img 0, .9, tp); npos 1: recall [0, 1], precision [0, .5]; AP = 1 * .5.
    Class 1: predictions, npos 0: recall = 0 / 0 = NaN, AP NaN.  Class 2: ground truth, no prediction: 0 and 0."""
    m = dm()
    gts = [anno([box(), box(x=4.0)], [0, 2]), dict(gt_num=0, gt_boxes_upright_depth=np.zeros((0, 7)), **{'class': np.zeros(0, np.int64)})]
    dts = [det([box(), box(x=4.0)], [0.9, 0.6], [0, 1]), det([box()], [0.95], [0])]
    with np.errstate(all='ignore'):
        res = m.indoor_eval(gts, dts, (0.25,), {0: 'bed', 1: 'sofa', 2: 'tv'})
    assert res['bed_AP_0.25'] == 0.5 and res['bed_rec_0.25'] == 1.0
    assert math.isnan(res['sofa_AP_0.25']) and math.isnan(res['sofa_rec_0.25'])
    assert res['tv_AP_0.25'] == 0.0 and res['tv_rec_0.25'] == 0.0
    assert math.isnan(res['mAP_0.25']) and math.isnan(res['mAR_0.25'])
    assert len(res) == 8
    curves = m.eval_det((gts, dts), (0.25,))
    assert sorted(curves) == [0, 1, 2]
    recall, precision, ap = curves[0][0]
    assert recall.tolist() == [0.0, 1.0] and precision.tolist() == [0.0, 0.5] and ap.tolist() == [0.5]
    # without the class nobody can match, the means are numbers
    res = m.indoor_eval(gts, [det([box()], [0.9], [0]), det([box()], [0.95], [0])], (0.25,))
    assert res['mAP_0.25'] == 0.25 and res['mAR_0.25'] == 0.5


def test_average_precision_of_a_known_staircase():
    """recall [.25, .5, .5, .75], precision [1, 1, 2/3, .75]: envelope from the right [1, 1, .75, .75], area
    .25 * 1 + .25 * 1 + .25 * .75 (+ .25 * 0 up to recall 1) = .6875; 11 points: 1 at recall 0 - .5 (six), .75 at .6, .7."""
    m = dm()
    rec, pre = np.array([.25, .5, .5, .75]), np.array([1.0, 1.0, 2.0 / 3.0, .75])
    ap = m.average_precision(rec, pre)
    assert ap.dtype == np.float64 and ap.shape == (1,) and ap[0] == pytest.approx(0.6875, abs=1e-15)
    assert m.average_precision(rec, pre, mode='11points')[0] == pytest.approx(7.5 / 11, abs=1e-15)
    both = m.average_precision(np.stack([rec, rec]), np.stack([pre, pre * 0.5]))
    assert both == pytest.approx([0.6875, 0.34375], abs=1e-15)
    with pytest.raises(ValueError, match='Unrecognized mode'):
        m.average_precision(rec, pre, mode='voc')


@pytest.fixture(scope='module')
def head():
    return H.build_head()


def test_decode_padded_equals_decode_sample_by_sample(head):
    coders = pkg('dense_heads.coders')
    for coder in (head.bbox_coder, coders.NMSFreeCoder(cases.PC_RANGE, post_center_range=[-6, -6, -3, 6, 6, 3], max_num=70,
                                                       score_threshold=0.99, num_classes=cases.CLASS_NUM)):
        preds = H.random_head_outputs(21, 3)
        want = coder.decode(preds)
        boxes, scores, labels, valid = coder.decode_padded(preds)
        k = coder.max_num
        assert boxes.shape == (3, k, 9) and scores.shape == labels.shape == valid.shape == (3, k)
        assert valid.dtype == torch.uint8 and labels.dtype == torch.int64
        kept = [int(v.sum()) for v in valid]
        assert 0 < min(kept) and max(kept) < k                                            # both kinds of slot occur
        for b in range(3):
            keep = valid[b].bool()
            assert torch.equal(boxes[b][keep], want[b]['bboxes']) and torch.equal(scores[b][keep], want[b]['scores'])
            assert torch.equal(labels[b][keep], want[b]['labels'])
            assert bool((scores[b][:-1] >= scores[b][1:]).all())
    got = head.get_bboxes_padded(preds)
    lists = head.get_bboxes(preds)
    for b in range(3):
        keep = got[3][b].bool()
        assert torch.equal(got[0][b][keep], lists[b][0]) and torch.equal(got[1][b][keep], lists[b][1])
        assert torch.equal(got[2][b][keep], lists[b][2])


def test_device_metrics_on_cpu_tensors_equal_indoor_eval_and_merge(head):
    m = dm()
    batches = H.head_batches(head)
    want = m.indoor_eval(*H.lists_to_annos(batches), H.THR)
    recalls = {t: [v for k, v in want.items() if k.endswith('_rec_%.2f' % t) and not math.isnan(v)] for t in H.THR}
    assert len(recalls[0.10]) >= 5 and 0.0 < sum(recalls[0.75]) < sum(recalls[0.10]) <= len(recalls[0.10])
    assert any(math.isnan(v) for v in want.values())                                     # a predicted class without ground truth
    whole = m.DeviceDetMetrics(cases.CLASS_NUM, H.THR)
    for preds, gts, *_ in batches:
        assert whole.add(head, preds, gts) is whole
    got = whole.get_stats()
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], abs=1e-12, nan_ok=True), k
    assert int(whole.npos.sum()) == sum(len(b[3][i]) for b in batches for i in range(len(b[3])))
    # two shards, merged in order, are the whole
    first, second = m.DeviceDetMetrics(cases.CLASS_NUM, H.THR), m.DeviceDetMetrics(cases.CLASS_NUM, H.THR)
    first.add(head, *batches[0][:2])
    second.add(head, *batches[1][:2]).add(head, *batches[2][:2])
    both = m.DeviceDetMetrics(cases.CLASS_NUM, H.THR).merge(first.state()).merge(second.state())
    assert both.get_stats() == pytest.approx(got, abs=0, nan_ok=True)
    first.merge(second.state())
    assert first.get_stats() == pytest.approx(got, abs=0, nan_ok=True)
    assert first.gather() is first and first.get_stats() == pytest.approx(got, abs=0, nan_ok=True)   # no process group
    names = {c: 'c%02d' % c for c in range(cases.CLASS_NUM)}
    assert 'mAP_0.25' in whole.get_stats(names) and any(k.startswith('c') and '_AP_0.50' in k for k in whole.get_stats(names))
    whole.reset()
    assert whole.state()['scores'].size == 0 and int(whole.npos.sum()) == 0
    # a valid prediction whose label lies outside the classes is an error of the caller, reported when the statistics are formed
    narrow = m.DeviceDetMetrics(5, H.THR)
    narrow.add(head, *batches[0][:2])
    with pytest.raises(ValueError, match='outside'):
        narrow.get_stats()
    with pytest.raises(ValueError, match='thresholds'):
        m.DeviceDetMetrics(17, ())
