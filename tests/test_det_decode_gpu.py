"""Device side of the fused detection decoding: ``ver_det_decode`` against its float64 host model (selection, labels and
queries exactly; boxes and scores within 4 x E32, the float32 rounding of the torch chain it stands in for), the hand-made tie
/ NaN / saturation cases, the layout form, the wiring into the head, ``DeviceDetMetrics`` and the detector, and graph capture."""
import math

import numpy as np
import pytest
import torch

import cases
import det_eval_helper as H
from test_det_decode_cpu import (SEEDS, distinct_top, e32_of, e32_of_selection, excluded_share, hand_boxes, hand_cases, random_outputs,
                                 second_coder)
from test_detector_cpu import _metas, _sparse, _store
from util import golden, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = torch.from_numpy
SHAPES = ((100, 17, 50), (100, 17, 70), (7, 3, 21), (1, 1, 1), (900, 10, 300), (1024, 16, 1024))


def dm():
    return pkg('detection_metrics')


def coder_for(nq, nc, k):
    coders = pkg('dense_heads.coders')
    if (nq, nc, k) == (100, 17, 50):                                                       # vocc.py's bbox_coder
        return coders.NMSFreeCoder(cases.PC_RANGE, post_center_range=[-10, -10, -5.0, 10, 10, 5.0], max_num=50,
                                   num_classes=cases.CLASS_NUM)
    if (nq, nc, k) == (100, 17, 70):
        return second_coder()
    return second_coder(k, nc, 0.9)


def layout_preds():
    g = golden('layout_vocc')
    return dict(all_layout_preds=torch.cat([T(g['layout_preds']), T(g['layout_preds']).flip(2) * 1.6], 1))


def wide(preds, width=12):
    """The same predictions with box rows of ``width`` columns (the extra ones hold values that must not be read)."""
    box = preds['all_bbox_preds']
    pad = torch.full(box.shape[:-1] + (width - box.shape[-1],), 77.0)
    return dict(preds, all_bbox_preds=torch.cat([box, pad], -1))


def screened(coder, preds):
    """fp32 logits without ties among the top K + 1, and no slot of either dtype that the 1e-5 margins exclude."""
    if not distinct_top(coder, preds):
        return False
    for cls in (preds['all_cls_scores'][-1], preds['all_cls_scores'][-1].bfloat16()):
        model = dm().det_decode_host(cls, preds['all_bbox_preds'][-1][..., :10], coder.post_center_range, coder.score_threshold,
                                     False, min(coder.max_num, cls[0].numel()))
        if excluded_share(model, coder)[0] != 0.0:
            return False
    return True


@pytest.fixture(scope='module')
def gpu_head():
    return H.build_head(DEV)


@pytest.fixture(scope='module')
def shared():
    """Per shape: (coder, [preds of 3 samples, box rows 12 wide]) -- the five named seeds for vocc's own shapes (taken as
    drawn: ``valid`` is checked on EVERY slot there), for the others the first of at most 20 draws that ``screened`` takes -- and E32
    over all of them and the layout inputs: the largest deviation of the float32 CPU run of the torch chain
    (``decode_padded`` and the bottom-centre shift) from its float64 run.  Here: boxes 3.1e-7, scores 8.7e-8."""
    inputs, box_dev, score_dev = {}, 0.0, 0.0
    for nq, nc, k in SHAPES:
        coder = coder_for(nq, nc, k)
        if (nq, nc) == (cases.QUERY_NUM, cases.CLASS_NUM):
            draws = [wide(H.random_head_outputs(seed, 3)) for seed in SEEDS]
            assert all(distinct_top(coder, p) for p in draws)
        else:
            for draw in range(20):
                preds = random_outputs(1000 * nq + draw, 3, nq, nc, 12)
                if screened(coder, preds):
                    break
            else:
                raise AssertionError('no screened draw in 20 for %s' % ((nq, nc, k),))
            draws = [preds]
        inputs[(nq, nc, k)] = (coder, draws)
        for preds in draws:
            dev = e32_of_selection(coder, preds)
            assert (nq, nc) != (cases.QUERY_NUM, cases.CLASS_NUM) or dev == e32_of(coder, preds)
            box_dev, score_dev = max(box_dev, dev[0]), max(score_dev, dev[1])
    lay = layout_preds()['all_layout_preds'][-1]
    lc = pkg('dense_heads.coders').LayoutCoder(cases.PC_RANGE, post_center_range=[-50, -50, -5.0, 50, 50, 5.0], max_num=10,
                                               num_classes=1)
    l32, l64 = (lc.decode_padded(dict(all_layout_preds=lay[None].to(dt)))[0] for dt in (torch.float32, torch.float64))
    for a, b in ((l32.double(), l64), (l32[..., 2].double() - l32[..., 5].double() * 0.5, l64[..., 2] - l64[..., 5] * 0.5)):
        box_dev = max(box_dev, float((a - b).abs().max()))
    print('E32 box %.3e score %.3e' % (box_dev, score_dev))
    assert 1e-8 < box_dev < 2e-6 and 1e-9 < score_dev < 1.2e-7                            # an ulp of a value below 16 / of a score
    return dict(inputs=inputs, box=box_dev, score=score_dev, layout=(lc, lay))


def run_kernel(cls, box, coder, threshold, bottom, k, codes=None):
    """``codes``: decode the first ``codes`` columns of the rows IN PLACE (a view of the device tensor: row pitch != codes)."""
    box = box.to(DEV)
    if codes is not None:
        box = box[..., :codes]
        assert box.stride(1) > codes
    out = pkg('hipops').det_decode(None if cls is None else cls.to(DEV), box, coder.post_center_range,
                                   coder.score_threshold if threshold else None, bottom, k)
    torch.cuda.synchronize()
    assert [t.dtype for t in out] == [torch.float32, torch.float32, torch.int32, torch.uint8, torch.int32]
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize('nq,nc,k', SHAPES, ids=['%dx%d_k%d' % s for s in SHAPES])
def test_kernel_against_the_float64_model(shared, nq, nc, k):
    """Every draw of the shape x B in {1, 3} x fp32 / bf16 logits x both flag bits x (codes, row pitch) in {(10, 12), (8, 12),
    (10, 10), (8, 10)}: slot order, labels and queries exact; boxes and scores within 4 x E32; ``valid`` exact on EVERY slot.
    For the drawn shapes that is the rule "exact outside 1e-5 of the threshold and of the range faces, with nothing excluded"
    (asserted).  For the five named seeds no slot is excluded either, whatever its margin: seed 5 at B = 3 with the second
    coder has one score 1.98e-6 from 0.99 (float64 model), inside the 1e-5 margin but 20 times the kernel's deviation, and it
    is checked like every other slot.  The nearest centre is 1.9e-4 from a face.
    Measured on an MI355X over all six shapes: boxes 3.3e-7 (bound 1.24e-6), scores 8.7e-8 (bound 3.5e-7)."""
    m = dm()
    coder, draws = shared['inputs'][(nq, nc, k)]
    named = (nq, nc) == (cases.QUERY_NUM, cases.CLASS_NUM)
    worst = [0.0, 0.0]
    for preds in draws:
        for bs in (1, 3):
            logits, rows = preds['all_cls_scores'][-1][:bs], preds['all_bbox_preds'][-1][:bs]
            for cls in (logits, logits.bfloat16()):
                for codes, packed in ((10, False), (8, False), (10, True), (8, True)):
                    box = rows[..., :codes].contiguous() if packed else rows[..., :codes]
                    for threshold in (False, True):
                        for bottom in (False, True):
                            want = m.det_decode_host(cls, box, coder.post_center_range,
                                                     coder.score_threshold if threshold else None, bottom, k)
                            assert named or excluded_share(want, coder)[0] == 0.0
                            got = run_kernel(cls, box, coder, threshold, bottom, k) if packed else run_kernel(
                                cls, rows, coder, threshold, bottom, k, codes)
                            assert got[0].shape == (bs, k, codes - 1)
                            assert np.array_equal(got[2], want[2]) and np.array_equal(got[4], want[4])
                            assert np.array_equal(got[3], want[3])
                            assert 0 < want[3].sum() or nq < 100
                            worst = [max(worst[0], float(np.abs(got[0] - want[0]).max())),
                                     max(worst[1], float(np.abs(got[1] - want[1]).max()))]
    print('kernel against the float64 model: boxes %.3e (4 x E32 = %.3e) scores %.3e (%.3e)'
          % (worst[0], 4 * shared['box'], worst[1], 4 * shared['score']))
    assert worst[0] <= 4 * shared['box'] and worst[1] <= 4 * shared['score']


@pytest.mark.parametrize('name,logits,k,want', hand_cases(), ids=[c[0] for c in hand_cases()])
def test_hand_made_cases_on_the_device(name, logits, k, want):
    nq, nc = logits.shape[1:]
    coder = second_coder(k, nc, None)
    coder.post_center_range = [-100] * 3 + [100] * 3
    for cls in (T(logits), T(logits).bfloat16()):
        boxes, scores, labels, valid, query = run_kernel(cls, T(hand_boxes(nq)), coder, False, False, k)
        assert (query[0] * nc + labels[0]).tolist() == want, name
        assert boxes[0, :, 0].tolist() == [float(i // nc) for i in want]
        picked = logits.reshape(-1)[want]
        assert valid[0].tolist() == [0 if math.isnan(v) else 1 for v in picked]
        if name == 'saturated':
            assert scores[0].tolist() == [1.0] * 6
        if name == 'signed zeros':
            assert scores[0, 1:5].tolist() == [0.5] * 4
        model = dm().det_decode_host(cls, hand_boxes(nq), coder.post_center_range, None, False, k)
        assert np.array_equal(model[4], query) and np.array_equal(model[3], valid)


def test_layout_form_on_the_device(shared, gpu_head):
    coder, lay = shared['layout']
    for bottom in (False, True):
        for box, codes in ((lay, None), (lay[..., :8], 8)):
            want = dm().det_decode_host(None, box, coder.post_center_range, None, bottom)
            got = run_kernel(None, lay, coder, False, bottom, None, codes)
            assert got[0].shape == (2, 100, box.shape[-1] - 1) and 0 < want[3][1].sum() < 100 == want[3][0].sum()
            assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
            assert not got[1].any() and not got[2].any()
            assert float(np.abs(got[0] - want[0]).max()) <= 4 * shared['box']
    head = gpu_head
    preds = {k: v.to(DEV) for k, v in layout_preds().items()}
    lists = head.get_layouts(preds)
    padded, ok = head.get_layouts_padded(preds, fused=True)
    for b in range(2):
        rows = padded[b][ok[b].bool()]
        assert rows.shape == lists[b][0].shape and float((rows - lists[b][0]).abs().max()) <= 4 * shared['box']


def test_wiring_into_the_head_and_the_metrics(shared, gpu_head):
    """``get_bboxes_padded(fused=True)`` against the torch chain on fp32 logits (the same slots; both sides are float32, each
    within E32 of the truth), and ``DeviceDetMetrics.add(fused=True)`` end to end against ``indoor_eval``."""
    m = dm()
    head = gpu_head
    preds = {k: v.to(DEV) for k, v in H.random_head_outputs(21, 3).items()}
    want, got = head.get_bboxes_padded(preds), head.get_bboxes_padded(preds, fused=True)
    assert got[2].dtype == torch.int32 and torch.equal(got[2].long(), want[2]) and torch.equal(got[3], want[3])
    assert float((got[0] - want[0]).abs().max()) <= 4 * shared['box']
    assert float((got[1] - want[1]).abs().max()) <= 4 * shared['score']
    batches = H.head_batches(head)
    ref = m.indoor_eval(*H.lists_to_annos(batches), H.THR)
    metrics = m.DeviceDetMetrics(cases.CLASS_NUM, H.THR, device=DEV)
    for p, gts, *_ in batches:
        metrics.add(head, p, gts, fused=True)
    assert metrics.npos.is_cuda and all(t.is_cuda for part in metrics._parts for t in part)
    stats = metrics.get_stats()
    assert sorted(stats) == sorted(ref) and len(ref) >= 2 * len(H.THR) * 6
    for key in ref:
        assert stats[key] == pytest.approx(ref[key], abs=1e-12, nan_ok=True), key


def test_decode_and_match_are_capturable(gpu_head):
    """``det_decode`` + ``det_match`` captured in one ``torch.cuda.graph`` from static inputs: the capture succeeding is the
    proof that nothing in the region synchronises, allocates behind a synchronisation or reads on the host.  New logits and
    boxes are copied into the static buffers; two replays each equal the eager result bit for bit."""
    hip = pkg('hipops')
    head = gpu_head
    coder = head.bbox_coder
    batches = H.head_batches(head, ((11, 3), (12, 3)))
    gts = batches[0][1]
    gb, gl = gts.boxes[..., :7].float().contiguous(), gts.labels.to(torch.int32)

    def step(cls, box, npos):
        boxes, scores, labels, valid, query = hip.det_decode(cls, box, coder.post_center_range, coder.score_threshold, True, coder.max_num)
        return (boxes, scores, labels, valid, query) + hip.det_match(boxes[..., :7].contiguous(), labels, scores, valid, gb, gl,
                                                                     gts.counts, H.THR, npos)

    first = batches[0][0]
    static_cls, static_box = first['all_cls_scores'][-1].clone(), first['all_bbox_preds'][-1].clone()
    static_npos = torch.zeros(cases.CLASS_NUM, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        step(static_cls, static_box, static_npos)                                          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        static_out = step(static_cls, static_box, static_npos)
    for preds in (first, batches[1][0], dict(first, all_cls_scores=first['all_cls_scores'].bfloat16().float())):
        cls, box = preds['all_cls_scores'][-1].contiguous(), preds['all_bbox_preds'][-1].contiguous()
        static_cls.copy_(cls)
        static_box.copy_(box)
        want = step(cls, box, torch.zeros_like(static_npos))
        for replay in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for got, ref in zip(static_out, want):
                assert torch.equal(got, ref), replay


def test_detector_with_the_fused_decode(tmp_path, shared):
    """``evaluate_detection`` and ``simple_test`` with ``fused_detection_decode`` on the vocc detector of
    test_detector_gpu.py: the records equal those of the torch chain, and ``simple_test``'s lists hold the same boxes in the
    same order (fp32: no ties).  The head runs once; its outputs are reused for the calls that follow."""
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    pkg()
    syn, reg = pkg('synthetic'), pkg('registry')
    det = reg.build_detector(dict(type='VoxelFormer', pts_bbox_head=cases.vocc_head_cfg(),
                                  train_cfg=dict(pts=cases.VOCC_TRAIN_CFG))).eval()
    assert det.fused_detection_decode is False
    head = det.pts_bbox_head
    syn.load_seeded(head, 7)
    det.to(DEV)
    names = ['scanA_vp0']
    store = _store(tmp_path, syn.vit_features(1, seed=0), names)
    gts = [cases.detection_gt(seed=40, num_gt=3)]
    dense = np.random.default_rng(9).integers(0, 17, size=(1, 504000))
    metas = _metas(tmp_path, store, names, gts, [_sparse(d) for d in dense])
    padded = head.pad_gts([T(b[:, :7]).to(DEV) for b, _ in gts], [T(l).to(DEV) for _, l in gts], capacity=8)
    calls, forward = [], head.forward

    def once(*args, **kwargs):
        if not calls:
            calls.append(forward(*args, **kwargs))
        return calls[0]
    head.forward = once
    fused = det.evaluate_detection(metas, padded, fused=True)
    plain = det.evaluate_detection(metas, padded)
    assert type(fused).__name__ == 'DeviceDetMetrics' and fused is not plain
    a, b = fused.state(), plain.state()
    assert len(a['scores']) > 0 and np.array_equal(a['labels'], b['labels']) and np.array_equal(a['tp_bits'], b['tp_bits'])
    assert np.array_equal(a['npos'], b['npos']) and int(a['npos'].sum()) == 3
    assert float(np.abs(a['scores'] - b['scores']).max()) <= 4 * shared['score']
    with torch.no_grad():
        want = det.simple_test(metas)[1]
        det.fused_detection_decode = True
        got = det.simple_test(metas)[1]
        assert det.evaluate_detection(metas, padded).state()['tp_bits'].tolist() == a['tp_bits'].tolist()   # fused=None: the attribute
    assert distinct_top(head.bbox_coder, calls[0])
    for g, w in zip(got, want):
        g, w = g['pts_bbox'], w['pts_bbox']
        assert g['boxes_3d'].device.type == 'cpu' and g['boxes_3d'].shape == w['boxes_3d'].shape and len(w['boxes_3d']) > 0
        assert g['labels_3d'].dtype == w['labels_3d'].dtype and torch.equal(g['labels_3d'], w['labels_3d'])
        assert float((g['boxes_3d'] - w['boxes_3d']).abs().max()) <= 4 * shared['box']
        assert float((g['scores_3d'] - w['scores_3d']).abs().max()) <= 4 * shared['score']
