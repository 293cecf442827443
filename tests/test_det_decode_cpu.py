"""CPU side of the fused detection decoding (``ver_det_decode``): the float64 host model of its rule against the torch chain
it stands in for, the tie rule on bf16 logits and hand-made cases, the layout form, the entry point's argument checks and
``DeviceDetMetrics.add(fused=True)`` on CPU tensors.  Also the inputs and the bound ``E32`` that test_det_decode_gpu.py shares."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import cases
import det_eval_helper as H
from util import ROOT, golden, pkg

SEEDS = (21, 11, 12, 13, 5)
T = torch.from_numpy


def dm():
    return pkg('detection_metrics')


def second_coder(max_num=70, classes=cases.CLASS_NUM, threshold=0.99):
    """The second coder of test_decode_padded_equals_decode_sample_by_sample: a tight range and a score threshold."""
    return pkg('dense_heads.coders').NMSFreeCoder(cases.PC_RANGE, post_center_range=[-6, -6, -3, 6, 6, 3], max_num=max_num,
                                                  score_threshold=threshold, num_classes=classes)


def random_outputs(seed, bs, nq, nc, width=10):
    """``random_head_outputs`` for any (Nq, C) and row width (>= 10: the columns past the codes are there to be skipped)."""
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(1, bs, nq, nc, generator=g) * 2.0
    box = torch.randn(1, bs, nq, width, generator=g)
    box[..., 0:2] *= 5.5
    box[..., 4] = box[..., 4] * 2.0
    box[..., [2, 3, 5]] = box[..., [2, 3, 5]] * 0.6
    return dict(all_cls_scores=cls, all_bbox_preds=box)


def torch_chain(coder, preds, dtype, bottom):
    """The path the fused decode stands in for, run in ``dtype``: ``decode_padded`` and, with ``bottom``, the bottom-centre
    shift of ``get_bboxes_padded``."""
    boxes, scores, labels, valid = coder.decode_padded({k: v.to(dtype) for k, v in preds.items()})
    if bottom:
        boxes = boxes.clone()
        boxes[..., 2] = boxes[..., 2] - boxes[..., 5] * 0.5
    return boxes, scores, labels, valid


def distinct_top(coder, preds):
    """No sample has two equal logits among its top K + 1: ``topk`` then has no choice and the two orders are one."""
    cls = preds['all_cls_scores'][-1].float()
    flat = cls.reshape(cls.shape[0], -1)
    k = min(coder.max_num, flat.shape[1])
    top = flat.topk(min(k + 1, flat.shape[1]), dim=1).values
    return bool((top[:, :-1] != top[:, 1:]).all()) if top.shape[1] > 1 else True


def e32_of(coder, preds):
    """(box, score) deviation of the float32 CPU run of the torch chain from its float64 run, with and without the shift."""
    box_dev = score_dev = 0.0
    for bottom in (False, True):
        b32, s32, l32, _ = torch_chain(coder, preds, torch.float32, bottom)
        b64, s64, l64, _ = torch_chain(coder, preds, torch.float64, bottom)
        assert torch.equal(l32, l64)
        box_dev = max(box_dev, float((b32.double() - b64).abs().max()))
        score_dev = max(score_dev, float((s32.double() - s64).abs().max()))
    return box_dev, score_dev


def e32_of_selection(coder, preds):
    """The same two deviations from the chain's per-slot arithmetic (float32 ``sigmoid`` and ``denormalize_bbox`` against
    float64) on the slots the stable order selects -- ``e32_of`` wherever ``topk`` has no choice, and defined where distinct
    logits share a float32 score (a thousand slots out of 16 384 logits) and the two runs of ``topk`` may order them apart."""
    coders = pkg('dense_heads.coders')
    cls, box = preds['all_cls_scores'][-1], preds['all_bbox_preds'][-1]
    flat = cls.reshape(cls.shape[0], -1)
    index = T(np.argsort(-flat.numpy(), axis=1, kind='stable')[:, :min(coder.max_num, flat.shape[1])].copy())
    score_dev = float((flat.sigmoid().gather(1, index).double() - flat.double().sigmoid().gather(1, index)).abs().max())
    rows = box.gather(1, (index // cls.shape[2])[..., None].expand(-1, -1, box.shape[-1])).reshape(-1, box.shape[-1])
    b32, b64 = coders.denormalize_bbox(rows), coders.denormalize_bbox(rows.double())
    shift = (b32[:, 2] - b32[:, 5] * 0.5).double() - (b64[:, 2] - b64[:, 5] * 0.5)
    return max(float((b32.double() - b64).abs().max()), float(shift.abs().max())), score_dev


def vocc_inputs(head):
    """[(seed, coder, preds of 3 samples)] for the five named seeds and the two coders."""
    return [(seed, coder, H.random_head_outputs(seed, 3)) for seed in SEEDS for coder in (head.bbox_coder, second_coder())]


def excluded_share(model, coder, margin=1e-5):
    """Share of the slots whose ``valid`` a float32 implementation may decide differently from the float64 model: a score
    within ``margin`` of the threshold or a centre within ``margin`` of a range face -> (share, mask of the slots to check)."""
    boxes, scores = model[0], model[1]
    rng = np.asarray(coder.post_center_range, np.float64)
    near = (np.abs(boxes[..., None, :3] - rng.reshape(2, 3)) < margin).any((-1, -2))
    if coder.score_threshold is not None:
        near |= np.abs(scores - float(np.float32(coder.score_threshold))) < margin
    return float(near.mean()), ~near


@pytest.fixture(scope='module')
def head():
    return H.build_head()


@pytest.fixture(scope='module')
def e32(head):
    """E32: the largest deviation of the float32 CPU run of ``decode_padded`` (and of the bottom-centre shift behind it) from
    its float64 run over the fp32 inputs of this module -- 3.1e-7 for boxes (|box| <= 19; 2.4e-7 is half an ulp of a
    dimension in [4, 8)) and 8.5e-8 for scores here.  Whatever is compared against the float64 model gets 4 x E32."""
    devs = [e32_of(coder, preds) for _, coder, preds in vocc_inputs(head)]
    assert devs == [e32_of_selection(coder, preds) for _, coder, preds in vocc_inputs(head)]
    out = dict(box=max(d[0] for d in devs), score=max(d[1] for d in devs))
    print('E32 box %.3e score %.3e' % (out['box'], out['score']))
    assert 1e-8 < out['box'] < 2e-6 and 1e-9 < out['score'] < 1.2e-7      # an ulp of a value below 16; of a score below 1
    return out


def test_entry_point_is_declared_and_exported_and_the_abi_number_stays():
    text = open(os.path.join(ROOT, 'include', 'ver_ops.h')).read()
    assert re.search(r'int ver_det_decode\(const void\* cls, int cls_dtype, const float\* box, int box_ld, float\* out_boxes, '
                     r'float\* out_scores,\s*int32_t\* out_labels, uint8_t\* out_valid, int32_t\* out_query, '
                     r'const float\* center_range,\s*float score_threshold, int flags, int B, int Q, int C, int K, int codes, '
                     r'void\* stream\);', text)
    for said in ('LOGIT DESCENDING, FLAT INDEX', 'A NaN logit comes after every number', 'about 17', 'non-decreasing',
                 '#define VER_ABI_VERSION 31'):
        assert said in text, said
    hip = pkg('hipops')
    pkg('csrc.build').build_hip(verbose=False)
    handle = ctypes.CDLL(hip.LIB_PATH)
    assert hasattr(handle, 'ver_det_decode') and handle.ver_abi_version() == 31 == hip.ABI_VERSION
    ptr, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert hip.PROTOTYPES['ver_det_decode'] == (i, [ptr, i, ptr, i] + [ptr] * 6 + [f] + [i] * 6 + [ptr])
    assert (hip.DET_DECODE_MAX_SLOTS, hip.DET_DECODE_MAX_KEYS) == (1024, 16384)


def test_argument_validation_without_gpu():
    """Null pointers and sizes outside the supported range come back as the documented codes, each with its message, before
    anything touches a device."""
    hip = pkg('hipops')
    lib = hip.lib()
    buf = (ctypes.c_float * 64)()
    rng = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)

    def decode(ptrs=None, ld=10, b=2, q=100, c=17, k=50, codes=10, dtype=0, flags=3):
        a = [buf] * 7 + [rng] if ptrs is None else ptrs
        return lib.ver_det_decode(a[0], dtype, a[1], ld, a[2], a[3], a[4], a[5], a[6], a[7], 0.5, flags, b, q, c, k, codes, None)

    assert decode([buf] + [None] * 7, b=0) == 0                                            # B == 0: nothing to do
    assert decode([None] * 8, k=0) == 0                                                    # K == 0: nothing to do
    for hole in (1, 2, 3, 4, 5, 7):                                                        # (0: the layout form, 6: out_query may be NULL)
        a = [buf] * 7 + [rng]
        a[hole] = None
        assert decode(a) == -1 and b'null' in lib.ver_last_error(), hole
    assert decode(codes=9) == -1 and b'codes=9' in lib.ver_last_error()
    assert decode(k=1701) == -1 and b'exceeds Q*C' in lib.ver_last_error()
    assert decode(q=10, c=3, k=31) == -1 and b'exceeds Q*C' in lib.ver_last_error()
    assert decode(q=1000, c=16, k=1025) == -2 and b'1024 slots' in lib.ver_last_error()
    assert decode(q=3277, c=5, k=50) == -2 and b'Q*C=16385' in lib.ver_last_error()
    assert decode(q=16385, c=1, k=50) == -2 and b'16384 keys' in lib.ver_last_error()
    assert decode(ld=9) == -1 and b'box_ld=9' in lib.ver_last_error()
    assert decode(ld=7, codes=8) == -1 and b'box_ld=7' in lib.ver_last_error()
    assert decode(dtype=2) == -1 and b'cls_dtype' in lib.ver_last_error()
    assert decode(flags=4) == -1 and b'flags' in lib.ver_last_error()
    for b, q, c, k in ((-1, 100, 17, 50), (2, 0, 17, 50), (2, 100, 0, 50), (2, 100, 17, -1)):
        assert decode(b=b, q=q, c=c, k=k) == -1 and b'bad sizes' in lib.ver_last_error(), (b, q, c, k)
    layout = [None] + [buf] * 6 + [rng]
    assert decode(layout, k=50) == -1 and b'layout form' in lib.ver_last_error()           # K must be Q there
    assert decode(layout, q=1025, k=1025) == -2 and b'1024 slots' in lib.ver_last_error()
    with pytest.raises(RuntimeError, match='GPU'):                                          # no torch fallback inside hipops
        hip.det_decode(torch.zeros(1, 4, 3), torch.zeros(1, 4, 10), [-1, -1, -1, 1, 1, 1])


def test_host_model_equals_the_torch_chain_where_the_scores_are_distinct(head, e32):
    """fp32 logits of the named seeds, both coders: no ties among the top K + 1 (asserted), so the fused decode's slots are
    ``decode_padded``'s -- labels, box rows and valid flags exactly, boxes and scores within 4 x E32 (the fused CPU path is
    the float64 model rounded to float32).  Measured: boxes 2.4e-7, scores 6e-8 at most."""
    worst = [0.0, 0.0]
    for seed, coder, preds in vocc_inputs(head):
        assert distinct_top(coder, preds), seed
        boxes, scores, labels, valid = coder.decode_padded(preds)
        got = coder.decode_padded(preds, fused=True, with_query=True)
        assert got[2].dtype == torch.int32 and got[3].dtype == torch.uint8 and got[4].dtype == torch.int32
        assert got[0].dtype == torch.float32 and got[0].shape == boxes.shape and len(got) == 5
        assert torch.equal(got[2].long(), labels) and torch.equal(got[3], valid), seed
        index = preds['all_cls_scores'][-1].sigmoid().reshape(3, -1).topk(coder.max_num, dim=1).indices
        assert torch.equal(got[4].long(), index // cases.CLASS_NUM), seed                   # the box rows
        worst = [max(worst[0], float((got[0] - boxes).abs().max())), max(worst[1], float((got[1] - scores).abs().max()))]
        bottom = coder.decode_padded(preds, fused=True, bottom_center=True)[0]
        assert float((bottom - torch_chain(coder, preds, torch.float32, True)[0]).abs().max()) <= 4 * e32['box']
        assert len(coder.decode_padded(preds, fused=True)) == 4
    print('fused CPU path against decode_padded: boxes %.3e scores %.3e' % tuple(worst))
    assert worst[0] <= 4 * e32['box'] and worst[1] <= 4 * e32['score']
    got, want = head.get_bboxes_padded(preds, fused=True), head.get_bboxes_padded(preds)
    assert torch.equal(got[2].long(), want[2]) and torch.equal(got[3], want[3])
    assert float((got[0] - want[0]).abs().max()) <= 4 * e32['box']


def test_the_tie_rule_on_bf16_logits(head):
    """The same logits as bf16: every sample has ties among its top K + 1, ``topk`` orders them as it likes (and not in the
    stable order), the fused selection is the stable argsort, reproducibly, and is one of the sets ``topk`` may return."""
    m = dm()
    agree, slots = 0, 0
    for seed, coder, preds in vocc_inputs(head):
        lowp = dict(preds, all_cls_scores=preds['all_cls_scores'].bfloat16())
        cls = lowp['all_cls_scores'][-1]
        flat = cls.float().reshape(3, -1)
        k = coder.max_num
        top = flat.topk(k + 1, dim=1).values
        assert bool((top[:, :-1] == top[:, 1:]).any(1).all()), seed                      # the case is real
        stable = np.argsort(-flat.numpy(), axis=1, kind='stable')[:, :k]
        got = coder.decode_padded(lowp, fused=True, with_query=True)
        index = got[4].long() * cases.CLASS_NUM + got[2].long()
        assert np.array_equal(index.numpy(), stable), seed
        again = coder.decode_padded(lowp, fused=True, with_query=True)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
        sig = flat.sigmoid()                                                               # fp32, as the torch chain forms it
        theirs = sig.topk(k, dim=1)
        mine = sig.gather(1, index)
        assert torch.equal(mine.sort(1, descending=True).values, theirs.values), seed    # the same multiset of scores
        assert bool((mine[:, :-1] >= mine[:, 1:]).all())                                  # ... already in score order
        assert float((got[1] - mine).abs().max()) <= 1.2e-7                                # the model's scores are those
        agree += int((theirs.indices.numpy() == stable).sum())
        slots += stable.size
        model = m.det_decode_host(cls, lowp['all_bbox_preds'][-1], coder.post_center_range, coder.score_threshold, False, k)
        assert np.array_equal(model[4], got[4].numpy()) and model[0].dtype == np.float64
    print('torch.topk agrees with the stable order in %.1f %% of the bf16 slots' % (100.0 * agree / slots))
    assert agree < slots                   # the old path does not satisfy the new contract: its order on ties is topk's own


def hand_cases():
    """[(name, logits [1, Q, C] float32, K, expected flat indices [K])]: the hand-made tie / NaN / zero / saturation cases."""
    nan = float('nan')
    out = [('all equal', np.full((1, 6, 4), 0.25, np.float32), 9, list(range(9)))]
    one_nan = np.array([[[0.5, nan, -1.0], [2.0, 0.5, -3.0]]], np.float32)
    out.append(('one NaN, K numbers exist', one_nan, 5, [3, 0, 4, 2, 5]))
    out.append(('one NaN, K = Q*C', one_nan, 6, [3, 0, 4, 2, 5, 1]))
    out.append(('signed zeros', np.array([[[-0.0, 0.0, -1e-30], [0.0, 1e-30, -0.0]]], np.float32), 6, [4, 0, 1, 3, 5, 2]))
    out.append(('saturated', np.array([[[20.0, 25.0], [30.0, 20.0], [25.0, 90.0]]], np.float32), 6, [5, 2, 1, 4, 0, 3]))
    out.append(('infinities', np.array([[[-np.inf, np.inf, nan, 0.0, np.inf, -np.inf]]], np.float32), 6, [1, 4, 3, 0, 5, 2]))
    return out


def hand_boxes(nq):
    box = np.zeros((1, nq, 10), np.float32)
    box[..., 0] = np.arange(nq)                                                            # cx names the query
    box[..., 7] = 1.0
    return box


@pytest.mark.parametrize('name,logits,k,want', hand_cases(), ids=[c[0] for c in hand_cases()])
def test_hand_made_ties_nan_zero_and_saturation(name, logits, k, want):
    m = dm()
    nq, nc = logits.shape[1:]
    for cls in (T(logits), T(logits).bfloat16()):                                          # (bf16 keeps every order and tie here)
        boxes, scores, labels, valid, query = m.det_decode_host(cls, hand_boxes(nq), [-100] * 3 + [100] * 3, None, False, k)
        assert (query[0] * nc + labels[0]).tolist() == want, name
        assert boxes[0, :, 0].tolist() == [float(i // nc) for i in want]
        picked = logits.reshape(-1)[want]
        assert valid[0].tolist() == [0 if math.isnan(v) else 1 for v in picked]            # a NaN is selected last, never valid
        if name == 'saturated':
            assert scores[0].astype(np.float32).tolist() == [1.0] * 6 and bool((np.diff(scores[0]) <= 0).all())
            assert np.all(1.0 / (1.0 + np.exp(-picked.astype(np.float32))) == np.float32(1.0))   # fp32: exactly 1 from 17 on
        if name == 'signed zeros':
            assert scores[0, 1:5].tolist() == [0.5] * 4


def test_layout_form_against_the_layout_coder(head):
    g = golden('layout_vocc')
    preds = dict(all_layout_preds=torch.cat([T(g['layout_preds']), T(g['layout_preds']).flip(2) * 1.6], 1))   # 2 samples
    coder = head.layout_coder
    want = coder.decode(preds)
    boxes, valid = coder.decode_padded(preds)
    fused, fvalid = coder.decode_padded(preds, fused=True)
    assert boxes.shape == fused.shape == (2, 100, 9) and valid.dtype == fvalid.dtype == torch.uint8
    kept = [int(v.sum()) for v in valid]
    assert kept[0] == len(want[0]['layouts']) and 0 < kept[1] < 100                       # both kinds of row occur
    assert torch.equal(valid, fvalid)
    for b in range(2):
        assert torch.equal(boxes[b][valid[b].bool()], want[b]['layouts'])
        assert torch.allclose(fused[b][valid[b].bool()], want[b]['layouts'], rtol=3e-7, atol=0)       # the model rounded to fp32
    assert torch.allclose(fused[0], T(g['decoded']), rtol=1e-5, atol=1e-6)                 # the reference's own decoding
    lists = head.get_layouts(preds)
    for use in (False, True):
        padded, ok = head.get_layouts_padded(preds, fused=use)
        for b in range(2):
            rows = padded[b][ok[b].bool()]
            assert rows.shape == lists[b][0].shape
            assert torch.allclose(rows, lists[b][0], rtol=3e-7, atol=1e-7) and (use or torch.equal(rows, lists[b][0]))
    model = dm().det_decode_host(None, preds['all_layout_preds'][-1], coder.post_center_range)
    assert not model[1].any() and not model[2].any() and np.array_equal(model[4], np.tile(np.arange(100), (2, 1)))
    with pytest.raises(ValueError, match='every query'):
        dm().det_decode_host(None, preds['all_layout_preds'][-1], coder.post_center_range, k=50)


def test_device_metrics_fused_on_cpu_tensors_equal_indoor_eval(head):
    m = dm()
    batches = H.head_batches(head)
    for preds, *_ in batches:
        assert distinct_top(head.bbox_coder, preds)
    want = m.indoor_eval(*H.lists_to_annos(batches), H.THR)
    whole = m.DeviceDetMetrics(cases.CLASS_NUM, H.THR)
    for preds, gts, *_ in batches:
        assert whole.add(head, preds, gts, fused=True) is whole
    got = whole.get_stats()
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == pytest.approx(want[k], abs=1e-12, nan_ok=True), k
    assert int(whole.npos.sum()) == sum(len(b[3][i]) for b in batches for i in range(len(b[3])))
