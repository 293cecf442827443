"""CPU side of the device Hungarian assignment (ABI 31): the entry point's declaration, export and argument checks, the
assigner's ``solver`` keyword, ``pad_gts``, the padded ``loss`` (scipy in place of the kernel on CPU tensors, the head's
``is_cuda`` convention) against the list form, and the device-form loss normalisers under two gloo ranks."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cases
from util import ROOT, golden, pkg

T = torch.from_numpy
DEVICE_TRAIN_CFG = dict(cases.VOCC_TRAIN_CFG, assigner=dict(cases.VOCC_TRAIN_CFG['assigner'], solver='device'))


def test_entry_point_is_declared_exported_and_versioned():
    text = open(os.path.join(ROOT, 'include', 'ver_ops.h')).read()
    assert re.search(r'int ver_lsa_solve\(const float\* cost, const int32_t\* ncols, int32_t\* match, int32_t\* bad,\s*'
                     r'int P, int R, int Ccap, void\* stream\);', text)
    assert 'hungarian_assigner_3d.py:129' in text and '#define VER_ABI_VERSION 31' in text
    hip = pkg('hipops')
    pkg('csrc.build').build_hip(verbose=False)
    handle = ctypes.CDLL(hip.LIB_PATH)
    assert hasattr(handle, 'ver_lsa_solve')
    assert handle.ver_abi_version() == 31 == hip.ABI_VERSION
    ret, params = hip.PROTOTYPES['ver_lsa_solve']
    assert ret is ctypes.c_int and params == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_void_p]


def test_argument_validation_without_gpu():
    """Null pointers, negative sizes and sizes past the supported range come back as the documented codes before anything
    touches a device."""
    hip = pkg('hipops')
    lib = hip.lib()
    buf = (ctypes.c_float * 16)()
    assert lib.ver_lsa_solve(None, None, None, None, 0, 100, 20, None) == 0            # P == 0: nothing to do
    rc = lib.ver_lsa_solve(None, buf, buf, None, 4, 100, 20, None)
    assert rc == -1 and b'null' in lib.ver_last_error()
    rc = lib.ver_lsa_solve(buf, None, buf, None, 4, 100, 20, None)
    assert rc == -1 and b'null' in lib.ver_last_error()
    rc = lib.ver_lsa_solve(buf, buf, None, None, 4, 100, 20, None)
    assert rc == -1 and b'null' in lib.ver_last_error()
    for p, r, c in ((-1, 100, 20), (4, 0, 20), (4, -3, 20), (4, 100, -1)):
        rc = lib.ver_lsa_solve(buf, buf, buf, None, p, r, c, None)
        assert rc == -1 and b'bad sizes' in lib.ver_last_error(), (p, r, c)
    for r, c in ((1025, 20), (100, 1025), (4096, 4096)):
        rc = lib.ver_lsa_solve(buf, buf, buf, None, 4, r, c, None)
        assert rc == -2 and b'at most 1024' in lib.ver_last_error(), (r, c)
    assert hip.LSA_MAX == 1024
    with pytest.raises(RuntimeError, match='GPU'):                                      # no torch fallback inside hipops
        hip.lsa_solve(torch.zeros(2, 3, 4), torch.zeros(2, dtype=torch.int32))


def _head(train_cfg):
    pkg()
    torch.manual_seed(3)
    return pkg('registry').build_head(dict(cases.vocc_head_cfg(), train_cfg=train_cfg)).eval()


def test_solver_keyword_of_the_assigner():
    reg = pkg('registry')
    asg = pkg('dense_heads.assigner')
    base = cases.VOCC_TRAIN_CFG['assigner']
    assert asg.build_assigner(dict(base)).solver == 'host'
    assert asg.build_assigner(dict(base, solver='device')).solver == 'device'
    with pytest.raises(ValueError, match='solver'):
        asg.build_assigner(dict(base, solver='gpu'))
    assert reg is not None
    # on CPU tensors the device solver's assign is the host's
    gh = golden('head_vocc')
    cls, box = T(gh['c3_b0_cls'][-1])[0], T(gh['c3_b0_bbox'][-1])[0]
    boxes, labels = cases.detection_gt()
    a = asg.build_assigner(dict(base)).assign(box, cls, T(boxes), T(labels))
    b = asg.build_assigner(dict(base, solver='device')).assign(box, cls, T(boxes), T(labels))
    assert torch.equal(a.gt_inds, b.gt_inds) and torch.equal(a.labels, b.labels)


def test_pad_gts_layout_and_capacity():
    h = _head(DEVICE_TRAIN_CFG)
    counts = (3, 0, 5, 1)
    gts = [cases.detection_gt(seed=50 + i, num_gt=max(n, 1)) for i, n in enumerate(counts)]
    gb = [T(b[:n, :7]) for (b, _), n in zip(gts, counts)]
    gl = [T(l[:n]) for (_, l), n in zip(gts, counts)]
    padded = h.pad_gts(gb, gl)
    assert type(padded).__name__ == 'PaddedGts' and padded._fields == ('boxes', 'labels', 'counts')
    assert padded.boxes.shape == (4, 5, 9) and padded.boxes.dtype == torch.float32
    assert padded.labels.shape == (4, 5) and padded.labels.dtype == torch.int64
    assert padded.counts.dtype == torch.int32 and padded.counts.tolist() == list(counts)
    for i, n in enumerate(counts):
        assert torch.equal(padded.boxes[i, :n, :7], gb[i]) and torch.equal(padded.labels[i, :n], gl[i].long())
        assert not padded.boxes[i, n:].any() and not padded.labels[i, n:].any()
    assert not padded.boxes[..., 7:].any()                                     # velocity columns (head:1316-1317)
    roomy = h.pad_gts(gb, gl, capacity=8)
    assert roomy.boxes.shape == (4, 8, 9) and torch.equal(roomy.boxes[:, :5], padded.boxes) and not roomy.boxes[:, 5:].any()
    with pytest.raises(ValueError, match='capacity'):
        h.pad_gts(gb, gl, capacity=4)
    nine = h.pad_gts([torch.cat([g, torch.ones(g.shape[0], 2)], 1) for g in gb], gl)   # boxes that carry a velocity keep it
    assert torch.equal(nine.boxes[..., :7], padded.boxes[..., :7]) and float(nine.boxes[0, 0, 8]) == 1.0
    empty = h.pad_gts([g[:0] for g in gb], [x[:0] for x in gl])
    assert empty.boxes.shape == (4, 0, 9) and empty.counts.tolist() == [0, 0, 0, 0]


def test_padded_loss_equals_the_list_form_on_the_golden_inputs():
    """``head.loss(PaddedGts, ...)`` with ``solver='device'`` (CPU tensors: scipy in place of the kernel, the same padded
    plumbing and tensor-valued ``num_pos``) against ``head.loss(lists, ...)`` with the default solver on the loss_vocc golden
    inputs, and on two samples with 3 and 0 boxes: every entry equal as Python floats."""
    g = golden('loss_vocc')
    gh = golden('head_vocc')
    host, dev = _head(cases.VOCC_TRAIN_CFG), _head(DEVICE_TRAIN_CFG)
    boxes, labels = cases.detection_gt()
    logits, gt_occ = cases.occupancy_loss_inputs()
    preds = dict(all_cls_scores=T(gh['c3_b0_cls']), all_bbox_preds=T(gh['c3_b0_bbox']), occupancy_preds=T(logits)[None])
    gb, gl = [T(boxes)[:, :7]], [T(labels)]
    want = host.loss(gb, gl, T(gt_occ)[None], preds)
    assert float(want['loss_cls']) == pytest.approx(float(g['loss_cls']), rel=1e-5)
    for gts in (dev.pad_gts(gb, gl), dev.pad_gts(gb, gl, capacity=11)):
        got = dev.loss(gts, None, T(gt_occ)[None], preds)
        assert sorted(got) == sorted(want)
        for k in want:
            assert float(got[k]) == float(want[k]), k
    lists = dev.loss(gb, gl, T(gt_occ)[None], preds)                       # the two lists on a device-solver head: padded inside
    assert all(float(lists[k]) == float(want[k]) for k in want)
    targets = dev._targets_device(preds['all_cls_scores'], preds['all_bbox_preds'], dev.pad_gts(gb, gl))
    assert torch.is_tensor(targets[3]) and targets[3].shape == (6,) and targets[3].tolist() == [len(boxes)] * 6
    with pytest.raises(ValueError, match="solver = 'device'"):
        host.loss(dev.pad_gts(gb, gl), None, T(gt_occ)[None], preds)
    cls2 = T(np.concatenate([gh['c3_b0_cls'], gh['c3_b0_cls'][:, :, ::-1].copy()], 1))
    box2 = T(np.concatenate([gh['c3_b0_bbox'], gh['c3_b0_bbox'][:, :, ::-1].copy()], 1))
    gb2, gl2 = [T(boxes)[:, :7], T(boxes)[:0, :7]], [T(labels), T(labels)[:0]]
    preds2 = dict(all_cls_scores=cls2, all_bbox_preds=box2, occupancy_preds=None)
    want2 = host.loss(gb2, gl2, None, preds2)
    got2 = dev.loss(dev.pad_gts(gb2, gl2), None, None, preds2)
    for k in want2:
        assert float(got2[k]) == float(want2[k]), k
    none = dev.loss(dev.pad_gts([b[:0] for b in gb2], [x[:0] for x in gl2]), None, None, preds2)   # no box at all
    assert float(none['loss_bbox']) == 0.0 and float(none['loss_cls']) > 0.0


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _normaliser_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import sys
        for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
            if p not in sys.path:
                sys.path.insert(0, p)
        head_mod = pkg('dense_heads.voxelformer_occupancy_head')
        gh = golden('head_vocc')
        cls = T(np.concatenate([gh['c3_b0_cls'], gh['c3_b1_cls']], 1))
        box = T(np.concatenate([gh['c3_b0_bbox'], gh['c3_b1_bbox']], 1))
        counts = ((3, 0), (7, 4))[rank]                                    # different G per rank (and per sample)
        gts = [cases.detection_gt(seed=70 + 2 * rank + i, num_gt=max(n, 1)) for i, n in enumerate(counts)]
        gb = [T(b[:n, :7]) for (b, _), n in zip(gts, counts)]
        gl = [T(l[:n]) for (_, l), n in zip(gts, counts)]
        preds = dict(all_cls_scores=cls, all_bbox_preds=box, occupancy_preds=None)
        rec = {}
        for sync, bg in ((False, 0), (True, 0), (True, 0.1), (False, 0.3)):
            host, dev = _head(cases.VOCC_TRAIN_CFG), _head(DEVICE_TRAIN_CFG)
            for h in (host, dev):
                h.sync_cls_avg_factor, h.bg_cls_weight = sync, bg
            targets = dev._targets_device(cls, box, dev.pad_gts(gb, gl))
            num_pos, per_layer = targets[3].tolist(), targets[2][0].numel()
            want = []
            for n in num_pos:                                              # the Python path of _losses_from_targets
                f = n * 1.0 + (per_layer - n) * bg
                if sync:
                    f = head_mod._mean_over_ranks(f, cls)
                want.append((max(f, 1), max(head_mod._mean_over_ranks(n, cls), 1.0)))
            want = torch.tensor(want, dtype=torch.float32).t()
            seen, calls = [], []
            real_norm, real_reduce = dev._device_normalisers, dist.all_reduce
            dev._device_normalisers = lambda *a: (seen.append(real_norm(*a)), seen[-1])[1]
            dist.all_reduce = lambda *a, **k: (calls.append(1), real_reduce(*a, **k))[1]
            try:
                dev._losses_from_targets(cls, box, *targets)
            finally:
                dist.all_reduce = real_reduce
                del dev._device_normalisers
            # and the loss dicts of the two solvers under the process group
            lh = host.loss(gb, gl, None, preds)
            ld = dev.loss(dev.pad_gts(gb, gl, capacity=9), None, None, preds)
            rec[(sync, bg)] = dict(got=seen[0], want=want, calls=len(calls), num_pos=num_pos, counts=counts,
                                   host={k: float(v) for k, v in lh.items()}, dev={k: float(v) for k, v in ld.items()})
        torch.save(rec, os.path.join(out, 'r%d.pt' % rank))
    finally:
        dist.destroy_process_group()


def test_device_normalisers_under_two_ranks_equal_mean_over_ranks(tmp_path):
    """Two gloo ranks on the CPU path with different G per rank: ``pad_gts`` -> ``_targets_device`` ->
    ``_losses_from_targets``.  The normalisers it forms from the tensor-valued ``num_pos`` -- one all-reduce for both rows,
    nothing read back -- equal the ``_mean_over_ranks`` values of the Python path entry by entry, with and without
    ``sync_cls_avg_factor`` and with a non-zero ``bg_cls_weight`` (values that are not exact in fp32), and the loss dict of
    ``solver='device'`` equals the host solver's as floats on every rank."""
    mp.spawn(_normaliser_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    recs = [torch.load(str(tmp_path / ('r%d.pt' % rank))) for rank in range(2)]
    for rank, rec in enumerate(recs):
        assert sorted(rec) == sorted([(False, 0), (True, 0), (True, 0.1), (False, 0.3)])
        for key, r in rec.items():
            assert r['num_pos'] == [sum(r['counts'])] * 6
            assert r['calls'] == 1, key
            assert r['got'].dtype == torch.float32 and r['got'].shape == (2, 6)
            assert torch.equal(r['got'], r['want']), (rank, key, r['got'], r['want'])
            assert sorted(r['host']) == sorted(r['dev'])
            for k in r['host']:
                assert r['host'][k] == r['dev'][k], (rank, key, k)
    # the positives differ per rank, their mean is what both ranks divide by
    assert recs[0][(True, 0)]['num_pos'] != recs[1][(True, 0)]['num_pos']
    assert recs[0][(True, 0)]['got'][1].tolist() == recs[1][(True, 0)]['got'][1].tolist() == [7.0] * 6
    # and without a process group the values are the Python path's own
    h = _head(DEVICE_TRAIN_CFG)
    got = h._device_normalisers(torch.tensor([0, 3, 250]), 200)
    assert got.tolist() == [[1.0, 3.0, 250.0], [1.0, 3.0, 250.0]]
    h.bg_cls_weight = 0.1
    want = torch.tensor([max(n + (200 - n) * 0.1, 1) for n in (0, 3, 250)], dtype=torch.float32)
    assert torch.equal(h._device_normalisers(torch.tensor([0, 3, 250]), 200)[0], want)
