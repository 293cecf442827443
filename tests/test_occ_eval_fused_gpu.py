"""Occupancy evaluation and class maps without logits (``ver_occ_mlp_confusion`` / ``ver_occ_mlp_classes``): every result
is held to exact integer / byte equality with the unfused pair run in the same process on the same x --
``occ_mlp_forward`` -> ``occ_confusion`` / ``occ_predict`` on its bf16 logits.  Nothing here has a tolerance.  ``-m gpu``."""
import ctypes

import numpy as np
import pytest
import torch

import cases
from test_detector_cpu import _metas, _sparse, _store
from test_occ_eval_gpu import THRESHOLDS, _labels
from util import pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = torch.from_numpy
MODES = [dict(first_linear=False, centered=True), dict(first_linear=True, centered=False)]


def _params(seed, mode, w3=None, b3=None):
    """(image, vectors) of a seeded MLP.  Folded + centred: what the head packs (W2 centred over its outputs in W1's
    image section, b1 = 0); otherwise the plain three Linears."""
    hip = pkg('hipops')
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    w1, w2 = r(128, 128) / 128 ** 0.5, r(128, 128) / 128 ** 0.5
    w3 = r(16, 128) * 0.3 if w3 is None else w3
    b1, b2 = r(128) * 0.1, r(128) * 0.1
    b3 = r(16) - 1.5 if b3 is None else b3
    g1, g2, be1, be2 = 1 + 0.1 * r(128), 1 + 0.1 * r(128), 0.1 * r(128), 0.1 * r(128)
    if mode['centered']:
        w2, b2 = w2 - w2.mean(0, keepdim=True), b2 - b2.mean()
    if not mode['first_linear']:
        w1, b1 = w2, torch.zeros(128)
    d = lambda t: t.to(DEV)
    return hip.occ_mlp_pack(d(w1), d(w2), d(w3)), hip.occ_mlp_vectors(*(d(v) for v in (b1, g1, be1, b2, g2, be2, b3)))


def _x(n, seed, mode):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 128, generator=gen) * 1.5
    if mode['centered'] and not mode['first_linear']:
        x = x - x.mean(-1, keepdim=True)                 # the folded, centred producer writes zero-mean rows
    return x.bfloat16().to(DEV)


def _unfused_classes(logits, thr):
    hip = pkg('hipops')
    pairs = hip.occ_predict(logits, thr)
    cls = torch.full((logits.shape[0],), 16, dtype=torch.uint8, device=logits.device)
    cls[pairs[:, 0]] = pairs[:, 1].to(torch.uint8)
    return cls


def _prob_is_row_argmax_pb(logits, prob, rows):
    """prob[r] is row_argmax's pb bit for bit: as the threshold it leaves the row occupied (thr > pb fails), the next
    float above it empties the row."""
    hip = pkg('hipops')
    p = prob.cpu().numpy()
    for r in rows:
        if np.isnan(p[r]):
            continue
        assert hip.occ_predict(logits[r:r + 1], float(p[r])).shape[0] == 1, r
        assert hip.occ_predict(logits[r:r + 1], float(np.nextafter(p[r], np.float32(2)))).shape[0] == 0, r


@pytest.mark.parametrize('mode', MODES, ids=['folded_centred', 'first_linear'])
def test_ragged_row_counts_in_classes_mode(mode):
    hip = pkg('hipops')
    image, vec = _params(1, mode)
    for n in (1, 15, 64, 65, 257, 6001):
        x = _x(n, n, mode)
        logits = hip.occ_mlp_forward(x, image, vec, **mode)
        guard = torch.full((n + 64,), 77, dtype=torch.uint8, device=DEV)
        with torch.no_grad():
            cls, prob = hip.occ_mlp_classes(x, image, vec, 0.25, want_prob=True, **mode)
            only = hip.occ_mlp_classes(x, image, vec, 0.25, **mode)
        assert cls.shape == (n,) and cls.dtype == torch.uint8 and prob.shape == (n,) and prob.dtype == torch.float32
        assert torch.equal(cls, _unfused_classes(logits, 0.25)), n
        assert torch.equal(only, cls)
        assert int((cls < 16).sum()) > 0 or n < 64
        for thr in (0.05, 0.6):
            with torch.no_grad():
                assert torch.equal(hip.occ_mlp_classes(x, image, vec, thr, **mode), _unfused_classes(logits, thr)), (n, thr)
        rows = sorted(set(np.linspace(0, n - 1, 12).astype(int).tolist()))
        _prob_is_row_argmax_pb(logits, prob, rows)
        # rows at or beyond N are not stored: a view into a larger buffer keeps its guard bytes
        lib = hip.lib()
        rc = lib.ver_occ_mlp_classes(x.data_ptr(), image.data_ptr(), vec.data_ptr(), guard.data_ptr(), None, n, 0.25, 128,
                                     16, 1e-5, (1 if mode['first_linear'] else 0) | (2 if mode['centered'] else 0),
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        assert torch.equal(guard[:n], cls) and bool((guard[n:] == 77).all())


def test_grid_stride_loop_in_both_modes():
    """140 003 rows: more than 512 workgroups x 256 rows, every workgroup of the classes launch loops; 18 chunks of the
    confusion launch, the last one ragged."""
    hip = pkg('hipops')
    mode = MODES[0]
    n = 140003
    image, vec = _params(2, mode)
    x = _x(n, 3, mode)
    lab = _labels(n, 16, torch.Generator().manual_seed(4)).to(DEV)
    logits = hip.occ_mlp_forward(x, image, vec, **mode)
    thr = THRESHOLDS[3]
    with torch.no_grad():
        cls = hip.occ_mlp_classes(x, image, vec, 0.25, **mode)
        hist = hip.occ_mlp_confusion(x, image, vec, lab, thr, 1, **mode)
    assert torch.equal(cls, _unfused_classes(logits, 0.25))
    assert torch.equal(hist, hip.occ_confusion(logits, lab, thr, 1))
    assert int(hist.sum()) == 3 * int((lab <= 16).sum())


@pytest.mark.parametrize('nt', [1, 3, 8])
@pytest.mark.parametrize('samples,rows', [(3, 1000), (5, 37), (2, 70001)])
def test_sample_boundaries_inside_blocks(samples, rows, nt):
    hip = pkg('hipops')
    thr = THRESHOLDS[nt]
    for k, mode in enumerate(MODES):
        image, vec = _params(5 + k, mode)
        x = _x(samples * rows, rows + nt, mode)
        lab = _labels(samples * rows, 16, torch.Generator().manual_seed(rows)).to(DEV)
        logits = hip.occ_mlp_forward(x, image, vec, **mode)
        with torch.no_grad():
            got = hip.occ_mlp_confusion(x, image, vec, lab, thr, samples, **mode)
        want = hip.occ_confusion(logits, lab, thr, samples)
        assert got.shape == (samples, nt, 17, 17) and torch.equal(got, want), (samples, rows, nt, mode)
        assert int(got.sum()) == nt * int((lab <= 16).sum())
        assert int(got[:, :, :, :16].sum()) > 0                       # not everything predicted empty


def test_accumulation_and_empty_batch():
    hip = pkg('hipops')
    mode = MODES[0]
    image, vec = _params(7, mode)
    x = _x(3 * 5000, 8, mode)
    lab = _labels(3 * 5000, 16, torch.Generator().manual_seed(9)).to(DEV)
    thr = THRESHOLDS[3]
    with torch.no_grad():
        once = hip.occ_mlp_confusion(x, image, vec, lab, thr, 3, **mode)
        twice = hip.occ_mlp_confusion(x, image, vec, lab, thr, 3, hist=once.clone(), **mode)
        assert torch.equal(twice, 2 * once) and int(once.sum()) > 0
        keep = twice.clone()
        out = hip.occ_mlp_confusion(x[:0], image, vec, lab[:0], thr, 3, hist=twice, **mode)
    assert out is twice and torch.equal(twice, keep)
    lib = hip.lib()
    host_thr = (ctypes.c_float * 3)(*thr)
    rc = lib.ver_occ_mlp_confusion(x.data_ptr(), image.data_ptr(), vec.data_ptr(), lab.data_ptr(), 5000, 0, host_thr, 3,
                                   twice.data_ptr(), 128, 16, 1e-5, 2, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(twice, keep)
    with pytest.raises(RuntimeError, match='no_grad'):
        hip.occ_mlp_confusion(x.clone().requires_grad_(True), image, vec, lab, thr, 3, **mode)
    with pytest.raises(RuntimeError, match='no_grad'):
        hip.occ_mlp_classes(x.clone().requires_grad_(True), image, vec, **mode)


def _both(x, image, vec, lab, thr, mode):
    """(classes per threshold, histogram) of the fused launches after checking them against the unfused pair."""
    hip = pkg('hipops')
    logits = hip.occ_mlp_forward(x, image, vec, **mode)
    with torch.no_grad():
        hist = hip.occ_mlp_confusion(x, image, vec, lab, thr, 1, **mode)
        cls = [hip.occ_mlp_classes(x, image, vec, t, **mode) for t in thr]
        prob = hip.occ_mlp_classes(x, image, vec, thr[0], want_prob=True, **mode)[1]
    assert torch.equal(hist, hip.occ_confusion(logits, lab, thr, 1))
    for t, c in zip(thr, cls):
        assert torch.equal(c, _unfused_classes(logits, t)), t
    return cls, hist, prob, logits


@pytest.mark.parametrize('mode', MODES, ids=['folded_centred', 'first_linear'])
def test_edges_of_the_classification_rule(mode):
    n = 333
    lab = _labels(n, 16, torch.Generator().manual_seed(11)).to(DEV)
    x = _x(n, 12, mode)
    zero = torch.zeros(16, 128)
    # every class equal: class 0 wins, through the cross-lane merge (ties go to the lower lane group)
    image, vec = _params(13, mode, w3=zero, b3=torch.full((16,), 0.75))
    cls, _, prob, logits = _both(x, image, vec, lab, (0.5, 0.9), mode)
    assert bool((cls[0] == 0).all()) and bool((cls[1] == 16).all())
    assert prob.unique().numel() == 1 and abs(float(prob[0]) - 0.6791787) < 1e-6
    _prob_is_row_argmax_pb(logits, prob, [0, 100, 332])
    # the maximum duplicated in classes 3 and 12 (different lanes): the first one
    b3 = torch.linspace(-3, -1, 16)
    b3[3] = b3[12] = 1.0
    image, vec = _params(13, mode, w3=zero, b3=b3)
    cls, _, _, _ = _both(x, image, vec, lab, (0.5,), mode)
    assert bool((cls[0] == 3).all())
    # probability exactly 0.5 against threshold 0.5 (occupied) and the next float above (empty)
    b3 = torch.full((16,), -40.0)
    b3[9] = 0.0
    image, vec = _params(13, mode, w3=zero, b3=b3)
    up = float(np.nextafter(np.float32(0.5), np.float32(1)))
    cls, hist, prob, _ = _both(x, image, vec, lab, (0.5, up), mode)
    assert bool((cls[0] == 9).all()) and bool((cls[1] == 16).all()) and bool((prob == 0.5).all())
    assert int(hist[0, 0, :, 9].sum()) == int((lab <= 16).sum()) == int(hist[0, 1, :, 16].sum())
    # rows of x holding NaN and +-inf (equality with the unfused pair is checked in _both): where a row's logits hold a
    # NaN it counts as the maximum, the first one wins, and the row is never empty
    image, vec = _params(14, mode)
    xb = x.clone()
    xb[5, 7] = float('nan')
    xb[70, 0] = float('inf')
    xb[200, 127] = float('-inf')
    xb[201] = float('nan')
    cls, _, prob, logits = _both(xb, image, vec, lab, (0.25, 0.999), mode)
    for r in logits.isnan().any(-1).nonzero().flatten().tolist():
        assert int(cls[1][r]) == int(logits[r].isnan().nonzero()[0]) and bool(prob[r].isnan()), r
    # a threshold equal to a row's own pb keeps it occupied, the next float above empties it
    row = int((cls[0] < 16).nonzero()[0])
    pb = float(prob[row])
    hip = pkg('hipops')
    with torch.no_grad():
        assert int(hip.occ_mlp_classes(xb, image, vec, pb, **mode)[row]) == int(cls[0][row])
        assert int(hip.occ_mlp_classes(xb, image, vec, float(np.nextafter(np.float32(pb), np.float32(2))), **mode)[row]) == 16
    _prob_is_row_argmax_pb(logits, prob, [row, 0, 332])


def test_head_and_detector_level(tmp_path, monkeypatch):
    """The vocc head on the two golden viewpoints under bf16 autocast: histograms, class map and the detector's
    evaluation are those of the logits path, and the fused launches are what ran."""
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    pkg()
    hip, syn, reg = pkg('hipops'), pkg('synthetic'), pkg('registry')
    det = reg.build_detector(dict(type='VoxelFormer', pts_bbox_head=cases.vocc_head_cfg(),
                                  train_cfg=dict(pts=cases.VOCC_TRAIN_CFG))).eval()
    h = det.pts_bbox_head
    cw = h.code_weights.detach().clone()
    syn.load_seeded(h, 7)
    h.code_weights.data.copy_(cw)
    det.to(DEV)
    calls = dict(confusion=0, classes=0)
    real_conf, real_cls = hip.occ_mlp_confusion, hip.occ_mlp_classes

    def counted(name, fn):
        def run(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return run
    monkeypatch.setattr(hip, 'occ_mlp_confusion', counted('confusion', real_conf))
    monkeypatch.setattr(hip, 'occ_mlp_classes', counted('classes', real_cls))
    w2p, org = syn.camera_batch(2, seed=1)
    feats = syn.vit_features(2, seed=0)
    mlvl = T(feats).to(DEV).permute(1, 0, 2, 3).contiguous()
    labels = _labels(2 * h.voxel_num, 16, torch.Generator().manual_seed(4)).view(2, -1).to(DEV)
    thr = (0.25, 0.5)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        emb = h(mlvl, None, only_bev=True, world2pixel=T(w2p).to(DEV), origin=T(org).to(DEV))
        rows = h.occupancy_from_volume(emb, rows_only=True)
        vox = h.occupancy_from_volume(emb)
        got = h.occupancy_confusion_from_volume(emb, labels, thr)
        n_groups = calls['confusion']
        cls = h.occupancy_classes_from_volume(emb, 0.25)
        pairs = h.get_occupancy_prediction_from_volume(emb, 0.25)['occupancy_preds']
    assert isinstance(rows, tuple) and rows[0].dtype == torch.bfloat16
    assert n_groups == len(rows[1].groups) >= 1 and calls['classes'] == 2
    assert got.shape == (2, 2, 17, 17) and torch.equal(got, h.occupancy_confusion(rows, labels, thr))
    assert int(got[:, :, :, :16].sum()) > 0
    want = h.get_occupancy_prediction(dict(occupancy_preds=vox), 0.25)['occupancy_preds']
    assert cls.shape == (2, h.voxel_num) and want.shape[0] > 0 and torch.equal(pairs, want)
    # fp32 (no autocast): the same methods compose the existing functions, no fused launch
    before = dict(calls)
    with torch.no_grad():
        emb32 = h(mlvl, None, only_bev=True, world2pixel=T(w2p).to(DEV), origin=T(org).to(DEV))
        got32 = h.occupancy_confusion_from_volume(emb32, labels, thr)
        want32 = h.occupancy_confusion(h.occupancy_from_volume(emb32, rows_only=True), labels, thr)
    assert calls == before and torch.equal(got32, want32)
    # detector: evaluate_occupancy(fused=True) == (fused=False), under bf16 autocast
    names = ['scanA_vp0', 'scanA_vp1']
    store = _store(tmp_path, feats, names)
    rng = np.random.default_rng(9)
    n = h.voxel_num
    dense = rng.integers(0, 17, size=(2, n))
    dense[rng.uniform(size=dense.shape) < 0.8] = 16
    metas = _metas(tmp_path, store, names, [cases.detection_gt()] * 2, [_sparse(d) for d in dense])
    a = det.evaluate_occupancy(metas, thresholds=thr, autocast_dtype='bf16', fused=True)
    assert calls['confusion'] == before['confusion'] + n_groups
    b = det.evaluate_occupancy(metas, thresholds=thr, autocast_dtype='bf16', fused=False)
    assert calls['confusion'] == before['confusion'] + n_groups
    assert torch.equal(a.hist, b.hist) and torch.equal(a.last, b.last) and int(a.hist.sum()) == 2 * 2 * n


def test_captured_launch_replays_with_its_thresholds():
    hip = pkg('hipops')
    mode = MODES[0]
    image, vec = _params(21, mode)
    x = _x(2 * 40000, 22, mode)
    lab = _labels(2 * 40000, 16, torch.Generator().manual_seed(8)).to(DEV)
    thr = THRESHOLDS[3]
    with torch.no_grad():
        eager = hip.occ_mlp_confusion(x, image, vec, lab, thr, samples=2, **mode)
        torch.cuda.synchronize()
        hist = torch.zeros_like(eager)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            hip.occ_mlp_confusion(x, image, vec, lab, thr, samples=2, hist=hist, **mode)
        torch.cuda.synchronize()
        assert int(hist.abs().sum()) == 0                                 # capture does not run the kernel
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
    assert int(eager.sum()) > 0 and torch.equal(hist, 3 * eager)
