"""Occupancy IoU / mIoU on the device (``ver_occ_confusion``): every histogram is held to exact integer equality with
the reference's golden histogram, with the existing device path (``occ_predict`` -> ``dense_labels`` -> ``SSCMetrics``)
or with the same counts made by torch ops.  ``-m gpu``."""
import numpy as np
import pytest
import torch

import cases
from test_detector_cpu import _metas, _sparse, _store
from util import golden, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = torch.from_numpy
THRESHOLDS = {1: (0.5,), 3: (0.25, 0.5, 0.7), 8: (0.05, 0.1, 0.25, 0.3, 0.5, 0.6, 0.75, 0.9)}


def _head(cfg=None):
    pkg()
    return pkg('registry').build_head(cfg or cases.vocc_head_cfg(only_occ=True))


def _predict_hist(logits, labels, thresholds, samples):
    """The existing path: ver_occ_predict pairs -> dense labels -> the reference's SSCMetrics, per sample and threshold.
    logits GPU [samples * rows, C], labels numpy [samples * rows]."""
    hip, metrics = pkg('hipops'), pkg('occupancy_metrics')
    c = logits.shape[1]
    rows = logits.shape[0] // samples
    out = np.zeros((samples, len(thresholds), c + 1, c + 1), dtype=np.int64)
    for s in range(samples):
        gt = labels[s * rows:(s + 1) * rows]
        for t, thr in enumerate(thresholds):
            pairs = hip.occ_predict(logits[s * rows:(s + 1) * rows], thr).cpu().numpy()
            m = metrics.SSCMetrics(c + 1)
            m.add_batch(metrics.dense_labels(pairs, rows, c), gt)
            out[s, t] = m.hist.astype(np.int64)
    return out


def _adversarial(n, c, gen):
    """Logits around the edges of the classification: equal logits, saturated sigmoids, NaN / +-inf, logit 0 (sigmoid
    exactly 0.5 = a threshold of the sweep), on a random background."""
    x = torch.randn(n, c, generator=gen) * 2 - 2
    x[::7] = x[::7, :1]                                  # every class equal: the first one wins
    x[1::11, 1:4] = torch.tensor([17.0, 18.5, 30.0])     # several fp32 sigmoids are 1.0
    x[2::13] = -40.0
    x[2::13, c // 2] = 0.0                               # best probability exactly 0.5
    x[3::17, 2] = float('nan')
    x[4::19, 0] = float('inf')
    x[5::23] = float('-inf')
    x[6::29, c - 1] = float('nan')
    x[6::29, 0] = float('inf')
    return x


def _labels(n, c, gen):
    lab = torch.randint(0, c + 1, (n,), generator=gen)
    lab[torch.rand(n, generator=gen) < 0.6] = c          # most voxels empty
    lab[torch.rand(n, generator=gen) < 0.05] = 255       # invisible
    odd = torch.rand(n, generator=gen) < 0.03
    lab[odd] = torch.randint(c + 1, 255, (int(odd.sum()),), generator=gen)    # any value above C is ignored too
    return lab.to(torch.uint8)


def test_golden_histogram_on_the_kernel():
    g = golden('post_vocc')
    h = _head()
    logits, gt = cases.occupancy_loss_inputs(seed=33, n=6000)
    labels = T(gt).to(torch.uint8)[None].to(DEV)
    hist = h.occupancy_confusion(T(logits)[None].to(DEV), labels)
    assert hist.is_cuda and hist.dtype == torch.int64
    hist = h.occupancy_confusion(T(logits[::-1].copy())[None].to(DEV), labels, hist=hist)
    assert np.array_equal(hist[0, 0].cpu().numpy(), g['hist'])
    m = pkg('occupancy_metrics').DeviceSSCMetrics(17, device=DEV)
    st = m.add_hist(hist).get_stats()
    assert float(st['miou']) == pytest.approx(float(g['miou']), rel=1e-12)
    assert float(st['iou']) == pytest.approx(float(g['iou']), rel=1e-12)


@pytest.mark.parametrize('rows', [6001, 504000])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_kernel_equals_the_predict_path(rows, dtype):
    hip = pkg('hipops')
    gen = torch.Generator().manual_seed(rows)
    for c, nt in ((8, 1), (16, 3), (32, 8), (16, 8)):
        thr = THRESHOLDS[nt]
        for samples in (1, 3):
            x = _adversarial(samples * rows, c, gen).to(dtype)
            lab = _labels(samples * rows, c, gen)
            got = hip.occ_confusion(x.to(DEV), lab.to(DEV), thr, samples).cpu().numpy()
            want = _predict_hist(x.to(DEV), lab.numpy(), thr, samples)
            assert np.array_equal(got, want), (rows, dtype, c, nt, samples)


def test_per_sample_slices_accumulation_and_empty_batch():
    hip = pkg('hipops')
    gen = torch.Generator().manual_seed(2)
    rows, thr = 70001, THRESHOLDS[3]
    x = _adversarial(3 * rows, 16, gen).bfloat16().to(DEV)
    lab = _labels(3 * rows, 16, gen).to(DEV)
    whole = hip.occ_confusion(x, lab, thr, samples=3)
    for s in range(3):
        one = hip.occ_confusion(x[s * rows:(s + 1) * rows], lab[s * rows:(s + 1) * rows], thr)
        assert torch.equal(whole[s], one[0])
    merged = hip.occ_confusion(x, lab, thr, samples=1)
    assert torch.equal(whole.sum(0), merged[0])
    assert int(merged[0, 0].sum()) == int((lab <= 16).sum())
    twice = hip.occ_confusion(x, lab, thr, samples=3, hist=whole.clone())
    assert torch.equal(twice, 2 * whole)
    keep = twice.clone()
    out = hip.occ_confusion(x[:0], lab[:0], thr, samples=3, hist=twice)
    assert out is twice and torch.equal(twice, keep)


def test_rows_tuple_equals_reference_order():
    """The row-order logits of the lattice path (labels permuted) give the per-sample histograms of the reference-order
    logits."""
    torch.backends.cuda.matmul.allow_tf32 = False
    syn = pkg('synthetic')
    h = _head(cases.vocc_head_cfg()).eval()
    syn.load_seeded(h, 7)
    h.to(DEV)
    w2p, org = syn.camera_batch(2, seed=1)
    feats = T(syn.vit_features(2, seed=0)).to(DEV).permute(1, 0, 2, 3).contiguous()
    gen = torch.Generator().manual_seed(4)
    labels = _labels(2 * h.voxel_num, 16, gen).view(2, -1).to(DEV)
    with torch.no_grad():
        emb = h(feats, None, only_bev=True, world2pixel=T(w2p).to(DEV), origin=T(org).to(DEV))
        rows = h.occupancy_from_volume(emb, rows_only=True)
        vox = h.occupancy_from_volume(emb)
    assert isinstance(rows, tuple)
    thr = (0.25, 0.5)
    a = h.occupancy_confusion(rows, labels, thr)
    b = h.occupancy_confusion(vox, labels, thr)
    assert a.shape == (2, 2, 17, 17) and torch.equal(a, b)
    assert int(a[:, :, :16, :16].sum()) > 0 and int(a[:, :, :, :16].sum()) > 0      # not all predicted empty


def _chunked_torch(x, lab, samples, thr, chunk=8):
    c = x.shape[1]
    k = c + 1
    rows = x.shape[0] // samples
    out = torch.zeros((samples, len(thr), k, k), dtype=torch.int64, device=x.device)
    for s0 in range(0, samples, chunk):
        s1 = min(samples, s0 + chunk)
        p = x[s0 * rows:s1 * rows].float().sigmoid()
        gt = lab[s0 * rows:s1 * rows].long().view(s1 - s0, rows)
        keep = gt < k
        first = torch.arange(s1 - s0, device=x.device)[:, None] * k + gt
        for t, v in enumerate(thr):
            pred = torch.cat((p, torch.full_like(p[:, :1], v)), -1).argmax(-1).view(s1 - s0, rows)
            out[s0:s1, t] = torch.bincount((first * k + pred)[keep], minlength=(s1 - s0) * k * k).view(-1, k, k)
        del p
    return out


@pytest.mark.parametrize('samples', [192, 280])
def test_regime_batches_against_torch(samples):
    """The evaluation batch (192 viewpoints x 504 000 rows x 16 bf16 classes, 1.55e9 logits) and one past 2^31 logit
    elements (280 viewpoints)."""
    hip = pkg('hipops')
    rows = 504000
    torch.manual_seed(samples)
    x = (torch.randn(samples * rows, 16, device=DEV, dtype=torch.bfloat16) * 2 - 2)
    assert samples < 270 or x.numel() > 2 ** 31
    lab = torch.randint(0, 17, (samples * rows,), device=DEV, dtype=torch.uint8)
    lab[torch.rand(samples * rows, device=DEV) < 0.7] = 16
    lab[torch.rand(samples * rows, device=DEV) < 0.02] = 255
    thr = THRESHOLDS[3]
    got = hip.occ_confusion(x, lab, thr, samples)
    want = _chunked_torch(x, lab, samples, thr)
    assert torch.equal(got, want)
    assert int(got[-1].sum()) == 3 * int((lab[-rows:] <= 16).sum())       # the last sample, past 2^31 at 280, counted


def test_detector_evaluate_occupancy_equals_forward_test_path(tmp_path):
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    pkg()
    syn, reg, metrics = pkg('synthetic'), pkg('registry'), pkg('occupancy_metrics')
    det = reg.build_detector(dict(type='VoxelFormer', pts_bbox_head=cases.vocc_head_cfg(),
                                  train_cfg=dict(pts=cases.VOCC_TRAIN_CFG))).eval()
    head = det.pts_bbox_head
    cw = head.code_weights.detach().clone()
    syn.load_seeded(head, 7)
    head.code_weights.data.copy_(cw)
    det.to(DEV)
    names = ['scanA_vp0', 'scanA_vp1']
    feats = syn.vit_features(2, seed=0)
    store = _store(tmp_path, feats, names)
    rng = np.random.default_rng(9)
    n = head.voxel_num
    dense = rng.integers(0, 17, size=(2, n))
    dense[rng.uniform(size=dense.shape) < 0.8] = 16
    metas = _metas(tmp_path, store, names, [cases.detection_gt()] * 2, [_sparse(d) for d in dense])
    invalid = rng.choice(n, 40000, replace=False)
    np.save(str(tmp_path / 'invalid_0.npy'), invalid)
    metas[0]['occ_invalid_path'] = str(tmp_path / 'invalid_0.npy')       # the second viewpoint has no invalid file
    thr = (0.25, 0.5)
    got = det.evaluate_occupancy(metas, thresholds=thr)
    assert got.hist.shape == (2, 17, 17) and got.last.shape == (2, 2, 17, 17)
    with torch.no_grad():
        _, occ = det.forward_test(img_metas=metas)
        pairs = {0.25: occ['occupancy_preds'].cpu().numpy()}
        _, occ = det.simple_test(metas, occ_threshold=0.5)[1:]
        pairs[0.5] = occ['occupancy_preds'].cpu().numpy()
    for t, v in enumerate(thr):
        total = metrics.SSCMetrics(17)
        for b in range(2):
            p = pairs[v]
            mine = p[(p[:, 0] >= b * n) & (p[:, 0] < (b + 1) * n)] - np.array([b * n, 0])
            vis = None
            if b == 0:
                vis = np.ones(n, dtype=np.uint8)
                vis[invalid] = 0
            one = metrics.SSCMetrics(17)
            one.add_batch(metrics.dense_labels(mine, n, 16), dense[b], visible_mask=vis)
            total.add_batch(metrics.dense_labels(mine, n, 16), dense[b], visible_mask=vis)
            assert np.array_equal(got.last[b, t].cpu().numpy(), one.hist), (b, v)
        assert np.array_equal(got.hist[t].cpu().numpy(), total.hist), v
        st, want = got.get_stats(t), total.get_stats()
        assert float(st['miou']) == float(want['miou']) and float(st['iou']) == float(want['iou'])
    again = det.evaluate_occupancy(metas, metrics=got)                    # accumulates into the metrics it is given
    assert again is got and torch.equal(got.hist, 2 * got.last.sum(0))


def test_captured_launch_replays_with_its_thresholds():
    hip = pkg('hipops')
    gen = torch.Generator().manual_seed(8)
    x = _adversarial(2 * 40000, 16, gen).to(DEV)
    lab = _labels(2 * 40000, 16, gen).to(DEV)
    thr = THRESHOLDS[3]
    eager = hip.occ_confusion(x, lab, thr, samples=2)
    torch.cuda.synchronize()
    hist = torch.zeros_like(eager)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.occ_confusion(x, lab, thr, samples=2, hist=hist)
    torch.cuda.synchronize()
    assert int(hist.abs().sum()) == 0                                     # capture does not run the kernel
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(hist, 3 * eager)
