"""Occupancy evaluation of one 192-viewpoint batch (504 000 rows x 128 bf16 features per viewpoint) with and without the
logits: the fused launches ver_occ_mlp_confusion / ver_occ_mlp_classes against the two-kernel pairs
ver_occ_mlp_forward + ver_occ_confusion and ver_occ_mlp_forward + ver_occ_predict, on the same x, the folded and centred
chain the head runs.  One and eight thresholds, HIP events, median of 20 launches after warm-up; every launch sequence
of one kind is timed back to back so that the run-to-run spread (min / max) comes from the same runs.  The histograms
and the class maps of the two paths are checked equal.  Prints one JSON line.

    timeout -k 10 600 python scratch/occ_eval_fused_bench.py
"""
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hip = importlib.import_module('vln-ver_amd.hipops')

S, N = int(os.environ.get('VIEWPOINTS', 192)), 504000
dev = torch.device('cuda')
torch.manual_seed(0)
MODE = dict(first_linear=False, centered=True)
w2 = torch.randn(128, 128, device=dev) / 128 ** 0.5
w2 = w2 - w2.mean(0, keepdim=True)
w3 = torch.randn(16, 128, device=dev) * 0.3
r = lambda n, s=0.1: torch.randn(n, device=dev) * s
b2 = r(128)
image = hip.occ_mlp_pack(w2, w2, w3)
vec = hip.occ_mlp_vectors(torch.zeros(128, device=dev), 1 + r(128), r(128), b2 - b2.mean(), 1 + r(128), r(128), r(16, 1.0) - 2.5)
x = torch.empty(S * N, 128, device=dev, dtype=torch.bfloat16)
for s in range(S):                                             # (per viewpoint: the fp32 temporary stays small)
    v = torch.randn(N, 128, device=dev) * 1.5
    x[s * N:(s + 1) * N] = v - v.mean(-1, keepdim=True)
del v
lab = torch.randint(0, 17, (S * N,), device=dev, dtype=torch.uint8)
lab[torch.rand(S * N, device=dev) < 0.9] = 16                 # ~10 % occupied, as a scene
lab[torch.rand(S * N, device=dev) < 0.1] = 255                # invisible voxels
thr8 = (0.05, 0.1, 0.2, 0.25, 0.3, 0.4, 0.5, 0.6)


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


res = dict(batch=[S, N, 128], x_bytes=x.numel() * 2, logit_bytes=S * N * 32, label_bytes=S * N)
torch.cuda.reset_peak_memory_stats()
base = torch.cuda.memory_allocated()
with torch.no_grad():
    for name, thr in (('T1', (0.25,)), ('T8', thr8)):
        hist_f = torch.zeros((S, len(thr), 17, 17), dtype=torch.int64, device=dev)
        hist_u = torch.zeros_like(hist_f)
        res['fused_confusion_%s_ms' % name] = timed(
            lambda: hip.occ_mlp_confusion(x, image, vec, lab, thr, S, hist_f, **MODE))
        res['pair_confusion_%s_ms' % name] = timed(
            lambda: hip.occ_confusion(hip.occ_mlp_forward(x, image, vec, **MODE), lab, thr, S, hist_u))
        res['equal_hist_%s' % name] = bool(torch.equal(hist_f, hist_u))
    res['forward_alone_ms'] = timed(lambda: hip.occ_mlp_forward(x, image, vec, **MODE))
    res['fused_classes_ms'] = timed(lambda: hip.occ_mlp_classes(x, image, vec, 0.25, **MODE))
    # (occ_predict ends in one device -> host read of the pair count, as the reference's torch.where: part of that path)
    res['pair_predict_ms'] = timed(lambda: hip.occ_predict(hip.occ_mlp_forward(x, image, vec, **MODE).view(-1, 16), 0.25))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    cls = hip.occ_mlp_classes(x, image, vec, 0.25, **MODE)
    torch.cuda.synchronize()
    res['fused_classes_peak_bytes'] = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    pairs = hip.occ_predict(hip.occ_mlp_forward(x, image, vec, **MODE).view(-1, 16), 0.25)
    torch.cuda.synchronize()
    res['pair_predict_peak_bytes'] = torch.cuda.max_memory_allocated() - base
    idx, = torch.where(cls < 16)
    res['equal_pairs'] = bool(torch.equal(torch.stack([idx, cls[idx].long()], -1), pairs))
res['fused_confusion_T1_GBps'] = (res['x_bytes'] + res['label_bytes']) / res['fused_confusion_T1_ms']['median'] / 1e6
print(json.dumps(res))
out = os.path.join(ROOT, os.environ.get('OUT', os.path.join('scratch', 'out')))      # logs and results: kept out of git
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, 'occ_eval_fused_bench.json'), 'w') as f:
    json.dump(res, f)
assert res['equal_hist_T1'] and res['equal_hist_T8'] and res['equal_pairs']
