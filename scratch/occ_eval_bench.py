"""Occupancy evaluation of one 192-viewpoint batch (504 000 rows x 16 classes, bf16 logits), two ways:
* ver_occ_confusion with 1 and with 8 thresholds (HIP events, median of 20 launches);
* the per-viewpoint host path of evaluate_occ_iou: occ_predict -> .cpu() -> dense_labels -> SSCMetrics.add_batch with a
  visible mask (wall clock over the whole batch).
The two histograms at threshold 0.25 are checked equal.  Prints one JSON line.

    timeout -k 10 600 python scratch/occ_eval_bench.py
"""
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hip = importlib.import_module('vln-ver_amd.hipops')
metrics = importlib.import_module('vln-ver_amd.occupancy_metrics')

S, N, C = 192, 504000, 16
dev = torch.device('cuda')
torch.manual_seed(0)
x = torch.randn(S * N, C, device=dev, dtype=torch.bfloat16) * 2 - 2
lab = torch.randint(0, C + 1, (S * N,), device=dev, dtype=torch.uint8)
lab[torch.rand(S * N, device=dev) < 0.9] = C                 # ~10 % occupied, as a scene
lab[torch.rand(S * N, device=dev) < 0.1] = 255                # invisible voxels
thr8 = (0.05, 0.1, 0.2, 0.25, 0.3, 0.4, 0.5, 0.6)


def kernel_ms(thr, reps=20):
    hist = torch.zeros((S, len(thr), C + 1, C + 1), dtype=torch.int64, device=dev)
    for _ in range(3):
        hip.occ_confusion(x, lab, thr, S, hist)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip.occ_confusion(x, lab, thr, S, hist)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


res = dict(batch=[S, N, C], dtype='bf16', logit_bytes=x.numel() * 2)
res['kernel_T1_ms'], res['kernel_T1_min_ms'] = kernel_ms((0.25,))
res['kernel_T8_ms'], res['kernel_T8_min_ms'] = kernel_ms(thr8)
res['kernel_T1_GBps'] = (x.numel() * 2 + lab.numel()) / res['kernel_T1_ms'] / 1e6

got = hip.occ_confusion(x, lab, (0.25,), S)[:, 0].sum(0).cpu().numpy()
torch.cuda.synchronize()
lab_host = lab.view(S, N).cpu().numpy()
m = metrics.SSCMetrics(C + 1)
t0 = time.perf_counter()
for s in range(S):
    pairs = hip.occ_predict(x[s * N:(s + 1) * N], 0.25).cpu().numpy()
    dense = metrics.dense_labels(pairs, N, C)
    gt = lab_host[s]
    m.add_batch(dense, gt, visible_mask=(gt != 255).astype(np.uint8))
res['host_path_ms'] = (time.perf_counter() - t0) * 1e3
res['host_path_ms_per_viewpoint'] = res['host_path_ms'] / S
res['equal'] = bool(np.array_equal(m.hist.astype(np.int64), got))
res['speedup_T1'] = res['host_path_ms'] / res['kernel_T1_ms']
print(json.dumps(res))
out = os.path.join(ROOT, os.environ.get('OUT', os.path.join('scratch', 'out')))      # logs and results: kept out of git
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, 'occ_eval_bench.json'), 'w') as f:
    json.dump(res, f)
assert res['equal']
