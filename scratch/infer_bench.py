"""Inference at the reference's batch point: the default ``simple_test`` against ``device_inference`` (eager ``head.infer``)
and ``graphs.GraphedInference``.

    timeout -k 10 600 python scratch/infer_bench.py [--out profiles/infer_eager_vs_graph.jsonl] [--iters 40] [--warmup 5]

vocc.py's head with seeded weights under bf16 autocast, synthetic viewpoints from a feature store on disk (every key is read
once and cached, so the timed calls do no file I/O).  Per batch size (1 and 8 viewpoints) the variants run ALTERNATING, one
call each per round, on one GPU in one process: wall clock from the call to its results on the host (every variant ends
with its own device -> host copy: that is the contract being compared), ``--warmup`` rounds dropped, min / median / max of
``--iters`` rounds.  Kernel launches of one call of each variant are counted with the torch profiler in a separate,
untimed call (null where the profiler reports no device activity).
  simple_test        the default path: full forward with voxel-order logits, ``ver_occ_predict`` + its host read, host decode
  device_inference   ``VoxelFormer.device_inference = True``: ``head.infer`` + one copy of all tables
  graphed            ``GraphedInference`` replay + ``results()`` (one viewpoint per graph; at 8 viewpoints one 8-wide graph)
"""
import argparse
import importlib
import json
import os
import pathlib
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)
BATCHES = (1, 8)


def setup(tmp, n):
    import torch
    import cases
    from test_detector_cpu import _metas, _sparse, _store
    syn, reg = importlib.import_module('vln-ver_amd.synthetic'), importlib.import_module('vln-ver_amd.registry')
    torch.backends.cuda.matmul.allow_tf32 = False
    det = reg.build_detector(dict(type='VoxelFormer', pts_bbox_head=cases.vocc_head_cfg(), train_cfg=dict(pts=cases.VOCC_TRAIN_CFG),
                                  autocast_dtype='bf16')).eval()
    head = det.pts_bbox_head
    cw = head.code_weights.detach().clone()
    syn.load_seeded(head, 7)
    head.code_weights.data.copy_(cw)
    det.to(torch.device('cuda'))
    names = ['scanA_vp%d' % i for i in range(n)]
    store = _store(tmp, syn.vit_features(n, seed=0), names)
    gts = [cases.detection_gt(seed=40 + i, num_gt=3) for i in range(n)]
    metas = _metas(tmp, store, names, gts, [_sparse(np.full(504000, 16)) for _ in range(n)])
    return torch, det, metas


def launches(torch, fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower()
                and 'memset' not in e.name.lower())
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    graphs = importlib.import_module('vln-ver_amd.graphs')
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        torch, det, metas_all = setup(pathlib.Path(tmp), max(BATCHES))
        head = det.pts_bbox_head
        for bs in BATCHES:
            metas = metas_all[:bs]
            bf16 = lambda: torch.autocast('cuda', dtype=torch.bfloat16, cache_enabled=False)

            def simple_test():
                det.device_inference = False
                with torch.no_grad(), bf16():
                    _, boxes, occ = det.simple_test(metas)
                return occ['occupancy_preds'].cpu()

            def device_inference():
                det.device_inference = True
                with torch.no_grad():
                    out = det.simple_test(metas)
                det.device_inference = False
                return out

            feats = det.viewpoint_features(metas)
            w2p, org = head.transformer.encoder._cameras(bs, feats.device, dict(img_metas=metas))
            step = graphs.GraphedInference(head, feats, w2p, org, pair_capacity=bs * head.voxel_num)

            def graphed():
                step(det.viewpoint_features(metas), w2p, org)
                return step.results(metas)

            variants = dict(simple_test=simple_test, device_inference=device_inference, graphed=graphed)
            ms = {k: [] for k in variants}
            for it in range(a.warmup + a.iters):
                for name, fn in variants.items():                  # alternating: one call of each per round
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if it >= a.warmup:
                        ms[name].append((time.perf_counter() - t0) * 1e3)
            s = lambda v: dict(min=round(min(v), 3), median=round(statistics.median(v), 3), max=round(max(v), 3))
            line = dict(viewpoints=bs, gpu=torch.cuda.get_device_name(0), autocast='bf16', iters=a.iters, warmup=a.warmup,
                        pair_capacity=bs * head.voxel_num, wall_ms={k: s(v) for k, v in ms.items()},
                        kernel_launches_per_call={k: launches(torch, fn) for k, fn in variants.items()})
            print(json.dumps(line), flush=True)
            lines.append(line)
            step = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(''.join(json.dumps(ln) + '\n' for ln in lines))


if __name__ == '__main__':
    main()
