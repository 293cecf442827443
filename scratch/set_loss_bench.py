"""Detection terms of a training step, ``solver='device'`` against ``solver='fused'``.

    timeout -k 10 300 python scratch/set_loss_bench.py time          one JSON line per batch size (1, 64, 192 viewpoints)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o set_loss -- python scratch/set_loss_bench.py trace
    python scratch/set_loss_bench.py report DIR                      launches and GPU time per call from that trace

What is measured: ``head.loss`` of the vocc head without the occupancy term on a ``PaddedGts`` (random predictions
[6, bs, 100, .], 5-20 boxes per viewpoint) plus the backward to the predictions.  ``time``: HIP events and wall clock, 30
calls after 5 warm-up calls.  ``trace``: per (batch size, solver) 20 calls between two marker launches (a bitwise xor of two
int tensors: no other kernel of the run carries that name), so ``report`` can count the dispatches of exactly those calls.
"""
import glob
import importlib
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)
BATCHES = (1, 64, 192)
SOLVERS = ('device', 'fused')
LAYERS, QUERIES, TRACE_CALLS = 6, 100, 20


def setup():
    import torch
    import cases
    reg = importlib.import_module('vln-ver_amd.registry')
    dev = torch.device('cuda')
    cfg = dict(cases.VOCC_TRAIN_CFG, assigner=dict(cases.VOCC_TRAIN_CFG['assigner'], solver='device'))
    torch.manual_seed(2)
    return torch, dev, reg.build_head(dict(cases.vocc_head_cfg(), train_cfg=cfg)).to(dev).eval()


def inputs(torch, dev, head, bs):
    syn = importlib.import_module('vln-ver_amd.synthetic')
    rng = np.random.default_rng(bs)
    counts = rng.integers(5, 21, bs)
    gts = [syn.detection_gt(1000 * bs + i, int(n), head.num_classes) for i, n in enumerate(counts)]
    gb = [torch.from_numpy(b[:, :7]).to(dev) for b, _ in gts]
    gl = [torch.from_numpy(l).to(dev) for _, l in gts]
    gen = torch.Generator(device=dev).manual_seed(bs)
    all_cls = torch.randn(LAYERS, bs, QUERIES, head.cls_out_channels, device=dev, generator=gen) * 2 - 2
    all_box = torch.randn(LAYERS, bs, QUERIES, 10, device=dev, generator=gen)
    all_box[..., [0, 1]] *= 4.0
    return all_cls.requires_grad_(True), all_box.requires_grad_(True), head.pad_gts(gb, gl, capacity=20)


def step(torch, head, solver, all_cls, all_box, gts):
    head.assigner.solver = solver
    d = head.loss(gts, None, None, dict(all_cls_scores=all_cls, all_bbox_preds=all_box, occupancy_preds=None))
    return d, torch.autograd.grad(sum(d.values()), [all_cls, all_box])


def timed(torch, fn, reps=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
        wall.append((time.perf_counter() - t0) * 1e3)
    s = lambda v: dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4))
    return dict(event_ms=s(ev), wall_ms=s(wall))


def main_time():
    torch, dev, head = setup()
    for bs in BATCHES:
        all_cls, all_box, gts = inputs(torch, dev, head, bs)
        out = {s: step(torch, head, s, all_cls, all_box, gts) for s in SOLVERS}
        rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-30))
        agree = dict(loss=max(abs(float(out['fused'][0][k]) - float(v)) / max(abs(float(v)), 1e-30) for k, v in out['device'][0].items()
                              if float(v) != 0.0),
                     grad_cls=rel(out['fused'][1][0], out['device'][1][0]), grad_box=rel(out['fused'][1][1], out['device'][1][1]))
        res = {s: timed(torch, lambda s=s: step(torch, head, s, all_cls, all_box, gts)) for s in SOLVERS}
        print(json.dumps(dict(viewpoints=bs, relative_difference=agree, gpu=torch.cuda.get_device_name(0), **res)), flush=True)


def main_trace():
    torch, dev, head = setup()
    a, b = torch.arange(64, device=dev, dtype=torch.int32), torch.ones(64, device=dev, dtype=torch.int32)
    for bs in BATCHES:
        all_cls, all_box, gts = inputs(torch, dev, head, bs)
        for solver in SOLVERS:
            for _ in range(5):
                step(torch, head, solver, all_cls, all_box, gts)
            torch.cuda.synchronize()
            torch.bitwise_xor(a, b)
            for _ in range(TRACE_CALLS):
                step(torch, head, solver, all_cls, all_box, gts)
            torch.bitwise_xor(a, b)
            torch.cuda.synchronize()


def main_report(root):
    import csv
    rows = []
    for path in glob.glob(os.path.join(root, '**', '*kernel_trace.csv'), recursive=True):
        rows += [(int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(open(path))]
    rows.sort()
    marks = [i for i, r in enumerate(rows) if 'xor' in r[2].lower()]
    regions = [(bs, s) for bs in BATCHES for s in SOLVERS]
    if len(marks) != 2 * len(regions):
        raise SystemExit('%d marker launches under %s, expected %d' % (len(marks), root, 2 * len(regions)))
    for k, (bs, solver) in enumerate(regions):
        part = rows[marks[2 * k] + 1:marks[2 * k + 1]]
        ours = [r for r in part if 'k_det_costs' in r[2] or 'k_set_loss' in r[2] or 'k_lsa_solve' in r[2]]
        per = {}
        for s, e, n in ours:
            per.setdefault(re.search(r'k_[a-z_0-9]+', n).group(0), []).append((e - s) / 1e3)
        print(json.dumps(dict(viewpoints=bs, solver=solver, calls=TRACE_CALLS, launches_per_call=len(part) / TRACE_CALLS,
                              gpu_us_per_call=round(sum(e - s for s, e, _ in part) / 1e3 / TRACE_CALLS, 2),
                              our_launches_per_call=len(ours) / TRACE_CALLS,
                              our_kernels_median_us={n: round(statistics.median(v), 2) for n, v in sorted(per.items())})))


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'time'
    if mode == 'time':
        main_time()
    elif mode == 'trace':
        main_trace()
    else:
        main_report(sys.argv[2])
