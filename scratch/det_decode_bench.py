"""``DeviceDetMetrics.add`` with the torch decode chain against ``fused=True``.

    timeout -k 10 300 python scratch/det_decode_bench.py time          one JSON line per batch size (1, 8, 192 viewpoints)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o det_decode -- python scratch/det_decode_bench.py trace
    python scratch/det_decode_bench.py report DIR                      launches and GPU time per call from that trace

What is measured: ``DeviceDetMetrics.add(head, preds, gts, fused=...)`` of the vocc head (random predictions [2, bs, 100, .],
fp32 and -- ``time`` only -- bf16 logits, 0-8 boxes per viewpoint in 8 slots): decode + ``det_match``.  ``time``: HIP events
and wall clock around blocks of 20 calls, 30 blocks per variant, the two variants ALTERNATING block by block after 3 warm-up
blocks each.  ``trace``: per (batch size, variant) 20 calls between two marker launches (a bitwise xor of two int tensors: no
other kernel of the run carries that name), so ``report`` can count the dispatches of exactly those calls.
"""
import glob
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)
BATCHES = (1, 8, 192)
VARIANTS = (('torch', False), ('fused', True))
BLOCK, BLOCKS, WARM = 20, 30, 3


def setup():
    import torch
    import cases
    import det_eval_helper as H
    head = H.build_head('cuda')
    metrics = importlib.import_module('vln-ver_amd.detection_metrics').DeviceDetMetrics(cases.CLASS_NUM, H.THR, device='cuda')
    return torch, H, head, metrics


def inputs(torch, H, head, bs, lowp=False):
    preds = {k: v.cuda() for k, v in H.random_head_outputs(100 + bs, bs).items()}
    lists = head.get_bboxes(preds)
    gts = [H.gts_near(lists[i], 1000 * bs + i, (3 * i + bs) % 9) for i in range(bs)]
    if lowp:
        preds = dict(preds, all_cls_scores=preds['all_cls_scores'].bfloat16())
    return preds, head.pad_gts([g[0] for g in gts], [g[1] for g in gts], capacity=8)


def block(metrics, head, preds, gts, fused):
    for _ in range(BLOCK):
        metrics.add(head, preds, gts, fused=fused)
    metrics._parts.clear()                               # (the records of a benchmark are not kept; no launch)


def main_time():
    torch, H, head, metrics = setup()
    for bs in BATCHES:
        for lowp in (False, True):
            preds, gts = inputs(torch, H, head, bs, lowp)
            for _ in range(WARM):
                for _, fused in VARIANTS:
                    block(metrics, head, preds, gts, fused)
            torch.cuda.synchronize()
            ev, wall = {n: [] for n, _ in VARIANTS}, {n: [] for n, _ in VARIANTS}
            for _ in range(BLOCKS):
                for name, fused in VARIANTS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record()
                    block(metrics, head, preds, gts, fused)
                    e1.record()
                    torch.cuda.synchronize()
                    ev[name].append(e0.elapsed_time(e1) * 1e3 / BLOCK)
                    wall[name].append((time.perf_counter() - t0) * 1e6 / BLOCK)
            s = lambda v: dict(min=round(min(v), 2), median=round(statistics.median(v), 2), max=round(max(v), 2))
            print(json.dumps(dict(viewpoints=bs, logits='bf16' if lowp else 'fp32', gpu=torch.cuda.get_device_name(0),
                                  **{n: dict(event_us_per_call=s(ev[n]), wall_us_per_call=s(wall[n])) for n, _ in VARIANTS})),
                  flush=True)


def main_trace():
    torch, H, head, metrics = setup()
    a, b = torch.arange(64, device='cuda', dtype=torch.int32), torch.ones(64, device='cuda', dtype=torch.int32)
    for bs in BATCHES:
        preds, gts = inputs(torch, H, head, bs)
        for _, fused in VARIANTS:
            block(metrics, head, preds, gts, fused)
            torch.cuda.synchronize()
            torch.bitwise_xor(a, b)
            block(metrics, head, preds, gts, fused)
            torch.bitwise_xor(a, b)
            torch.cuda.synchronize()
    # the kernel alone at its limit: 8 samples of 1 024 queries x 16 classes (16 384 keys), all 1 024 slots
    hip = importlib.import_module('vln-ver_amd.hipops')
    gen = torch.Generator(device='cuda').manual_seed(0)
    cls = torch.randn(8, 1024, 16, device='cuda', generator=gen)
    box = torch.randn(8, 1024, 10, device='cuda', generator=gen)
    decode = lambda: hip.det_decode(cls, box, [-10, -10, -5, 10, 10, 5], 0.5, True, 1024)
    decode()
    torch.cuda.synchronize()
    torch.bitwise_xor(a, b)
    for _ in range(BLOCK):
        decode()
    torch.bitwise_xor(a, b)
    torch.cuda.synchronize()


def main_report(root):
    import csv
    rows = []
    for path in glob.glob(os.path.join(root, '**', '*kernel_trace.csv'), recursive=True):
        rows += [(int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(open(path))]
    rows.sort()
    marks = [i for i, r in enumerate(rows) if 'xor' in r[2].lower()]
    regions = [(bs, name) for bs in BATCHES for name, _ in VARIANTS] + [('8 x 16384 keys, K = 1024', 'kernel alone')]
    if len(marks) != 2 * len(regions):
        raise SystemExit('%d marker launches under %s, expected %d' % (len(marks), root, 2 * len(regions)))
    for k, (bs, name) in enumerate(regions):
        part = rows[marks[2 * k] + 1:marks[2 * k + 1]]
        ours = {}
        for s, e, n in part:
            for kernel in ('k_det_decode', 'k_det_match'):
                if kernel in n:
                    ours.setdefault(kernel, []).append((e - s) / 1e3)
        print(json.dumps(dict(viewpoints=bs, decode=name, calls=BLOCK, launches_per_call=len(part) / BLOCK,
                              gpu_us_per_call=round(sum(e - s for s, e, _ in part) / 1e3 / BLOCK, 2),
                              our_kernels_median_us={n: round(statistics.median(v), 2) for n, v in sorted(ours.items())})))


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'time'
    if mode == 'time':
        main_time()
    elif mode == 'trace':
        main_trace()
    else:
        main_report(sys.argv[2])
