"""The class-weighted focal-loss pass against the unweighted one.

    python scratch/focal_weight_bench.py                 one JSON line per size into $OUT/focal_weight_u8_vs_cw.jsonl
    timeout -k 10 300 python scratch/focal_weight_bench.py one 192      one size, in this process

What is measured: ``ver_focal_loss_forward_grad_u8`` against ``ver_focal_loss_forward_grad_u8_cw`` through the C ABI -- the pass
of a training step: loss partials + unscaled gradient in one read and one write of the logits -- on bf16 logits
[504 000 * V, 16] with byte labels, V = 1, 64, 192 viewpoints, gamma = 2, alpha = 0.25, weights drawn from [0.25, 4].  The
gradient goes to a buffer of its own, so every call reads the same logits (the step writes it over them: same traffic).
HIP events around blocks of 20 calls, 15 blocks per entry, the two entries ALTERNATING block by block after 3 warm-up blocks
each; median / min / max of the per-call time over the blocks, and the bytes the pass must move (logits in, gradient out,
labels) over the median.  The unweighted entry is the yardstick: the same process, the same buffers.

Without arguments every size runs as a child process of its own under ``timeout`` and the first failure ends the run; the
parent never opens the GPU.  There is no CPU fall-back: without a device the child fails.
"""
import ctypes
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VIEWPOINTS = (1, 64, 192)
VOXELS, CLASSES = 504000, 16
BLOCK, BLOCKS, WARM = 20, 15, 3
LIMIT_S = 300


def one(v):
    import torch
    hip = importlib.import_module('vln-ver_amd.hipops')
    L = hip.lib()
    n = VOXELS * v
    gen = torch.Generator(device='cuda').manual_seed(v)
    logits = torch.empty(n, CLASSES, device='cuda', dtype=torch.bfloat16)
    for part in logits.split(VOXELS * 16):                                   # (no fp32 copy of the whole tensor)
        part.copy_(torch.randn(part.shape, device='cuda', generator=gen) * 2)
    labels = torch.randint(0, CLASSES + 1, (n,), device='cuda', generator=gen, dtype=torch.uint8)
    table = torch.rand(CLASSES + 1, device='cuda', generator=gen) * 3.75 + 0.25
    grad = torch.empty_like(logits)
    blocks = L.ver_focal_loss_blocks(ctypes.c_long(n), CLASSES)
    partial = torch.zeros(blocks, dtype=torch.float32, device='cuda')
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    tail = (hip._p(partial), hip._p(grad), ctypes.c_long(n), CLASSES, ctypes.c_float(2.0), ctypes.c_float(0.25), 1,
            hip._p(flag), hip._stream())
    entries = (('unweighted', lambda: L.ver_focal_loss_forward_grad_u8(hip._p(logits), hip._p(labels), *tail)),
               ('weighted', lambda: L.ver_focal_loss_forward_grad_u8_cw(hip._p(logits), hip._p(labels), hip._p(table), *tail)))

    def block(call):
        for _ in range(BLOCK):
            if call() != 0:
                raise SystemExit('launch failed: %s' % L.ver_last_error())

    sums = {}
    for name, call in entries:
        for _ in range(WARM):
            block(call)
        sums[name] = float(partial.double().sum())
    torch.cuda.synchronize()
    if int(flag) != 0 or not all(map(lambda s: s == s and s > 0, sums.values())):
        raise SystemExit('bad results: flag %d, sums %r' % (int(flag), sums))
    us = {name: [] for name, _ in entries}
    for _ in range(BLOCKS):
        for name, call in entries:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            block(call)
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / BLOCK)
    moved = n * (CLASSES * 2 * 2 + 1)                                         # logits in, gradient out, one byte per label
    stat = lambda t: dict(median=round(statistics.median(t), 2), min=round(min(t), 2), max=round(max(t), 2))
    med = {name: statistics.median(t) for name, t in us.items()}
    return dict(viewpoints=v, rows=n, logits='bf16', labels='u8', gpu=torch.cuda.get_device_name(0),
                calls_per_block=BLOCK, blocks=BLOCKS, bytes_moved=moved,
                us_per_call={name: stat(t) for name, t in us.items()},
                gb_per_s_at_median={name: round(moved / m / 1e3, 1) for name, m in med.items()},
                weighted_over_unweighted=round(med['weighted'] / med['unweighted'], 4))


def main():
    out = os.environ.get('OUT', os.path.join(ROOT, 'scratch', 'out'))
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, 'focal_weight_u8_vs_cw.jsonl')
    open(path, 'w').close()
    for v in VIEWPOINTS:
        cmd = ['timeout', '-k', '10', str(LIMIT_S), sys.executable, os.path.abspath(__file__), 'one', str(v)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:
            raise SystemExit('%s ended with %d: stopping' % (' '.join(cmd), res.returncode))
        line = res.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        with open(path, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == 'one':
        print(json.dumps(one(int(sys.argv[2]))), flush=True)
    else:
        main()
