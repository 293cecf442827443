"""One decoder layer's self-attention branch, forward + backward: ``MultiheadAttention`` with the switch off (torch's
nn.MultiheadAttention, need_weights=True) against ``fused=True`` (``hipops.mha_core_joint``).

    timeout -k 10 600 python scratch/mha_bench.py [OUT.jsonl]     one JSON line per batch size

Shape: the vocc.py decoder (100 queries, 8 heads x 96, dropout 0.1), training mode, bf16 autocast, B = 1, 8 and 64.  Both
variants run the same module object (the switch is flipped between blocks), from the query / query_pos leaves through the
in-projection, the attention and out_proj, and back to the gradients of the query and the four parameters; the residual add
and its dropout are in neither (``defer_residual=True``: they belong to the LayerNorm that follows).

Timing: device events around blocks of 50 forward + backward calls, 20 blocks per variant, the two variants ALTERNATING
block by block after 3 warm-up blocks each; wall clock around the same blocks (each ends in a synchronise).  Launches per call:
torch profiler, kernels and memsets of 10 calls of each variant, in a pass of its own after the timing.  Every line carries
a hash of the sources it ran and the box.
"""
import hashlib
import importlib
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCHES = (1, 8, 64)
BLOCK, BLOCKS, WARM = 50, 20, 3
SHAPE = dict(nq=100, heads=8, embed=768, dropout=0.1)


def tree_hash():
    h = hashlib.sha256()
    pkg = os.path.join(ROOT, 'vln-ver_amd')
    files = sorted(os.path.join(pkg, 'csrc', f) for f in os.listdir(os.path.join(pkg, 'csrc')) if f.endswith(('.hip', '.h', '.py')))
    files += [os.path.join(ROOT, 'include', 'ver_ops.h'), os.path.join(pkg, 'hipops.py'), os.path.join(pkg, 'modules', 'voxel_decoder.py')]
    for f in files:
        h.update(os.path.relpath(f, ROOT).encode() + b'\0' + open(f, 'rb').read())
    return h.hexdigest()[:12]


def call(torch, mod, x, fused):
    mod.fused = fused
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = mod(x['query'], query_pos=x['pos'], defer_residual=True).branch
    return torch.autograd.grad(out, x['wrt'], x['grad'][out.dtype])


def launches(torch, mod, x, fused, calls=10):
    from torch.profiler import ProfilerActivity, profile
    call(torch, mod, x, fused)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            call(torch, mod, x, fused)
        torch.cuda.synchronize()
    names = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            names[e.name] = names.get(e.name, 0) + 1
    kernels = sum(n for k, n in names.items() if 'mem' not in k.lower()[:6])
    return dict(per_call=sum(names.values()) / calls, kernels_per_call=kernels / calls,
                memsets_and_copies_per_call=(sum(names.values()) - kernels) / calls,
                names=sorted(k[:60] for k in names))


def main(out_path=None):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('mha_bench: needs a GPU; nothing is timed without one')
    importlib.import_module('vln-ver_amd')
    dec = importlib.import_module('vln-ver_amd.modules.voxel_decoder')
    syn = importlib.import_module('vln-ver_amd.synthetic')
    stamp = dict(tree=tree_hash(), box=dict(host=socket.gethostname(), gpu=torch.cuda.get_device_name(0)), torch=torch.__version__)
    sink = open(out_path, 'a') if out_path else None
    s = SHAPE
    mod = dec.MultiheadAttention(embed_dims=s['embed'], num_heads=s['heads'], dropout=s['dropout'])
    syn.load_seeded(mod, 7)
    mod = mod.cuda().train()
    variants = (('chain', False), ('fused', True))
    for bs in BATCHES:
        gen = torch.Generator(device='cuda').manual_seed(1000 + bs)
        r = lambda: torch.randn(s['nq'], bs, s['embed'], device='cuda', generator=gen)
        g = r()
        x = dict(query=r().requires_grad_(True), pos=r(), grad={torch.float32: g, torch.bfloat16: g.bfloat16()})
        x['wrt'] = [x['query']] + list(mod.parameters())
        # relative L2 between the two variants' gradients with the attention dropout off (with it on the masks differ)
        mod.attn.dropout = 0.0
        agree = {k: float((a.float() - b.float()).norm() / b.float().norm()) for k, a, b in
                 zip(['query'] + [n for n, _ in mod.named_parameters()], call(torch, mod, x, True), call(torch, mod, x, False))}
        mod.attn.dropout = s['dropout']
        for _ in range(WARM):
            for _, fused in variants:
                for _ in range(BLOCK):
                    call(torch, mod, x, fused)
        torch.cuda.synchronize()
        ev, wall = {n: [] for n, _ in variants}, {n: [] for n, _ in variants}
        for _ in range(BLOCKS):
            for name, fused in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                for _ in range(BLOCK):
                    call(torch, mod, x, fused)
                e1.record()
                torch.cuda.synchronize()
                ev[name].append(e0.elapsed_time(e1) * 1e3 / BLOCK)
                wall[name].append((time.perf_counter() - t0) * 1e6 / BLOCK)
        st = lambda v: dict(min=round(min(v), 2), median=round(statistics.median(v), 2), max=round(max(v), 2))
        line = dict(what='decoder self-attention branch (in-projection .. out_proj), forward + backward, training, bf16 autocast',
                    batch=bs, queries=s['nq'], heads=s['heads'], embed=s['embed'], attn_dropout=s['dropout'],
                    gradient_rel_l2_fused_vs_chain_without_dropout=agree,
                    **{n: dict(event_us_per_call=st(ev[n]), wall_us_per_call=st(wall[n]), launches=launches(torch, mod, x, f))
                       for n, f in variants}, **stamp)
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + '\n')
            sink.flush()


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else None)
