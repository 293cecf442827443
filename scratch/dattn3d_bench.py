"""One decoder cross-attention's sampling, forward + backward: the present chain (torch softmax + location arithmetic +
``voxel_msda``) against the fused op ``voxel_deform_attn``.

    timeout -k 10 600 python scratch/dattn3d_bench.py [time] [OUT.jsonl]     one JSON line per (viewpoints, dtype)

Shape: the vocc.py decoder (900 keys, 100 queries, 8 heads x 96, 1 level, 4 points) for 1, 8 and 64 viewpoints.  ``fp32``: f32
operands.  ``bf16``: what the three Linears emit under bf16 autocast (bf16 value / offsets / logits); the chain widens them as
``VoxelMSDeformAttnFunction`` does, the fused op takes them as they are.  The operands stand for the Linear outputs: both
variants start from the same leaf tensors and end with their gradients (value, offsets, logits, reference points), so the
Linears themselves are in neither.

Timing: device events around blocks of 50 forward + backward calls, 20 blocks per variant, the two variants ALTERNATING
block by block after 3 warm-up blocks each; wall clock around the same blocks (each ends in a synchronise).  Launches per call:
torch profiler, kernels and memsets of 10 calls of each variant, in a pass of its own after the timing.  Every line carries
a hash of the sources it ran (``tree``: sha256 over the kernel sources, the header and the two Python files, first 12 hex
digits) and the box (host name, device name).
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
SHAPE = dict(nk=900, nq=100, heads=8, hd=96, levels=1, points=4, dhw=(4, 15, 15))


def tree_hash():
    h = hashlib.sha256()
    pkg = os.path.join(ROOT, 'vln-ver_amd')
    files = sorted(os.path.join(pkg, 'csrc', f) for f in os.listdir(os.path.join(pkg, 'csrc')) if f.endswith(('.hip', '.h', '.py')))
    files += [os.path.join(ROOT, 'include', 'ver_ops.h'), os.path.join(pkg, 'hipops.py'), os.path.join(pkg, 'modules', 'voxel_decoder.py')]
    for f in files:
        h.update(os.path.relpath(f, ROOT).encode() + b'\0' + open(f, 'rb').read())
    return h.hexdigest()[:12]


def operands(torch, bs, lowp):
    gen = torch.Generator(device='cuda').manual_seed(1000 + bs)
    s = SHAPE
    dt = torch.bfloat16 if lowp else torch.float32
    r = lambda *shape: torch.randn(*shape, device='cuda', generator=gen)
    value = r(bs, s['nk'], s['heads'], s['hd']).to(dt).requires_grad_(True)
    offsets = (r(bs, s['nq'], s['heads'], s['levels'], s['points'], 3) * 2).to(dt).requires_grad_(True)
    logits = r(bs, s['nq'], s['heads'], s['levels'] * s['points']).to(dt).requires_grad_(True)
    ref = torch.rand(bs, s['nq'], s['levels'], 3, device='cuda', generator=gen).requires_grad_(True)
    grad_out = r(bs, s['nq'], s['heads'] * s['hd'])
    grad_out = {torch.float32: grad_out, torch.bfloat16: grad_out.bfloat16()}      # (the chain's out is f32, the fused op's value's dtype)
    shapes = torch.tensor([list(s['dhw'])], device='cuda')
    return dict(value=value, offsets=offsets, logits=logits, ref=ref, grad_out=grad_out, shapes=shapes,
                lsi=torch.zeros(1, dtype=torch.int64, device='cuda'),
                normalizer=torch.tensor([[s['dhw'][2], s['dhw'][1], s['dhw'][0]]], device='cuda', dtype=dt))


def chain(torch, hip, x):
    """VoxelCustomMSDeformableAttention.forward between its Linears and output_proj, fused off."""
    b, nq, heads, nlev, npt, _ = x['offsets'].shape
    w = x['logits'].softmax(-1).view(b, nq, heads, nlev, npt)
    loc = x['ref'][:, :, None, :, None, :] + x['offsets'] / x['normalizer'][None, None, None, :, None, :]
    return hip.voxel_msda(x['value'], x['shapes'], x['lsi'], loc, w)


def fused(torch, hip, x):
    return hip.voxel_deform_attn(x['value'], x['shapes'], x['lsi'], x['ref'], x['offsets'], x['logits'])


VARIANTS = (('chain', chain), ('fused', fused))


def call(torch, hip, fn, x):
    # bf16 operands: under autocast, as in a training step (the chain's softmax then runs in fp32, its division in bf16)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=x['value'].dtype == torch.bfloat16):
        out = fn(torch, hip, x)
    return torch.autograd.grad(out, [x['value'], x['offsets'], x['logits'], x['ref']], x['grad_out'][out.dtype])


def launches(torch, hip, fn, x, calls=10):
    from torch.profiler import ProfilerActivity, profile
    call(torch, hip, fn, x)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            call(torch, hip, fn, x)
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
        raise SystemExit('dattn3d_bench: needs a GPU; nothing is timed without one')
    hip = importlib.import_module('vln-ver_amd.hipops')
    stamp = dict(tree=tree_hash(), box=dict(host=socket.gethostname(), gpu=torch.cuda.get_device_name(0)), torch=torch.__version__)
    sink = open(out_path, 'a') if out_path else None
    for bs in BATCHES:
        for lowp in (False, True):
            x = operands(torch, bs, lowp)
            # relative L2 between the two variants' gradients.  fp32: summation order only.  bf16: the chain rounds offsets / (W, H, D)
            # to bf16 before the add, the fused op does not, and on random operands some samples change their cell
            agree = {k: float((a.float() - b.float()).norm() / b.float().norm()) for k, a, b in
                     zip(('value', 'offsets', 'logits', 'ref'), call(torch, hip, fused, x), call(torch, hip, chain, x))}
            for _ in range(WARM):
                for _, fn in VARIANTS:
                    for _ in range(BLOCK):
                        call(torch, hip, fn, x)
            torch.cuda.synchronize()
            ev, wall = {n: [] for n, _ in VARIANTS}, {n: [] for n, _ in VARIANTS}
            for _ in range(BLOCKS):
                for name, fn in VARIANTS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record()
                    for _ in range(BLOCK):
                        call(torch, hip, fn, x)
                    e1.record()
                    torch.cuda.synchronize()
                    ev[name].append(e0.elapsed_time(e1) * 1e3 / BLOCK)
                    wall[name].append((time.perf_counter() - t0) * 1e6 / BLOCK)
            s = lambda v: dict(min=round(min(v), 2), median=round(statistics.median(v), 2), max=round(max(v), 2))
            line = dict(what='decoder cross-attention sampling, forward + backward', viewpoints=bs, operands='bf16' if lowp else 'fp32',
                        gradient_rel_l2_fused_vs_chain=agree,
                        **{n: dict(event_us_per_call=s(ev[n]), wall_us_per_call=s(wall[n]), launches=launches(torch, hip, fn, x))
                           for n, fn in VARIANTS}, **stamp)
            text = json.dumps(line)
            print(text, flush=True)
            if sink:
                sink.write(text + '\n')
                sink.flush()


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != 'time']
    main(args[0] if args else None)
