"""One-viewpoint training steps under data parallelism, three routes, and the two exchange kernels.

    python -m torch.distributed.run --nproc-per-node 1 scratch/ddp_graph_bench.py nccl lift      one-rank RCCL group
    python -m torch.distributed.run --nproc-per-node 2 scratch/ddp_graph_bench.py gloo multi     two gloo ranks on one GPU
    python scratch/ddp_graph_bench.py kernels                                                    no process group

Rank 0 prints one JSON line and appends it to $OUT/ddp_graph_vs_eager.jsonl (default scratch/out).  Run every command under
its own ``timeout``.

Steps: bench.py's init, inputs and optimizer settings (``ClipAdamW`` lr 1e-4, weight decay 0.01, max_norm 300), bf16 autocast,
train mode, ONE viewpoint per rank; ``lift`` = bench.py's LiftTrainer, ``multi`` = the whole vocc head.  Three identical models per
process, routes ALTERNATING block by block:

  (a) graph   ``GraphedLiftStep`` / ``GraphedTrainStep`` with ``exchange=``: graph A, one eager all-reduce of the flat buffer, graph B;
  (b) eager   the eager exchanged step: backward, ``pack``, ``all_reduce``, ``step(exchange)`` (multi: ``solver='fused'``);
  (c) ddp     the route before the exchange: ``ddp.wrap_ddp`` (bf16 compression hook under RCCL, as bench.py sets it) + eager
              ``ClipAdamW`` on the bucket views (multi: bench.py's FullTrainer, Hungarian targets solved on the host).

The wire of (a) and (b) is what (c) puts on it: bf16 under RCCL, fp32 under gloo.  A block is 5 steps of one route between two
device synchronisations, timed on the host clock of rank 0; 2 warm-up blocks and 7 measured blocks per route; median / min /
max of the per-step time over the blocks.

``kernels``: ``ver_grad_pack`` and ``ver_clip_adamw_step_flat`` on both wires and ``ver_clip_adamw_step_tensors`` over the
lifting step's parameter list (random values), HIP events around blocks of 10 calls, 7 blocks alternating, with the bytes each
moves per parameter."""
import copy
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS, BLOCKS, WARM = 5, 7, 2


def _stat(t):
    return dict(median=round(statistics.median(t), 3), min=round(min(t), 3), max=round(max(t), 3))


def _emit(rec):
    out = os.environ.get('OUT', os.path.join(ROOT, 'scratch', 'out'))
    os.makedirs(out, exist_ok=True)
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(out, 'ddp_graph_vs_eager.jsonl'), 'a') as f:
        f.write(line + '\n')


def _lift_models(torch, bench, dev, n):
    import argparse
    args = argparse.Namespace(config=None, workload='vocc_c2f_train', dtype='bf16')
    _, syn, head, _ = bench.build_model(args, dev)
    return syn, [bench.LiftTrainer(h, 1, 'bf16').to(dev).train() for h in [head] + [copy.deepcopy(head) for _ in range(n - 1)]]


def steps(backend, workload):
    import numpy as np
    import torch
    import torch.distributed as dist
    import bench
    pkg = importlib.import_module('vln-ver_amd')
    syn, config, graphs, hip, ddp, optim = (importlib.import_module('vln-ver_amd.' + m)
                                            for m in ('synthetic', 'config', 'graphs', 'hipops', 'ddp', 'optim'))
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    if backend == 'nccl':
        dist.init_process_group('nccl', device_id=dev)
    else:
        dist.init_process_group('gloo')
    rank, world = dist.get_rank(), dist.get_world_size()
    wire = torch.bfloat16 if backend == 'nccl' else torch.float32
    w2p_np, org_np = syn.camera_batch(1, seed=1 + rank)
    feats = torch.from_numpy(syn.vit_features(1, seed=100 + rank)).to(dev).permute(1, 0, 2, 3).contiguous()
    w2p, org = torch.from_numpy(w2p_np).to(dev), torch.from_numpy(org_np).to(dev)
    new_opt = lambda params: optim.ClipAdamW(params, lr=1e-4, weight_decay=0.01, max_norm=300.0)
    named = lambda m: [(k, p) for k, p in m.named_parameters() if p.requires_grad]

    def exchanged(model, opt, ex, args, total):
        def run():
            opt.zero_grad(set_to_none=True)
            total(model(*args)).backward()
            ex.pack()
            ex.all_reduce()
            opt.step(exchange=ex)
        return run

    def through_ddp(net, opt, args):
        def run():
            net(*args).backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
        return run

    if workload == 'lift':
        _, models = _lift_models(torch, bench, dev, 3)
        head = models[0].head
        dense = torch.from_numpy(np.random.default_rng(7 + rank).integers(0, 17, size=(1, head.voxel_num))).to(dev)
        args = (feats, w2p, org, dense)
        ex_a, ex_b = (ddp.GradExchange(named(m), wire_dtype=wire) for m in models[:2])
        opts = [new_opt([p for _, p in named(m)]) for m in models]
        step = graphs.GraphedLiftStep(models[0], opts[0], *args, exchange=ex_a)
        graph = lambda: step(*args)
        eager = exchanged(models[1], opts[1], ex_b, args, lambda loss: loss)
        ddp_run = through_ddp(ddp.wrap_ddp(models[2], device=dev, bf16_gradients=backend == 'nccl'), opts[2], args)
        finite = lambda: bool(torch.isfinite(step.loss))
    else:
        torch.manual_seed(2)
        head = pkg.registry.build_head(config.head_cfg(config.load_model_cfg(None), train=True))
        head.init_weights()
        for k, p in head.named_parameters():
            if k.startswith(('layout_branches.', 'query_layout_embedding.')):
                p.requires_grad_(False)
        head = head.to(dev)
        trainer = bench.FullTrainer(head, 'bf16').to(dev).train()
        dense_np = np.random.default_rng(7 + rank).integers(0, 17, size=(1, head.voxel_num))
        dense = torch.from_numpy(dense_np).to(dev)
        g = syn.detection_gt(seed=40 + rank, num_gt=3 + 2 * rank)
        boxes, labels = [torch.from_numpy(g[0][:, :7]).to(dev)], [torch.from_numpy(g[1]).to(dev)]
        trainer(feats, w2p, org, dense, boxes, labels).backward()             # the probing step bench.py freezes by
        for p in head.parameters():
            if p.requires_grad and p.grad is None:
                p.requires_grad_(False)
            p.grad = None
        fused = [copy.deepcopy(head), copy.deepcopy(head)]
        for h in fused:
            h.assigner.solver = 'fused'
        pairs = [np.stack([np.nonzero(row < 16)[0], row[row < 16]], axis=1) for row in dense_np]
        occ = hip.pack_occ_gts(pairs, pinned=False).to(dev)
        padded = fused[0].pad_gts(boxes, labels, capacity=8)
        models = [graphs.MultiTaskStep(h, torch.bfloat16).train() for h in fused]
        args = (feats, w2p, org, padded, occ)
        ex_a, ex_b = (ddp.GradExchange(named(h), wire_dtype=wire) for h in fused)
        opts = [new_opt([p for _, p in named(h)]) for h in fused + [head]]
        step = graphs.GraphedTrainStep(models[0], opts[0], *args, exchange=ex_a)
        graph = lambda: step(*args)
        eager = exchanged(models[1], opts[1], ex_b, args, lambda d: sum(d.values()))
        ddp_run = through_ddp(ddp.wrap_ddp(trainer, device=dev, bf16_gradients=backend == 'nccl'), opts[2],
                              (feats, w2p, org, dense, boxes, labels))
        finite = lambda: bool(torch.isfinite(step.total))
    routes = (('graph', graph), ('eager', eager), ('ddp', ddp_run))
    ms = {name: [] for name, _ in routes}
    for block in range(WARM + BLOCKS):
        for name, run in routes:
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                run()
            torch.cuda.synchronize()
            if block >= WARM:
                ms[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
    if not finite():
        raise SystemExit('non-finite loss after the timed steps')
    launches = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        for name, run in routes:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                run()
                torch.cuda.synchronize()
            launches[name] = sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA') and 'memcpy' not in e.name.lower()
                                 and 'memset' not in e.name.lower()) or None
    except Exception as exc:
        print('profiler unavailable: %r' % (exc,), file=sys.stderr)
    med = {name: statistics.median(t) for name, t in ms.items()}
    if rank == 0:
        _emit(dict(what='steps', workload=workload, backend=backend, world=world, wire=str(wire).split('.')[-1], dtype='bf16',
                   mode='train', viewpoints_per_rank=1, gpu=torch.cuda.get_device_name(0), steps_per_block=STEPS, blocks=BLOCKS,
                   warmup_blocks=WARM, parameters=int(sum(ex_a.sizes)), tensors=len(ex_a.sizes),
                   ms_per_step={name: _stat(t) for name, t in ms.items()}, kernels_per_step=launches,
                   eager_over_graph=round(med['eager'] / med['graph'], 3), ddp_over_graph=round(med['ddp'] / med['graph'], 3)))
    dist.barrier()
    dist.destroy_process_group()


def kernels():
    import torch
    import bench
    importlib.import_module('vln-ver_amd')
    ddp, optim = importlib.import_module('vln-ver_amd.ddp'), importlib.import_module('vln-ver_amd.optim')
    dev = torch.device('cuda', 0)
    _, (model,) = _lift_models(torch, bench, dev, 1)
    sizes = [p.numel() for p in model.parameters() if p.requires_grad]
    del model
    gen = torch.Generator(device=dev).manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(n, device=dev, generator=gen)) for n in sizes]
    for p in ps:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 0.01
    opt = optim.ClipAdamW(ps, lr=1e-6, weight_decay=0.01, max_norm=300.0)
    ex = {w: ddp.GradExchange(ps, wire_dtype=w) for w in (torch.float32, torch.bfloat16)}
    routes = (('grad_pack_f32', ex[torch.float32].pack, 8), ('grad_pack_bf16', ex[torch.bfloat16].pack, 6),
              ('step_flat_f32', lambda: opt.step(exchange=ex[torch.float32]), 32),
              ('step_flat_bf16', lambda: opt.step(exchange=ex[torch.bfloat16]), 28), ('step_tensors', opt.step, 32))
    calls, us = 10, {name: [] for name, _, _ in routes}
    for block in range(WARM + BLOCKS):
        for name, run, _ in routes:
            run()                                           # (the pointer-table upload of a changed route is not timed)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                run()
            e1.record()
            torch.cuda.synchronize()
            if block >= WARM:
                us[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    n = sum(sizes)
    _emit(dict(what='kernels', gpu=torch.cuda.get_device_name(0), parameters=n, tensors=len(sizes), calls_per_block=calls,
               blocks=BLOCKS, us_per_call={name: _stat(t) for name, t in us.items()},
               bytes_per_parameter={name: b for name, _, b in routes},
               gb_per_s={name: round(b * n / statistics.median(us[name]) / 1e3, 1) for name, _, b in routes}))


if __name__ == '__main__':
    if sys.argv[1] == 'kernels':
        kernels()
    else:
        steps(sys.argv[1], sys.argv[2])
