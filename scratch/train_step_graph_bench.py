"""The full multi-task training step three ways: eager, ``GraphedHead`` + eager loss / optimizer, and
``GraphedTrainStep``.

    python scratch/train_step_graph_bench.py                       one JSON line per batch into $OUT/train_step_graph.jsonl
    timeout -k 10 420 python scratch/train_step_graph_bench.py one 8     one batch size, in this process

What is measured: ms per training step of vocc.py's head at V = 1 and 8 viewpoints per step, bf16 autocast, train mode
(dropout on), ``ClipAdamW`` (lr 1e-4, weight decay 0.01, max_norm 300), bench.py's init, inputs and ground truth
(``synthetic``; 3 .. 7 boxes per viewpoint, 17 random labels per voxel), on one GPU, three routes ALTERNATING block by block in
ONE process:

  (a) eager     bench.py's ``FullTrainer`` step: Hungarian targets solved on the host under the occupancy head;
  (b) two_graphs  bench.py's ``graph_step``: ``GraphedHead`` replays forward and backward, the host solver, the loss terms, the
                clip and AdamW run eagerly in between -- the best route before ``GraphedTrainStep``;
  (c) one_graph   ``GraphedTrainStep``: one replay; ``solver='fused'``, occupancy targets from the sparse pairs of the same
                labels (``ver_occ_targets`` inside the graph), fresh ground truth copied in on every step.

(a) and (b) train one head with one optimizer, (c) a copy of it with its own.  A block is 5 steps of one route between two
device synchronisations, timed on the host clock; 2 warm-up blocks and 7 measured blocks per route; median / min / max of the
per-step time over the blocks.  ``launches``: GPU kernels of one step of route (c), counted by the profiler around one replay
(null where the profiler is not available).

Without arguments every batch size runs as a child process of its own under ``timeout`` and the first failure ends the run;
the parent never opens the GPU.  There is no CPU fall-back: without a device the child fails.
"""
import copy
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VIEWPOINTS = (1, 8)
STEPS, BLOCKS, WARM = 5, 7, 2
LIMIT_S = 420


def one(v):
    import numpy as np
    import torch
    import bench
    pkg = importlib.import_module('vln-ver_amd')
    syn, config, graphs, hip = (importlib.import_module('vln-ver_amd.' + m) for m in ('synthetic', 'config', 'graphs', 'hipops'))
    dev = torch.device('cuda', 0)
    torch.manual_seed(2)
    head = pkg.registry.build_head(config.head_cfg(config.load_model_cfg(None), train=True))
    head.init_weights()
    for k, p in head.named_parameters():
        if k.startswith(('layout_branches.', 'query_layout_embedding.')):
            p.requires_grad_(False)
    head = head.to(dev)
    trainer = bench.FullTrainer(head, 'bf16').to(dev).train()
    w2p_np, org_np = syn.camera_batch(v, seed=1)
    feats = torch.from_numpy(syn.vit_features(v, seed=100)).to(dev).permute(1, 0, 2, 3).contiguous()
    w2p, org = torch.from_numpy(w2p_np).to(dev), torch.from_numpy(org_np).to(dev)
    dense_np = np.random.default_rng(7).integers(0, 17, size=(v, head.voxel_num))
    dense = torch.from_numpy(dense_np).to(dev)
    gts = [syn.detection_gt(seed=40 + i, num_gt=3 + i % 5) for i in range(v)]
    boxes = [torch.from_numpy(g[0][:, :7]).to(dev) for g in gts]
    labels = [torch.from_numpy(g[1]).to(dev) for g in gts]
    # one probing step: what ends it without a gradient is not part of the workload (bench.py freezes it the same way)
    trainer(feats, w2p, org, dense, boxes, labels).backward()
    for p in head.parameters():
        if p.requires_grad and p.grad is None:
            p.requires_grad_(False)
        p.grad = None
    fused = copy.deepcopy(head)
    fused.assigner.solver = 'fused'
    params = [p for p in head.parameters() if p.requires_grad]
    opt, update = bench.make_optimizer(params)

    def eager():
        loss = trainer(feats, w2p, org, dense, boxes, labels)
        loss.backward()
        update()

    graphed = graphs.GraphedHead(head, feats, w2p, org, autocast_dtype=torch.bfloat16)

    def two_graphs():
        loss = sum(head.loss(boxes, labels, dense, graphed(feats, w2p, org)).values())
        loss.backward()
        update()

    # route (c): the same labels as sparse (voxel, class) pairs, the same boxes padded to a capacity of 8
    pairs = [np.stack([np.nonzero(row < 16)[0], row[row < 16]], axis=1) for row in dense_np]
    occ = hip.pack_occ_gts(pairs, pinned=False).to(dev)
    padded = fused.pad_gts(boxes, labels, capacity=8)
    model = graphs.MultiTaskStep(fused, torch.bfloat16).train()
    opt_c, _ = bench.make_optimizer([p for p in fused.parameters() if p.requires_grad])
    step = graphs.GraphedTrainStep(model, opt_c, feats, w2p, org, padded, occ)

    def one_graph():
        step(feats, w2p, org, padded, occ)                      # (copies all five inputs into the static buffers)

    routes = (('eager', eager), ('two_graphs', two_graphs), ('one_graph', one_graph))
    ms = {name: [] for name, _ in routes}
    for block in range(WARM + BLOCKS):
        for name, run in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                run()
            torch.cuda.synchronize()
            if block >= WARM:
                ms[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
    if not all(bool(torch.isfinite(p).all()) for p in params) or not bool(torch.isfinite(step.total)):
        raise SystemExit('non-finite parameters or loss after the timed steps')
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            one_graph()
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA') and 'memcpy' not in e.name.lower()
                       and 'memset' not in e.name.lower()) or None
    except Exception as exc:                                    # the record says so; the timings stand
        print('profiler unavailable: %r' % (exc,), file=sys.stderr)
    stat = lambda t: dict(median=round(statistics.median(t), 3), min=round(min(t), 3), max=round(max(t), 3))
    med = {name: statistics.median(t) for name, t in ms.items()}
    return dict(viewpoints=v, dtype='bf16', mode='train', gpu=torch.cuda.get_device_name(0), steps_per_block=STEPS, blocks=BLOCKS,
                warmup_blocks=WARM, pairs=int(occ.n_total), boxes=[int(b.shape[0]) for b in boxes],
                ms_per_step={name: stat(t) for name, t in ms.items()}, launches_one_graph=launches,
                two_graphs_over_one_graph=round(med['two_graphs'] / med['one_graph'], 3),
                eager_over_one_graph=round(med['eager'] / med['one_graph'], 3), flags=step.flags())


def main():
    out = os.environ.get('OUT', os.path.join(ROOT, 'scratch', 'out'))
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, 'train_step_graph.jsonl')
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
