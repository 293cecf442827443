"""Helper of tests/test_ddp_graph_gpu.py: the captured training steps under data parallelism, on two gloo ranks that share
the one GPU (``ddp.GradExchange``; no DistributedDataParallel wrapper anywhere).

    torchrun --nproc-per-node 2 ddp_graph_helper.py lift <out>    bench.py's LiftTrainer, fp32, dropout p = 0, ONE viewpoint per
                                                                   rank (different data per rank), fp32 wire: three steps through
                                                                   graphs.GraphedLiftStep(exchange=) and the same three steps
                                                                   of an identical model as eager exchanged steps; then one more
                                                                   backward of the eager model packed onto a bf16 wire.  Every
                                                                   rank saves <out>.<rank>
    python ddp_graph_helper.py lift_single <out>                   one process, no process group: the gradients of both ranks'
                                                                   data, their mean as .grad, one ClipAdamW step
    torchrun --nproc-per-node 2 ddp_graph_helper.py multi <out>   the vocc head of tests/test_train_graph_gpu.py at one viewpoint
                                                                   per rank, different box counts per rank (a step without boxes
                                                                   on rank 0): three steps through graphs.GraphedTrainStep(
                                                                   exchange=) against the eager exchanged twin, whose loss
                                                                   normalisers are all-reduced inside head.loss

The package is imported (bench.py / util.pkg) before the first GPU call of the process: importing it sets what hipGraph replay
needs in the environment."""
import argparse
import hashlib
import importlib
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
importlib.import_module('vln-ver_amd')

LR, MAX_NORM = 1e-4, 1e-3      # tests/ddp_grad_helper.py's update: bench.py's optimizer, the clip well under the gradient norm
SAMPLE = 70000                 # leading elements of every gradient kept for the bf16-wire comparison (two chunks and a tail)
DEV = torch.device('cuda', 0)


def _lift_model():
    args = argparse.Namespace(config=None, workload='vocc_c2f_train', dtype='fp32')
    pkg, syn, head, _ = bench.build_model(args, DEV)           # torch.manual_seed(2) + init_weights: same weights everywhere
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return syn, head, bench.LiftTrainer(head, 1, 'fp32').to(DEV).train()


def _lift_data(syn, head, data_rank):
    w2p_np, org_np = syn.camera_batch(1, seed=1 + data_rank)
    feats = torch.from_numpy(syn.vit_features(1, seed=100 + data_rank)).to(DEV).permute(1, 0, 2, 3).contiguous()
    gt = torch.from_numpy(np.random.default_rng(7 + data_rank).integers(0, 17, size=(1, head.voxel_num))).to(DEV)
    return feats, torch.from_numpy(w2p_np).to(DEV), torch.from_numpy(org_np).to(DEV), gt


def _named(model):
    return [(k, p) for k, p in model.named_parameters() if p.requires_grad]


def _optimizer(model):
    return importlib.import_module('vln-ver_amd.optim').ClipAdamW([p for _, p in _named(model)], lr=LR, weight_decay=0.01,
                                                                  max_norm=MAX_NORM)


def _record(model):
    torch.cuda.synchronize()
    rec = dict(digest={}, sample={})
    for k, p in _named(model):
        host = p.detach().cpu().contiguous()
        rec['digest'][k] = hashlib.sha256(host.numpy().tobytes()).hexdigest()
        rec['sample'][k] = host.reshape(-1)[::97].clone()
    return rec


def _norm(tensors):
    return float(torch.sqrt(sum(t.double().pow(2).sum() for t in tensors)))


def _updates(model, twin, before):
    """Relative L2 difference of every parameter's update between ``model`` and ``twin`` -> {name: figure}."""
    out = {}
    for (k, p), (_, q) in zip(_named(twin), _named(model)):
        d_e, d_g = (p.detach() - before[k]).double(), (q.detach() - before[k]).double()
        n = float(d_e.norm())
        out[k] = float((d_e - d_g).norm()) / n if n else (0.0 if float(d_g.norm()) == 0 else float('inf'))
    return out


def lift(out):
    graphs, ddp = importlib.import_module('vln-ver_amd.graphs'), importlib.import_module('vln-ver_amd.ddp')
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    torch.cuda.set_device(0)
    dist.init_process_group('gloo')
    rank = dist.get_rank()
    syn, head, model = _lift_model()
    _, twin_head, twin = _lift_model()
    batch = _lift_data(syn, head, rank)
    before = {k: p.detach().clone() for k, p in _named(model)}
    rec = dict(rank=rank, world=dist.get_world_size(), tensors=len(before))
    # ---- the eager exchanged twin: three steps, records after the first
    opt = _optimizer(twin)
    ex = ddp.GradExchange(_named(twin), wire_dtype=torch.float32)
    ex.broadcast_parameters()
    eager = dict(loss=[], clip_norm=[], held_norm=[])
    for it in range(3):
        opt.zero_grad(set_to_none=True)
        loss = twin(*batch)
        loss.backward()
        own = _norm([p.grad for _, p in _named(twin)])
        ex.pack()
        ex.all_reduce()
        norm = opt.step(exchange=ex)
        eager['loss'].append(float(loss))
        eager['clip_norm'].append(float(norm))
        eager['held_norm'].append(_norm(ex.grads()))
        if it == 0:
            rec['first'] = dict(_record(twin), clip_norm=float(norm), own_grad_norm=own)
    loss = None
    rec['eager'] = dict(eager, **_record(twin))
    # ---- the same three steps through the captured step: 1 eager exchanged warm-up step + 2 replays
    opt_g = _optimizer(model)
    ex_g = ddp.GradExchange(_named(model), wire_dtype=torch.float32)
    step = graphs.GraphedLiftStep(model, opt_g, *batch, warmup=1, exchange=ex_g)
    graph = dict(loss=[], clip_norm=[], held_norm=[])
    for it in range(2):
        graph['loss'].append(float(step(*batch)))
        graph['clip_norm'].append(float(step.grad_norm))
        graph['held_norm'].append(_norm(ex_g.grads()))
    rec['graph'] = dict(graph, **_record(model))
    rec['graph']['steps'] = sorted({opt_g.state[p]['step'] for _, p in _named(model)})
    rec['updates'] = _updates(model, twin, before)
    # ---- one more backward of the eager model, packed onto a bf16 wire and exchanged
    opt.zero_grad(set_to_none=True)
    twin(*batch).backward()
    wire = ddp.GradExchange(_named(twin), wire_dtype=torch.bfloat16)
    wire.pack()
    wire.all_reduce()
    torch.cuda.synchronize()
    rec['bf16'] = dict(
        own={k: p.grad.detach().reshape(-1)[:SAMPLE].cpu().clone() for k, p in _named(twin)},
        held={k: wire.flat[o:o + min(n, SAMPLE)].cpu().clone() for (k, _), o, n in zip(_named(twin), wire.offsets, wire.sizes)})
    torch.save(rec, '%s.%d' % (out, rank))
    dist.barrier()
    dist.destroy_process_group()


def lift_single(out):
    torch.cuda.set_device(0)
    syn, head, model = _lift_model()
    grads = []
    for data_rank in (0, 1):
        model.zero_grad(set_to_none=True)
        model(*_lift_data(syn, head, data_rank)).backward()
        grads.append([p.grad.detach().clone() for _, p in _named(model)])
    for (_, p), a, b in zip(_named(model), *grads):
        p.grad = 0.5 * a + 0.5 * b
    mean_norm = _norm([p.grad for _, p in _named(model)])
    norm = _optimizer(model).step()
    torch.save(dict(_record(model), clip_norm=float(norm), grad_norm=mean_norm), out)


COUNTS = (4, 0, 6, 3, 5, 2)                            # boxes of (rank 0: steps 0-2 | rank 1: steps 0-2)
PAIRS = (30000, 12000, 40000, 500, 22000, 8000)


def multi(out):
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))          # (cases.py, as tests/conftest.py arranges for the suite)
    import grad_exchange_cases as gx
    import test_train_graph_gpu as tg
    graphs, ddp = importlib.import_module('vln-ver_amd.graphs'), importlib.import_module('vln-ver_amd.ddp')
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    torch.cuda.set_device(0)
    dist.init_process_group('gloo')
    rank = dist.get_rank()
    torch.manual_seed(2)
    heads = [tg._build(init=True), tg._build(init=True)]
    heads[1].load_state_dict(heads[0].state_dict())
    models = [graphs.MultiTaskStep(h, None).eval() for h in heads]              # fp32, no dropout
    view = tg._viewpoints()[rank]
    gt = [tg._ground_truth(heads[0], 3 * rank + s, counts=COUNTS, pairs=PAIRS) for s in range(3)]
    tg._freeze_unused(heads, models[0], view + gt[0])
    before = {k: p.detach().clone() for k, p in gx.trainable(heads[0])}
    rec = dict(rank=rank, tensors=len(before), counts=[int(g[0].counts.sum()) for g in gt])
    # ---- the eager exchanged twin: its normalisers are all-reduced inside head.loss
    opt, _ = tg._optimizer(heads[0], lr=tg.LR, eps=tg.EPS)
    ex = ddp.GradExchange(gx.trainable(heads[0]), wire_dtype=torch.float32)
    ex.broadcast_parameters()
    rec['eager'] = gx.eager_steps(models[0], opt, ex, [view + g for g in gt], lambda d: sum(d.values()))
    # ---- the captured step: 1 eager exchanged warm-up step + 2 replays with the preset normalisers
    opt_g, params = tg._optimizer(heads[1], lr=tg.LR, eps=tg.EPS)
    ex_g = ddp.GradExchange(gx.trainable(heads[1]), wire_dtype=torch.float32)
    step = graphs.GraphedTrainStep(models[1], opt_g, *view, *gt[0], pair_capacity=tg.PAIR_CAP, warmup=1, exchange=ex_g)
    rec['graph'], rec['clip_norm'] = [], []
    for s in (1, 2):
        rec['graph'].append(tg._floats(step(*view, *gt[s])))
        rec['clip_norm'].append(float(step.grad_norm))
    rec['steps'] = sorted({opt_g.state[p]['step'] for p in params})
    rec['flags'] = step.flags()
    rec['updates'] = _updates(heads[1], heads[0], before)
    rec.update(_record(heads[1]))
    torch.save(rec, '%s.%d' % (out, rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    dict(lift=lift, lift_single=lift_single, multi=multi)[sys.argv[1]](sys.argv[2])
