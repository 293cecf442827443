"""Host-fed against index-fed captured steps, and the fetch call alone.

    timeout -k 10 900 python scratch/resident_bench.py [--out profiles/resident_vs_host_fed.jsonl] [--iters 30] [--warmup 5]

The method of scratch/infer_bench.py: one MI355X, vocc.py's seeded head under bf16 autocast, the variants ALTERNATING call by
call in one process, wall clock from the call to its results on the host, ``--warmup`` rounds dropped, median (min - max) of
``--iters`` rounds.  Per batch size (1 and 8 viewpoints):
  infer / host_fed    features out of a warm ``volume_io.FeatureStore`` (every key cached: no file I/O), stacked, copied;
                      ``GraphedInference`` replay; ``results()``                       -- the parent commit's route, unchanged
  infer / index_fed   ``step.fetch(store, idx)`` out of a ``resident.ResidentStore``; the same replay; ``results()``
  train / host_fed    the same features, ``head.pad_gts``, ``hipops.pack_occ_gts(...).to(device)``, ``GraphedTrainStep`` replay,
                      ``float(step.total)``                                             -- the parent commit's route, unchanged
  train / index_fed   ``step.fetch(store, idx)``; the same replay on the static buffers; ``float(step.total)``
Then the fetch alone at 192 viewpoints (HIP events, 20 calls after 3): all four groups out of a 256-viewpoint store, f32 and
bf16, next to a device-to-device ``copy_`` of the same feature bytes, each as GB/s moved (read + written) and as a fraction
of the 8 TB/s peak.  Not measured here: more than one rank, a real split's pair density, a real run's DataLoader."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)
BATCHES = (1, 8)
CAP, PAIR_CAP_PER_VIEWPOINT = 8, 40000
PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    import torch
    from test_train_graph_gpu import _boxes, _build, _freeze_unused, _optimizer
    pkg = lambda sub: importlib.import_module('vln-ver_amd.' + sub)
    graphs, hip, res, syn = pkg('graphs'), pkg('hipops'), pkg('resident'), pkg('synthetic')
    dev = torch.device('cuda', 0)
    T = torch.from_numpy
    nmax = max(BATCHES)
    names = ['scanA_vp%d' % i for i in range(nmax)]
    w2p, org = syn.camera_batch(nmax, seed=1)
    feats = syn.vit_features(nmax, seed=0)
    rng = np.random.default_rng(3)
    counts, npairs = [2 + i % 5 for i in range(nmax)], [20000 + 2500 * i for i in range(nmax)]
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, name in enumerate(names):
            for deg in range(6):                                   # the reference's files: [1, 197, 768] with the CLS token
                np.save(os.path.join(tmp, '%s_i1_%d.npy' % (name, deg)),
                        np.concatenate([np.zeros((1, 1, 768), np.float32), feats[i, deg][None]], axis=1))
        fstore = pkg('volume_io').FeatureStore(tmp)
        head = _build()
        ann = []
        for i in range(nmax):
            b, l = _boxes(50 + i, counts[i])
            p = np.stack([rng.choice(head.voxel_num, size=npairs[i], replace=False), rng.integers(0, 16, npairs[i])], axis=1).astype(np.int64)
            ann.append((b, l, p))
        store = res.ResidentStore(device=dev, viewpoints=nmax)
        for i, name in enumerate(names):
            store.append(name, fstore.viewpoint(name), w2p[i], org[i], *ann[i])
        store.freeze()
        model = graphs.MultiTaskStep(head, torch.bfloat16).eval()
        frozen = False
        for bs in BATCHES:
            idx = list(range(bs))
            cams = (T(w2p[:bs]).to(dev), T(org[:bs]).to(dev))
            host_feats = lambda: T(np.stack([fstore.viewpoint(n)[:, 0] for n in names[:bs]], axis=1)).to(dev, non_blocking=True)
            host_gts = lambda: (head.pad_gts([T(ann[i][0]).to(dev) for i in idx], [T(ann[i][1]).to(dev) for i in idx], capacity=CAP),
                                hip.pack_occ_gts([ann[i][2] for i in idx]).to(dev))
            head.eval()
            infer = graphs.GraphedInference(head, host_feats(), *cams, pair_capacity=bs * head.voxel_num)

            def infer_host_fed():
                infer(host_feats(), *cams)
                return infer.results()

            def infer_index_fed():
                infer.fetch(store, idx)
                infer(*infer.inputs)
                return infer.results()

            if not frozen:
                _freeze_unused([head], model, (host_feats(),) + cams + host_gts())
                frozen = True
            opt, _ = _optimizer(head, lr=1e-6, eps=0.1)
            train = graphs.GraphedTrainStep(model, opt, host_feats(), *cams, *host_gts(), pair_capacity=bs * PAIR_CAP_PER_VIEWPOINT, warmup=1)

            def train_host_fed():
                train(host_feats(), *cams, *host_gts())
                return float(train.total)

            def train_index_fed():
                train.fetch(store, idx)
                train(*train.inputs, train.gts, train.occ)
                return float(train.total)

            variants = dict(infer_host_fed=infer_host_fed, infer_index_fed=infer_index_fed, train_host_fed=train_host_fed,
                            train_index_fed=train_index_fed)
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
            line = dict(what='step', viewpoints=bs, gpu=torch.cuda.get_device_name(0), autocast='bf16', iters=a.iters, warmup=a.warmup,
                        wall_ms={k: s(v) for k, v in ms.items()})
            print(json.dumps(line), flush=True)
            lines.append(line)
            infer = train = opt = None
    # ---- the fetch alone at 192 viewpoints -----------------------------------------------------------------------------
    V, bs, ncam, row = 256, 192, 6, 196 * 768
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(0))[:bs].to(torch.int32).to(dev)
    for dtype in (torch.float32, torch.bfloat16):
        one = res.ResidentStore(device=dev, feat_dtype=dtype, viewpoints=1)
        one.append('seed_vp', feats[0], w2p[0], org[0], *ann[0])
        one.freeze()
        # V viewpoints without V appends: random features, the one appended viewpoint's small tables repeated on the device
        n = one.pairs.shape[0]
        big = res.ResidentStore.from_tables(
            ['v%d' % i for i in range(V)], torch.randn(V, ncam, row, device=dev).to(dtype), one.world2pixel.repeat(V, 1, 1, 1),
            one.origin.repeat(V, 1), one.boxes.repeat(V, 1, 1), one.labels.repeat(V, 1), one.counts.repeat(V), one.pairs.repeat(V, 1),
            torch.arange(V + 1, device=dev, dtype=torch.int64) * n, feat_tail=one.feat_tail)
        batch = big.new_batch(bs, CAP, bs * n)
        plain = torch.empty_like(batch.feats)
        src = torch.randn(ncam, bs, row, device=dev).to(dtype).view_as(plain)

        def events(fn, calls=20, warm=3):
            out = []
            for it in range(warm + calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= warm:
                    out.append(e0.elapsed_time(e1))
            return out

        t_fetch = events(lambda: big.fetch(perm, out=batch))
        feats_only = batch._replace(world2pixel=None, origin=None, gts=None, occ=None)
        t_feats = events(lambda: big.fetch(perm, out=feats_only))
        t_copy = events(lambda: plain.copy_(src))
        assert big.check(batch.status) == (0, 0, 0, bs * n) and torch.equal(batch.feats[:, 5], big.feats[int(perm[5])].view_as(batch.feats[:, 5]))
        moved = 2 * batch.feats.numel() * batch.feats.element_size()
        rate = lambda v: dict(ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4),
                              gb_per_s=round(moved / (statistics.median(v) * 1e-3) / 1e9, 1),
                              of_peak=round(moved / (statistics.median(v) * 1e-3) / PEAK, 3))
        line = dict(what='fetch_alone', viewpoints=bs, store_viewpoints=V, feat_dtype=str(dtype), feature_bytes_each_way=moved // 2,
                    pairs=bs * n, fetch_all_groups=rate(t_fetch), fetch_features_only=rate(t_feats), copy_same_bytes=rate(t_copy),
                    store_gb=round(big.nbytes / 1e9, 3))
        print(json.dumps(line), flush=True)
        lines.append(line)
        big = batch = plain = src = None
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(''.join(json.dumps(ln) + '\n' for ln in lines))


if __name__ == '__main__':
    main()
