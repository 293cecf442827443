"""Shared by tests/test_occ_targets_gpu.py, and the measurement behind profiles/occ_targets_chain_vs_device.jsonl:

    python tests/occ_targets_helper.py [--bs 1 8 64 192] [--density 0.05 0.2] [--reps 5] [--out FILE]       # host wall time
    rocprofv3 --kernel-trace --stats --output-format csv -d ROOT/tr_<route>_<bs>_<density>_<reps> -o trace -- \
        python tests/occ_targets_helper.py --trace chain|device --bs 64 --density 0.05 --reps 1|5                 # GPU time
    python tests/occ_targets_helper.py --merge ROOT --out profiles/occ_targets_chain_vs_device.jsonl            # no GPU

At vocc.py's geometry (504 000 voxels per viewpoint, Z = 35, the 120 x 120 plan) and SYNTHETIC densities (uniformly random
distinct voxels, uniformly random classes) it times, from the per-sample numpy arrays to labels + count ready on the device:
  chain   the dense route: ``head.occupancy_targets`` (an int64 volume, one pageable copy and one index_put per sample)
          followed by the clamp / narrow / permute / ``voxels_to_rows`` / byte-sum count of ``_occ_mlp_focal_loss``
  device  ``pack_occ_gts`` -> one copy -> ``occ_targets`` with the plan's row table
Both end in a device synchronisation.  ``--trace`` runs one route ``reps + 1`` times and nothing else, for a kernel trace;
every (route, batch size, density) is traced twice, with ``--reps 1`` and ``--reps 5``, and ``--merge`` takes the DIFFERENCE of
the two ``*kernel_stats.csv`` (kernel time and launches of four calls in the steady state: the process's one-time work --
the plan's table uploads -- cancels) and joins it with ROOT/wall.jsonl (the first command's ``--out``) into the committed file."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

CLASSES, Z, ROWS = 16, 35, 14400
VOXELS = Z * ROWS


def annotation(rng, bs, voxel_num, density, classes=CLASSES, dtype=np.int64):
    """Per sample: [n, 2] (distinct flat voxel index, class) in random order, n = density * voxel_num."""
    n = int(round(density * voxel_num))
    return [np.stack([rng.choice(voxel_num, n, replace=False), rng.integers(0, classes, n)], 1).astype(dtype)
            for _ in range(bs)]


def flat(gts):
    """(pairs [n_total, 2], int32 offsets [bs + 1]) of a list of per-sample arrays."""
    pairs = np.concatenate(gts) if len(gts) else np.zeros((0, 2), np.int64)
    return pairs, np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int32)


def _pkg(sub):
    import importlib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    return importlib.import_module('vln-ver_amd.' + sub)


def chain(Head, stub, gts, plan, bs, dev):
    """The dense route, as the head runs it today."""
    opl = _pkg('dense_heads.occ_proj_lattice')
    gt = Head.occupancy_targets(stub, gts, device=dev)
    gt = gt.clamp(-1, 255).to(torch.uint8)
    gt = gt.reshape(bs, Z, plan.rows).permute(0, 2, 1)
    gt = opl.voxels_to_rows(gt, plan, bs).reshape(-1)
    occupied = gt < CLASSES
    words = occupied.view(torch.uint8).view(torch.int64)
    return gt, ((words * 0x0101010101010101) >> 56).sum() * 1.0


def device(hip, gts, table, dev):
    p = hip.pack_occ_gts(gts).to(dev)
    labels, count, _ = hip.occ_targets(p.pairs, p.offsets, VOXELS, Z, CLASSES, table)
    return labels, count[-1] * 1.0


def _stats(root, route, bs, density, reps):
    """{kernel name: (calls, total ns)} of the kernel_stats.csv under ROOT/tr_<route>_<bs>_<density>_<reps>."""
    import csv
    import glob
    d = os.path.join(root, 'tr_%s_%d_%s_%d' % (route, bs, density, reps))
    files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    assert len(files) == 1, 'one kernel_stats.csv expected under %s, found %d' % (d, len(files))
    return {r['Name']: (int(r['Calls']), float(r['TotalDurationNs'])) for r in csv.DictReader(open(files[0]))}


def merge(root, out, reps=(1, 5)):
    lines = []
    for w in (json.loads(ln) for ln in open(os.path.join(root, 'wall.jsonl'))):
        line = dict(viewpoints=w['bs'], density=w['density'], pairs=w['pairs'], gpu=w['gpu'], voxels_per_viewpoint=VOXELS, zdim=Z,
                    annotation='synthetic: uniformly random distinct voxels and classes, int64 pairs')
        for route in ('chain', 'device'):
            few, many = (_stats(root, route, w['bs'], w['density'], r) for r in reps)
            calls = reps[1] - reps[0]
            per = {k: ((many[k][0] - few.get(k, (0, 0.0))[0]) / calls, (many[k][1] - few.get(k, (0, 0.0))[1]) / calls / 1e3) for k in many}
            top = sorted(((k, n, us) for k, (n, us) in per.items() if n > 0), key=lambda t: -t[2])[:4]
            line[route] = dict(host_wall_ms=w[route + '_wall_ms'],
                               gpu_kernel_us_per_call=round(sum(us for _, us in per.values()), 1),
                               launches_per_call=round(sum(n for n, _ in per.values()), 2),
                               top_kernels=[[k[:60], round(n, 2), round(us, 1)] for k, n, us in top])
        lines.append(line)
        print(json.dumps(line)[:400])
    with open(out, 'w') as f:
        f.write(''.join(json.dumps(ln) + '\n' for ln in lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[1, 8, 64, 192])
    ap.add_argument('--density', type=float, nargs='+', default=[0.05, 0.2])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--trace', choices=['chain', 'device'])
    ap.add_argument('--out')
    ap.add_argument('--merge', metavar='ROOT')
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.out)
    assert torch.cuda.is_available(), 'the measurement needs a GPU'
    dev = torch.device('cuda', 0)
    hip, opl = _pkg('hipops'), _pkg('dense_heads.occ_proj_lattice')
    Head = _pkg('dense_heads.voxelformer_occupancy_head').VoxelFormerOccupancyHead
    stub = types.SimpleNamespace(voxel_num=VOXELS, occupancy_classes=CLASSES, code_weights=torch.zeros(1, device=dev))
    plan = opl.lattice_plan(128, 4, 60, 60, dev)
    table = opl.row_table(plan, dev)
    routes = dict(chain=lambda g, bs: chain(Head, stub, g, plan, bs, dev), device=lambda g, bs: device(hip, g, table, dev))
    lines = []
    for bs in a.bs:
        for density in a.density:
            gts = annotation(np.random.default_rng(bs), bs, VOXELS, density)
            ms = {}
            for name in ([a.trace] if a.trace else ['chain', 'device', 'chain', 'device']):       # alternating
                for rep in range(a.reps + 1):                                                   # the first is the warm-up
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    labels, avg = routes[name](gts, bs)
                    torch.cuda.synchronize()
                    if rep:
                        ms.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
                ms.setdefault(name + '_check', (int(labels.long().sum()), float(avg)))
            if not a.trace:
                assert ms['chain_check'] == ms['device_check'], (ms['chain_check'], ms['device_check'])
            line = dict(bs=bs, density=density, pairs=int(sum(len(g) for g in gts)), gpu=torch.cuda.get_device_name(0),
                        **{name + '_wall_ms': dict(min=round(min(v), 3), median=round(float(np.median(v)), 3), max=round(max(v), 3))
                           for name, v in ms.items() if not name.endswith('_check')})
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(''.join(json.dumps(ln) + '\n' for ln in lines))


if __name__ == '__main__':
    main()
