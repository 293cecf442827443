"""A few launches of the implicit-operand GEMMs of lattice layer 3 (the shapes of scratch/lattice_mfma_shape_ab.py) for a
counter pass under rocprofv3, which serialises the kernels and is never timed:

    VER_HIP_LIB=LIB.so rocprofv3 --kernel-trace --pmc <counters> -d DIR -o pmc -- python scratch/lattice_gemm_launch.py [viewpoints] [calls]
    python scratch/lattice_gemm_launch.py report DIR/pmc_results.db ARM      # one JSON line: counters per dispatch and kernel

The forward (ver_gemm_nn_segments, the four parity classes, planar z-split lattice -> k_gemm_nn<3>) and d(input)
(ver_gemm_nn_planes over the four class planes of the output gradient, z-split -> k_gemm_nn<2>) on N(0,1) operands."""
import collections
import importlib
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def report(path, arm):
    cur = sqlite3.connect(path).cursor()
    rows = cur.execute("select kernel_name, counter_name, sum(value), count(distinct dispatch_id) from counters_collection "
                       "group by kernel_name, counter_name").fetchall()
    out = collections.defaultdict(dict)
    for k, c, v, n in rows:
        if 'k_gemm_nn' in k:
            name = k.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
            out[name][c] = round(v / n, 1)
            out[name]['dispatches'] = n
    for d in out.values():
        if 'GRBM_GUI_ACTIVE' in d and 'SQ_VALU_MFMA_BUSY_CYCLES' in d:
            # GRBM_GUI_ACTIVE is summed over the 8 XCDs; 1 024 SIMDs (scratch/r05/mfma_summary.py)
            d['mfma_util'] = round(d['SQ_VALU_MFMA_BUSY_CYCLES'] / (d['GRBM_GUI_ACTIVE'] / 8.0 * 1024.0), 4)
    print(json.dumps(dict(kind='counters', arm=arm, per_dispatch=out)))


def main():
    import torch
    hip = importlib.import_module('vln-ver_amd.hipops')
    ups = importlib.import_module('vln-ver_amd.dense_heads.upsample')
    lattice_plan = importlib.import_module('vln-ver_amd.dense_heads.lattice_plan')
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 192
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    dev, C, N, hc = torch.device('cuda'), 768, 1536, 30
    torch.manual_seed(0)
    plan = ups._layer_plan_z4(C, dev)[0]
    table, _ = ups._const_rows_z4(C, hc, hc, dev, torch.bfloat16)
    cls = [(ups._class_segments_z4(c, C), plan[c][1] - plan[c][0]) for c in ups._CLASSES]
    _, dtaps, dplanes, nb = lattice_plan._dgrad_plan('lat', C, dev)
    e = torch.randn(4, B, 2, hc // 2, hc // 2, 2, C, device=dev).bfloat16()
    ws = [torch.randn(k, N, device=dev).bfloat16() for _, k in cls]
    gp = torch.randn(4, B, 2, hc, hc, 2, C, device=dev).bfloat16()
    wd = torch.randn(nb * 2 * C, 2 * C, device=dev).bfloat16()
    m = B * 2 * hc * hc
    y = torch.empty(m, N, dtype=torch.bfloat16, device=dev)
    for _ in range(calls):
        for (segs, _), w in zip(cls, ws):
            hip.gemm_nn_taps(e, 3, (hc, hc), segs, w, const_rows=table, out=y)
        hip.gemm_nn_taps(gp, 2, (hc, hc), dtaps, wd, planes=dplanes, out=y)
    torch.cuda.synchronize()


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'report':
        report(sys.argv[2], sys.argv[3])
    else:
        main()
