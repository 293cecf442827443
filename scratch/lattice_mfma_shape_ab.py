"""Wall-time A/B of builds of libver_hip.so on the IMPLICIT-operand products of lattice layer 3 at 192 viewpoints (planar z-split
lattice 30 x 30, C = 768, N = 1 536; M = 345 600 rows; the four parity classes added up), on N(0,1), constant and zero operands -- the companion of
scratch/gemm_mfma_shape_ab.py for the families that read the lattice themselves:

    python scratch/lattice_mfma_shape_ab.py parent=PARENT.so new=NEW.so [other=OTHER.so ...] [--reps 5] [--out FILE.jsonl]

All libraries are loaded into ONE process (the parent a second time from a copy, as its own control) and timed in turn, `reps`
times over.  Never under a profiler.  Families: gemm_nn_segments (forward), gemm_nn_planes (d(input): one product over the four
class planes of the output gradient, K = 38 400), wgrad_tn_segments (weight gradient).  Before the timing every arm's forward and
d(input) products on N(0,1) are compared with the parent's by torch.equal (a 'bit_identity' line per arm)."""
import argparse
import importlib
import json
import os
import shutil
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
hip = importlib.import_module('vln-ver_amd.hipops')
ups = importlib.import_module('vln-ver_amd.dense_heads.upsample')
lattice_plan = importlib.import_module('vln-ver_amd.dense_heads.lattice_plan')


def load(path):
    hip._lib, hip.LIB_PATH = None, os.path.abspath(path)
    return hip.lib()


def timed(f, n=5):
    f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('arms', nargs='+', help='name=path; the first is the parent')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--families', default='gemm_nn_segments,gemm_nn_planes,wgrad_tn_segments')
    ap.add_argument('--viewpoints', type=int, default=192)
    args = ap.parse_args()
    arms = [a.split('=', 1) for a in args.arms]
    tmp = tempfile.mkdtemp()
    arms.append(['parent_copy', shutil.copy(arms[0][1], os.path.join(tmp, 'libver_hip_parent_copy.so'))])
    handles = [(name, load(path)) for name, path in arms]
    out = open(args.out, 'a') if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    B, DEV, C, N, layout, hc = args.viewpoints, 'cuda', 768, 1536, 3, 30
    plan = ups._layer_plan_z4(C, torch.device(DEV))[0]
    m = B * 2 * hc * hc
    table, _ = ups._const_rows_z4(C, hc, hc, torch.device(DEV), torch.bfloat16)
    cls = [(ups._class_segments_z4(c, C), plan[c][1] - plan[c][0]) for c in ups._CLASSES]
    # d(input) of the same layer (upsample._dgrad_implicit): ONE product over the four class planes of the output gradient,
    # z-split [4, B, 2, hc, hc, 2, Co], 50 taps of Co = 768 channels (K = 38 400) -> [M, 2 Ci = 1 536]
    _, dtaps, dplanes, nb = lattice_plan._dgrad_plan('lat', C, torch.device(DEV))
    kd = nb * 2 * C
    makes = (('N(0,1)', lambda *s: torch.randn(*s, device=DEV).bfloat16()),
             ('constant 0.5', lambda *s: torch.full(s, 0.5, device=DEV, dtype=torch.bfloat16)),
             ('zeros', lambda *s: torch.zeros(*s, device=DEV, dtype=torch.bfloat16)))
    for dist, make in makes:
        e = make(4, B, 2, hc // 2, hc // 2, 2, C)
        g = make(m, N)
        ws = [make(k, N) for _, k in cls]
        dws = [torch.empty(k, N, dtype=torch.bfloat16, device=DEV) for _, k in cls]
        y = torch.empty(m, N, dtype=torch.bfloat16, device=DEV)
        gp = make(4, B, 2, hc, hc, 2, C)
        wd = make(kd, 2 * C)
        de = torch.empty(m, 2 * C, dtype=torch.bfloat16, device=DEV)
        kf = sum(k for _, k in cls)

        def forward():
            for (segs, _), w in zip(cls, ws):
                hip.gemm_nn_taps(e, layout, (hc, hc), segs, w, const_rows=table, out=y)

        def wgrad():
            for (segs, _), dw in zip(cls, dws):
                hip.wgrad_tn_segments(e, layout, (hc, hc), segs, g, out=dw, const_rows=table)

        def planes():
            hip.gemm_nn_taps(gp, 2, (hc, hc), dtaps, wd, planes=dplanes, out=de)

        # bit-identity first: every arm's products against the parent's (same K order, fragments and MFMA order)
        if dist == 'N(0,1)':
            want = {}
            for name, h in handles:
                hip._lib = h
                res = [hip.gemm_nn_taps(e, layout, (hc, hc), segs, w, const_rows=table) for (segs, _), w in zip(cls, ws)]
                planes()
                res.append(de.clone())
                torch.cuda.synchronize()
                if not want:
                    want = res
                else:
                    emit(dict(kind='bit_identity', arm=name, against=arms[0][0], operands=dist,
                              gemm_nn_segments=all(torch.equal(a, b) for a, b in zip(res[:-1], want[:-1])),
                              gemm_nn_planes=bool(torch.equal(res[-1], want[-1]))))
                del res
            del want
            torch.cuda.empty_cache()

        fams = (('gemm_nn_segments', forward, kf, 2.0 * m * N * kf), ('gemm_nn_planes', planes, kd, 2.0 * m * kd * 2 * C),
                ('wgrad_tn_segments', wgrad, kf, 2.0 * m * N * kf))
        for fam, f, kk, flops in fams:
            if fam not in args.families.split(','):
                continue
            samples = {name: [] for name, _ in handles}
            for _ in range(args.reps):
                for name, h in handles:
                    hip._lib = h
                    samples[name].append(timed(f))
            med = {k: statistics.median(v) for k, v in samples.items()}
            spread = abs(med[arms[0][0]] - med['parent_copy'])
            for name, _ in handles:
                emit(dict(kind='microbench', family=fam, operands=dist, arm=name, M=m, K=kk, N=N,
                          ms=[round(x, 4) for x in samples[name]], ms_median=round(med[name], 4), tflops=round(flops / med[name] / 1e9, 1)))
            for name, _ in handles[1:-1]:
                gain = med[arms[0][0]] - med[name]
                emit(dict(kind='verdict', family=fam, operands=dist, arm=name, parent_ms=round(med[arms[0][0]], 4), new_ms=round(med[name], 4),
                          parent_aa_spread_ms=round(spread, 4), gain_ms=round(gain, 4), speedup=round(med[arms[0][0]] / med[name], 4),
                          clears_twice_the_spread=bool(gain > 2 * spread)))
        del e, g, ws, dws, y, gp, wd, de
        torch.cuda.empty_cache()
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
