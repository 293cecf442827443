"""Wall-time A/B of two builds of libver_hip.so on the layer-3 product of the 192-viewpoint step (the shapes and method of
profiles/r05_power_wall.txt: M = 345 600, K = 14 304, N = 1 536, bf16, fp32 accumulation), for the MFMA-shape decision of
DESIGN 3.3:

    python scratch/gemm_mfma_shape_ab.py PARENT.so NEW.so [--reps 5] [--out FILE.jsonl] [--families gemm_nn,wgrad_tn]

Both libraries are loaded into ONE process (the parent a second time from a copy, as its own control) and timed in turn --
parent, new, parent copy, `reps` times over -- on N(0,1), constant and zero operands.  Never under a profiler.  One JSON
line per (family, operands, arm): every sample, the median, TFLOP/s; and per (family, operands) the verdict of the decision
rule: the new median beats the parent's by more than twice the spread between the parent and its copy."""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile

import torch

M, K, N = 345600, 14304, 1536
c_long, c_int, c_void = ctypes.c_long, ctypes.c_int, ctypes.c_void_p


def load(path):
    L = ctypes.CDLL(path)
    L.ver_gemm_nn.argtypes = [c_void, c_long, c_void, c_long, c_void, c_void, c_long, c_long, c_int, c_int, c_int, c_void]
    L.ver_wgrad_tn.argtypes = [c_void, c_long, c_void, c_long, c_long, c_int, c_int, c_void, c_long, c_int, c_int, c_int, c_void,
                               c_long, c_void]
    L.ver_wgrad_tn_splits_ld.argtypes = [c_long, c_int, c_int, c_long]
    L.ver_wgrad_tn_workspace.argtypes = [c_long, c_int, c_int, c_int]
    L.ver_wgrad_tn_workspace.restype = c_long
    return L


def timed(f, n=6):
    for _ in range(2):
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
    ap.add_argument('parent')
    ap.add_argument('new')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--families', default='gemm_nn,wgrad_tn')
    args = ap.parse_args()
    tmp = tempfile.mkdtemp()
    copy = shutil.copy(args.parent, os.path.join(tmp, 'libver_hip_parent_copy.so'))
    arms = [('parent', load(args.parent)), ('new', load(args.new)), ('parent_copy', load(copy))]
    dev = 'cuda'
    st = torch.cuda.current_stream().cuda_stream
    out = open(args.out, 'a') if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    def check(rc, what):
        if rc != 0:
            sys.exit('%s returned %d' % (what, rc))

    makes = (('N(0,1)', lambda *s: torch.randn(*s, device=dev).bfloat16()),
             ('constant 0.5', lambda *s: torch.full(s, 0.5, device=dev, dtype=torch.bfloat16)),
             ('zeros', lambda *s: torch.zeros(*s, device=dev, dtype=torch.bfloat16)))
    fl = 2.0 * M * K * N
    for dist, make in makes:
        a, g, w = make(M, K), make(M, N), make(K, N)
        c = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        dw = torch.empty(K, N, dtype=torch.bfloat16, device=dev)
        for fam in args.families.split(','):
            samples = {name: [] for name, _ in arms}
            for _ in range(args.reps):
                for name, L in arms:
                    if fam == 'gemm_nn':
                        f = lambda: check(L.ver_gemm_nn(a.data_ptr(), K, w.data_ptr(), N, None, c.data_ptr(), N, M, K, N, 0, st), fam)
                    else:
                        s = L.ver_wgrad_tn_splits_ld(M, K, N, K)
                        nb = L.ver_wgrad_tn_workspace(M, K, N, s)
                        ws = torch.empty(nb // 4, dtype=torch.float32, device=dev)
                        f = lambda: check(L.ver_wgrad_tn(a.data_ptr(), K, g.data_ptr(), N, M, K, N, dw.data_ptr(), N, 1, s, 0,
                                                         ws.data_ptr(), nb, st), fam)
                    samples[name].append(timed(f))
            med = {k: statistics.median(v) for k, v in samples.items()}
            for name, _ in arms:
                emit(dict(kind='microbench', family=fam, operands=dist, arm=name, M=M, K=K, N=N, ms=[round(x, 4) for x in samples[name]],
                          ms_median=round(med[name], 4), tflops=round(fl / med[name] / 1e9, 1)))
            spread = abs(med['parent'] - med['parent_copy'])
            gain = med['parent'] - med['new']
            emit(dict(kind='verdict', family=fam, operands=dist, parent_ms=round(med['parent'], 4), new_ms=round(med['new'], 4),
                      parent_aa_spread_ms=round(spread, 4), gain_ms=round(gain, 4), speedup=round(med['parent'] / med['new'], 4),
                      clears_twice_the_spread=bool(gain > 2 * spread)))
        del a, g, w, c, dw
        torch.cuda.empty_cache()
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
