"""Occupancy evaluation and class maps without logits, the parts that need no GPU: the two prototypes and their argument
checks (``ver_occ_mlp_confusion`` / ``ver_occ_mlp_classes``), the head methods on CPU tensors (where they compose the
existing functions), and the merge rule of csrc/ver_classify.h against the sequential arg-max, compiled for the host."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cases
from util import golden, pkg

T = torch.from_numpy
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'vln-ver_amd', 'csrc')


def test_prototypes_parse_and_resolve():
    hip = pkg('hipops')
    protos = hip.prototypes()
    ptr, i, l, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    assert protos['ver_occ_mlp_confusion'] == (i, [ptr, ptr, ptr, ptr, l, i, ptr, i, ptr, i, i, f, i, ptr])
    assert protos['ver_occ_mlp_classes'] == (i, [ptr, ptr, ptr, ptr, ptr, l, f, i, i, f, i, ptr])
    lib = hip.lib()
    assert lib.ver_occ_mlp_confusion.argtypes == protos['ver_occ_mlp_confusion'][1]
    assert lib.ver_occ_mlp_classes.argtypes == protos['ver_occ_mlp_classes'][1]


def _aligned(nbytes, align=16):
    raw = (ctypes.c_uint8 * (nbytes + align))()
    return raw, (ctypes.addressof(raw) + align - 1) // align * align


def test_argument_validation_without_gpu():
    """Every bad argument comes back as an error code with a message, before anything is launched."""
    lib = pkg('hipops').lib()
    keep_x, x = _aligned(4 * 256)
    keep_img, img = _aligned(256)
    keep_h, hist = _aligned(8 * 8 * 17 * 17, 8)
    vec = (ctypes.c_float * 784)()
    lab = (ctypes.c_uint8 * 64)()
    cls = (ctypes.c_uint8 * 64)()
    thr = (ctypes.c_float * 9)(*([0.25] * 9))

    def conf(x=x, image=img, vectors=vec, labels=lab, rows=4, samples=1, thresholds=thr, T=1, h=hist, width=128,
             classes=16, flags=0):
        return lib.ver_occ_mlp_confusion(x, image, vectors, labels, rows, samples, thresholds, T, h, width, classes, 1e-5,
                                         flags, None)

    def klass(x=x, image=img, vectors=vec, c=cls, prob=None, n=4, width=128, classes=16, flags=0):
        return lib.ver_occ_mlp_classes(x, image, vectors, c, prob, n, 0.25, width, classes, 1e-5, flags, None)

    assert conf(flags=4) == -1 and b'flags' in lib.ver_last_error()
    assert conf(T=0) == -2 and b'thresholds' in lib.ver_last_error()
    assert conf(T=9) == -2 and b'thresholds' in lib.ver_last_error()
    assert conf(h=hist + 4) == -1 and b'8-byte' in lib.ver_last_error()
    assert conf(width=64) == -2 and b'width' in lib.ver_last_error()
    assert conf(classes=8) == -2 and b'classes' in lib.ver_last_error()
    assert conf(rows=-1) == -1 and b'shape' in lib.ver_last_error()
    assert conf(x=x + 8) == -1 and b'16-byte' in lib.ver_last_error()
    assert conf(labels=None) == -1 and b'null' in lib.ver_last_error()
    assert conf(h=None) == -1 and b'null' in lib.ver_last_error()
    assert conf(thresholds=None) == -1 and b'null' in lib.ver_last_error()
    assert conf(samples=70000) == -2 and b'grid' in lib.ver_last_error()
    # an empty batch launches nothing (no device is needed) and succeeds with null pointers
    assert conf(x=None, image=None, vectors=None, labels=None, thresholds=None, h=None, rows=0) == 0
    assert conf(x=None, image=None, vectors=None, labels=None, thresholds=None, h=None, samples=0) == 0
    assert all(v == 0 for v in keep_h)

    assert klass(flags=8) == -1 and b'flags' in lib.ver_last_error()
    assert klass(width=256) == -2 and b'width' in lib.ver_last_error()
    assert klass(n=-1) == -1 and b'negative' in lib.ver_last_error()
    assert klass(c=None) == -1 and b'null' in lib.ver_last_error()
    assert klass(image=img + 2) == -1 and b'16-byte' in lib.ver_last_error()
    assert klass(x=None, image=None, vectors=None, c=None, n=0) == 0
    del keep_x, keep_img


def test_wrappers_refuse_cpu_tensors_and_autograd():
    hip = pkg('hipops')
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        hip.occ_mlp_classes(x, None, None)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        hip.occ_mlp_confusion(x, None, None, torch.zeros(4, dtype=torch.uint8))


@pytest.fixture(scope='module')
def head_and_logits():
    """The seeded vocc head (the one tests/golden/head_vocc.npz was recorded from) on two CPU volumes; the logits once."""
    pkg()
    h = pkg('registry').build_head(cases.vocc_head_cfg()).eval()
    pkg('synthetic').load_seeded(h, 7)
    emb = T(np.random.default_rng(4).standard_normal((2, 900, 768)).astype(np.float32))
    with torch.no_grad():
        logits = h.occupancy_from_volume(emb)
    return h, emb, logits


def test_cpu_confusion_from_volume_composes_the_existing_functions(head_and_logits):
    h, emb, logits = head_and_logits
    gen = torch.Generator().manual_seed(5)
    labels = torch.randint(0, 17, (2, h.voxel_num), generator=gen)
    labels[torch.rand(2, h.voxel_num, generator=gen) < 0.6] = 16
    labels[torch.rand(2, h.voxel_num, generator=gen) < 0.05] = 255
    labels = labels.to(torch.uint8)
    thr = (0.25, 0.5)
    with torch.no_grad():
        got = h.occupancy_confusion_from_volume(emb, labels, thr)
    want = h.occupancy_confusion(logits, labels, thr)
    assert got.shape == (2, 2, 17, 17) and got.dtype == torch.int64 and torch.equal(got, want)
    assert int(got[:, 0].sum()) == int((labels <= 16).sum())
    with torch.no_grad():
        again = h.occupancy_confusion_from_volume(emb, labels, thr, hist=got.clone())
    assert torch.equal(again, 2 * want)
    m = pkg('occupancy_metrics').DeviceSSCMetrics(17, thr)
    with torch.no_grad():
        m.add_volume(h, emb, labels)
    assert torch.equal(m.last, want) and torch.equal(m.hist, want.sum(0))


def test_cpu_class_map_reproduces_the_sparse_prediction(head_and_logits):
    h, emb, logits = head_and_logits
    with torch.no_grad():
        cls = h.occupancy_classes_from_volume(emb, 0.25)
        res = h.get_occupancy_prediction_from_volume(emb, 0.25)
    assert cls.dtype == torch.uint8 and cls.shape == (2, h.voxel_num)
    want = h.get_occupancy_prediction(dict(occupancy_preds=logits), 0.25)['occupancy_preds']
    assert want.shape[0] > 0
    assert res['occupancy_preds'].dtype == torch.int64 and torch.equal(res['occupancy_preds'], want)
    assert torch.equal(h.occupancy_pairs_from_classes(cls), want) and res['flow_preds'] is None
    # the reference's own sparse prediction (tests/golden/post_vocc.npz) through the class map
    g = golden('post_vocc')
    lg, _ = cases.occupancy_loss_inputs(seed=33, n=6000)
    pairs = h.occupancy_pairs_from_classes(h._classes_from_logits(T(lg)[None], 0.25))
    assert np.array_equal(pairs.numpy(), g['sparse'])


_MERGE_MAIN = r'''
#include <cstdio>
#include <cstring>
#include <limits>
#include "ver_classify.h"

static void sequential(const float* p, int lo, int hi, int& best, float& pb) {
    best = lo;
    pb = p[lo];
    for (int j = lo + 1; j < hi; ++j)
        if (ver_class_takes(p[j], pb)) {
            best = j;
            pb = p[j];
        }
}

static bool same(int ba, float pa, int bb, float pb) { return ba == bb && std::memcmp(&pa, &pb, 4) == 0; }

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float vals[6] = {-inf, -1.0f, 0.0f, 1.0f, inf, nan};
    unsigned long long state = 12345;
    long rows = 0, bad = 0;
    for (int it = 0; it < 40000; ++it) {
        float p[16];
        // few distinct values per row: equal maxima and several NaNs are the rule, not the exception
        const int kinds = 1 + it % 6, first_kind = (it / 6) % 6;
        for (int j = 0; j < 16; ++j) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            p[j] = vals[(first_kind + (state >> 33) % kinds) % 6];
        }
        int best;
        float pb;
        sequential(p, 0, 16, best, pb);
        for (int s = 1; s < 16; ++s) {
            int ba, bb, bm;
            float pa, pbb, pm;
            sequential(p, 0, s, ba, pa);
            sequential(p, s, 16, bb, pbb);
            ver_class_merge(ba, pa, bb, pbb, bm, pm);
            if (!same(bm, pm, best, pb)) ++bad;
        }
        // the kernel's tree: four lanes of four classes, merged xor 16 then xor 32
        int b4[4], b2[2], bm;
        float p4[4], p2[2], pm;
        for (int g = 0; g < 4; ++g) sequential(p, 4 * g, 4 * g + 4, b4[g], p4[g]);
        for (int h = 0; h < 2; ++h) ver_class_merge(b4[2 * h], p4[2 * h], b4[2 * h + 1], p4[2 * h + 1], b2[h], p2[h]);
        ver_class_merge(b2[0], p2[0], b2[1], p2[1], bm, pm);
        if (!same(bm, pm, best, pb)) ++bad;
        // NaN is the maximum, the first one wins; otherwise the first of the equal maxima
        int first = 0;
        for (int j = 0; j < 16; ++j)
            if (p[j] != p[j]) { first = j; goto done; }
        for (int j = 1; j < 16; ++j)
            if (p[j] > p[first]) first = j;
    done:
        if (first != best) ++bad;
        if (threshold_class(best, pb, 0.5f, 16) != ((pb == pb && 0.5f > pb) ? 16 : best)) ++bad;
        ++rows;
    }
    std::printf("rows %ld bad %ld\n", rows, bad);
    return bad ? 1 : 0;
}
'''


def test_merge_rule_equals_the_sequential_rule_on_the_host(tmp_path):
    """csrc/ver_classify.h as plain C++: merging the partial arg-maxima of any split of a 16-class row (and the kernel's
    four-lane tree) gives the sequential result bit for bit -- index and probability -- over rows drawn from
    {-inf, -1, 0, 1, +inf, NaN} with many equal values."""
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'),
                            '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx, 'no host C++ compiler'
    src, exe = tmp_path / 'merge_main.cpp', tmp_path / 'merge_main'
    src.write_text(_MERGE_MAIN)
    subprocess.run([cxx, '-O1', '-std=c++17', '-I', CSRC, str(src), '-o', str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split() == ['rows', '40000', 'bad', '0']
