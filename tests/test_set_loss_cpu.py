"""CPU side of the fused detection set loss (``HungarianAssigner3D(solver='fused')``; ``ver_det_costs``,
``ver_det_set_loss_forward`` / ``_backward``): the setting itself, the loss dicts of the three entry points on CPU tensors
against the host solver, the entry points' declaration, export and argument checks.  Also home of the inputs and the float64
model that tests/test_set_loss_gpu.py measures the kernels against."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import cases
from util import ROOT, golden, pkg

T = torch.from_numpy

# (L, B, Q, C, Gcap, counts): the smallest shapes at which each kernel can go wrong
SHAPES = {
    'A': (2, 3, 100, 17, 5, (3, 0, 5)),        # Q and C no multiple of a wave or of 8; one sample is empty
    'B': (1, 2, 7, 17, 12, (12, 1)),           # more boxes than queries
    'C': (6, 2, 100, 17, 65, (65, 33)),        # more than one wave of columns; the reference's layer count
    'D': (1, 1, 1, 1, 1, (1,)),                # the degenerate single problem
}
W_CLS, W_REG, ALPHA, GAMMA, EPS = 2.0, 0.25, 0.25, 2.0, 1e-12      # vocc.py:182-207
CODE_WEIGHTS = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2)   # (the velocity codes carry weight here, so k = 8, 9 count)


def make_inputs(shape, seed):
    """Seeded inputs of one shape: logits 2 N(0,1) - 2, box codes N(0,1), centres uniform in pc_range, dimensions uniform in
    [0.2, 2.0], yaw uniform in (-pi, pi), zero velocity, labels uniform in [0, C); rows past a sample's count are zero padding."""
    nl, bs, nq, ncls, cap, counts = SHAPES[shape]
    rng = np.random.default_rng(seed)
    cls = (2.0 * rng.standard_normal((nl, bs, nq, ncls)) - 2.0).astype(np.float32)
    box = rng.standard_normal((nl, bs, nq, 10)).astype(np.float32)
    lo, hi = np.array(cases.PC_RANGE[:3]), np.array(cases.PC_RANGE[3:])
    gt = np.zeros((bs, cap, 9), dtype=np.float32)
    gt[..., :3] = rng.uniform(lo, hi, (bs, cap, 3))
    gt[..., 3:6] = rng.uniform(0.2, 2.0, (bs, cap, 3))
    gt[..., 6] = rng.uniform(-math.pi, math.pi, (bs, cap))
    labels = rng.integers(0, ncls, (bs, cap)).astype(np.int64)
    for b, n in enumerate(counts):
        gt[b, n:] = 0.0
        labels[b, n:] = 0
    return dict(cls=T(cls), box=T(box), gt=T(gt), labels=T(labels), counts=torch.tensor(counts, dtype=torch.int32))


class _Float64(torch.Tensor):
    """``_assignment_costs`` casts its operands with ``.float()``; the model keeps them float64."""

    def float(self):
        return self


def formulas(ncls):
    """The head's own ``_assignment_costs`` / ``_targets_from_match`` / ``_losses_from_targets`` on a bare object with the
    vocc.py assigner and losses for ``ncls`` classes: the formulas the kernels restate, free of the network around them."""
    head = pkg('dense_heads.voxelformer_occupancy_head').VoxelFormerOccupancyHead
    losses, assigner = pkg('dense_heads.losses'), pkg('dense_heads.assigner')
    names = ('_assignment_costs', '_targets_from_match', '_losses_from_targets', '_device_normalisers')
    m = type('SetLossFormulas', (), {n: getattr(head, n) for n in names})()
    m.assigner = assigner.HungarianAssigner3D(cls_cost=dict(type='FocalLossCost', weight=W_CLS),
                                              reg_cost=dict(type='BBox3DL1Cost', weight=W_REG), pc_range=list(cases.PC_RANGE))
    m.num_classes = m.cls_out_channels = ncls
    m.loss_cls = losses.FocalLoss(gamma=GAMMA, alpha=ALPHA, loss_weight=W_CLS)
    m.loss_bbox = losses.L1Loss(loss_weight=W_REG)
    m.code_weights = torch.tensor(CODE_WEIGHTS)
    m.pc_range, m.bg_cls_weight, m.sync_cls_avg_factor = list(cases.PC_RANGE), 0, False
    return m


def model_costs(m, cls, box, gt, labels, dtype=torch.float64):
    """``_assignment_costs`` in ``dtype`` on copies of the inputs -> [L, B, Q, Gcap] (None logits: the regression term alone)."""
    with torch.no_grad():
        box, gt = box.to(dtype), gt.to(dtype)
        if cls is None:                                       # assign(..., layout=True): the class term is left out
            zero = torch.zeros(box.shape[:3] + (1,), dtype=dtype)
            free = formulas(1)
            free.assigner.cls_cost.weight = 0.0
            return model_costs(free, zero, box, gt, torch.zeros_like(labels), dtype)
        cls = cls.to(dtype)
        if dtype == torch.float64:
            cls, box = cls.as_subclass(_Float64), box.as_subclass(_Float64)
        out = m._assignment_costs(cls, box, gt, labels).as_subclass(torch.Tensor)
        assert out.dtype == dtype
        return out


def model_losses(m, cls, box, match, gt, labels):
    """``_targets_from_match`` + ``_losses_from_targets`` in float64 with autograd, from a match int64 [L, B, Q] ->
    (loss_cls [L], loss_bbox [L], positives per layer, d/d cls, d/d box) of the sum of all terms."""
    c = cls.double().clone().requires_grad_(True)
    b = box.double().clone().requires_grad_(True)
    lab, targets, pos = m._targets_from_match(match.long(), gt.double(), labels)
    npos = pos.reshape(pos.shape[0], -1).sum(1).tolist()
    lc, lb = m._losses_from_targets(c, b, lab, targets, pos, npos)
    lc, lb = torch.stack(lc), torch.stack(lb)
    (lc.sum() + lb.sum()).backward()
    return lc.detach(), lb.detach(), npos, c.grad, b.grad


# ------------------------------------------------------------------------------------------------------------
def test_fused_is_a_solver_setting_and_an_unknown_one_still_raises():
    a = pkg('dense_heads.assigner')
    cfg = dict(cases.VOCC_TRAIN_CFG['assigner'])
    for solver in ('host', 'device', 'fused'):
        assert a.build_assigner(dict(cfg, solver=solver)).solver == solver
    assert a.build_assigner(cfg).solver == 'host'
    for other in ('gpu', 'Fused', None, ''):
        with pytest.raises(ValueError, match="solver must be 'host' or 'device'"):
            a.build_assigner(dict(cfg, solver=other))


@pytest.fixture(scope='module')
def layout_head():
    pkg()
    return pkg('registry').build_head(dict(cases.vocc_head_cfg(), train_cfg=cases.VOCC_TRAIN_CFG, add_layout=True,
                                           loss_layout=dict(cases.LAYOUT_LOSS_CFG))).eval()


def head_case(device='cpu'):
    """Two samples of stored decoder outputs (detection and layout boxes of all six layers), ragged ground truth."""
    gh, gl = golden('head_vocc'), golden('layout_vocc')
    cls = np.concatenate([gh['c3_b0_cls'], gh['c3_b1_cls']], 1)
    box = np.concatenate([gh['c3_b0_bbox'], gh['c3_b1_bbox']], 1)
    lay = np.concatenate([gl['layout_preds'], gl['layout_preds'][:, :, ::-1] * 0.9], 1)
    gts = [cases.detection_gt(seed=40 + i, num_gt=n) for i, n in enumerate((5, 3))]
    boxes = [T(b[:, :7]).to(device) for b, _ in gts]
    labels = [T(l).to(device) for _, l in gts]
    room = cases.layout_gt()
    layouts = [T(room).to(device), T(room * np.float32(1.1)).to(device)]
    preds = dict(all_cls_scores=T(cls.copy()).to(device), all_bbox_preds=T(box.copy()).to(device),
                 all_layout_preds=T(lay.copy()).to(device), occupancy_preds=None)
    return preds, boxes, labels, layouts


def test_fused_on_cpu_tensors_gives_the_host_solvers_loss_dicts(layout_head):
    """``loss``, ``loss_only_detection`` and ``loss_addlayout`` with 'fused' on CPU tensors run the torch formulas of
    'device' (scipy in place of the solver) and agree with the host path within 1e-6; lists and a ``PaddedGts`` alike."""
    h = layout_head
    preds, boxes, labels, layouts = head_case()
    calls = {
        'loss': lambda g=None: h.loss(g or boxes, None if g else labels, None, preds),
        'only_det': lambda g=None: h.loss_only_detection(g or boxes, None if g else labels, preds),
        'add_layout': lambda g=None: h.loss_addlayout(boxes, labels, layouts, None, preds),
    }
    try:
        for name, call in calls.items():
            h.assigner.solver = 'host'
            want = call()
            h.assigner.solver = 'fused'
            padded = h.pad_gts(boxes, labels, capacity=9)
            for got in (call(), call(padded)):
                assert sorted(got) == sorted(want), name
                for k in want:
                    assert float(got[k]) == pytest.approx(float(want[k]), rel=1e-6, abs=1e-6), (name, k)
            assert float(want['loss_cls']) > 0 and float(want['loss_bbox']) > 0 and len(want) >= 12
            if name == 'add_layout':
                assert float(want['loss_layout']) > 0
        h.assigner.solver = 'host'
        with pytest.raises(ValueError, match='PaddedGts'):
            h.loss_only_detection(padded, None, preds)
    finally:
        h.assigner.solver = 'host'


def test_entry_points_are_declared_exported_and_the_abi_number_stays():
    text = open(os.path.join(ROOT, 'include', 'ver_ops.h')).read()
    shared = (r'const void\* cls, int cls_dtype, const float\* box, int box_ld, ')
    assert re.search(r'int ver_det_costs\(' + shared + r'const float\* gt,\s*const int64_t\* gt_labels, const int32_t\* counts, '
                     r'float\* cost, int L, int B, int Q, int C, int Gcap,\s*float w_cls, float alpha, float gamma, float eps, '
                     r'float w_reg, void\* stream\);', text)
    tail = (r'const int32_t\* match,\s*const float\* gt, const int64_t\* gt_labels, const int32_t\* counts,\s*'
            r'const float\* code_weights, ')
    assert re.search(r'int ver_det_set_loss_forward\(' + shared + tail + r'float\* sums, int32_t\* npos, int32_t\* bad, int L, '
                     r'int B, int Q,\s*int C, int Gcap, float alpha, float gamma, void\* stream\);', text)
    assert re.search(r'int ver_det_set_loss_backward\(' + shared + tail + r'const float\* scale, void\* grad_cls, '
                     r'float\* grad_box, int L,\s*int B, int Q, int C, int Gcap, float alpha, float gamma, void\* stream\);', text)
    assert '#define VER_ABI_VERSION 31' in text
    for phrase in ('WRITTEN IN FULL', 'WRITTEN, not accumulated', 'bit-reproducible', 'never cleared here'):
        assert phrase in text, phrase
    hip = pkg('hipops')
    pkg('csrc.build').build_hip(verbose=False)
    handle = ctypes.CDLL(hip.LIB_PATH)
    for name in ('ver_det_costs', 'ver_det_set_loss_forward', 'ver_det_set_loss_backward'):
        assert hasattr(handle, name), name
    assert handle.ver_abi_version() == 31 == hip.ABI_VERSION
    ptr, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert hip.PROTOTYPES['ver_det_costs'] == (i, [ptr, i, ptr, i] + [ptr] * 4 + [i] * 5 + [f] * 5 + [ptr])
    assert hip.PROTOTYPES['ver_det_set_loss_forward'] == (i, [ptr, i, ptr, i] + [ptr] * 8 + [i] * 5 + [f] * 2 + [ptr])
    assert hip.PROTOTYPES['ver_det_set_loss_backward'] == (i, [ptr, i, ptr, i] + [ptr] * 8 + [i] * 5 + [f] * 2 + [ptr])
    assert 'ver_setloss.hip' in pkg('csrc.build').SOURCES
    # the launchers queue kernels and nothing else: no runtime call in the file that would add a memset node, copy or allocate
    # (a proxy on the source; what a capture can show is in tests/test_set_loss_gpu.py)
    src = open(os.path.join(ROOT, 'vln-ver_amd', 'csrc', 'ver_setloss.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    assert 'hipLaunchKernelGGL' in code
    for call in ('hipMemset', 'hipMalloc', 'hipMemcpy', 'ver_zero_async', 'hipStreamSynchronize', 'hipDeviceSynchronize', '<<<'):
        assert call not in code, call


def test_argument_validation_without_gpu():
    """Sizes outside the supported range and missing pointers come back as the documented codes, with a message, before
    anything touches a device; empty problems are no error."""
    hip = pkg('hipops')
    lib = hip.lib()
    buf = (ctypes.c_float * 64)()

    def costs(ptrs=None, dtype=0, ld=10, dims=(6, 2, 100, 17, 20)):
        a = [buf] * 6 if ptrs is None else ptrs                 # cls, box, gt, gt_labels, counts, cost
        return lib.ver_det_costs(a[0], dtype, a[1], ld, a[2], a[3], a[4], a[5], *dims, W_CLS, ALPHA, GAMMA, EPS, W_REG, None)

    def forward(ptrs=None, dtype=0, ld=10, dims=(6, 2, 100, 17, 20)):
        a = [buf] * 10 if ptrs is None else ptrs                # cls, box, match, gt, gt_labels, counts, code_weights, sums, npos, bad
        return lib.ver_det_set_loss_forward(a[0], dtype, a[1], ld, *a[2:10], *dims, ALPHA, GAMMA, None)

    def backward(ptrs=None, dtype=0, ld=10, dims=(6, 2, 100, 17, 20)):
        a = [buf] * 10 if ptrs is None else ptrs                # ..., code_weights, scale, grad_cls, grad_box
        return lib.ver_det_set_loss_backward(a[0], dtype, a[1], ld, *a[2:10], *dims, ALPHA, GAMMA, None)

    for fn, name in ((costs, b'ver_det_costs'), (forward, b'ver_det_set_loss_forward'), (backward, b'ver_det_set_loss_backward')):
        for dims in ((6, 2, 1025, 17, 20), (6, 2, 100, 65, 20), (6, 2, 100, 17, 1025)):      # Q, C, Gcap beyond the build
            assert fn(dims=dims) == -2 and name in lib.ver_last_error() and b'at most' in lib.ver_last_error(), (name, dims)
        for hole in range(5):
            dims = [6, 2, 100, 17, 20]
            dims[hole] = -1
            assert fn(dims=tuple(dims)) == -1 and b'bad sizes' in lib.ver_last_error(), (name, hole)
        assert fn(dtype=2) == -1 and b'cls_dtype' in lib.ver_last_error()
    assert costs(ld=7) == -1 and b'box_ld' in lib.ver_last_error()
    assert costs(ld=8, dims=(0, 2, 100, 17, 20)) == 0                                         # nothing to do
    for ld in (8, 9):
        assert forward(ld=ld) == -1 and b'box_ld' in lib.ver_last_error(), ld
        assert backward(ld=ld) == -1 and b'box_ld' in lib.ver_last_error(), ld
    for empty in ((0, 2, 100, 17, 20), (6, 0, 100, 17, 20), (6, 2, 0, 17, 20), (6, 2, 100, 17, 0)):
        assert costs([None] * 6, dims=empty) == 0, empty                                      # an empty dimension launches nothing
    assert forward([None] * 10, dims=(0, 2, 100, 17, 20)) == 0
    assert backward([None] * 10, dims=(0, 2, 100, 17, 20)) == 0 and backward([None] * 10, dims=(6, 0, 100, 17, 20)) == 0
    for hole in (1, 2, 4, 5):                                                                 # box, gt, counts, cost
        a = [buf] * 6
        a[hole] = None
        assert costs(a) == -1 and b'null' in lib.ver_last_error(), hole
    assert costs([buf, buf, buf, None, buf, buf]) == -1 and b'null' in lib.ver_last_error()   # logits without labels
    for hole in (1, 2, 3, 4, 5, 6, 7, 8):                                                     # (bad may be NULL)
        a = [buf] * 10
        a[hole] = None
        assert forward(a) == -1 and b'null' in lib.ver_last_error(), hole
    for hole in (1, 2, 3, 4, 5, 6, 7, 8, 9):
        a = [buf] * 10
        a[hole] = None
        assert backward(a) == -1 and b'null' in lib.ver_last_error(), hole
    assert (hip.LSA_MAX, hip.SET_LOSS_MAX_CLASSES) == (1024, 64)
    gts = (torch.zeros(1, 3, 9), torch.zeros(1, 3, dtype=torch.long), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='GPU'):                                            # no torch fallback inside hipops
        hip.det_costs(torch.zeros(1, 1, 2, 17), torch.zeros(1, 1, 2, 10), gts)
    with pytest.raises(RuntimeError, match='GPU'):
        hip.det_set_loss(torch.zeros(1, 1, 2, 17), torch.zeros(1, 1, 2, 10), torch.zeros(1, 1, 2, dtype=torch.int32), gts,
                         torch.ones(10), torch.ones(2, 1))


def test_float64_model_is_the_existing_formulas():
    """The yardstick itself: float64 ``_assignment_costs`` equals the assigner's per-problem costs in float64, stays within
    the 5.1e-5 the fp32 chain was measured at, and the layout form is the regression term alone."""
    m = formulas(17)
    x = make_inputs('A', 0)
    want = model_costs(m, x['cls'], x['box'], x['gt'], x['labels'])
    assert want.dtype == torch.float64 and want.shape == (2, 3, 100, 5)
    a = m.assigner
    norm = pkg('dense_heads.coders').normalize_bbox
    for lvl, b in ((0, 0), (1, 2)):
        n = x['counts'][b]
        one = a.cls_cost(x['cls'][lvl, b].double(), x['labels'][b, :n]) + a.reg_cost(x['box'][lvl, b, :, :8].double(),
                                                                                    norm(x['gt'][b, :n].double())[:, :8])
        assert float((one - want[lvl, b, :, :n]).abs().max()) < 1e-12
    f32 = model_costs(m, x['cls'], x['box'], x['gt'], x['labels'], torch.float32)
    valid = torch.arange(5)[None, :] < x['counts'][:, None]
    err = (f32.double() - want).abs() / want.abs().clamp(min=1.0)
    assert float(err[valid[None, :, None, :].expand_as(err)].max()) < 1e-4
    reg = model_costs(m, None, x['box'], x['gt'], x['labels'])
    alone = (x['box'][0, 0, :, None, :8].double() - norm(x['gt'][0, :3].double())[None, :, :8]).abs().sum(-1) * W_REG
    assert float((reg[0, 0, :, :3] - alone).abs().max()) < 1e-12
