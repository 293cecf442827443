"""The fused detection set loss on the device (``ver_det_costs``, ``ver_det_set_loss_forward`` / ``_backward`` around
``ver_lsa_solve``; ``HungarianAssigner3D(solver='fused')``) against the float64 evaluation of the formulas it restates
(``_assignment_costs``, ``_targets_from_match``, ``_losses_from_targets`` with autograd; tests/test_set_loss_cpu.py), and the
head's three loss entry points against the solver settings they had before."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import cases
from test_set_loss_cpu import (ALPHA, CODE_WEIGHTS, EPS, GAMMA, SHAPES, W_CLS, W_REG, formulas, head_case, make_inputs,
                               model_costs, model_losses)
from util import pkg

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
T = torch.from_numpy
BOUND = 1e-4                   # the project's fp32 contract: |delta| <= 1e-4 max(1, |value|)


def hip():
    return pkg('hipops')


def on_device(x, bf16=False):
    d = {k: v.to(DEV) for k, v in x.items()}
    if bf16:
        d['cls'] = d['cls'].bfloat16()
    return d


def kernel_costs(d, layout=False):
    return hip().det_costs(None if layout else d['cls'], d['box'], (d['gt'], d['labels'], d['counts']), W_CLS, ALPHA, GAMMA, EPS, W_REG)


def kernel_match(d, layout=False, bad=None):
    nl, bs = d['box'].shape[:2]
    return hip().lsa_solve(kernel_costs(d, layout), d['counts'][None].expand(nl, bs), bad=bad)


def normalisers(m, match):
    """``_device_normalisers`` of the positives per layer, as ``_set_loss_fused`` forms them."""
    return m._device_normalisers((match >= 0).sum((1, 2)), match.shape[1] * match.shape[2])


def kernel_losses(m, d, match, bad=None, layout=False):
    """``det_set_loss`` + backward of the sum of all terms -> (loss_cls, loss_bbox, npos, d/d cls, d/d box)."""
    c = None if layout else d['cls'].clone().requires_grad_(True)
    b = d['box'].clone().requires_grad_(True)
    cw = torch.tensor(CODE_WEIGHTS, device=DEV)
    lc, lb, npos = hip().det_set_loss(c, b, match, (d['gt'], d['labels'], d['counts']), cw, normalisers(m, match),
                                      (W_CLS, W_REG), ALPHA, GAMMA, bad=bad)
    (lc.sum() + lb.sum()).backward()
    torch.cuda.synchronize()
    return lc.detach().cpu(), lb.detach().cpu(), npos.cpu(), None if layout else c.grad.cpu(), b.grad.cpu()


def valid_columns(x):
    cap = x['gt'].shape[1]
    return torch.arange(cap)[None, :] < x['counts'][:, None].long()                # [B, Gcap]


def check_costs(got, want, x, what):
    valid = valid_columns(x)[None, :, None, :].expand_as(want)
    err = (got.double() - want).abs() / want.abs().clamp(min=1.0)
    worst = float(err[valid].max()) if bool(valid.any()) else 0.0
    print('%s: worst |delta| / max(1, |cost|) = %.3e, largest |cost| = %.3f' % (what, worst, float(want[valid].abs().max()) if bool(valid.any()) else 0.0))
    assert worst <= BOUND, what
    assert not bool(got[~valid].any()), what + ': padded columns are exactly 0'


def scipy_match(cost, counts):
    nl, bs, nq, _ = cost.shape
    out = np.full((nl, bs, nq), -1, dtype=np.int64)
    for lvl in range(nl):
        for b, n in enumerate(counts):
            if n:
                rows, cols = linear_sum_assignment(cost[lvl, b, :, :n])
                out[lvl, b, rows] = cols
    return out


def assert_close_to_model(got, want, what):
    """Losses within 1e-4 relative, gradients within 1e-4 max|grad| elementwise."""
    lc, lb, npos, gc, gb = got
    wlc, wlb, wnpos, wgc, wgb = want
    assert npos.tolist() == [int(n) for n in wnpos], what
    for name, a, b in (('loss_cls', lc, wlc), ('loss_bbox', lb, wlb)):
        err = (a.double() - b).abs()
        print('%s %s: %s vs %s' % (what, name, a.tolist(), b.tolist()))
        assert bool((err <= BOUND * b.abs()).all()), (what, name)
    for name, a, b in (('grad_cls', gc, wgc), ('grad_box', gb, wgb)):
        if a is None:
            continue
        worst, scale = float((a.double() - b).abs().max()), float(b.abs().max())
        print('%s %s: worst |delta| %.3e, max |grad| %.3e' % (what, name, worst, scale))
        assert worst <= BOUND * scale, (what, name)


# ------------------------------------------------------------------------------------------------------------ 1. costs
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_costs_against_the_float64_model(shape, bf16):
    x = make_inputs(shape, 0)
    d = on_device(x, bf16)
    m = formulas(SHAPES[shape][3])
    want = model_costs(m, d['cls'].float().cpu(), x['box'], x['gt'], x['labels'])   # (bf16: the model reads the rounded logits)
    got = kernel_costs(d)
    assert got.dtype == torch.float32 and got.shape == want.shape
    check_costs(got.cpu(), want, x, 'costs %s' % shape)
    reg = kernel_costs(d, layout=True)
    check_costs(reg.cpu(), model_costs(m, None, x['box'], x['gt'], x['labels']), x, 'layout costs %s' % shape)


def test_costs_of_a_zero_width_ground_truth_and_of_a_label_outside_the_classes():
    """``log 0`` of a zero dimension counts as 0 in the cost, as the ``nan_to_num`` of ``_assignment_costs`` has it; a label
    outside [0, C) in a valid column poisons exactly that column."""
    x = make_inputs('A', 3)
    x['gt'][0, 1, 3] = 0.0                                   # w = 0: log w = -inf
    x['gt'][2, 4, 5] = -1.0                                  # h < 0: log h = NaN
    m = formulas(17)
    d = on_device(x)
    want = model_costs(m, x['cls'], x['box'], x['gt'], x['labels'])
    assert bool(torch.isfinite(want).all())
    check_costs(kernel_costs(d).cpu(), want, x, 'degenerate boxes')
    x['labels'][2, 0], x['labels'][0, 2] = 17, -1
    got = kernel_costs(on_device(x)).cpu()
    poisoned = torch.zeros(3, 5, dtype=torch.bool)
    poisoned[2, 0] = poisoned[0, 2] = True
    by_column = got.permute(0, 2, 1, 3)                                     # [L, Q, B, Gcap]
    assert bool(torch.isnan(by_column[:, :, poisoned]).all()) and bool(torch.isfinite(by_column[:, :, ~poisoned]).all())
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    match = kernel_match(on_device(x), bad=bad).cpu()
    assert int(bad) == 1 and bool((match[:, 0] == -1).all()) and bool((match[:, 2] == -1).all())   # the solver flags them


# ------------------------------------------------------------------------------------------------------------ 2. assignment
@pytest.mark.parametrize('seed', [0, 1])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_assignment_through_the_kernels_costs(shape, seed):
    """Every problem: the float64 total over the kernel path's match exceeds scipy's float64 optimum by at most
    2 min(Q, n) 1e-4 (how far an optimum moves when every entry moves by the cost bound).  On these seeds scipy on the fp32
    torch costs agrees with scipy on the float64 costs for every problem (asserted first), and then the match is scipy's
    float64 match index for index."""
    x = make_inputs(shape, seed)
    nl, bs, nq, ncls, cap, counts = SHAPES[shape]
    m = formulas(ncls)
    c64 = model_costs(m, x['cls'], x['box'], x['gt'], x['labels']).numpy()
    c32 = model_costs(m, x['cls'], x['box'], x['gt'], x['labels'], torch.float32).numpy()
    want = scipy_match(c64, counts)
    assert np.array_equal(scipy_match(c32, counts), want), 'precondition: the optimum is stable between fp32 and fp64'
    got = kernel_match(on_device(x)).cpu().numpy()
    for lvl in range(nl):
        for b, n in enumerate(counts):
            rows = np.nonzero(got[lvl, b] >= 0)[0]
            cols = got[lvl, b, rows]
            assert rows.size == min(nq, n) and np.unique(cols).size == cols.size and (cols.size == 0 or cols.max() < n)
            wrows = np.nonzero(want[lvl, b] >= 0)[0]
            total, best = c64[lvl, b, rows, cols].sum(), c64[lvl, b, wrows, want[lvl, b, wrows]].sum()
            assert total - best <= 2 * min(nq, n) * BOUND, (lvl, b, total, best)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------ 3. loss and gradients
@pytest.mark.parametrize('shape', list(SHAPES))
def test_loss_and_gradients_against_the_float64_model(shape):
    x = make_inputs(shape, 0)
    d = on_device(x)
    m = formulas(SHAPES[shape][3])
    match = kernel_match(d)
    want = model_losses(m, x['cls'], x['box'], match.cpu(), x['gt'], x['labels'])
    got = kernel_losses(m, d, match)
    assert got[2].tolist() == [sum(min(SHAPES[shape][2], n) for n in SHAPES[shape][5])] * SHAPES[shape][0]
    assert_close_to_model(got, want, 'set loss %s' % shape)
    # the layout form: no class term, the same box term
    lay = kernel_losses(m, d, match, layout=True)
    assert not bool(lay[0].any()) and torch.equal(lay[1], got[1]) and torch.equal(lay[4], got[4]) and torch.equal(lay[2], got[2])


@pytest.mark.parametrize('shape', ['A', 'C'])
def test_bf16_logits_against_the_float64_model_of_the_rounded_logits(shape):
    """fp32 arithmetic on bf16 logits: the losses and ``grad_box`` keep the fp32 bounds; ``grad_cls`` is the model's gradient
    rounded to bf16, within one bf16 ulp."""
    x = make_inputs(shape, 1)
    d = on_device(x, bf16=True)
    m = formulas(17)
    match = kernel_match(d)
    rounded = d['cls'].float().cpu()
    want = model_losses(m, rounded, x['box'], match.cpu(), x['gt'], x['labels'])
    got = kernel_losses(m, d, match)
    assert got[3].dtype == torch.bfloat16
    assert_close_to_model(got[:3] + (None, got[4]), want, 'bf16 set loss %s' % shape)
    ref = want[3].float().bfloat16().float()
    ulp = torch.ldexp(torch.ones_like(ref), torch.frexp(ref.abs().clamp(min=1e-30))[1] - 8)      # 2^(e - 7), |ref| in [2^e, 2^(e+1))
    off = (got[3].float() - ref).abs() / ulp
    print('bf16 grad_cls: worst %.2f ulp' % float(off.max()))
    assert float(off.max()) <= 1.0


def test_rows_that_must_not_count_and_a_layer_with_a_nan_logit():
    """Shape A (counts 3, 0, 5) with: a matched ground truth whose normalised target is not finite (neither loss nor
    gradient); a box code equal to its target (gradient 0 there); the empty sample (no box term, background focal terms);
    a NaN logit in layer 1 (that layer's loss_cls is cleaned to 0 and passes no gradient, everything else is unaffected)."""
    x = make_inputs('A', 2)
    x['gt'][0, 1, 4] = 0.0                                   # l = 0: log l = -inf in the target of every row matched to (0, 1)
    m = formulas(17)
    match = kernel_match(on_device(x)).cpu()
    q_dead = [int((match[lvl, 0] == 1).nonzero()[0]) for lvl in range(2)]
    q_exact = int((match[0, 2] == 3).nonzero()[0])
    x['box'][0, 2, q_exact, 0] = x['gt'][2, 3, 0]            # code 0 is the centre's x itself: |box - n| = 0 exactly
    d = on_device(x)
    want = model_losses(m, x['cls'], x['box'], match, x['gt'], x['labels'])
    got = kernel_losses(m, d, match.to(DEV).int())
    assert_close_to_model(got, want, 'special rows')
    assert got[2].tolist() == [8, 8]                         # npos counts the matched rows, kept or not
    for lvl in range(2):
        assert not bool(got[4][lvl, 0, q_dead[lvl]].any()) and bool(want[4][lvl, 0].any())
    assert float(got[4][0, 2, q_exact, 0]) == 0.0 and float(got[4][0, 2, q_exact, 1]) != 0.0
    assert not bool(got[4][:, 1].any())
    # the empty sample alone: L1 sum exactly 0, npos 0, background-only focal terms
    one = {k: (v[:, 1:2] if k in ('cls', 'box') else v[1:2]).contiguous() for k, v in x.items()}
    none = torch.full((2, 1, 100), -1, dtype=torch.int32)
    got1 = kernel_losses(m, on_device(one), none.to(DEV))
    want1 = model_losses(m, one['cls'], one['box'], none, one['gt'], one['labels'])
    assert got1[1].tolist() == [0.0, 0.0] and got1[2].tolist() == [0, 0] and not bool(got1[4].any())
    assert_close_to_model(got1, want1, 'empty sample')
    # a NaN logit in layer 1
    x['cls'][1, 0, 5, 3] = float('nan')
    gotn = kernel_losses(m, on_device(x), match.to(DEV).int())
    assert float(gotn[0][1]) == 0.0 and not bool(gotn[3][1].any())                              # cleaned, and no gradient
    assert torch.equal(gotn[0][0], got[0][0]) and torch.equal(gotn[3][0], got[3][0])            # layer 0 is unaffected
    assert torch.equal(gotn[1], got[1]) and torch.equal(gotn[4], got[4]) and gotn[2].tolist() == [8, 8]   # so are the box terms


# ------------------------------------------------------------------------------------------------------------ 4. flags, reproducibility
def test_two_runs_are_bit_identical():
    x = make_inputs('C', 0)
    d = on_device(x)
    m = formulas(17)
    match = kernel_match(d)
    cw = torch.tensor(CODE_WEIGHTS, device=DEV)
    gts = (d['gt'], d['labels'], d['counts'])
    runs = []
    for _ in range(2):
        sums, npos = hip().det_set_loss_sums(d['cls'], d['box'], match, gts, cw, ALPHA, GAMMA)
        runs.append((sums.cpu(), npos.cpu()) + kernel_losses(m, d, match)[3:])
    assert bool(torch.isfinite(runs[0][0]).all()) and float(runs[0][0].min()) > 0
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_a_bad_match_or_label_is_flagged_and_contained_to_its_layer():
    x = make_inputs('A', 0)
    d = on_device(x)
    m = formulas(17)
    cw = torch.tensor(CODE_WEIGHTS, device=DEV)
    gts = (d['gt'], d['labels'], d['counts'])
    match = kernel_match(d)
    clean_flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    clean, npos = hip().det_set_loss_sums(d['cls'], d['box'], match, gts, cw, ALPHA, GAMMA, bad=clean_flag)
    assert int(clean_flag) == 0 and bool(torch.isfinite(clean).all())
    # a match entry equal to its sample's count (3 of capacity 5): layer 0 is poisoned, layer 1 as before
    broken = match.clone()
    broken[0, 0, 99] = 3
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    sums, _ = hip().det_set_loss_sums(d['cls'], d['box'], broken, gts, cw, ALPHA, GAMMA, bad=bad)
    assert int(bad) == 1 and bool(torch.isnan(sums[:, 0]).all()) and torch.equal(sums[:, 1], clean[:, 1])
    got = kernel_losses(m, d, broken, bad=bad)
    assert got[0][0] == 0 and got[1][0] == 0 and not bool(got[3][0].any()) and not bool(got[4][0].any())   # cleaned, no gradient
    assert float(got[0][1]) > 0 and bool(got[3][1].any()) and bool(got[4][1].any())
    # a matched label equal to C, with its row unmatched in layer 0: layer 1 alone is poisoned
    labels = d['labels'].clone()
    labels[2, 4] = 17
    partly = match.clone()
    partly[0, 2][partly[0, 2] == 4] = -1
    bad2 = torch.zeros(1, dtype=torch.int32, device=DEV)
    sums, npos2 = hip().det_set_loss_sums(d['cls'], d['box'], partly, (d['gt'], labels, d['counts']), cw, ALPHA, GAMMA, bad=bad2)
    assert int(bad2) == 1 and bool(torch.isnan(sums[:, 1]).all()) and bool(torch.isfinite(sums[:, 0]).all())
    assert npos2.tolist() == [7, 8] and npos.tolist() == [8, 8]
    assert int(clean_flag) == 0                              # (the flag is the caller's: nothing else was touched)


# ------------------------------------------------------------------------------------------------------------ 5. head
def _head(solver, layout=False, seed=7):
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    pkg()
    train_cfg = dict(cases.VOCC_TRAIN_CFG, assigner=dict(cases.VOCC_TRAIN_CFG['assigner'], solver=solver))
    extra = dict(add_layout=True, loss_layout=dict(cases.LAYOUT_LOSS_CFG)) if layout else {}
    h = pkg('registry').build_head(dict(cases.vocc_head_cfg(), train_cfg=train_cfg, **extra)).eval()
    code_weights = h.code_weights.detach().clone()
    pkg('synthetic').load_seeded(h, seed)
    h.code_weights.data.copy_(code_weights)                  # (the seeded fill also hits this fixed loss-weight vector)
    return h.to(DEV)


def _gt_lists(counts, seed=40):
    gts = [cases.detection_gt(seed=seed + i, num_gt=max(n, 1)) for i, n in enumerate(counts)]
    return ([T(b[:n, :7]).to(DEV) for (b, _), n in zip(gts, counts)], [T(l[:n]).to(DEV) for (_, l), n in zip(gts, counts)])


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-30))


def _same_dict(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        a, b = float(got[k]), float(want[k])
        print('%s %s: %.9g vs %.9g' % (what, k, a, b))
        assert abs(a - b) <= BOUND * abs(b), (what, k)


def test_head_loss_and_parameter_gradients_equal_the_device_solver():
    """One forward of the multi-task head on two viewpoints with ragged ground truth (4 boxes and none), then ``loss`` with
    ``solver='device'`` and with ``'fused'`` -- the assigner's keyword switched on the same head, so both read the same
    graph: the loss dict within 1e-4 relative and every parameter gradient within 1e-4 relative L2.  The gradient of the
    DIFFERENCE of the two totals is taken by one backward pass and measured against the gradient of the device total: two
    separate passes over the decoder's cross-attention differ by their fp32 atomics alone (tests/test_assign_gpu.py)."""
    syn = pkg('synthetic')
    head = _head('device')
    w2p, org = syn.camera_batch(2, seed=1)
    feats = T(syn.vit_features(2, seed=0)).to(DEV).permute(1, 0, 2, 3).contiguous()
    gb, gl = _gt_lists((4, 0))
    outs = head(feats, None, world2pixel=T(w2p).to(DEV), origin=T(org).to(DEV))
    outs = dict(outs, occupancy_preds=None)                  # (the occupancy term is not what differs)
    named = [(k, p) for k, p in head.named_parameters() if p.requires_grad]
    totals, dicts = [], []
    try:
        for solver, args in (('device', (gb, gl)), ('fused', (gb, gl)), ('fused', (head.pad_gts(gb, gl, capacity=6), None))):
            head.assigner.solver = solver
            dicts.append(head.loss(args[0], args[1], None, outs))
            totals.append(sum(dicts[-1].values()))
    finally:
        head.assigner.solver = 'device'
    for d in dicts[1:]:
        _same_dict(d, dicts[0], 'loss')
    assert all(float(dicts[1][k]) == float(dicts[2][k]) for k in dicts[1])                  # lists or a PaddedGts: the same
    preds = [outs['all_cls_scores'], outs['all_bbox_preds']]
    want = torch.autograd.grad(totals[0], preds + [p for _, p in named], retain_graph=True, allow_unused=True)
    diff = torch.autograd.grad(totals[0] - totals[1], preds + [p for _, p in named], allow_unused=True)
    reached = 0
    for name, w, dlt in zip(['all_cls_scores', 'all_bbox_preds'] + [k for k, _ in named], want, diff):
        if w is None:
            continue
        reached += 1
        assert float(w.norm()) > 0 and float(dlt.double().norm()) <= BOUND * float(w.double().norm()), (name, _rel(w - dlt, w))
    assert reached > 100                                     # (everything under the detection terms)
    hip().AssignmentFlag.of(DEV).poll(sync=True)


@pytest.mark.parametrize('entry', ['only_det', 'add_layout'])
def test_only_det_and_add_layout_equal_the_host_solver(entry):
    """``loss_only_detection`` and ``loss_addlayout`` from stored decoder outputs of two viewpoints (detection and layout
    boxes of all six layers): 'fused' against 'host', the loss dict within 1e-4 relative and the gradients with respect to
    everything the loss reads within 1e-4 relative L2."""
    head = _head('host', layout=True)
    results = []
    try:
        for solver in ('host', 'fused'):
            head.assigner.solver = solver
            preds, boxes, labels, layouts = head_case(DEV)
            leaves = [preds[k].requires_grad_(True) for k in ('all_cls_scores', 'all_bbox_preds', 'all_layout_preds')]
            if entry == 'only_det':
                d = head.loss_only_detection(boxes, labels, preds)
                leaves = leaves[:2]
            else:
                d = head.loss_addlayout(boxes, labels, layouts, None, preds)
            sum(d.values()).backward()
            results.append((d, [t.grad for t in leaves]))
    finally:
        head.assigner.solver = 'host'
    _same_dict(results[1][0], results[0][0], entry)
    assert len(results[0][0]) == (12 if entry == 'only_det' else 15)
    for got, want in zip(results[1][1], results[0][1]):
        assert float(want.norm()) > 0 and _rel(got, want) <= BOUND, (entry, _rel(got, want))
    if entry == 'only_det':                                  # a PaddedGts takes the same path
        head.assigner.solver = 'fused'
        try:
            preds, boxes, labels, _ = head_case(DEV)
            again = head.loss_only_detection(head.pad_gts(boxes, labels, capacity=8), None, preds)
        finally:
            head.assigner.solver = 'host'
        assert all(float(again[k]) == float(results[1][0][k]) for k in again)
    hip().AssignmentFlag.of(DEV).poll(sync=True)


# ------------------------------------------------------------------------------------------------------------ 6. capture
def test_loss_and_backward_are_capturable_with_a_padded_gts():
    """``loss()`` of a 'fused' head plus its backward, captured in ONE ``torch.cuda.graph`` from static prediction and
    ``PaddedGts`` buffers: a capture fails on a host read, a synchronisation or an allocation through the runtime, so its
    success rules those out.  New ground truth (other counts, inside the capacity) is copied into the same three tensors;
    two replays each equal the eager result bit for bit -- with the previous replay's outputs still in the static buffers,
    so a result that leaned on a cleared buffer would show.  A memset NODE would not show here: that the three launchers
    queue nothing but their kernel is asserted on their source in tests/test_set_loss_cpu.py."""
    head = _head('fused')
    preds, _, _, _ = head_case(DEV)
    cap = 12
    first = _gt_lists((5, 3))
    static_gts = head.pad_gts(*first, capacity=cap)
    static = [preds['all_cls_scores'].clone().requires_grad_(True), preds['all_bbox_preds'].clone().requires_grad_(True)]

    def step(c, b, gts):
        d = head.loss(gts, None, None, dict(all_cls_scores=c, all_bbox_preds=b, occupancy_preds=None))
        grads = torch.autograd.grad(sum(d.values()), [c, b])
        return [d[k] for k in sorted(d)] + list(grads)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static[0], static[1], static_gts)               # warm-up outside the capture (library handles, constants)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step(static[0], static[1], static_gts)
    for gts_lists in (first, _gt_lists((12, 0), seed=60), _gt_lists((1, 7), seed=70)):
        fresh = head.pad_gts(*gts_lists, capacity=cap)
        for dst, src in zip(static_gts, fresh):
            dst.copy_(src)
        want = step(static[0].detach().clone().requires_grad_(True), static[1].detach().clone().requires_grad_(True), fresh)
        assert float(want[-1].abs().max()) > 0 or int(fresh.counts.sum()) == 0
        for replay in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for got, ref in zip(static_out, want):
                assert torch.equal(got, ref), replay
    hip().AssignmentFlag.of(DEV).poll(sync=True)
