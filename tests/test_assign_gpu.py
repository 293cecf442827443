"""Hungarian target assignment on the device (ABI 31, ``ver_lsa_solve``): the solver against scipy, and the head's
``solver='device'`` path -- padded ground truth, targets, normalisers and losses without a host round trip -- against the
host path it replaces."""
import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import cases
from util import golden, pkg

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
T = torch.from_numpy

DEVICE_TRAIN_CFG = dict(cases.VOCC_TRAIN_CFG, assigner=dict(cases.VOCC_TRAIN_CFG['assigner'], solver='device'))


def _random_costs(rng, p, r, ccap):
    """A normal plus a uniform term per entry, fp32: continuous, so an optimum is unique."""
    return (rng.standard_normal((p, r, ccap)) + rng.uniform(0.0, 10.0, (p, r, ccap))).astype(np.float32)


def _scipy_match(cost, ncols):
    want = np.full(cost.shape[:2], -1, dtype=np.int32)
    for p in range(cost.shape[0]):
        if ncols[p]:
            rows, cols = linear_sum_assignment(cost[p, :, :ncols[p]])
            want[p, rows] = cols
    return want


def _total(cost, match):
    rows = np.nonzero(match >= 0)[0]
    return float(cost[rows, match[rows]].astype(np.float64).sum())


def _solve(cost, ncols, bad=None):
    hip = pkg('hipops')
    got = hip.lsa_solve(T(cost).to(DEV), T(np.asarray(ncols, dtype=np.int32)).to(DEV), bad=bad)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize('p,r,ccap,seed', [(6 * 192, 100, 40, 11), (6 * 192, 100, 129, 12), (1200, 1, 1, 13), (3, 1024, 1024, 14)],
                         ids=['100x40', '100x129', '1x1', '1024x1024'])
def test_solver_equals_scipy_exactly(p, r, ccap, seed):
    """Random fp32 costs, ``ncols`` drawn from 0..Ccap (Ccap below and above R; R = ncols = 1; the largest supported shape
    with full, nearly full and half-filled columns): every row's column is scipy's, for every problem."""
    rng = np.random.default_rng(seed)
    cost = _random_costs(rng, p, r, ccap)
    ncols = rng.integers(0, ccap + 1, p).astype(np.int32)
    if ccap == 1:
        ncols[:] = 1
    elif r == 1024:
        ncols[:] = (1024, 1000, 517)
    else:
        ncols[:3] = (0, ccap, min(r, ccap))
    got = _solve(cost, ncols)
    want = _scipy_match(cost, ncols)
    wrong = np.nonzero((got != want).any(1))[0]
    for q in wrong[:10]:          # equal totals would mean a tie in the input: then another seed, never a tolerance
        print('problem %d (ncols %d): total %.17g, scipy %.17g' % (q, ncols[q], _total(cost[q], got[q]), _total(cost[q], want[q])))
    assert wrong.size == 0, '%d of %d problems differ from scipy' % (wrong.size, p)


def test_ties_give_a_valid_assignment_of_scipys_total():
    """Integer costs in 0..3: the optimum is far from unique and the indices may differ from scipy's; the assignment is
    valid (distinct columns below ncols, min(R, ncols) rows matched) and its total, exact in fp64, EQUALS scipy's."""
    rng = np.random.default_rng(21)
    p, r, ccap = 600, 100, 129
    cost = rng.integers(0, 4, (p, r, ccap)).astype(np.float32)
    ncols = rng.integers(0, ccap + 1, p).astype(np.int32)
    got = _solve(cost, ncols)
    want = _scipy_match(cost, ncols)
    for q in range(p):
        cols = got[q][got[q] >= 0]
        assert cols.size == min(r, ncols[q]) and np.unique(cols).size == cols.size, q
        assert cols.size == 0 or cols.max() < ncols[q], q
        assert _total(cost[q], got[q]) == _total(cost[q], want[q]), q


def test_bad_input_is_flagged_and_contained():
    """A NaN (or a -inf, or no finite assignment) inside the valid columns of one problem: ``bad`` is set, that problem's rows
    are -1, the other problems are solved as before; a NaN in a padded column changes nothing."""
    rng = np.random.default_rng(31)
    p, r, ccap = 64, 100, 24
    cost = _random_costs(rng, p, r, ccap)
    ncols = rng.integers(1, ccap, p).astype(np.int32)           # (at least one padded column everywhere)
    want = _scipy_match(cost, ncols)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    padded = cost.copy()
    for q in range(p):
        padded[q, :, ncols[q]:] = np.nan
    assert np.array_equal(_solve(padded, ncols, bad), want) and int(bad) == 0
    broken = cost.copy()
    broken[5, 17, ncols[5] - 1] = np.nan
    broken[9, 3, 0] = -np.inf
    broken[13, :, 0] = np.inf                  # fewer columns than rows: every column has to be taken, nobody can take this one
    broken[20, 7, 0] = np.inf                  # (one forbidden pair: legal)
    for q in (5, 9, 13):
        with pytest.raises(ValueError):
            linear_sum_assignment(broken[q, :, :ncols[q]])
    got = _solve(broken, ncols, bad)
    assert int(bad) == 1
    want[20] = _scipy_match(broken[20:21], ncols[20:21])[0]
    for q in range(p):
        if q in (5, 9, 13):
            assert (got[q] == -1).all(), q
        else:
            assert np.array_equal(got[q], want[q]), q
    clean = torch.zeros(1, dtype=torch.int32, device=DEV)        # the flag is sticky, never cleared by the kernel
    _solve(cost, ncols, bad)
    _solve(cost, ncols, clean)
    assert int(bad) == 1 and int(clean) == 0


def _heads(seed=7):
    """The vocc head twice on the GPU, same seeded weights: host solver (the default) and ``solver='device'``."""
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    pkg()
    out = []
    for train_cfg in (cases.VOCC_TRAIN_CFG, DEVICE_TRAIN_CFG):
        h = pkg('registry').build_head(dict(cases.vocc_head_cfg(), train_cfg=train_cfg)).eval()
        code_weights = h.code_weights.detach().clone()
        pkg('synthetic').load_seeded(h, seed)
        h.code_weights.data.copy_(code_weights)      # (the seeded fill also hits this fixed, non-trainable loss-weight vector)
        out.append(h.to(DEV))
    assert out[0].assigner.solver == 'host' and out[1].assigner.solver == 'device'
    return out


def _golden_predictions(repeat=1):
    gh = golden('head_vocc')
    cls = np.concatenate([gh['c3_b0_cls'], gh['c3_b1_cls']] * repeat, 1)
    box = np.concatenate([gh['c3_b0_bbox'], gh['c3_b1_bbox']] * repeat, 1)
    if repeat > 1:                                              # (repeated samples: not the same rows twice)
        cls[:, 2:] = cls[:, 2:, ::-1]
        box[:, 2:] = box[:, 2:, ::-1]
    return T(cls.copy()).to(DEV), T(box.copy()).to(DEV)


def _gt_lists(counts, seed=40):
    gts = [cases.detection_gt(seed=seed + i, num_gt=max(n, 1)) for i, n in enumerate(counts)]
    return ([T(b[:n, :7]).to(DEV) for (b, _), n in zip(gts, counts)], [T(l[:n]).to(DEV) for (_, l), n in zip(gts, counts)])


@pytest.mark.parametrize('counts', [(3, 4), (5, 0, 17, 1)], ids=['golden_pair', 'ragged_with_empty'])
def test_device_targets_and_losses_equal_the_host_path(counts):
    """``_targets_device`` against ``_batched_targets`` on the two golden viewpoints' predictions (and on a batch whose
    samples hold 5, 0, 17 and 1 boxes): labels, bbox_targets, pos_mask, num_pos equal; the loss dict equal entry by entry
    as floats; the gradients w.r.t. the predictions equal."""
    host, dev = _heads()
    all_cls, all_box = _golden_predictions(len(counts) // 2)
    gb, gl = _gt_lists(counts)
    padded, labels = host._prepare_gts(gb, gl, DEV)
    want = host._batched_targets(all_cls, all_box, padded, labels)
    gts = dev.pad_gts(gb, gl)
    assert gts.boxes.shape == (len(counts), max(counts), 9) and gts.counts.tolist() == list(counts)
    got = dev._targets_device(all_cls, all_box, gts)
    for a, b, name in zip(got[:3], want[:3], ('labels', 'bbox_targets', 'pos_mask')):
        assert torch.equal(a, b), name
    assert torch.is_tensor(got[3]) and got[3].is_cuda and got[3].tolist() == list(want[3])
    # more capacity than boxes: the same targets
    roomy = dev._targets_device(all_cls, all_box, dev.pad_gts(gb, gl, capacity=max(counts) + 7))
    assert torch.equal(roomy[0], want[0]) and torch.equal(roomy[2], want[2])
    assert torch.equal(roomy[1], want[1])
    grads = []
    dicts = []
    for h, args in ((host, (gb, gl)), (dev, (gts, None)), (dev, (gb, gl))):
        c, b = all_cls.clone().requires_grad_(True), all_box.clone().requires_grad_(True)
        d = h.loss(args[0], args[1], None, dict(all_cls_scores=c, all_bbox_preds=b, occupancy_preds=None))
        sum(d.values()).backward()
        grads.append((c.grad, b.grad))
        dicts.append(d)
    for d, g in zip(dicts[1:], grads[1:]):
        assert sorted(d) == sorted(dicts[0])
        for k in d:
            assert float(d[k]) == float(dicts[0][k]), k
        assert torch.equal(g[0], grads[0][0]) and torch.equal(g[1], grads[0][1])
    pkg('hipops').AssignmentFlag.of(DEV).poll(sync=True)


def test_full_head_losses_and_parameter_gradients_equal_the_host_solver():
    """The two golden viewpoints end to end: ONE forward of the multi-task head, then ``loss`` with the host solver and with
    ``solver='device'`` (the assigner's keyword switched on the same head, so both read the same graph).  No tolerance
    anywhere:
    * the loss dict is equal entry by entry as floats;
    * the gradients of ``sum(losses)`` w.r.t. everything the loss reads of the network -- ``all_cls_scores``,
      ``all_bbox_preds``, ``occupancy_preds`` -- are ``torch.equal``;
    * the gradient of EVERY parameter is the same: the difference of the two totals is back-propagated once, and every
      parameter gradient of it is exactly zero (backward is linear in its upstream gradient, so this is
      grad(host) - grad(device) with both taken by the SAME backward pass);
    * the parameters of the cls / reg branches, taken by two separate ``backward`` passes, are ``torch.equal``.
    Two separate passes cannot be compared over all parameters: on an MI355X 104 of the 300 parameter gradients --
    everything upstream of the decoder's cross-attention value gradient, which ``ver_msda3d_backward`` accumulates with fp32
    atomics in scheduling order -- differ in their last bits (up to 6.7e-6) between two passes of the SAME host-solver loss.
    ``forward(..., targets_for=...)`` queues no host copy on a device-solver head."""
    syn = pkg('synthetic')
    head = _heads()[0]
    w2p, org = syn.camera_batch(2, seed=1)
    feats = T(syn.vit_features(2, seed=0)).to(DEV).permute(1, 0, 2, 3).contiguous()
    gb, gl = _gt_lists((3, 4))
    gt_occ = T(np.random.default_rng(9).integers(0, 17, size=(2, 504000))).to(DEV)
    outs = head(feats, None, world2pixel=T(w2p).to(DEV), origin=T(org).to(DEV))
    named = [(k, p) for k, p in head.named_parameters() if p.requires_grad]
    preds = [outs['all_cls_scores'], outs['all_bbox_preds'], outs['occupancy_preds']]
    branches = [(k, p) for k, p in named if k.startswith(('cls_branches.', 'reg_branches.'))]
    assert len(branches) >= 40
    totals, dicts, grads = [], [], []
    for solver in ('host', 'device'):
        head.assigner.solver = solver
        args = (gb, gl) if solver == 'host' else (head.pad_gts(gb, gl), None)
        losses = head.loss(args[0], args[1], gt_occ, outs)
        totals.append(sum(losses.values()))
        dicts.append({k: float(v) for k, v in losses.items()})
        grads.append(torch.autograd.grad(totals[-1], preds + [p for _, p in branches], retain_graph=True))
    head.assigner.solver = 'host'
    assert sorted(dicts[0]) == sorted(dicts[1])
    for k in dicts[0]:
        assert dicts[0][k] == dicts[1][k], k
    for name, a, b in zip(['all_cls_scores', 'all_bbox_preds', 'occupancy_preds'] + [k for k, _ in branches], *grads):
        assert float(a.abs().max()) > 0 and torch.equal(a, b), (name, float((a - b).abs().max()))
    diff = torch.autograd.grad(totals[0] - totals[1], [p for _, p in named], retain_graph=True, allow_unused=True)
    reached = 0
    for (k, _), g in zip(named, diff):
        if g is not None:
            reached += 1
            assert not bool(g.any()), (k, float(g.abs().max()))
    assert reached > 250                                          # (the whole network is under the loss)
    with torch.no_grad():
        head.assigner.solver = 'device'
        early = head(feats, None, world2pixel=T(w2p).to(DEV), origin=T(org).to(DEV), targets_for=(gb, gl))
        head.assigner.solver = 'host'
    assert 'pending_targets' not in early


def test_device_assign_of_a_single_problem():
    """``HungarianAssigner3D(solver='device').assign`` on GPU tensors: the golden matching of loss_vocc.npz, as the host
    solver gives it (detection and layout form)."""
    g = golden('loss_vocc')
    gh = golden('head_vocc')
    host, dev = _heads()
    cls, box = T(gh['c3_b0_cls'][-1]).to(DEV), T(gh['c3_b0_bbox'][-1]).to(DEV)
    boxes, labels = cases.detection_gt()
    gb, gl = T(boxes).to(DEV), T(labels).to(DEV)
    res = dev.assigner.assign(box[0], cls[0], gb, gl)
    assert res.gt_inds.tolist() == g['gt_inds'].tolist() and res.labels.tolist() == g['assigned_labels'].tolist()
    for layout in (False, True):
        a = host.assigner.assign(box[0], cls[0], gb, gl, layout=layout)
        b = dev.assigner.assign(box[0], cls[0], gb, gl, layout=layout)
        assert torch.equal(a.gt_inds, b.gt_inds) and torch.equal(a.labels, b.labels) and b.gt_inds.dtype == torch.long
    pkg('hipops').AssignmentFlag.of(DEV).poll(sync=True)


def test_targets_and_losses_are_capturable():
    """``_targets_device`` + ``_losses_from_targets`` captured in a ``torch.cuda.graph`` from static prediction / PaddedGts
    buffers: the capture succeeding is the proof that nothing on the path synchronises.  New ground truth (other counts,
    inside the capacity) and new predictions are copied into the static buffers; two replays each equal the eager device
    path on the same values."""
    dev = _heads()[1]
    all_cls, all_box = _golden_predictions(2)
    cap = 20
    first = _gt_lists((3, 4, 9, 2))
    static_gts = dev.pad_gts(*first, capacity=cap)
    static_cls, static_box = all_cls.clone(), all_box.clone()

    def step(c, b, gts):
        targets = dev._targets_device(c, b, gts)
        lc, lb = dev._losses_from_targets(c, b, *targets)
        return targets[:3] + (targets[3] + 0, torch.stack(lc), torch.stack(lb))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        step(static_cls, static_box, static_gts)                  # warm-up outside the capture (library handles, caches)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        static_out = step(static_cls, static_box, static_gts)
    cases_ = [(first, all_cls, all_box),
              (_gt_lists((20, 0, 1, 12), seed=60), all_cls.flip(2).contiguous(), all_box.flip(2).contiguous())]
    for gts_lists, c, b in cases_:
        fresh = dev.pad_gts(*gts_lists, capacity=cap)
        for dst, src in zip(static_gts, fresh):
            dst.copy_(src)
        static_cls.copy_(c)
        static_box.copy_(b)
        with torch.no_grad():
            want = step(c, b, fresh)
        for replay in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for got, ref in zip(static_out, want):
                assert torch.equal(got, ref), replay
    pkg('hipops').AssignmentFlag.of(DEV).poll(sync=True)
