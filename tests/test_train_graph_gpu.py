"""``graphs.GraphedTrainStep``: the full multi-task training step -- encoder, decoder, branches, occupancy, occupancy targets
from sparse pairs, set loss, focal loss, backward, ``ClipAdamW`` -- as ONE hipGraph with fresh ground truth per replay, against
``graphs.MultiTaskStep`` called eagerly.  vocc.py's head at ONE viewpoint per step, ``solver='fused'``; inputs from
``synthetic``, boxes from ``cases.detection_gt`` (thinned so that no two centres are close), random sparse pairs.

The bounds are those of ``test_graphed_lift_step_replays_the_eager_training_steps`` (tests/test_head_gpu.py), the project's
bound for "same kernels, replayed": losses within 1e-5 (fp32) / 2e-3 (bf16 autocast) relative, the update of every parameter
within 0.05 / 0.2 relative L2 (AdamW's early updates are ~ lr * sign(g): an element whose tiny gradient changes sign between
two runs moves by 2 lr, so the bound is on a tensor's update, not element-wise).  Two EAGER twins are held to them first.

The optimizer of the five compared steps is ``ClipAdamW(lr=1e-6, eps=0.1)``, not vocc.py's (lr 1e-4, eps 1e-8), because two
EAGER runs do not stay inside these bounds at vocc.py's settings, measured on this head before any graph was involved.  The
gather backward adds with fp32 atomics, so gradients differ in their last bits from run to run.  With eps = 1e-8 AdamW's first
steps move every element by ~lr * sign(g), whatever |g|: an element whose gradient IS rounding noise (the key third of the
decoder's ``in_proj_bias``, whose true gradient is zero) moves by +-lr at random.  Under bf16 autocast that separated two eager
runs by 0.30 - 0.33 in the update of every ``in_proj_bias`` (bound 0.2) and, once a bf16 copy of a weight rounds the other way,
by 1e-3 at the second step and 1e-2 ... 4e-2 at the third to fifth in the detection terms (bound 2e-3) -- at lr 1e-4 and at
1e-6 alike.  In fp32 the pair stayed within 7e-7, but one of three graph-against-eager runs reached 1.1e-5 (bound 1e-5).  With
eps far above sqrt(v) an element's update is proportional to its gradient, noise moves nothing, and the separation scales
with lr: measured, the eager pair then agrees to the last digit of every loss in bf16 (updates within 3e-7) and within 6e-7
in fp32.  What the comparison holds is unchanged: the update bound is relative to the update, and a replay that did not advance
the device-side counts is still off by the ratio of AdamW's first-moment corrections (1.9 at k = 2)."""
import copy
import warnings

import numpy as np
import pytest
import torch

import cases
from util import pkg

warnings.filterwarnings('ignore')
pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = torch.device('cuda', 0)
CAP, PAIR_CAP = 8, 40000
COUNTS = (4, 0, 6, 2, 5)                       # boxes of step k (one sample per step): a step without any among them
PAIRS = (30000, 12000, 40000, 500, 22000)      # sparse occupancy pairs of step k
LR = 1e-6                                      # of the five compared steps (module docstring)
EPS = 0.1                                      # of the five compared steps (module docstring)
INIT = True                                    # the five compared steps start from init_weights(), as bench.py's do


def _build(seed=7, init=False):
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    pkg()
    train_cfg = dict(cases.VOCC_TRAIN_CFG, assigner=dict(cases.VOCC_TRAIN_CFG['assigner'], solver='fused'))
    head = pkg('registry').build_head(dict(cases.vocc_head_cfg(), train_cfg=train_cfg)).eval()
    if init:
        head.init_weights()
    else:
        code_weights = head.code_weights.detach().clone()
        pkg('synthetic').load_seeded(head, seed)
        head.code_weights.data.copy_(code_weights)      # (the seeded fill also hits this fixed, non-trainable loss-weight vector)
    return head.to(DEV)


def _viewpoints():
    syn = pkg('synthetic')
    w2p, org = syn.camera_batch(2, seed=1)
    feats = T(syn.vit_features(2, seed=0)).to(DEV)
    return [(feats[b].unsqueeze(1).contiguous(), T(w2p[b:b + 1]).to(DEV), T(org[b:b + 1]).to(DEV)) for b in range(2)]


def _boxes(seed, n, apart=2.5):
    """``n`` boxes of ``cases.detection_gt`` whose centres are at least ``apart`` metres from each other: a Hungarian match
    between well separated boxes does not flip on a last-bit difference of the costs."""
    boxes, labels = cases.detection_gt(seed=seed, num_gt=64)
    keep = []
    for i in range(len(boxes) if n else 0):
        if all(np.linalg.norm(boxes[i, :3] - boxes[j, :3]) >= apart for j in keep):
            keep.append(i)
        if len(keep) == n:
            break
    assert len(keep) == n
    return boxes[keep, :7], labels[keep]


def _ground_truth(head, k, counts=COUNTS, pairs=PAIRS, spoil=None):
    """(PaddedGts at the capacity, PackedOccGts on the GPU) of step ``k``; ``spoil``: the class of pair 0."""
    boxes, labels = _boxes(50 + k, counts[k])
    gts = head.pad_gts([T(boxes).to(DEV)], [T(labels).to(DEV)], capacity=CAP)
    rng = np.random.default_rng(70 + k)
    p = np.stack([rng.choice(head.voxel_num, size=pairs[k], replace=False), rng.integers(0, 16, pairs[k])], axis=1).astype(np.int32)
    if spoil is not None:
        p[0, 1] = spoil
    return gts, pkg('hipops').pack_occ_gts([p], pinned=False).to(DEV)


def _freeze_unused(heads, model, args):
    """One probing backward on ``model`` (no update): parameters it leaves without a gradient are not part of the step
    (bench.py freezes them the same way); frozen by name in every head."""
    sum(model(*args).values()).backward()
    names = [k for k, p in model.head.named_parameters() if p.grad is None]
    model.head.zero_grad(set_to_none=True)
    for h in heads:
        for k, p in h.named_parameters():
            if k in names:
                p.requires_grad_(False)


def _optimizer(head, lr=1e-4, weight_decay=0.01, max_norm=35.0, eps=1e-8):
    params = [p for p in head.parameters() if p.requires_grad]
    return pkg('optim').ClipAdamW(params, lr=lr, eps=eps, weight_decay=weight_decay, max_norm=max_norm), params


def _floats(d):
    return {k: float(v) for k, v in d.items()}


_RUNS = {}                                     # autocast -> what the five-step comparison shares


def _five_steps(autocast):
    """Three identical heads and the five steps two of them take EAGERLY (computed once per precision)."""
    if autocast not in _RUNS:
        graphs = pkg('graphs')
        torch.manual_seed(2)
        base = _build(init=INIT)
        heads = [base, copy.deepcopy(base), copy.deepcopy(base)]
        models = [graphs.MultiTaskStep(h, torch.bfloat16 if autocast else None).eval() for h in heads]
        ins = _viewpoints()
        gt = [_ground_truth(base, k) for k in range(5)]
        _freeze_unused(heads, models[0], ins[0] + gt[0])
        before = {k: p.detach().clone() for k, p in base.named_parameters() if p.requires_grad}
        eager = []
        for model in models[:2]:
            opt, _ = _optimizer(model.head, lr=LR, eps=EPS)
            losses = []
            for it in range(5):
                opt.zero_grad(set_to_none=True)
                d = model(*ins[it % 2], *gt[it])
                sum(d.values()).backward()
                opt.step()
                losses.append(_floats(d))
            d = None
            opt.zero_grad(set_to_none=True)
            eager.append(losses)
        _RUNS[autocast] = dict(heads=heads, models=models, ins=ins, gt=gt, before=before, eager=eager)
    return _RUNS[autocast]


def _same_steps(got, want, autocast, what):
    """Prints every figure, then returns the entries outside the bound as (step, name, got, want)."""
    tol = 2e-3 if autocast else 1e-5
    assert len(got) == len(want)
    outside = []
    for it, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w) and len(w) == 14          # six layers' (cls, bbox), occupancy, flow
        for k in w:
            ok = abs(g[k] - w[k]) <= tol * abs(w[k])
            print('%s step %d %s: %.9g vs %.9g%s' % (what, it, k, g[k], w[k], '' if ok else '   <-- outside %g' % tol))
            if not ok:
                outside.append((it, k, g[k], w[k]))
    return outside


def _same_updates(head, twin, before, autocast, what):
    """Prints the worst figure, then returns the parameters outside the bound as (name, relative difference)."""
    worst, outside, still = 0.0, [], []
    for (k, p), q in zip([(k, p) for k, p in twin.named_parameters() if p.requires_grad],
                         [q for q in head.parameters() if q.requires_grad]):
        d_e, d_g = (p.detach() - before[k]).double(), (q.detach() - before[k]).double()
        if float(d_e.norm()) == 0:
            # five updates below the fp32 resolution of the parameter (a constant-initialised bias at this learning rate): the
            # other run must not have moved it either
            still.append(k)
            if float(d_g.norm()) != 0:
                outside.append((k, float('inf')))
            continue
        r = float((d_e - d_g).norm() / d_e.norm())
        worst = max(worst, r)
        if not r < (0.2 if autocast else 0.05):
            outside.append((k, r))
    print('%s, %s: worst relative difference of a parameter update %.2e; outside the bound: %s; not moved in either run: %s'
          % (what, 'bf16' if autocast else 'fp32', worst, outside, still))
    assert len(still) < len(before) // 10, still                # (the comparison is about parameters that moved)
    return outside


@pytest.mark.parametrize('autocast', [False, True], ids=['fp32', 'bf16'])
def test_two_eager_twins_take_the_same_five_steps(autocast):
    """The yardstick of the replay test: two eager runs of the five steps (alternating viewpoints, ground truth with 4, 0, 6,
    2, 5 boxes and 30 000 ... 500 pairs) stay inside the bound themselves, and the losses do move from step to step."""
    run = _five_steps(autocast)
    losses = _same_steps(run['eager'][1], run['eager'][0], autocast, 'eager vs eager')
    updates = _same_updates(run['heads'][1], run['heads'][0], run['before'], autocast, 'eager vs eager')
    assert not losses and not updates, (losses, updates)
    first, third = run['eager'][0][1], run['eager'][0][3]
    assert all(first[k] != third[k] for k in first if k != 'loss_flow')
    assert run['eager'][0][1]['loss_bbox'] == 0.0 and run['eager'][0][0]['loss_bbox'] > 0     # the step without boxes


@pytest.mark.parametrize('autocast', [False, True], ids=['fp32', 'bf16'])
def test_replays_equal_the_eager_training_steps(autocast):
    """The third head takes the same five steps as 1 eager warm-up step + 4 replays of ONE graph -- the inputs of every replay
    differ from the ones captured with, in viewpoint, box count and pair count: every entry of the loss dict of every step,
    the update counts and every parameter's update agree with the eager twin."""
    graphs = pkg('graphs')
    run = _five_steps(autocast)
    yardstick = _same_steps(run['eager'][1], run['eager'][0], autocast, 'eager vs eager')
    assert not yardstick, yardstick                             # only then is eager vs graph meaningful
    head, model, ins, gt = run['heads'][2], run['models'][2], run['ins'], run['gt']
    opt, params = _optimizer(head, lr=LR, eps=EPS)
    step = graphs.GraphedTrainStep(model, opt, *ins[0], *gt[0], pair_capacity=PAIR_CAP, warmup=1)   # = step 0, eagerly
    assert step.capacity == CAP and step.pair_capacity == PAIR_CAP
    losses = []
    for it in range(1, 5):
        out = step(*ins[it % 2], *gt[it])
        assert out is step.losses and all(v.dim() == 0 and v.grad_fn is None for v in out.values())
        losses.append(_floats(out))
        assert float(step.total) == pytest.approx(sum(losses[-1].values()), rel=1e-5)
    outside = _same_steps(losses, run['eager'][0][1:], autocast, 'graph vs eager')
    assert all(opt.state[p]['step'] == 5 for p in params)
    updates = _same_updates(head, run['heads'][0], run['before'], autocast, 'graph vs eager')
    assert not outside and not updates, (outside, updates)
    flags = step.flags()                                        # (the two sticky flags are the process's: not asserted here)
    assert sorted(flags) == ['assignment', 'label_range', 'lost_listings', 'rejected_pairs']
    assert flags['rejected_pairs'] == 0 and flags['lost_listings'] == 0
    del _RUNS[autocast]                                         # (three heads and a graph's pool)


@pytest.fixture(scope='module')
def frozen():
    """One captured step whose optimizer moves nothing (lr = 0, no weight decay), eval mode, bf16 autocast: every replay and
    every eager call of its model see the same parameters, so a replay's losses can be compared with an eager forward."""
    graphs = pkg('graphs')
    head = _build()
    model = graphs.MultiTaskStep(head, torch.bfloat16).eval()
    ins = _viewpoints()
    gt = {k: _ground_truth(head, k) for k in (2, 3)}            # long: 6 boxes, 40 000 pairs; short: 2 boxes, 500 pairs
    _freeze_unused([head], model, ins[0] + gt[2])
    opt, params = _optimizer(head, lr=0.0, weight_decay=0.0)
    step = graphs.GraphedTrainStep(model, opt, *ins[0], *gt[2], pair_capacity=PAIR_CAP, warmup=1)
    yield dict(step=step, model=model, head=head, opt=opt, params=params, ins=ins, gt=gt)


def _eager_losses(model, args):
    return _floats(model(*args))                                # (with autograd on, as the captured forward ran)


def test_no_stale_tail_of_a_longer_step(frozen):
    """Long ground truth, then short ground truth in the same buffers (the long step's boxes and pairs still lie behind the
    short one's), then long again: each replay gives the eager losses of ITS ground truth."""
    step, model, ins, gt = frozen['step'], frozen['model'], frozen['ins'], frozen['gt']
    want = {k: _eager_losses(model, ins[1] + gt[k]) for k in (2, 3)}
    assert abs(want[2]['loss_occupancy'] - want[3]['loss_occupancy']) > 0.05 * want[2]['loss_occupancy']
    assert abs(want[2]['loss_bbox'] - want[3]['loss_bbox']) > 0.05 * want[2]['loss_bbox']
    for k in (2, 3, 2, 3):
        got = _floats(step(*ins[1], *gt[k]))
        for name in want[k]:
            print('replay with ground truth %d, %s: %.9g vs eager %.9g' % (k, name, got[name], want[k][name]))
        for name in want[k]:
            assert abs(got[name] - want[k][name]) <= 2e-3 * abs(want[k][name]), (k, name, got[name], want[k][name])
    # ... and a caller that fills the static buffers itself: the long pairs stay where they are, only the offsets shrink
    step(*ins[1], *gt[2])
    step.occ.offsets.copy_(gt[3][1].offsets)
    step.occ.pairs[:PAIRS[3]].copy_(gt[3][1].pairs)
    step.gts.counts.copy_(gt[3][0].counts)
    step.gts.boxes[:, :CAP].copy_(gt[3][0].boxes)
    step.gts.labels[:, :CAP].copy_(gt[3][0].labels)
    got = _floats(step(*ins[1], step.gts, step.occ))
    for name in want[3]:
        assert abs(got[name] - want[3][name]) <= 2e-3 * abs(want[3][name]), (name, got[name], want[3][name])


def test_flags_report_what_a_replay_could_not_raise(frozen):
    """A pair with a class out of range in a replayed step: the call does not raise (nothing is read back), ``flags()`` shows
    the rejected pair, and the next clean replay clears the count (it belongs to the last step)."""
    step, ins, head = frozen['step'], frozen['ins'], frozen['head']
    bad = _ground_truth(head, 3, spoil=99)
    out = step(*ins[0], *bad)
    assert np.isfinite(float(out['loss_occupancy']))
    flags = step.flags()
    assert flags['rejected_pairs'] == 1 and flags['lost_listings'] == 0
    step(*ins[0], *frozen['gt'][3])
    assert step.flags()['rejected_pairs'] == 0


def test_refusals_name_the_limit_and_replay_nothing(frozen):
    graphs = pkg('graphs')
    step, model, head, opt, params = (frozen[k] for k in ('step', 'model', 'head', 'opt', 'params'))
    ins, gt = frozen['ins'], frozen['gt']
    f, w, o = ins[0]
    gts, occ = gt[3]
    counts = [opt.state[p]['step'] for p in params]
    wide = head.pad_gts([T(_boxes(50, 4)[0]).to(DEV)], [T(_boxes(50, 4)[1]).to(DEV)], capacity=CAP + 1)
    with pytest.raises(ValueError, match='gts.boxes holds 9 boxes per sample, the box capacity captured is 8'):
        step(f, w, o, wide, occ)
    rng = np.random.default_rng(5)
    many = np.stack([rng.choice(head.voxel_num, size=PAIR_CAP + 1, replace=False), rng.integers(0, 16, PAIR_CAP + 1)], 1)
    with pytest.raises(ValueError, match='occ.pairs holds 40001 pairs, the pair capacity captured is 40000'):
        step(f, w, o, gts, pkg('hipops').pack_occ_gts([many], pinned=False).to(DEV))
    with pytest.raises(ValueError, match='feats is .* captured with'):
        step(torch.cat([f, f], 1), w, o, gts, occ)
    with pytest.raises(ValueError, match='origin is .*torch.float64, captured with .*torch.float32'):
        step(f, w, o.double(), gts, occ)
    with pytest.raises(ValueError, match='gts.counts is .*torch.int64'):
        step(f, w, o, type(gts)(gts.boxes, gts.labels, gts.counts.long()), occ)
    with pytest.raises(RuntimeError, match='GPU tensors.*on the CPU: feats'):
        step(f.cpu(), w, o, gts, occ)
    with pytest.raises(TypeError, match='PaddedGts'):
        step(f, w, o, [gts.boxes[0]], occ)
    model.train()
    try:
        with pytest.raises(RuntimeError, match='model.training differs'):
            step(f, w, o, gts, occ)
    finally:
        model.eval()
    assert [opt.state[p]['step'] for p in params] == counts     # nothing was replayed
    # construction: decided from the head, the optimizer and the tensors' devices, before any step
    args = (f, w, o, gts, occ)
    head.assigner.solver = 'host'
    try:
        with pytest.raises(ValueError, match="solver is 'host'"):
            graphs.GraphedTrainStep(model, opt, *args)
    finally:
        head.assigner.solver = 'fused'
    head.add_layout = True
    try:
        with pytest.raises(NotImplementedError, match='add_layout=True'):
            graphs.GraphedTrainStep(model, opt, *args)
    finally:
        head.add_layout = False
    head.getbev = object()
    try:
        with pytest.raises(NotImplementedError, match='getbev'):
            graphs.GraphedTrainStep(model, opt, *args)
    finally:
        head.getbev = None
    with pytest.raises(TypeError, match='can be captured'):
        graphs.GraphedTrainStep(model, torch.optim.AdamW(params, lr=1e-4), *args)
    with pytest.raises(RuntimeError, match='GPU tensors'):
        graphs.GraphedTrainStep(model, opt, f.cpu(), w.cpu(), o.cpu(), gts, occ)
    ddp = torch.nn.parallel.DistributedDataParallel
    with pytest.raises(RuntimeError, match='DistributedDataParallel'):
        graphs.GraphedTrainStep(ddp.__new__(ddp), opt, *args)
    with pytest.raises(ValueError, match='holds 500 pairs, the pair capacity is 100'):
        graphs.GraphedTrainStep(model, opt, *args, pair_capacity=100)
    assert [opt.state[p]['step'] for p in params] == counts


def test_many_replays_train_and_an_eager_step_follows():
    """Train mode (dropout on), bench.py's init and optimizer settings, bf16 autocast, as
    ``test_graphed_lift_step_trains_for_many_replays``.  Two replays with lr = 0 first: the same inputs and parameters, so
    the losses differ by the dropout masks alone (fresh seeds per replay).  Then lr = 1e-4, which ``refresh()`` uploads:
    twelve replays, every gradient norm finite, the total loss lower at the end, every parameter finite.  A live loss of an
    earlier eager step is refused at construction.  An eager step of the same optimizer after the replays advances every
    update count by one (the ``ClipAdamW`` pointer-table contract)."""
    graphs = pkg('graphs')
    torch.manual_seed(2)
    head = _build(init=True).train()
    model = graphs.MultiTaskStep(head, torch.bfloat16)
    f, w, o = _viewpoints()[0]
    gts, occ = _ground_truth(head, 0)
    _freeze_unused([head], model, (f, w, o, gts, occ))
    opt, params = _optimizer(head, lr=0.0, max_norm=300.0)
    kept = sum(model(f, w, o, gts, occ).values())
    with pytest.raises(RuntimeError, match='still alive'):
        graphs.GraphedTrainStep(model, opt, f, w, o, gts, occ, warmup=1)
    kept = float(kept)
    done = opt.state[params[0]]['step']                         # (the refused construction had run its warm-up step)
    step = graphs.GraphedTrainStep(model, opt, f, w, o, gts, occ, warmup=1)
    f, w, o = step.inputs
    a = float(step(f, w, o, step.gts, step.occ)['loss_cls'])
    b = float(step(f, w, o, step.gts, step.occ)['loss_cls'])
    assert a != b and np.isfinite(a) and np.isfinite(b)
    for group in opt.param_groups:
        group['lr'] = 1e-4
    totals = []
    for _ in range(12):
        step(f, w, o, step.gts, step.occ)
        totals.append(float(step.total))
        assert bool(torch.isfinite(step.grad_norm)), totals
    assert all(np.isfinite(totals)) and totals[-1] < totals[0], totals
    assert all(bool(torch.isfinite(p).all()) for p in params)
    assert all(opt.state[p]['step'] == done + 1 + 14 for p in params)
    opt.zero_grad(set_to_none=True)
    sum(model(f, w, o, step.gts, step.occ).values()).backward()
    opt.step()
    assert all(opt.state[p]['step'] == done + 1 + 15 for p in params)
    assert all(bool(torch.isfinite(p).all()) for p in params)
