"""The flat gradient exchange on one GPU and one process: ``ver_grad_pack`` bit for bit against ``hipops.pack_host``,
``ver_clip_adamw_step_flat`` bit for bit against ``ver_clip_adamw_step_tensors`` on fp32 gradient tensors of the same values
(eagerly and captured), and the two captured training steps with an exchange and no process group (world = 1, scale 1)
against their eager twins.  Sizes, values, scripts and the reasons for the bounds: tests/grad_exchange_cases.py."""
import copy
import warnings

import numpy as np
import pytest
import torch

import grad_exchange_cases as gx
from util import pkg

warnings.filterwarnings('ignore')
pytestmark = pytest.mark.gpu
DEV = gx.DEV
WIRES = [torch.float32, torch.bfloat16]
IDS = ['f32wire', 'bf16wire']


def _params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=gen).to(DEV)) for n in gx.SIZES]


def _groups(ps):
    return [dict(params=ps[:6], lr=3e-3, weight_decay=0.05), dict(params=ps[6:], lr=3e-4, weight_decay=0.0)]


# ------------------------------------------------------------------------------------------ ver_grad_pack
@pytest.mark.parametrize('scale', [1.0, 1 / 3], ids=['scale1', 'scale1/3'])
@pytest.mark.parametrize('wire', WIRES, ids=IDS)
def test_pack_equals_the_host_model_and_leaves_the_padding(wire, scale):
    hip, ddp = pkg('hipops'), pkg('ddp')
    ps = _params()
    ex = ddp.GradExchange([('p%d' % n, p) for n, p in zip(gx.SIZES, ps)], wire_dtype=wire)
    assert ex.world == 1 and ex.scale == 1.0 and (ex.offsets, ex.total) == ddp.flat_layout(gx.SIZES)
    assert ex.flat.dtype == wire and ex.flat.numel() == ex.total and ex.flat.data_ptr() % 16 == 0
    assert not bool(ex.flat.any())                                         # zero-filled once
    if scale != 1.0:
        ex.world = 3                                                       # (what a process group of three would set)
    values = gx.gradient_values(11)
    for p, g in zip(ps, gx.gradient_tensors(values)):
        p.grad = g
    sentinel = -7.0
    ex.flat.fill_(sentinel)
    ex.pack()
    torch.cuda.synchronize()
    flat = ex.flat.cpu()
    raw = flat.view(torch.int32 if wire == torch.float32 else torch.int16).numpy()
    covered = np.zeros(ex.total, dtype=bool)
    for n, o, g in zip(gx.SIZES, ex.offsets, values):
        want = hip.pack_host(g, scale, wire)
        got = raw[o:o + n].view(want.dtype if wire == torch.bfloat16 else np.float32)
        covered[o:o + n] = True
        if wire == torch.bfloat16:
            diff = got != want
        else:                       # (an fp32 NaN keeps whatever payload the multiplier hands on: NaN where the model has NaN)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), n
            diff = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
        assert not diff.any(), 'size %d: %d elements differ from pack_host, first at %d' % (n, diff.sum(), np.argmax(diff))
    pad = flat.float().numpy()[~covered]
    assert pad.size == ex.total - sum(gx.SIZES) > 0 and np.all(pad == sentinel)
    back = ex.grads()
    assert [tuple(b.shape) for b in back] == [tuple(p.shape) for p in ps] and all(b.dtype == torch.float32 for b in back)
    assert back[7].data_ptr() != ex.flat.data_ptr() + ex.offsets[7] * ex.flat.element_size()      # copies, not views


# ------------------------------------------------------------------------------------------ ver_clip_adamw_step_flat
def _rounded(gen, scale=0.01):
    """Random gradients that a bf16 wire holds exactly, so that both wires and the fp32 twin see the same values."""
    return [(torch.randn(n, generator=gen) * scale).to(torch.bfloat16).float() for n in gx.SIZES]


def _assert_same_state(tag, ps, opt, qs, twin, norm, twin_norm):
    assert torch.equal(gx.bits(norm.reshape(1)), gx.bits(twin_norm.reshape(1))), (tag, float(norm), float(twin_norm))
    for i, (p, q) in enumerate(zip(ps, qs)):
        sp, sq = opt.state[p], twin.state[q]
        assert sp['step'] == sq['step'], (tag, i, sp['step'], sq['step'])
        for name, a, b in (('parameter', p, q), ('exp_avg', sp['exp_avg'], sq['exp_avg']),
                           ('exp_avg_sq', sp['exp_avg_sq'], sq['exp_avg_sq'])):
            a, b = gx.bits(a), gx.bits(b)
            assert torch.equal(a, b), '%s: %s of tensor %d (%d elements) differs from the fp32-tensor twin in %d' % (
                tag, name, i, a.numel(), int((a != b).sum()))


@pytest.mark.parametrize('case', ['clip', 'noclip', 'nan'])
@pytest.mark.parametrize('wire', WIRES, ids=IDS)
def test_flat_step_equals_the_tensor_step_bit_for_bit(wire, case):
    opt_mod, ddp = pkg('optim'), pkg('ddp')
    ps, qs = _params(), _params()
    max_norm = 0.0 if case == 'noclip' else 1.0
    opt = opt_mod.ClipAdamW(_groups(ps), betas=(0.9, 0.99), max_norm=max_norm)
    twin = opt_mod.ClipAdamW(_groups(qs), betas=(0.9, 0.99), max_norm=max_norm)
    ex = ddp.GradExchange(ps, wire_dtype=wire)
    gen = torch.Generator().manual_seed(5)
    for it in range(3):
        grads = _rounded(gen)
        if case == 'nan' and it == 1:
            grads[4][3] = float('nan')
        for o, n, g, q in zip(ex.offsets, gx.SIZES, grads, qs):
            ex.flat[o:o + n].copy_(g.to(DEV))
            q.grad = g.to(DEV).clone()                                   # a fresh fp32 tensor, 16-byte aligned
            assert q.grad.data_ptr() % 16 == 0
        assert all(p.grad is None for p in ps)                           # (p.grad is not consulted)
        norm = opt.step(ex)
        twin_norm = twin.step()
        tag = '%s step %d' % (case, it + 1)
        _assert_same_state(tag, ps, opt, qs, twin, norm, twin_norm)
        want = float(torch.sqrt(sum(g.double().pow(2).sum() for g in grads)))
        if case == 'nan' and it >= 1:
            # the non-finite norm poisons EVERY parameter of both groups, in both runs alike (compared bitwise above)
            assert all(bool(torch.isnan(p).all()) for p in ps) and all(bool(torch.isnan(q).all()) for q in qs)
        else:
            assert abs(float(norm) - want) <= 1e-5 * want and want > 2 * 1.0         # (max_norm = 1 clips)
            assert all(bool(torch.isfinite(p).all()) for p in ps)
    assert all(opt.state[p]['step'] == 3 for p in ps)


@pytest.mark.parametrize('wire', WIRES, ids=IDS)
def test_captured_pack_and_flat_step_replay_like_the_eager_twin(wire):
    """One eager exchanged step, ``prepare_capture`` of both, ONE graph of ``p.grad = gin * 1`` + ``pack`` + ``step(exchange)``,
    three replays on new gradient values, an eager exchanged step from the first step's buffers (the exchange's own
    stale-pointer case: the replays rewrote its device table), then an eager ``step()`` without an exchange -- all bit for bit
    the all-eager twin's."""
    opt_mod, ddp = pkg('optim'), pkg('ddp')
    ps, qs = _params(), _params()
    opt = opt_mod.ClipAdamW(_groups(ps), betas=(0.9, 0.99), max_norm=1.0)
    twin = opt_mod.ClipAdamW(_groups(qs), betas=(0.9, 0.99), max_norm=1.0)
    ex, twin_ex = ddp.GradExchange(ps, wire_dtype=wire), ddp.GradExchange(qs, wire_dtype=wire)
    E = [torch.zeros(n, device=DEV) for n in gx.SIZES]
    twin_E = [torch.zeros(n, device=DEV) for n in gx.SIZES]
    gen = torch.Generator().manual_seed(9)
    taken = [0]

    def fresh():
        taken[0] += 1
        return [torch.randn(n, generator=gen) * (0.1 if taken[0] % 3 == 2 else 0.01) for n in gx.SIZES]

    def twin_step(grads, exchanged=True):
        for q, buf, g in zip(qs, twin_E, grads):
            buf.copy_(g)
            q.grad = buf
        if not exchanged:
            return twin.step()
        twin_ex.pack()
        return twin.step(exchange=twin_ex)

    def eager_step(grads, exchanged=True):
        for p, buf, g in zip(ps, E, grads):
            buf.copy_(g)
            p.grad = buf
        if not exchanged:
            return opt.step()
        ex.pack()
        return opt.step(exchange=ex)

    grads = fresh()
    _assert_same_state('eager 1', ps, opt, qs, twin, eager_step(grads), twin_step(grads))
    gin = [torch.zeros(n, device=DEV) for n in gx.SIZES]
    torch.cuda.synchronize()
    opt.prepare_capture()
    ex.prepare_capture()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for p, x in zip(ps, gin):
            p.grad = x * 1.0
        ex.pack()
        norm = opt.step(exchange=ex)
    for it in range(3):
        grads = fresh()
        for buf, g in zip(gin, grads):
            buf.copy_(g)
        opt.refresh()
        graph.replay()
        opt.replayed()
        ex.replayed()
        _assert_same_state('replay %d' % (it + 1), ps, opt, qs, twin, norm, twin_step(grads))
    grads = fresh()
    _assert_same_state('eager exchanged step after the replays', ps, opt, qs, twin, eager_step(grads), twin_step(grads))
    grads = fresh()
    _assert_same_state('eager step() after the replays', ps, opt, qs, twin, eager_step(grads, False), twin_step(grads, False))
    assert all(opt.state[p]['step'] == 6 for p in ps)


# ------------------------------------------------------------------------------------------ the captured training steps
@pytest.mark.parametrize('autocast', [False, True], ids=['fp32', 'bf16'])
def test_graphed_lift_step_with_an_exchange_replays_the_eager_steps(autocast):
    """The five-step script of ``test_graphed_lift_step_replays_the_eager_training_steps`` with ``exchange=`` and no process
    group: 1 eager exchanged warm-up step + 4 replays of graph A, the (empty) all-reduce and graph B.  fp32: fp32 wire, the
    twin takes PLAIN eager steps -- the exchange adds no rounding.  bf16 autocast: bf16 wire, the twin takes eager exchanged
    steps."""
    graphs, ddp = pkg('graphs'), pkg('ddp')
    wire = torch.bfloat16 if autocast else torch.float32
    base = gx.lift_head()
    heads = [base, copy.deepcopy(base)]
    before = {k: p.detach().clone() for k, p in gx.trainable(base)}
    ins = gx.lift_inputs()
    models = [gx.LiftModel(h, autocast) for h in heads]
    opts = [gx.optimizer(h) for h in heads]
    twin_ex = ddp.GradExchange(gx.trainable(heads[0]), wire_dtype=wire) if autocast else None
    want = gx.eager_steps(models[0], opts[0], twin_ex, [ins[it % 2] for it in range(5)])
    ex = ddp.GradExchange(gx.trainable(heads[1]), wire_dtype=wire)
    step = graphs.GraphedLiftStep(models[1], opts[1], *ins[0], warmup=1, exchange=ex)      # = step 0, eagerly, then two captures
    got = [float(step(*ins[it % 2])) for it in range(1, 5)]
    assert want[1] != want[3]                                              # (the steps do move the loss)
    assert all(opts[1].state[p]['step'] == 5 for _, p in gx.trainable(heads[1]))
    losses = gx.same_losses(got, want[1:], autocast, 'exchanged graph vs eager')
    updates = gx.same_updates(heads[1], heads[0], before, autocast, 'exchanged lifting graph vs eager')
    assert not losses and not updates, (losses, updates)
    # the clip norm graph B returned is the norm of what the exchange holds
    held = float(torch.sqrt(sum(g.double().pow(2).sum() for g in ex.grads())))
    assert abs(float(step.grad_norm) - held) <= 1e-5 * held
    # an eager step of the same optimizer after the replays, without the exchange
    opts[1].zero_grad(set_to_none=True)
    models[1](*ins[1]).backward()
    opts[1].step()
    assert all(opts[1].state[p]['step'] == 6 for _, p in gx.trainable(heads[1]))


@pytest.mark.parametrize('autocast', [False, True], ids=['fp32', 'bf16'])
def test_graphed_train_step_with_an_exchange_replays_the_eager_steps(autocast):
    """The five-step script of tests/test_train_graph_gpu.py (its head, viewpoints, ground truth with 4, 0, 6, 2, 5 boxes,
    optimizer and bounds) with ``exchange=`` and no process group; the loss normalisers of every replay are the preset rows
    (``clamp(counts, max=Nq).sum()``), the twin's are counted from its matches.  fp32: fp32 wire against that file's PLAIN
    eager run; bf16 autocast: bf16 wire against an eager exchanged twin."""
    import test_train_graph_gpu as tg
    graphs, ddp = pkg('graphs'), pkg('ddp')
    wire = torch.bfloat16 if autocast else torch.float32
    run = tg._five_steps(autocast)                                        # (shared with that file's tests; not modified here)
    before, ins, gt = run['before'], run['ins'], run['gt']

    def restored():
        head = tg._build(init=tg.INIT)                                   # a fresh head with the values the five steps began from
        head.load_state_dict(run['heads'][0].state_dict())
        with torch.no_grad():
            for k, p in head.named_parameters():
                p.requires_grad_(k in before)
                if k in before:
                    p.copy_(before[k])
        return head, graphs.MultiTaskStep(head, torch.bfloat16 if autocast else None).eval()

    total = lambda d: sum(d.values())
    if autocast:
        twin, twin_model = restored()
        opt, _ = tg._optimizer(twin, lr=tg.LR, eps=tg.EPS)
        want = gx.eager_steps(twin_model, opt, ddp.GradExchange(gx.trainable(twin), wire_dtype=wire),
                              [ins[it % 2] + gt[it] for it in range(5)], total)
    else:
        twin, want = run['heads'][0], run['eager'][0]
    head, model = restored()
    opt, params = tg._optimizer(head, lr=tg.LR, eps=tg.EPS)
    ex = ddp.GradExchange(gx.trainable(head), wire_dtype=wire)
    step = graphs.GraphedTrainStep(model, opt, *ins[0], *gt[0], pair_capacity=tg.PAIR_CAP, warmup=1, exchange=ex)
    assert getattr(head, 'preset_normalisers', None) is None              # set for the capture alone
    got = []
    for it in range(1, 5):
        got.append(tg._floats(step(*ins[it % 2], *gt[it])))
    outside = tg._same_steps(got, want[1:], autocast, 'exchanged graph vs eager')
    assert all(opt.state[p]['step'] == 5 for p in params)
    updates = tg._same_updates(head, twin, before, autocast, 'exchanged graph vs eager')
    assert not outside and not updates, (outside, updates)
    assert got[0]['loss_bbox'] == 0.0 and got[1]['loss_bbox'] > 0         # the step without boxes: normalisers clamped to 1
    flags = step.flags()
    assert flags['rejected_pairs'] == 0 and flags['lost_listings'] == 0


# ------------------------------------------------------------------------------------------ refusals
def test_refusals():
    opt_mod, ddp, graphs = pkg('optim'), pkg('ddp'), pkg('graphs')
    ps = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (5, 9)]
    other = torch.nn.Parameter(torch.randn(3, device=DEV))
    opt = opt_mod.ClipAdamW(ps, lr=1e-3)
    # an exchange over a parameter the optimizer does not hold
    foreign = ddp.GradExchange([('a', ps[0]), ('stranger', other)], wire_dtype=torch.float32)
    with pytest.raises(ValueError, match='stranger of the exchange is not a parameter of this optimizer'):
        opt.step(exchange=foreign)
    assert not opt.state[ps[0]] or opt.state[ps[0]]['step'] == 0           # nothing was updated
    # a captured step whose exchange does not cover the optimizer's parameters: refused before any step
    part = ddp.GradExchange([ps[0]], wire_dtype=torch.float32)
    x = torch.zeros(1, device=DEV)
    with pytest.raises(ValueError, match='the exchange lists 1 parameters, the optimizer trains 2'):
        graphs.GraphedLiftStep(torch.nn.Identity(), opt, x, x, x, x, exchange=part)
    # a parameter without a gradient at pack()
    ex = ddp.GradExchange([('first.weight', ps[0]), ('second.bias', ps[1])])
    ps[0].grad = torch.ones_like(ps[0])
    with pytest.raises(RuntimeError, match='second.bias has no gradient'):
        ex.pack()
    # a model wrapped in DistributedDataParallel: still refused, and the message names the way out
    wrapped = torch.nn.parallel.DistributedDataParallel
    with pytest.raises(RuntimeError, match='DistributedDataParallel.*exchange='):
        graphs.GraphedTrainStep(wrapped.__new__(wrapped), opt, x, x, x, None, None, exchange=ex)
    with pytest.raises(RuntimeError, match='DistributedDataParallel.*exchange='):
        graphs.GraphedTrainStep(wrapped.__new__(wrapped), opt, x, x, x, None, None)
    with pytest.raises(TypeError, match='wire_dtype'):
        ddp.GradExchange(ps, wire_dtype=torch.float16)
    with pytest.raises(TypeError, match='dense fp32 GPU parameters only'):
        ddp.GradExchange([torch.nn.Parameter(torch.zeros(3))])
    with pytest.raises(ValueError, match='twice'):
        ddp.GradExchange([ps[0], ps[0]])
