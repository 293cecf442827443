"""``optim.ClipAdamW`` where host bookkeeping meets device state that a captured hipGraph rewrites: eager steps between
replays, hyper-parameters across that boundary, two graphs on one optimizer, captures that outlive the buffers they read --
and the kernels themselves (csrc/ver_optim.hip) over more than 256 chunks and at their edges.

The references: an all-eager ``ClipAdamW`` twin (same kernels on the same values, partials summed in order: ``torch.equal``)
and the float64 model of tests/optim_model_helper.py, which tests/test_optim_model_cpu.py pins to ``clip_grad_norm_`` +
``torch.optim.AdamW`` in float64.  Bounds against the model: ``near()`` of
tests/test_hip_ops_gpu.py::test_clip_adamw_survives_state_reload_groups_late_parameters_and_nan (atol 3e-6 max |ref|, rtol 3e-6),
the norm 1e-5 relative (test_clip_adamw_equals_clip_grad_norm_plus_torch_adamw).

The tests write the gradients themselves, so their addresses are known: eager steps use persistent buffers E filled in
place, a captured region does ``p.grad = gin[i] * 1.0`` (G, in the graph's pool) on static inputs ``gin``, a replay runs
``refresh(); replay(); replayed()`` as ``graphs.GraphedLiftStep.__call__`` does."""
import copy
import pickle

import pytest
import torch

from optim_model_helper import AdamWModel
from util import pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(1,), (5,), (33, 7), (32768,), (32769,)]           # one chunk to the element, one element into a second chunk
VIEW = 65537                                                 # + a view 4 bytes off a 16-byte boundary: the scalar path over three chunks
MAX_NORM = 10.0                                              # gradient norms are ~3.6, every third step ~36
BETAS = (0.9, 0.99)


def _ratio(got, want):
    """max |got - want| / (atol + rtol |want|) with near()'s atol = 3e-6 max |want|, rtol = 3e-6: <= 1 is inside the bound."""
    got, want = got.detach().cpu().double().reshape(-1), want.detach().cpu().double().reshape(-1)
    if got.numel() == 0:
        return 0.0
    bound = 3e-6 * max(float(want.abs().max()), 1e-30) + 3e-6 * want.abs()
    return float(((got - want).abs() / bound).max())


def _groups(ps):
    return [dict(params=ps[:4], lr=3e-3, weight_decay=0.05), dict(params=ps[4:], lr=3e-4, weight_decay=0.0)]


class _Rig:
    """The parameter set twice on the GPU, identically, alignment included (``opt``: the optimizer under test, ``twin``: all
    eager) and once in the float64 model; ``step('e')`` / ``step('r', capture)`` take one step of all three on fresh seeded
    gradients and check them against each other."""

    def __init__(self, seed):
        opt_mod = pkg('optim')
        self.gen = torch.Generator(device='cpu').manual_seed(seed)
        base = [torch.randn(s, generator=self.gen) for s in SHAPES]
        flat = torch.randn(VIEW + 7, generator=self.gen)

        def make():
            ps = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
            ps.append(torch.nn.Parameter(flat.clone().to(DEV)[1:1 + VIEW]))
            return ps
        self.ours, self.theirs = make(), make()
        assert [p.data_ptr() % 16 for p in self.ours] == [q.data_ptr() % 16 for q in self.theirs] == [0] * len(SHAPES) + [4]
        self.opt = opt_mod.ClipAdamW(_groups(self.ours), betas=BETAS, max_norm=MAX_NORM)
        self.twin = opt_mod.ClipAdamW(_groups(self.theirs), betas=BETAS, max_norm=MAX_NORM)
        self.model = AdamWModel(_groups(base + [flat[1:1 + VIEW]]), betas=BETAS, max_norm=MAX_NORM)
        self.E = [torch.zeros(p.shape, device=DEV) for p in self.ours]
        self.twin_E = [torch.zeros(p.shape, device=DEV) for p in self.theirs]
        self.taken, self.worst, self.clipped = 0, 0.0, 0

    def set_lr(self, group, lr):
        self.opt.param_groups[group]['lr'] = self.twin.param_groups[group]['lr'] = self.model.groups[group]['lr'] = lr

    def capture(self):
        """As GraphedLiftStep captures: after an eager step, synchronised, ``prepare_capture()``, one chain on one stream."""
        gin = [torch.zeros(p.shape, device=DEV) for p in self.ours]
        torch.cuda.synchronize()
        self.opt.prepare_capture()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for p, x in zip(self.ours, gin):
                p.grad = x * 1.0
            norm = self.opt.step()
        assert [p.grad.data_ptr() % 16 for p in self.ours] == [0] * len(self.ours)
        return graph, gin, norm

    def step(self, kind, capture=None):
        scale = 0.01 * (10.0 if self.taken % 3 == 2 else 1.0)
        grads = [torch.randn(p.shape, generator=self.gen) * scale for p in self.ours]
        for q, buf, g in zip(self.theirs, self.twin_E, grads):
            buf.copy_(g)
            q.grad = buf
        twin_norm = self.twin.step()
        model_norm = self.model.step(grads)
        if kind == 'e':
            for p, buf, g in zip(self.ours, self.E, grads):
                buf.copy_(g)
                p.grad = buf
            norm = self.opt.step()
        else:
            graph, gin, norm = capture
            for buf, g in zip(gin, grads):
                buf.copy_(g)
            self.opt.refresh()
            graph.replay()
            self.opt.replayed()
        self.taken += 1
        self.clipped += int(float(model_norm) > MAX_NORM)
        tag = 'step %d (%s)' % (self.taken, kind)
        # (1) bit-equal to the all-eager twin
        assert torch.equal(norm, twin_norm), '%s: norm %.9g, all-eager twin %.9g' % (tag, float(norm), float(twin_norm))
        for i, (p, q) in enumerate(zip(self.ours, self.theirs)):
            sp, sq = self.opt.state[p], self.twin.state[q]
            for name, a, b in (('parameter', p.detach(), q.detach()), ('exp_avg', sp['exp_avg'], sq['exp_avg']),
                               ('exp_avg_sq', sp['exp_avg_sq'], sq['exp_avg_sq'])):
                if not torch.equal(a, b):
                    d = (a - b).abs()
                    pytest.fail('%s: %s of tensor %d differs from the all-eager twin in %d of %d elements, by up to %.3e (max |twin| %.3e)'
                                % (tag, name, i, int((a != b).sum()), a.numel(), float(d.max()), float(b.abs().max())))
            # (3) the host's update counts
            assert sp['step'] == sq['step'] == self.taken, (tag, i, sp['step'])
        # (2) the twin against the float64 model
        assert abs(float(twin_norm) - float(model_norm)) <= 1e-5 * float(model_norm), (tag, float(twin_norm), float(model_norm))
        for i, q in enumerate(self.theirs):
            sq = self.twin.state[q]
            for name, a, b in (('parameter', q, self.model.p[i]), ('exp_avg', sq['exp_avg'], self.model.m[i]),
                               ('exp_avg_sq', sq['exp_avg_sq'], self.model.v[i])):
                r = _ratio(a, b)
                self.worst = max(self.worst, r)
                assert r <= 1.0, '%s: %s of tensor %d is %.2f times the near() bound from the float64 model' % (tag, name, i, r)

    def report(self, what):
        assert 0 < self.clipped < self.taken                       # (one max_norm that clips on some steps and not on others)
        print('%s: %d steps bit-equal to the all-eager twin; twin vs float64 model at most %.3f of the near() bound '
              '(atol 3e-6 max |ref|, rtol 3e-6)' % (what, self.taken, self.worst))


def test_eager_steps_between_replays_read_their_own_gradients():
    """B1: ``e, capture, r, r, e, r, e, r, e, e, r`` with every eager step's gradients in the SAME buffers E.  A replay
    rewrites the device's pointer table to the capture's buffers G; the host's record must not go on claiming E, or the
    second eager step after a replay reads G -- the previous replay's gradients -- and the update is finite, plausible and
    wrong (before the fix, step 6 of this script, the second ``e`` after a replay, returned the norm of step 5's gradients,
    3.61799502, where the all-eager twin returned 36.0701332)."""
    rig = _Rig(101)
    rig.step('e')
    cap = rig.capture()
    for kind in 'rrerereer':
        rig.step(kind, cap)
    rig.report('eager steps between replays')


def test_hyper_parameters_cross_the_eager_replay_boundary():
    """B2: a learning rate moved before an eager step is uploaded by ``_upload``, one moved before a replay by ``refresh()``;
    either is what the next step of the other kind then reads."""
    rig = _Rig(102)
    rig.step('e')
    cap = rig.capture()
    rig.step('r', cap)
    rig.set_lr(1, 1e-3)
    rig.step('e')
    rig.step('r', cap)
    rig.set_lr(1, 2e-3)
    rig.step('r', cap)
    rig.step('e')
    rig.set_lr(0, 1e-3)
    rig.step('r', cap)
    rig.report('learning rates across eager steps and replays')


def test_two_graphs_share_one_optimizer():
    """B3 (bench.py's two latency batch sizes on one optimizer): a second capture with its own inputs and staging buffer;
    each replay restores the pointer table of ITS capture, an eager step in between its own."""
    rig = _Rig(103)
    rig.step('e')
    a = rig.capture()
    rig.step('r', a)
    rig.step('e')
    b = rig.capture()
    assert a[1][0].data_ptr() != b[1][0].data_ptr()
    for kind, cap in (('r', b), ('r', a), ('e', None), ('r', b), ('e', None), ('r', a)):
        rig.step(kind, cap)
    rig.report('two graphs on one optimizer')


@pytest.mark.parametrize('how', ['load_state_dict', 'late_gradient', 'pickle'])
def test_a_capture_whose_buffers_were_replaced_refuses_before_the_replay(how):
    """B4: ``load_state_dict``, an eager step over one more tensor (a first gradient that arrives after the capture) and
    ``__setstate__`` replace or drop the device buffers a captured graph reads by raw address.  ``refresh()`` and
    ``replayed()`` -- what ``GraphedLiftStep.__call__`` runs around the replay -- then raise until a new capture.  The graph
    is NOT replayed after the invalidating action."""
    opt_mod = pkg('optim')
    gen = torch.Generator(device='cpu').manual_seed(104)
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen).to(DEV)) for s in [(5,), (300,), (9,)]]
    opt = opt_mod.ClipAdamW(ps, lr=1e-3, max_norm=1.0)

    def eager(opt, ps, n):
        for p in ps[:n]:
            p.grad = torch.randn(p.shape, generator=gen).to(DEV)
        for p in ps[n:]:
            p.grad = None
        return opt.step()

    def capture(opt, ps, n):
        gin = [torch.randn(p.shape, generator=gen).to(DEV) for p in ps[:n]]
        torch.cuda.synchronize()
        opt.prepare_capture()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for p, x in zip(ps, gin):
                p.grad = x * 1.0
            norm = opt.step()
        return graph, gin, norm
    eager(opt, ps, 2)
    old = capture(opt, ps, 2)
    opt.refresh()                                                  # a live capture passes the guard
    old[0].replay()
    opt.replayed()
    assert [opt.state[p]['step'] for p in ps[:2]] == [2, 2] and not opt.state[ps[2]]
    n = 2
    if how == 'load_state_dict':
        opt.load_state_dict(opt.state_dict())
    elif how == 'late_gradient':
        n = 3
        eager(opt, ps, n)
    else:
        captured_with = opt                                        # (stays alive next to its graph)
        opt = pickle.loads(pickle.dumps(opt))
        ps = opt.param_groups[0]['params']
        assert opt is not captured_with and ps[0].is_cuda
    for guard in (opt.refresh, opt.replayed):
        with pytest.raises(RuntimeError, match='new capture is needed'):
            guard()
    # ... until a new capture: one eager step, prepare_capture(), capture
    eager(opt, ps, n)
    with pytest.raises(RuntimeError, match='new capture is needed'):
        opt.refresh()
    new = capture(opt, ps, n)
    before = [opt.state[p]['step'] for p in ps[:n]]
    opt.refresh()
    new[0].replay()
    opt.replayed()
    assert [opt.state[p]['step'] for p in ps[:n]] == [s + 1 for s in before]
    assert bool(torch.isfinite(new[2])) and all(bool(torch.isfinite(p).all()) for p in ps)


# ------------------------------------------------------------------------------- the kernels against the float64 model
def _against_model(opt, model, ps, grad_steps, norm_rel=1e-5, set_grads=None):
    """Drive optimizer and model with the same gradients; -> worst near() ratio, worst relative norm distance."""
    worst, worst_norm = 0.0, 0.0
    for it, grads in enumerate(grad_steps):
        if set_grads is None:
            for p, g in zip(ps, grads):
                p.grad = None if g is None else g.to(DEV)
        else:
            set_grads(ps, grads)
        norm = float(opt.step())
        want = float(model.step(grads))
        d = abs(norm - want) / want if want > 0 else abs(norm)
        worst_norm = max(worst_norm, d)
        assert d <= norm_rel, (it, norm, want)
        have = [i for i, g in enumerate(grads) if g is not None]
        # (one transfer per quantity, then tensor by tensor on the host: the bound is per tensor)
        cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).cpu().split([ps[i].numel() for i in have])
        got = (cat([ps[i] for i in have]), cat([opt.state[ps[i]]['exp_avg'] for i in have]), cat([opt.state[ps[i]]['exp_avg_sq'] for i in have]))
        for j, i in enumerate(have):
            for name, a, b in (('parameter', got[0][j], model.p[i]), ('exp_avg', got[1][j], model.m[i]), ('exp_avg_sq', got[2][j], model.v[i])):
                r = _ratio(a, b)
                worst = max(worst, r)
                assert r <= 1.0, 'step %d: %s of tensor %d is %.2f times the near() bound from the float64 model' % (it, name, i, r)
            assert opt.state[ps[i]]['step'] == model.k[i]
    return worst, worst_norm


def test_700_chunks_take_three_trips_of_the_partial_sum_loop():
    """B5 (a): 700 tensors of 1 to 9 elements = 700 chunks; ``k_clip_adamw`` adds the partials up with
    ``for (i = threadIdx.x; i < n_chunks; i += 256)``, three trips here (the largest other kernel-level test has ~31 chunks).
    Gradient magnitudes go with the tensor index as [1, 1.5) * (1 + (i % 4) / 4) / sqrt(size), so every partial lies in
    [1, 6.9) and holds at least 1 / (700 * 6.9) = 2e-4 of the squared norm: one partial dropped or counted twice moves the
    norm by >= 1e-4 relative, ten times the bound, and with clipping active (max_norm 1 under a norm above 26) every
    parameter through the factor."""
    opt_mod = pkg('optim')
    gen = torch.Generator(device='cpu').manual_seed(105)
    sizes = [1 + i % 9 for i in range(700)]
    base = [torch.randn(n, generator=gen) for n in sizes]
    ps = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    groups = lambda ts: [dict(params=ts[:400], lr=3e-3, weight_decay=0.05), dict(params=ts[400:], lr=3e-4, weight_decay=0.0)]
    opt = opt_mod.ClipAdamW(groups(ps), betas=BETAS, max_norm=1.0)
    model = AdamWModel(groups(base), betas=BETAS, max_norm=1.0)
    steps = []
    for it in range(3):
        grads = []
        for i, n in enumerate(sizes):
            sign = (torch.rand(n, generator=gen) < 0.5).float() * 2 - 1
            grads.append(sign * (1 + 0.5 * torch.rand(n, generator=gen)) * (1 + (i % 4) / 4) / n ** 0.5)
        sq = torch.stack([(g.double() ** 2).sum() for g in grads])
        assert float(sq.min() / sq.sum()) >= 2e-4 and float(sq.sum().sqrt()) > 26          # (what the docstring claims)
        steps.append(grads)
    assert sum(-(-n // opt.CHUNK) for n in sizes) == 700
    worst, worst_norm = _against_model(opt, model, ps, steps)
    print('700 chunks, 3 clipped steps: norm within %.2e relative of the float64 norm (bound 1e-5); parameters and moments '
          'at most %.3f of the near() bound' % (worst_norm, worst))


def test_misaligned_gradient_with_an_aligned_parameter():
    """B5 (b): the gradient a view 4 bytes off a 16-byte boundary, parameter and moments aligned -- ``k_sqnorm`` takes its
    scalar loop, ``k_clip_adamw`` must not read the gradient as float4 -- over two chunks, next to an aligned tensor."""
    opt_mod = pkg('optim')
    gen = torch.Generator(device='cpu').manual_seed(106)
    base = [torch.randn(40001, generator=gen), torch.randn(260, generator=gen)]
    ps = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    opt = opt_mod.ClipAdamW(ps, lr=3e-3, betas=BETAS, weight_decay=0.05, max_norm=5.0)
    model = AdamWModel([dict(params=base)], lr=3e-3, betas=BETAS, weight_decay=0.05, max_norm=5.0)
    raw = torch.zeros(40001 + 8, device=DEV)

    def set_grads(ps, grads):
        raw[1:40002].copy_(grads[0])
        ps[0].grad = raw[1:40002]
        ps[1].grad = grads[1].to(DEV)
        assert ps[0].grad.data_ptr() % 16 == 4 and ps[0].data_ptr() % 16 == 0 and ps[0].grad.is_contiguous()
    steps = [[torch.randn(b.shape, generator=gen) * (0.01 if it == 1 else 1.0) for b in base] for it in range(3)]
    worst, worst_norm = _against_model(opt, model, ps, steps, set_grads=set_grads)
    assert opt.state[ps[0]]['exp_avg'].data_ptr() % 16 == 0
    print('misaligned gradient, aligned parameter: norm %.2e relative (bound 1e-5), at most %.3f of the near() bound' % (worst_norm, worst))


@pytest.mark.parametrize('max_norm', [0.7, 0.0])
def test_an_inf_gradient_behaves_as_clip_grad_norm_plus_torch_adamw(max_norm):
    """B5 (c): one ``inf`` in one gradient, against ``clip_grad_norm_`` + ``torch.optim.AdamW`` on the GPU, element by
    element.  With clipping the norm is inf, the factor 0, and 0 * inf = NaN poisons that element alone -- every other one
    sees a zero gradient; without clipping the element's moments become inf and the parameter NaN.  Two ordinary steps
    come first; the inf step is the last, because torch forms the first moment as a lerp, m + w (g - m), which turns an inf
    moment into NaN one step later where b1 m + (1 - b1) g keeps it inf -- not what is compared here.  The NaN / inf pattern is
    equal, the finite elements are within the bound this suite holds ClipAdamW to against torch
    (test_clip_adamw_equals_clip_grad_norm_plus_torch_adamw: atol 2e-6 max |ref|, rtol 2e-6)."""
    opt_mod = pkg('optim')
    gen = torch.Generator(device='cpu').manual_seed(107)
    base = [torch.randn(s, generator=gen) for s in [(3000,), (17, 5), (40000,)]]
    ours = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    ref = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    a = opt_mod.ClipAdamW(ours, lr=3e-3, betas=BETAS, weight_decay=0.05, max_norm=max_norm)
    b = torch.optim.AdamW(ref, lr=3e-3, betas=BETAS, weight_decay=0.05)
    for it in range(3):
        for i, (p, q) in enumerate(zip(ours, ref)):
            g = torch.randn(p.shape, generator=gen)
            if it == 2 and i == 2:
                g[33001] = float('inf')
            p.grad, q.grad = g.clone().to(DEV), g.clone().to(DEV)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(ref, max_norm)
        b.step()
        norm = a.step()
        assert bool(torch.isinf(norm)) == (it == 2) and not bool(torch.isnan(norm))
        for i, (p, q) in enumerate(zip(ours, ref)):
            for name, x, y in (('parameter', p.detach(), q.detach()), ('exp_avg', a.state[p]['exp_avg'], b.state[q]['exp_avg']),
                               ('exp_avg_sq', a.state[p]['exp_avg_sq'], b.state[q]['exp_avg_sq'])):
                x, y = x.cpu().double().reshape(-1), y.cpu().double().reshape(-1)
                assert torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.isinf(x), torch.isinf(y)), (it, i, name)
                odd = ~torch.isfinite(y)
                assert int(odd.sum()) == (1 if (it == 2 and i == 2) else 0), (it, i, name, int(odd.sum()))
                assert torch.equal(x[odd].nan_to_num(nan=7.0), y[odd].nan_to_num(nan=7.0))         # (the sign of an inf too)
                x, y = x[~odd], y[~odd]
                assert bool(((x - y).abs() <= 2e-6 * float(y.abs().max()) + 2e-6 * y.abs()).all()), (it, i, name, float((x - y).abs().max()))
    assert bool(torch.isnan(ours[2].detach().reshape(-1)[33001]))


def test_steps_with_all_zero_gradients():
    """B5 (d): a zero norm clips nothing (max_norm / (0 + 1e-6) clamps to 1) and divides nothing by zero: as the very first
    step (both moments 0: 0 / (0 + eps)) and between ordinary steps (the moments decay, the parameter keeps moving)."""
    opt_mod = pkg('optim')
    gen = torch.Generator(device='cpu').manual_seed(108)
    base = [torch.randn(s, generator=gen) for s in [(7,), (33000,)]]
    ps = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    opt = opt_mod.ClipAdamW(ps, lr=3e-3, betas=BETAS, weight_decay=0.05, max_norm=0.7)
    model = AdamWModel([dict(params=base)], lr=3e-3, betas=BETAS, weight_decay=0.05, max_norm=0.7)
    steps = [[torch.zeros(b.shape) if it % 2 == 0 else torch.randn(b.shape, generator=gen) for b in base] for it in range(4)]
    worst, _ = _against_model(opt, model, ps, steps)
    assert all(bool(torch.isfinite(p).all()) for p in ps)
    for p in ps:
        p.grad = torch.zeros_like(p)
    before = [p.detach().clone() for p in ps]
    assert float(opt.step()) == 0.0
    assert all(not torch.equal(p.detach(), q) for p, q in zip(ps, before))        # (weight decay and the first moment still act)
    print('all-zero gradient steps: at most %.3f of the near() bound' % worst)


def test_loaded_step_counts_beyond_the_bias_corrections():
    """B5 (e): a checkpoint with ``step`` = 100 000 for one tensor (0.9^k and 0.99^k vanish: both bias corrections are 1 in
    fp32) and 3 for the other, then two steps: each tensor keeps its own count."""
    opt_mod = pkg('optim')
    gen = torch.Generator(device='cpu').manual_seed(109)
    base = [torch.randn(s, generator=gen) for s in [(33000,), (17, 5)]]
    ps = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    opt = opt_mod.ClipAdamW(ps, lr=3e-3, betas=BETAS, weight_decay=0.05, max_norm=0.7)
    model = AdamWModel([dict(params=base)], lr=3e-3, betas=BETAS, weight_decay=0.05, max_norm=0.7)
    grads = lambda: [torch.randn(b.shape, generator=gen) for b in base]
    _against_model(opt, model, ps, [grads()])
    sd = copy.deepcopy(opt.state_dict())
    sd['state'][0]['step'], sd['state'][1]['step'] = 100000, 3
    opt.load_state_dict(sd)
    model.k = [100000, 3]
    worst, worst_norm = _against_model(opt, model, ps, [grads(), grads()])
    assert [opt.state[p]['step'] for p in ps] == [100002, 5]
    print('step counts 100 000 and 3 from a checkpoint: norm %.2e relative, at most %.3f of the near() bound' % (worst_norm, worst))


# ------------------------------------------------------------------------------- the same through GraphedLiftStep
class _Mlp(torch.nn.Module):
    """(feats, w2p, org, gt) -> MSE of a two-Linear fp32 MLP: the call ``graphs.GraphedLiftStep`` makes, without a head."""

    def __init__(self):
        super().__init__()
        self.a, self.b = torch.nn.Linear(24, 32), torch.nn.Linear(32, 8)

    def forward(self, feats, w2p, org, gt):
        return torch.nn.functional.mse_loss(self.b(torch.relu(self.a(feats))), gt)


@pytest.mark.parametrize('set_to_none', [False, True])
def test_graphed_lift_step_with_eager_steps_in_between(set_to_none):
    """B6: two identical models take eight steps on alternating inputs -- one eagerly, one as GraphedLiftStep's warm-up step,
    then ``replay, eager, replay, eager, replay, eager, replay`` with ``zero_grad(set_to_none=...)``, backward, ``step()`` as
    the eager step.  The criterion of test_graphed_lift_step_replays_the_eager_training_steps in fp32: the relative L2
    difference of each parameter's total update below 0.05, losses 1e-5 relative.

    With ``set_to_none=False`` the gradients stay in the capture's own buffers for good, which is also what a replay leaves
    in the device table: that case passed before the fix (both distances 0).  With ``set_to_none=True`` every eager step
    frees its gradients and the caching allocator hands the same blocks to the next one -- the second and third eager step
    then found the host record unchanged and read the buffers of the previous replay: two of the seven updates used the
    other batch's gradients (before the fix: 0.226 for the worst parameter update, 7.6e-3 for the worst loss)."""
    graphs, opt_mod = pkg('graphs'), pkg('optim')
    torch.manual_seed(110)
    base = _Mlp().to(DEV)
    models = [base, copy.deepcopy(base)]
    before = [p.detach().clone() for p in base.parameters()]
    gen = torch.Generator(device='cpu').manual_seed(111)
    ins = [(torch.randn(16, 24, generator=gen).to(DEV), torch.zeros(1, 6, 4, 4, device=DEV), torch.zeros(1, 3, device=DEV),
            torch.randn(16, 8, generator=gen).to(DEV)) for _ in range(2)]
    opts = [opt_mod.ClipAdamW(list(m.parameters()), lr=1e-3, weight_decay=0.01, max_norm=35.0) for m in models]

    def eager(k, it):
        opts[k].zero_grad(set_to_none=set_to_none)
        loss = models[k](*ins[it % 2])
        loss.backward()
        opts[k].step()
        return float(loss)
    losses = [[eager(0, it) for it in range(8)], []]
    step = graphs.GraphedLiftStep(models[1], opts[1], *ins[0], warmup=1)          # = step 0, eagerly, then the capture
    for it in range(1, 8):
        losses[1].append(float(step(*ins[it % 2])) if it % 2 else eager(1, it))
    assert all(opts[1].state[p]['step'] == 8 for p in models[1].parameters())
    worst = 0.0
    for p, q, b in zip(models[0].parameters(), models[1].parameters(), before):
        d_e, d_g = (p.detach() - b).double(), (q.detach() - b).double()
        assert float(d_e.norm()) > 0
        worst = max(worst, float((d_e - d_g).norm() / d_e.norm()))
    worst_loss = max(abs(a - b) / abs(a) for a, b in zip(losses[0][1:], losses[1]))
    print('GraphedLiftStep with eager steps in between, set_to_none=%s: worst relative difference of a parameter update '
          '%.3e (bound 0.05), of a loss %.3e (bound 1e-5)' % (set_to_none, worst, worst_loss))
    assert worst < 0.05, worst
    assert worst_loss <= 1e-5, (losses[0][1:], losses[1])
    assert losses[0][1] != losses[0][3]                                # (the steps do move the loss)
