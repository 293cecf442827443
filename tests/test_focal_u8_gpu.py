"""Byte labels through the separate focal-loss passes on the GPU: ``ver_focal_loss_forward_u8`` / ``_backward_u8`` and their
``_cw`` forms against the int64 entries on the same labels (further instantiations of the same kernels: partials and
gradients BIT-identical, the NaN sum and the flag of an out-of-range label included), ``FocalLoss`` on uint8 targets
against itself on the widened ones, and ``head.occupancy_loss`` on an ``OccupancyTargets`` against the dense int64 route,
with no int64 tensor of label size in between."""
import ctypes

import numpy as np
import pytest
import torch

import cases
from util import pkg

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def hip():
    return pkg('hipops')


def bits(t):
    """The tensor's bytes as integers: equality of these is bit identity (NaN payloads and signed zeros included)."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _labels(n, c, spoil, gen):
    """int64 [n]: every class and the empty label ``c`` wherever n allows it, in random order; ``spoil``: one label is 255
    (a wrapped -1: outside [0, c] for both label types)."""
    lab = (torch.arange(n) % (c + 1))[torch.randperm(n, generator=gen)]
    if spoil:
        lab[n // 2] = 255
    return lab


@pytest.mark.parametrize('spoil', [False, True], ids=['clean', 'out_of_range'])
@pytest.mark.parametrize('n', [1, 255, 256, 4099])
@pytest.mark.parametrize('c', [8, 16])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_u8_entries_equal_the_int64_entries_bit_for_bit(dtype, c, n, spoil):
    L = hip().lib()
    p, st = hip()._p, hip()._stream
    gen = torch.Generator().manual_seed(1000 * c + n)
    logits = (torch.randn(n, c, generator=gen) * 3).to(dtype).to(DEV)
    lab = _labels(n, c, spoil, gen)
    if n >= c + 1:
        assert sorted(set(lab.tolist()) - {255}) == list(range(c + 1)) or spoil
    table = (torch.rand(c + 1, generator=gen) * 2 + 0.25).to(DEV)
    scale = torch.tensor([0.37], device=DEV)
    dt = 1 if dtype == torch.bfloat16 else 0
    blocks = L.ver_focal_loss_blocks(ctypes.c_long(n), c)
    assert blocks == (n * (c // 8) + 255) // 256               # more than one workgroup at 4099 rows
    tail = (ctypes.c_long(n), c, ctypes.c_float(2.0), ctypes.c_float(0.25), dt)
    results = {}
    for kind, target in (('i64', lab.to(DEV)), ('u8', lab.to(torch.uint8).to(DEV))):
        u8 = '_u8' if kind == 'u8' else ''
        out = []
        for cw in (False, True):
            suffix = u8 + ('_cw' if cw else '')
            extra = (p(table),) if cw else ()
            partial = torch.full((blocks,), -7.0, device=DEV)
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            grad = torch.full_like(logits, 9.0)
            rc = getattr(L, 'ver_focal_loss_forward' + suffix)(p(logits), p(target), *extra, p(partial), *tail, p(flag), st())
            assert rc == 0, L.ver_last_error()
            rc = getattr(L, 'ver_focal_loss_backward' + suffix)(p(logits), p(target), *extra, p(scale), p(grad), *tail, st())
            assert rc == 0, L.ver_last_error()
            out += [partial, flag, grad]
        torch.cuda.synchronize()
        results[kind] = out
    for name, a, b in zip(('partial', 'flag', 'grad', 'partial_cw', 'flag_cw', 'grad_cw'), results['u8'], results['i64']):
        assert torch.equal(bits(a), bits(b)), name
    partial, flag, grad = results['u8'][:3]
    assert int(flag) == int(spoil) and bool(torch.isnan(partial.sum())) == spoil
    assert float(grad.float().abs().max()) > 0 and bool((grad != 9.0).all())      # written in full
    assert not torch.equal(bits(results['u8'][5]), bits(grad))                     # (the table does weigh)


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'class_weight'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_focal_loss_module_on_bytes_equals_itself_on_widened_labels(dtype, weighted):
    pkg()
    fl = pkg('dense_heads.losses').FocalLoss(use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.5).to(DEV)
    gen = torch.Generator().manual_seed(5)
    n, c = 4099, 16                                             # (the fused path starts at 4096 rows)
    lab = _labels(n, c, False, gen)
    table = (torch.rand(c + 1, generator=gen) * 2 + 0.25).to(DEV) if weighted else None
    avg = float((lab < c).sum())
    base = (torch.randn(n, c, generator=gen) * 3).to(dtype).to(DEV)
    launched = []
    timer = hip().KernelTimer()
    out = []
    for target in (lab.to(DEV), lab.to(torch.uint8).to(DEV)):
        pred = base.clone().requires_grad_(True)
        hip().KERNEL_TIMER = timer
        try:
            loss = fl(pred, target, avg_factor=avg, class_weight=table)
            loss.backward()
        finally:
            hip().KERNEL_TIMER = None
        out.append((loss.detach(), pred.grad))
        launched.append([r[0] for r in timer.records])
        timer.records.clear()
    cw = '_cw' if weighted else ''
    assert launched[0] == ['ver_focal_loss_forward' + cw, 'ver_focal_loss_backward' + cw]
    assert launched[1] == ['ver_focal_loss_forward_u8' + cw, 'ver_focal_loss_backward_u8' + cw]
    assert torch.equal(bits(out[0][0]), bits(out[1][0])) and torch.equal(bits(out[0][1]), bits(out[1][1]))
    assert float(out[0][0]) > 0 and float(out[0][1].float().abs().max()) > 0
    # a call the kernels are not built for (an element weight) takes the torch formulas on the widened bytes
    small = fl(base[:64].float(), lab[:64].to(torch.uint8).to(DEV), weight=torch.ones(64, device=DEV), avg_factor=avg)
    want = fl(base[:64].float(), lab[:64].to(DEV), weight=torch.ones(64, device=DEV), avg_factor=avg)
    assert float(small) == float(want)
    hip().LabelRangeFlag.of(DEV).poll(sync=True)


@pytest.mark.parametrize('order', ['rows', 'voxels'])
def test_occupancy_loss_on_device_targets_equals_the_dense_route_without_an_int64_copy(order):
    """``head.occupancy_loss`` with the ``OccupancyTargets`` of ``occupancy_targets_device`` against the dense int64 labels
    of ``occupancy_targets``: the same loss and the same gradient bit for bit; ``FocalLoss`` is handed the bytes, and the
    call allocates less than one int64 per label (the widening copy alone was 8 bytes per label)."""
    pkg()
    torch.manual_seed(0)
    head = pkg('registry').build_head(cases.vocc_head_cfg()).to(DEV)
    nvox, c = head.voxel_num, head.occupancy_classes
    rng = np.random.default_rng(11)
    vox = rng.choice(nvox, size=30000, replace=False)
    pairs = np.stack([vox, np.arange(30000) % c], axis=1).astype(np.int64)
    plan = head.occupancy_row_plan(DEV) if order == 'rows' else None
    gen = torch.Generator().manual_seed(3)
    if order == 'rows':
        assert plan is not None
        logits = torch.randn(plan.rows, head.occ_zdim, c, generator=gen).bfloat16().to(DEV)
        form = lambda t: (t, plan, 1)
    else:
        logits = torch.randn(1, nvox, c, generator=gen).bfloat16().to(DEV)
        form = lambda t: t
    dense = head.occupancy_targets([pairs], device=DEV)
    assert dense.dtype == torch.int64 and tuple(dense.shape) == (1, nvox)
    targets = head.occupancy_targets_device([pairs], rows=order == 'rows', device=DEV)
    assert targets.labels.dtype == torch.uint8 and targets.order == order and int(targets.count[-1]) == 30000
    seen = []
    inner = head.loss_occupancy.forward
    head.loss_occupancy.forward = lambda pred, target, *a, **k: (seen.append((target.dtype, target.numel())), inner(pred, target, *a, **k))[1]
    results = []
    for gt in (dense, targets):
        pred = logits.clone().requires_grad_(True)
        loss = head.occupancy_loss(form(pred), gt)
        loss.backward()
        results.append((loss.detach(), pred.grad))
    assert seen == [(torch.int64, nvox), (torch.uint8, nvox)]
    assert torch.equal(bits(results[0][0]), bits(results[1][0])) and torch.equal(bits(results[0][1]), bits(results[1][1]))
    assert float(results[0][0]) > 0
    # allocation of the call on the device targets, without autograd: partial sums and scalars, nothing of label size
    with torch.no_grad():
        head.occupancy_loss(form(logits), targets)              # (one-time allocations: the flag, its pinned mirror)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        head.occupancy_loss(form(logits), targets)
        torch.cuda.synchronize()
        grew = torch.cuda.max_memory_allocated() - before
    print('occupancy_loss on device targets (%s): peak allocation %d bytes for %d labels' % (order, grew, nvox))
    assert grew < nvox, grew                                    # less than one BYTE per label; int64 labels are 8
    hip().LabelRangeFlag.of(DEV).poll(sync=True)
