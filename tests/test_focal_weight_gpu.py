"""Class-weighted occupancy focal loss on the device: the ``_cw`` entries of ver_loss.hip, the two autograd Functions that
carry a ``class_weight`` table, and the head's three loss routes with ``occ_weights``.

The model (tests/focal_weight_helper.py): the formula of ``oracle.ver_oracle.focal_loss`` in float64 on
the dtype-rounded logits times ``class_weight[target][:, None]``.  Bounds: those of
tests/test_hip_ops_gpu.py::test_focal_loss_fused -- loss 1e-5 relative, gradients rtol 1e-4 (fp32) / 1e-2 (bf16), atol 1e-9."""
import ctypes

import numpy as np
import pytest
import torch

import cases
from focal_weight_helper import model_elements, weights_for
from util import close, pkg, rel_l2

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda'


def _model(logits, target, w, gamma, alpha, scale):
    """(float64 loss sum * scale, its gradient) on the logits as the kernel reads them."""
    lr = logits.detach().double().requires_grad_(True)
    s = model_elements(lr, target, w, gamma, alpha).sum() * scale
    s.backward()
    return float(s), lr.grad


@pytest.mark.parametrize('C', [8, 16, 24])                     # 24: three vectors per row, the division form of row_of
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('gamma,alpha', [(2.0, 0.25), (1.5, 0.4)])
def test_weighted_focal_loss_equals_the_model(C, dtype, gamma, alpha):
    hip = pkg('hipops')
    gen = torch.Generator(device='cpu').manual_seed(10 + C)
    n = 70001
    logits = (torch.randn(n, C, generator=gen) * 4).to(dtype)
    logits[0, :4] = torch.tensor([60.0, -60.0, 0.0, 20.0]).to(dtype)      # saturated sigmoid both ways
    target = torch.randint(0, C + 1, (n,), generator=gen)
    target[0] = 0
    w = weights_for(C, C)
    avg = float((target < C).sum())
    scale = 0.7 / avg
    ld = logits.to(DEV).requires_grad_(True)
    wd = w.to(DEV)
    s = hip.sigmoid_focal_loss_sum(ld, target.to(DEV), gamma, alpha, class_weight=wd)
    (s * scale).backward()
    want, want_grad = _model(logits, target, w, gamma, alpha, scale)
    assert abs(float(s) * scale - want) <= 1e-5 * abs(want), (float(s) * scale, want)
    assert ld.grad.dtype == dtype and wd.grad is None
    assert close(ld.grad.float().cpu(), want_grad, atol=1e-9, rtol=1e-4 if dtype == torch.float32 else 1e-2)
    assert int((target == 3).sum()) > 0 and bool((ld.grad[(target == 3).to(DEV)] == 0).all())   # the zero-weight class
    # the registered loss routes a large GPU input with a table through the same kernels
    got = pkg('dense_heads.losses').FocalLoss(gamma=gamma, alpha=alpha, loss_weight=0.7)(
        logits.to(DEV), target.to(DEV), avg_factor=avg, class_weight=wd)
    assert abs(float(got) - want) <= 1e-5 * abs(want)
    # one row, no row
    l1 = logits[:1].to(DEV).requires_grad_(True)
    s1 = hip.sigmoid_focal_loss_sum(l1, target[:1].to(DEV), gamma, alpha, class_weight=wd)
    s1.backward()
    want1, grad1 = _model(logits[:1], target[:1], w, gamma, alpha, 1.0)
    assert abs(float(s1) - want1) <= 1e-5 * abs(want1)
    assert close(l1.grad.float().cpu(), grad1, atol=1e-9, rtol=1e-4 if dtype == torch.float32 else 1e-2)
    l0 = torch.zeros(0, C, device=DEV, dtype=dtype, requires_grad=True)
    s0 = hip.sigmoid_focal_loss_sum(l0, torch.zeros(0, dtype=torch.long, device=DEV), gamma, alpha, class_weight=wd)
    assert float(s0) == 0.0
    s0.backward()
    assert l0.grad.shape == (0, C)
    # the table is checked, not converted
    for bad in (wd[:-1], wd.double(), w, torch.ones(2 * (C + 1), device=DEV)[::2]):
        with pytest.raises((ValueError, TypeError)):
            hip.sigmoid_focal_loss_sum(ld, target.to(DEV), gamma, alpha, class_weight=bad)


def _fwd_args(hip, x, labels, table, partial, grad, n, c, gamma, dt, flag):
    head = (hip._p(x), hip._p(labels)) + (() if table is None else (hip._p(table),))
    return head + (hip._p(partial), hip._p(grad), ctypes.c_long(n), c, ctypes.c_float(gamma), ctypes.c_float(0.25), dt,
                   hip._p(flag), hip._stream())


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('gamma', [2.0, 1.5])
def test_a_table_of_ones_is_the_unweighted_kernel_bit_for_bit(dtype, gamma):
    """``ver_focal_loss_forward_grad`` / ``_u8`` and their ``_cw`` twins with w = 1 through the C ABI, as
    tests/test_hip_ops_gpu.py::test_focal_forward_grad_with_byte_labels_is_bit_identical calls them: the same partials and
    the same gradient buffer, written in place (``grad == logits``) or beside the logits."""
    hip = pkg('hipops')
    L = hip.lib()
    gen = torch.Generator(device='cpu').manual_seed(57)
    n, c = 100003, 16
    dt = 1 if dtype == torch.bfloat16 else 0
    logits = (torch.randn(n, c, generator=gen) * 2).to(dtype).to(DEV)
    lab = torch.randint(0, c + 1, (n,), generator=gen)
    ones = torch.ones(c + 1, device=DEV)
    blocks = L.ver_focal_loss_blocks(ctypes.c_long(n), c)
    res = {}
    for name, labels, table in (('i64', lab.to(DEV), None), ('i64_cw', lab.to(DEV), ones),
                                ('u8', lab.to(torch.uint8).to(DEV), None), ('u8_cw', lab.to(torch.uint8).to(DEV), ones)):
        entry = getattr(L, 'ver_focal_loss_forward_grad' + ('_u8' if name.startswith('u8') else '') + ('_cw' if table is not None else ''))
        for in_place in (True, False):
            x = logits.clone()
            grad = x if in_place else torch.empty_like(x)
            partial = torch.zeros(blocks, dtype=torch.float32, device=DEV)
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            assert entry(*_fwd_args(hip, x, labels, table, partial, grad, n, c, gamma, dt, flag)) == 0
            assert int(flag) == 0
            assert in_place or torch.equal(x, logits)
            res[name, in_place] = (partial, grad)
    ref = res['i64', False]
    assert float(ref[0].sum()) > 0 and float(ref[1].float().abs().max()) > 0
    for key, (partial, grad) in res.items():
        assert torch.equal(partial, ref[0]) and torch.equal(grad, ref[1]), key
    # ... and so is the loss-only forward
    labels, scale = lab.to(DEV), torch.full((1,), 0.37, device=DEV)
    p0, p1 = (torch.zeros(blocks, dtype=torch.float32, device=DEV) for _ in range(2))
    g0, g1 = torch.empty_like(logits), torch.empty_like(logits)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    tail = (ctypes.c_long(n), c, ctypes.c_float(gamma), ctypes.c_float(0.25), dt)
    assert L.ver_focal_loss_forward(hip._p(logits), hip._p(labels), hip._p(p0), *tail, hip._p(flag), hip._stream()) == 0
    assert L.ver_focal_loss_forward_cw(hip._p(logits), hip._p(labels), hip._p(ones), hip._p(p1), *tail, hip._p(flag), hip._stream()) == 0
    assert L.ver_focal_loss_backward(hip._p(logits), hip._p(labels), hip._p(scale), hip._p(g0), *tail, hip._stream()) == 0
    assert L.ver_focal_loss_backward_cw(hip._p(logits), hip._p(labels), hip._p(ones), hip._p(scale), hip._p(g1), *tail, hip._stream()) == 0
    assert torch.equal(p0, p1) and int(flag) == 0
    # (the separate backward multiplies by the incoming scalar as well; the compiler contracts that product chain
    #  differently around a per-row factor than around two constants, so its twins agree at the gradient bounds, not in bits)
    assert close(g1.float().cpu(), g0.float().cpu(), atol=1e-9, rtol=1e-4 if dtype == torch.float32 else 1e-2)


def test_both_loops_of_the_weighted_kernel():
    """2 200 003 rows of 16 bf16 logits: 4 400 006 vectors > 4 x 4096 x 256, so the four-in-flight loop AND its tail run.
    With a 0/1 table the weighted gradient is the unweighted one times the row's factor, exactly."""
    hip = pkg('hipops')
    L = hip.lib()
    n, c = 2200003, 16
    gen = torch.Generator(device=DEV).manual_seed(3)
    logits = (torch.randn(n, c, generator=gen, device=DEV) * 2).bfloat16()
    lab = torch.randint(0, c + 1, (n,), generator=gen, device=DEV)
    lab8 = lab.to(torch.uint8)
    w = T(np.random.default_rng(8).integers(0, 2, c + 1).astype(np.float32)).to(DEV)
    w[0], w[c] = 1.0, 0.0
    blocks = L.ver_focal_loss_blocks(ctypes.c_long(n), c)
    assert blocks == 4096 and n * (c // 8) > 4 * 4096 * 256
    out = {}
    for table in (None, w):
        entry = L.ver_focal_loss_forward_grad_u8 if table is None else L.ver_focal_loss_forward_grad_u8_cw
        grad = torch.empty_like(logits)
        partial = torch.zeros(blocks, dtype=torch.float32, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        assert entry(*_fwd_args(hip, logits, lab8, table, partial, grad, n, c, 2.0, 1, flag)) == 0
        assert int(flag) == 0
        out[table is None] = (partial, grad)
    assert torch.equal(out[False][1], (out[True][1].float() * w[lab][:, None]).bfloat16())
    want = float(model_elements(logits, lab, w).sum())                    # float64, on the device
    got = float(out[False][0].double().sum())
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    assert abs(float(out[True][0].double().sum()) - want) > 1e-2 * abs(want)


def test_a_bad_label_never_indexes_the_table():
    """One 23 among int64 labels, one 255 among byte labels: the sum is NaN, the device flag is raised, the call returns."""
    hip = pkg('hipops')
    gen = torch.Generator(device='cpu').manual_seed(12)
    n = 8192
    logits = torch.randn(n, 16, generator=gen).bfloat16().to(DEV)
    good = torch.randint(0, 17, (n,), generator=gen)
    w = weights_for(16, 2).to(DEV)
    p = [torch.randn(s, generator=gen).to(DEV) * 0.1 for s in ((128,), (128,), (128, 128), (128,), (128,), (128,), (16, 128), (16,))]
    x = torch.randn(n, 128, generator=gen).bfloat16().to(DEV)
    flag = hip.LabelRangeFlag.of(torch.device(DEV))
    flag.reset()
    try:
        assert bool(torch.isfinite(hip.sigmoid_focal_loss_sum(logits, good.to(DEV), class_weight=w)))
        flag.poll(sync=True)
        bad = good.clone()
        bad[4321] = 23
        s = hip.sigmoid_focal_loss_sum(logits, bad.to(DEV), class_weight=w)
        assert bool(torch.isnan(s))
        with pytest.raises(RuntimeError, match='outside'):
            flag.poll(sync=True)
        flag.reset()
        bad8 = good.to(torch.uint8)
        bad8[77] = 255
        s = hip.occ_mlp_focal_loss_sum(x, *p, bad8.to(DEV), class_weight=w)          # the byte path: _u8_cw
        assert bool(torch.isnan(s))
        with pytest.raises(RuntimeError, match='outside'):
            flag.poll(sync=True)
    finally:
        flag.reset()


def test_fused_mlp_route_carries_the_table():
    """``occ_mlp_focal_loss_sum(..., class_weight=w)`` against ``occ_mlp`` + ``sigmoid_focal_loss_sum(..., class_weight=w)``:
    shapes and bounds of tests/test_hip_ops_gpu.py::test_occ_mlp_focal_loss_fused_equals_the_two_ops."""
    hip = pkg('hipops')
    gen = torch.Generator(device='cpu').manual_seed(5)
    p = dict(g1=torch.randn(128, generator=gen) * 0.3 + 1.0, be1=torch.randn(128, generator=gen) * 0.3,
             w2=torch.randn(128, 128, generator=gen) * 0.12, b2=torch.randn(128, generator=gen) * 0.3,
             g2=torch.randn(128, generator=gen) * 0.3 + 1.0, be2=torch.randn(128, generator=gen) * 0.3,
             w3=torch.randn(16, 128, generator=gen) * 0.12, b3=torch.randn(16, generator=gen) * 0.3)
    n = 64 * 400 + 9
    a1 = (torch.randn(n, 128, generator=gen) * 1.5).bfloat16()
    tgt = torch.randint(0, 17, (n,), generator=gen)
    w = weights_for(16, 9).to(DEV)
    keys = ('g1', 'be1', 'w2', 'b2', 'g2', 'be2', 'w3', 'b3')
    res = {}
    for route in ('fused_u8', 'fused_i64', 'two_ops', 'fused_unweighted'):
        pd = {k: p[k].to(DEV).requires_grad_(True) for k in keys}
        xd = a1.to(DEV).requires_grad_(True)
        if route == 'two_ops':
            s = hip.sigmoid_focal_loss_sum(hip.occ_mlp(xd, None, None, *(pd[k] for k in keys)), tgt.to(DEV), class_weight=w)
        else:
            labels = tgt.to(torch.uint8) if route == 'fused_u8' else tgt
            s = hip.occ_mlp_focal_loss_sum(xd, *(pd[k] for k in keys), labels.to(DEV),
                                           class_weight=None if route == 'fused_unweighted' else w)
        (s * 0.37 / 1234.0).backward()
        res[route] = (float(s), xd.grad.float().cpu(), {k: v.grad.float().cpu() for k, v in pd.items()})
    assert res['fused_u8'][0] == res['two_ops'][0] == res['fused_i64'][0]
    assert abs(res['fused_unweighted'][0] - res['two_ops'][0]) > 1e-2 * abs(res['two_ops'][0])
    for route in ('fused_u8', 'fused_i64'):
        assert rel_l2(res[route][1], res['two_ops'][1]) < 1e-2
        for k in keys:
            assert rel_l2(res[route][2][k], res['two_ops'][2][k]) < 1e-2, (route, k)


def _head(cfg, seed):
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    pkg()
    h = pkg('registry').build_head(cfg).eval()
    code_weights = h.code_weights.detach().clone()
    pkg('synthetic').load_seeded(h, seed)
    h.code_weights.data.copy_(code_weights)
    return h.to(DEV)


OCC_WEIGHTS = [round(float(v), 4) for v in weights_for(16, 5)]


@pytest.mark.parametrize('autocast', [False, True])
def test_head_routes_carry_occ_weights(autocast):
    """tests/test_head_gpu.py::test_occupancy_loss_in_row_order_equals_voxel_order with ``class_weights=True``: the row-order
    route (under autocast: the fused MLP + loss Function) against the voxel-order one, and the voxel-order loss against the
    float64 model of its own logits."""
    syn = pkg('synthetic')
    w2p, org = syn.camera_batch(2, seed=1)
    feats = T(syn.vit_features(2, seed=0)).to(DEV).permute(1, 0, 2, 3).contiguous()
    gt = T(np.random.default_rng(5).integers(0, 17, size=(2, 504000))).to(DEV)
    head = _head(dict(cases.vocc_head_cfg(), occ_weights=list(OCC_WEIGHTS)), 7).train()
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    res = {}
    for route in ('voxels', 'rows', 'rows_unweighted'):
        head.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
            emb = head(feats, None, only_bev=True, world2pixel=T(w2p).to(DEV), origin=T(org).to(DEV))
            if route == 'rows':
                loss = head.occupancy_loss_from_volume(emb, gt, class_weights=True)
            elif route == 'rows_unweighted':
                loss = head.occupancy_loss_from_volume(emb, gt)
            else:
                logits = head.occupancy_from_volume(emb)
                loss = head.occupancy_loss(logits, gt, class_weights=True)
        if route != 'rows_unweighted':
            loss.backward()
        res[route] = (float(loss), {k: p.grad.float().cpu() for k, p in head.named_parameters() if p.grad is not None})
    assert abs(res['rows'][0] - res['voxels'][0]) <= 1e-5 * abs(res['voxels'][0]), (res['rows'][0], res['voxels'][0])
    assert set(res['rows'][1]) == set(res['voxels'][1]) and res['voxels'][1]
    for k, g in res['voxels'][1].items():
        assert rel_l2(res['rows'][1][k], g) < (1.5e-2 if autocast else 1e-5), k
    flat = logits.detach().reshape(-1, 16)
    want = float(model_elements(flat, gt.reshape(-1), torch.tensor(OCC_WEIGHTS, device=DEV)).sum() / (gt < 16).sum())
    assert abs(res['voxels'][0] - want) <= 1e-5 * abs(want), (res['voxels'][0], want)
    assert abs(res['rows_unweighted'][0] - want) > 1e-2 * abs(want)
    assert len(head.state_dict()) == 341 and not any(b.numel() == 17 for b in head.buffers())


def test_loss_only_occupancy_is_weighted_on_the_device():
    head = _head(dict(cases.vocc_head_cfg(only_occ=True), occ_weights=list(OCC_WEIGHTS)), 7)
    gen = torch.Generator(device='cpu').manual_seed(11)
    logits = torch.randn(1, 8192, 16, generator=gen).to(DEV).requires_grad_(True)
    gt = torch.randint(0, 17, (1, 8192), generator=gen).to(DEV)
    w = torch.tensor(OCC_WEIGHTS, device=DEV)
    out = head.loss_only_occupancy(None, None, gt, dict(occupancy_preds=logits))
    avg = float((gt < 16).sum())
    want, want_grad = _model(logits[0], gt[0], w, 2.0, 0.25, 1.0 / avg)
    plain = float(model_elements(logits[0].detach(), gt[0], torch.ones(17, device=DEV)).sum() / avg)
    assert float(out['loss_occupancy']) == pytest.approx(want, rel=1e-5)
    assert abs(float(out['loss_occupancy']) - plain) > 1e-2 * abs(plain)
    assert float(out['loss_flow']) == 0.0
    out['loss_occupancy'].backward()
    assert close(logits.grad[0].cpu(), want_grad.cpu(), atol=1e-9, rtol=1e-4)
    # the table is a cached constant: the same tensor on every step (no copy per step)
    assert head.class_weight_table(True, logits.device) is head.class_weight_table(True, logits.device)
    head.occ_weights = None
    assert float(head.loss_only_occupancy(None, None, gt, dict(occupancy_preds=logits))['loss_occupancy']) == pytest.approx(plain, rel=1e-5)


def test_weighted_loss_and_backward_are_capturable():
    """Weighted ``sigmoid_focal_loss_sum`` + backward on static [8192, 16] logits in ONE ``torch.cuda.graph`` after an eager
    warm-up; the table is read on the device at replay time: overwritten in place, the next replay follows it."""
    hip = pkg('hipops')
    gen = torch.Generator(device='cpu').manual_seed(21)
    static = (torch.randn(8192, 16, generator=gen) * 2).to(DEV).requires_grad_(True)
    target = torch.randint(0, 17, (8192,), generator=gen).to(DEV)
    tables = [weights_for(16, 31).to(DEV), weights_for(16, 32).to(DEV)]
    table = tables[0].clone()

    def step(x, w):
        s = hip.sigmoid_focal_loss_sum(x, target, 2.0, 0.25, class_weight=w)
        g, = torch.autograd.grad(s * 0.5, [x])
        return [s, g]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static, table)                                  # warm-up outside the capture (library handle, the label flag)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step(static, table)
    for w in (tables[0], tables[1], tables[0]):
        table.copy_(w)
        want = step(static.detach().clone().requires_grad_(True), w)
        for replay in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for got, ref in zip(static_out, want):
                assert torch.equal(got, ref), replay
    assert not torch.equal(step(static, tables[0])[1], step(static, tables[1])[1])
    hip.LabelRangeFlag.of(torch.device(DEV)).poll(sync=True)
