"""Class-weighted occupancy focal loss (``occ_weights`` -> ``class_weight``) on the CPU: the torch path of ``FocalLoss``,
the head's ``loss_only_occupancy`` (head:1417-1425 of the reference), the routes that must NOT read the table, and the
argument checks of the four ``_cw`` C entries.

The model (tests/focal_weight_helper.py): the formula of ``oracle.ver_oracle.focal_loss`` in float64 times
``class_weight[target][:, None]``."""
import ctypes

import numpy as np
import pytest
import torch

import cases
from focal_weight_helper import model_elements, weights_for
from util import golden, maxdiff, pkg


@pytest.mark.parametrize('C', [16, 24])
def test_focal_loss_class_weight_equals_the_model(C):
    pkg()
    losses = pkg('dense_heads.losses')
    gen = torch.Generator().manual_seed(C)
    n = 257
    pred = (torch.randn(n, C, generator=gen) * 3).requires_grad_(True)
    target = torch.randint(0, C + 1, (n,), generator=gen)
    target[:C + 1] = torch.arange(C + 1)                       # every label value, the empty one included
    w = weights_for(C, C)
    avg = float((target < C).sum())
    fl = losses.FocalLoss(use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0)
    got = fl(pred, target, avg_factor=avg, class_weight=w)
    ref_in = pred.detach().double().requires_grad_(True)
    want = model_elements(ref_in, target, w).sum() / avg
    assert float(got) == pytest.approx(float(want), rel=1e-6)
    got.backward()
    want.backward()
    assert maxdiff(pred.grad, ref_in.grad) < 1e-6
    assert bool((pred.grad[target == 3] == 0).all())
    # the mmdet spelling of the same thing: an [N] element weight
    same = fl(pred.detach(), target, weight=w[target], avg_factor=avg)
    assert float(same) == pytest.approx(float(got), rel=1e-6)
    # both at once multiply
    both = fl(pred.detach(), target, weight=torch.full((n,), 2.0), avg_factor=avg, class_weight=w)
    assert float(both) == pytest.approx(2 * float(got), rel=1e-6)
    # a bad label raises as it does without a table; it is never used as an index
    bad = target.clone()
    bad[5] = C + 7
    with pytest.raises(RuntimeError):
        fl(pred.detach(), bad, avg_factor=avg, class_weight=w)
    with pytest.raises(ValueError, match='class_weight'):
        fl(pred.detach(), target, avg_factor=avg, class_weight=w[:-1])


OCC_WEIGHTS = [round(float(v), 4) for v in weights_for(16, 5)]


@pytest.fixture(scope='module')
def head():
    pkg()
    h = pkg('registry').build_head(dict(cases.vocc_head_cfg(), train_cfg=cases.VOCC_TRAIN_CFG, occ_weights=list(OCC_WEIGHTS)))
    pkg('synthetic').load_seeded(h, 7)
    return h.eval()


def test_loss_only_occupancy_reads_occ_weights(head):
    """Fails without the feature: the table was stored and never read."""
    assert head.occ_weights == OCC_WEIGHTS
    gen = torch.Generator().manual_seed(11)
    logits = (torch.randn(1, head.voxel_num, 16, generator=gen) * 2).requires_grad_(True)
    gt = torch.randint(0, 17, (1, head.voxel_num), generator=gen)
    w = torch.tensor(OCC_WEIGHTS)
    avg = float((gt < 16).sum())
    ref_in = logits.detach()[0].double().requires_grad_(True)
    want = model_elements(ref_in, gt[0], w).sum() / avg
    plain = model_elements(ref_in.detach(), gt[0], torch.ones(17)).sum() / avg
    out = head.loss_only_occupancy(None, None, gt, dict(occupancy_preds=logits))
    assert sorted(out) == ['loss_flow', 'loss_occupancy'] and float(out['loss_flow']) == 0.0
    assert float(out['loss_occupancy']) == pytest.approx(float(want), rel=1e-5)
    assert abs(float(out['loss_occupancy']) - float(plain)) > 1e-2 * float(plain)
    out['loss_occupancy'].backward()
    want.backward()
    assert maxdiff(logits.grad[0], ref_in.grad) < 1e-9 + 1e-4 * float(ref_in.grad.abs().max())
    # the three spellings of the table agree; None is the unweighted loss
    a = head.occupancy_loss(logits.detach(), gt, class_weights=True)
    b = head.occupancy_loss(logits.detach(), gt, class_weights=list(OCC_WEIGHTS))
    c = head.occupancy_loss(logits.detach(), gt, class_weights=w)
    assert float(a) == float(b) == float(c) == float(out['loss_occupancy'])
    assert float(head.occupancy_loss(logits.detach(), gt)) == pytest.approx(float(plain), rel=1e-5)


def test_occ_weights_table_is_cached_validated_and_not_in_the_state_dict(head):
    g = golden('head_vocc')
    assert list(head.state_dict()) == [str(s) for s in g['sd_names']]          # the reference's 341 entries
    assert not any(b is not None and b.numel() == 17 for b in head.buffers())
    cpu = torch.device('cpu')
    t = head.class_weight_table(True, cpu)
    assert t.dtype == torch.float32 and t.tolist() == pytest.approx(OCC_WEIGHTS) and not t.requires_grad
    assert head.class_weight_table(True, cpu) is t                              # built once
    keep = head.occ_weights
    try:
        head.occ_weights = [1.0] * 17                                           # reassigned: another table
        t1 = head.class_weight_table(True, cpu)
        assert t1 is not t and t1.tolist() == [1.0] * 17
        head.occ_weights = None
        assert head.class_weight_table(True, cpu) is None
        logits = torch.zeros(1, head.voxel_num, 16)
        gt = torch.zeros(1, head.voxel_num, dtype=torch.long)
        for bad in ([1.0] * 16, [1.0] * 18, [1.0] * 16 + [float('nan')], [1.0] * 16 + [float('inf')]):
            head.occ_weights = bad
            with pytest.raises(ValueError, match='occ_weights'):
                head.loss_only_occupancy(None, None, gt, dict(occupancy_preds=logits))
        with pytest.raises(ValueError):
            head.occupancy_loss(logits, gt, class_weights=torch.ones(16))
    finally:
        head.occ_weights = keep


def test_loss_ignores_occ_weights_as_the_reference_does(head):
    """``loss`` (head:981) passes no weight to the occupancy FocalLoss: the dict is the same with and without a table."""
    T = torch.from_numpy
    gh = golden('head_vocc')
    g = golden('loss_vocc')
    boxes, labels = cases.detection_gt()
    logits, gt_occ = cases.occupancy_loss_inputs()
    preds = dict(all_cls_scores=T(gh['c3_b0_cls']), all_bbox_preds=T(gh['c3_b0_bbox']), occupancy_preds=T(logits)[None])
    with_table = head.loss([T(boxes)[:, :7]], [labels], T(gt_occ)[None], preds)
    keep = head.occ_weights
    try:
        head.occ_weights = None
        without = head.loss([T(boxes)[:, :7]], [labels], T(gt_occ)[None], preds)
    finally:
        head.occ_weights = keep
    assert sorted(with_table) == sorted(without)
    for k in without:
        assert float(with_table[k]) == float(without[k]), k
    assert float(with_table['loss_occupancy']) == pytest.approx(float(g['loss_occ']), rel=1e-5)


CW_ENTRIES = ('ver_focal_loss_forward_cw', 'ver_focal_loss_forward_grad_cw', 'ver_focal_loss_forward_grad_u8_cw',
              'ver_focal_loss_backward_cw')


def test_cw_entries_prototypes_and_argument_checks():
    hip = pkg('hipops')
    lib = hip.lib()
    i, l, f, ptr = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
    tail = [l, i, f, f, i]
    assert hip.PROTOTYPES['ver_focal_loss_forward_cw'] == (i, [ptr] * 4 + tail + [ptr, ptr])
    assert hip.PROTOTYPES['ver_focal_loss_forward_grad_cw'] == (i, [ptr] * 5 + tail + [ptr, ptr])
    assert hip.PROTOTYPES['ver_focal_loss_forward_grad_u8_cw'] == (i, [ptr] * 5 + tail + [ptr, ptr])
    assert hip.PROTOTYPES['ver_focal_loss_backward_cw'] == (i, [ptr] * 5 + tail + [ptr])
    # each twin's prototype with `class_weight` after `target`
    for name in CW_ENTRIES:
        ret, params = hip.PROTOTYPES[name[:-3]]
        assert hip.PROTOTYPES[name] == (ret, params[:2] + [ptr] + params[2:])
    assert lib.ver_abi_version() == 31 == hip.ABI_VERSION
    buf = torch.zeros(1024)                                    # host memory, 64-byte aligned; nothing is launched below
    p = buf.data_ptr()

    def call(name, n, c, table=p):
        fn = getattr(lib, name)
        common = (l(n), c, f(2.0), f(0.25), 0)
        if name == 'ver_focal_loss_forward_cw':
            return fn(p, p, table, p, *common, None, None)
        if name == 'ver_focal_loss_backward_cw':
            return fn(p, p, table, p, p, *common, None)
        return fn(p, p, table, p, p, *common, None, None)

    for name in CW_ENTRIES:
        assert call(name, 8, 10) == -2 and b'multiple of 8' in lib.ver_last_error(), name      # VER_EUNSUPPORTED
        assert call(name, 8, 256) == -2 and b'class weights' in lib.ver_last_error(), name
        assert call(name, 8, 16, table=None) == -1 and b'class_weight' in lib.ver_last_error(), name   # VER_EINVAL
        assert call(name, 0, 16) == 0, name
        assert call(name, 0, 16, table=None) == 0, name
        assert call(name, 0, 248) == 0, name                   # the largest table: 249 entries
