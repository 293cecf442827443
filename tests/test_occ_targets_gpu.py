"""``ver_occ_targets`` on the GPU against its numpy model (``hipops.occ_targets_host``): labels, counts and the two ``bad``
counters as integers, bit for bit -- and the head / detector routes that take an ``OccupancyTargets`` in place of the dense
tensor: the kernels behind them receive the same bytes and the same count, so losses, gradients and histograms computed
from one encoder output are identical."""
import inspect

import numpy as np
import pytest
import torch

import cases
from focal_weight_helper import weights_for
from occ_targets_helper import annotation, flat
from test_detector_cpu import _metas, _sparse, _store
from util import pkg

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda'
CLASSES = 16


def _run(gts, voxel_num, zdim, table=None, invalid=None, dtype=torch.int32, out=None, classes=CLASSES):
    """The kernel and the model on one annotation -> ((labels, count, bad) of the kernel as numpy, of the model)."""
    hip = pkg('hipops')
    pairs, off = flat(gts)
    inv = ioff = None
    if invalid is not None:
        inv, ioff = np.concatenate(invalid).astype(np.int64), np.concatenate([[0], np.cumsum([len(i) for i in invalid])]).astype(np.int32)
    want = hip.occ_targets_host(pairs, off, voxel_num, zdim, classes, None if table is None else table.cpu().numpy(), inv, ioff)
    got = hip.occ_targets(T(pairs).to(dtype).to(DEV), T(off).to(DEV), voxel_num, zdim, classes, table,
                          None if inv is None else T(inv).to(dtype).to(DEV), None if inv is None else T(ioff).to(DEV), out=out)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in got), want


def _same(got, want):
    for g, w, name in zip(got, want, ('labels', 'count', 'bad')):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, int((g != w).sum()) if g.shape == w.shape else (g.shape, w.shape))


@pytest.fixture(scope='module')
def small_plan():
    opl = pkg('dense_heads.occ_proj_lattice')
    plan = opl.get_plan(16, 4, 40, 48, torch.device(DEV, torch.cuda.current_device()))
    return plan, opl.row_table(plan, DEV)


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_row_order(small_plan, dtype):
    plan, table = small_plan
    bs, Z = 3, 35
    voxel_num = plan.rows * Z
    gts = annotation(np.random.default_rng(1), bs, voxel_num, 0.1)
    got, want = _run(gts, voxel_num, Z, table, dtype=dtype)
    _same(got, want)
    assert want[1].tolist() == [len(g) for g in gts] + [sum(len(g) for g in gts)] and want[2].tolist() == [0, 0]
    # ... and they are the bytes the dense chain hands the loss kernels
    opl = pkg('dense_heads.occ_proj_lattice')
    dense = torch.full((bs, voxel_num), CLASSES, dtype=torch.uint8)
    for b, g in enumerate(gts):
        dense[b, T(g[:, 0])] = T(g[:, 1]).to(torch.uint8)
    chain = opl.voxels_to_rows(dense.to(DEV).reshape(bs, Z, plan.rows).permute(0, 2, 1), plan, bs).reshape(-1)
    assert np.array_equal(got[0], chain.cpu().numpy())


@pytest.mark.parametrize('bs', [3, 1])
def test_voxel_order_with_a_partial_last_word(bs):
    voxel_num = 4099                                         # 12 297 (4 099) bytes: the last word of the buffer is a partial one
    gts = annotation(np.random.default_rng(2), bs, voxel_num, 0.3)
    gts[-1] = np.concatenate([gts[-1], [[voxel_num - 1, 7], [voxel_num - 2, 15], [voxel_num - 3, 0]]])     # (repeats may lose: the model says which)
    _same(*_run(gts, voxel_num, 1, dtype=torch.int64))


def test_every_byte_of_a_word_lands(small_plan):
    """All voxels of a sample listed once: in an order that puts the four bytes of every word into four lanes of one wave
    (lanes j, j + 16, j + 32, j + 48 of a 64-pair chunk), in random order, and in row order with Z = 35, where a word
    straddles two rows."""
    rng = np.random.default_rng(3)
    voxel_num = 16384
    j = np.arange(64)
    order = (np.arange(voxel_num // 64)[:, None] * 64 + ((j % 16) * 4 + j // 16)[None, :]).reshape(-1)
    assert np.array_equal(np.sort(order), np.arange(voxel_num)) and order[0] // 4 == order[16] // 4 == order[48] // 4
    cls = rng.integers(0, CLASSES, voxel_num)
    for idx in (order, rng.permutation(voxel_num)):
        got, want = _run([np.stack([idx, cls[idx]], 1)], voxel_num, 1)
        _same(got, want)
        assert np.array_equal(got[0], cls.astype(np.uint8)) and got[1].tolist() == [voxel_num] * 2
    plan, table = small_plan
    voxel_num = plan.rows * 35
    full = [np.stack([rng.permutation(voxel_num), rng.integers(0, CLASSES, voxel_num)], 1) for _ in range(2)]
    got, want = _run(full, voxel_num, 35, table)
    _same(got, want)
    assert int((got[0] == CLASSES).sum()) == 0


def test_repeated_listings():
    voxel_num = 4099
    rng = np.random.default_rng(4)
    base = annotation(rng, 2, voxel_num, 0.1)
    free = np.setdiff1d(np.arange(voxel_num), base[0][:, 0])
    same = np.stack([np.full(64, free[0]), np.full(64, 5)], 1)                       # 64 listings, one class
    every = np.stack([np.full(CLASSES, free[1]), rng.permutation(CLASSES)], 1)       # one voxel, all 16 classes
    mixed = np.concatenate([base[0], same, every])
    got, want = _run([mixed[rng.permutation(len(mixed))], base[1]], voxel_num, 1)
    _same(got, want)
    assert got[0][free[0]] == 5 and got[0][free[1]] == CLASSES - 1
    assert got[1].tolist() == [len(base[0]) + 2, len(base[1]), len(base[0]) + len(base[1]) + 2] and got[2].tolist() == [0, CLASSES - 1]


def test_rejected_pairs_touch_nothing_outside_the_buffer():
    hip = pkg('hipops')
    voxel_num, bs = 4099, 2
    total, guard = bs * voxel_num, 64
    padded = (total + 3) // 4 * 4
    base = annotation(np.random.default_rng(5), bs, voxel_num, 0.1)
    junk = np.array([[-1, 3], [voxel_num, 3], [2 ** 31 - 1, 0], [-2 ** 31, 0], [10, -1], [11, CLASSES + 1], [12, 2 ** 31 - 1]])
    gts = [np.concatenate([junk, base[0]]), np.concatenate([base[1], junk])]
    big = torch.full((guard + padded + guard,), 0xAB, dtype=torch.uint8, device=DEV)
    cnt = torch.full((8 + bs + 1 + 8,), -77, dtype=torch.int32, device=DEV)
    bad = torch.full((8 + 2 + 8,), -77, dtype=torch.int32, device=DEV)
    out = (big[guard:guard + total], cnt[8:8 + bs + 1], bad[8:10])
    for dtype in (torch.int32, torch.int64):
        got, want = _run(gts, voxel_num, 1, invalid=[np.array([-1, 7, voxel_num]), np.array([2 ** 31 - 1])], dtype=dtype, out=out)
        _same(got, want)
        assert got[2].tolist() == [2 * len(junk) + 3, 0]
        assert bool((big[:guard] == 0xAB).all()) and bool((big[guard + padded:] == 0xAB).all())
        assert bool((big[guard + total:guard + padded] == CLASSES).all())            # the padding of the last word is the call's
        assert cnt[:8].tolist() == [-77] * 8 == cnt[-8:].tolist() and bad[:8].tolist() == [-77] * 8 == bad[-8:].tolist()
    with pytest.raises(ValueError, match='multiple of 4'):                          # a buffer that ends with its last label
        hip.occ_targets(T(flat(gts)[0]).to(DEV), T(flat(gts)[1]).to(DEV), voxel_num, 1, CLASSES,
                        out=(torch.empty(total, dtype=torch.uint8, device=DEV), out[1], out[2]))


def test_edge_samples():
    hip = pkg('hipops')
    voxel_num, Z = 960 * 5, 5
    rng = np.random.default_rng(6)
    a, c = annotation(rng, 2, voxel_num, 0.2)
    gts = [a, np.zeros((0, 2), np.int64), c]                                        # an empty sample in the middle
    got, want = _run(gts, voxel_num, Z)
    _same(got, want)
    assert got[1].tolist() == [len(a), 0, len(c), len(a) + len(c)]
    # invalid voxels over pairs and over empty voxels, a sample without any
    invalid = [np.concatenate([a[:100, 0], rng.integers(0, voxel_num, 50)]), rng.integers(0, voxel_num, 30), np.zeros(0, np.int64)]
    got, want = _run(gts, voxel_num, Z, invalid=invalid, dtype=torch.int64)
    _same(got, want)
    assert int((got[0] == 255).sum()) >= 130 and got[1].tolist() == [len(a), 0, len(c), len(a) + len(c)]
    # no pairs at all
    got, want = _run([np.zeros((0, 2), np.int64)] * 2, voxel_num, Z)
    _same(got, want)
    assert bool((got[0] == CLASSES).all()) and got[1].tolist() == [0, 0, 0]
    # readable errors, no launch
    off = T(flat(gts)[1]).to(DEV)
    pairs = T(flat(gts)[0]).to(DEV)
    for args in ((pairs.float(), off), (pairs.cpu(), off), (pairs, off.long()), (pairs[:, :1], off)):
        with pytest.raises((TypeError, ValueError, RuntimeError)):
            hip.occ_targets(*args, voxel_num, Z, CLASSES)
    with pytest.raises(RuntimeError, match='255'):
        hip.occ_targets(pairs, off, voxel_num, Z, 255)


def test_out_is_rewritten_in_full_and_the_call_is_capturable():
    hip = pkg('hipops')
    voxel_num, bs = 4099, 2
    rng = np.random.default_rng(7)
    first, second = annotation(rng, bs, voxel_num, 0.3), annotation(rng, bs, voxel_num, 0.05)
    got1, want1 = _run(first, voxel_num, 1)
    out = tuple(T(a.copy()).to(DEV) for a in (np.concatenate([got1[0], np.zeros(2, np.uint8)]), got1[1], got1[2]))
    out = (out[0][:bs * voxel_num], out[1], out[2])
    got2, want2 = _run(second, voxel_num, 1, out=out)                                # into the first result's buffers
    _same(got2, want2)
    assert not np.array_equal(want1[0], want2[0])
    # captured once, replayed on other annotations written into the same static buffers
    n = max(sum(len(g) for g in first), sum(len(g) for g in second))
    pairs = torch.zeros(n, 2, dtype=torch.int32, device=DEV)
    off = torch.zeros(bs + 1, dtype=torch.int32, device=DEV)
    hip.occ_targets(pairs, off, voxel_num, 1, CLASSES, out=out)                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.occ_targets(pairs, off, voxel_num, 1, CLASSES, out=out)
    for gts, want in ((first, want1), (second, want2), (first, want1)):
        p, o = flat(gts)
        pairs[:len(p)].copy_(T(p).to(torch.int32))
        off.copy_(T(o))
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            _same(tuple(t.cpu().numpy() for t in out), want)


# ---------------------------------------------------------------------------------------------- head and detector
OCC_WEIGHTS = [round(float(v), 4) for v in weights_for(16, 5)]


@pytest.fixture(scope='module')
def head_case():
    """The vocc.py head (tests/golden/cases.py) with ``occ_weights``, one bf16 encoder output of two viewpoints, one sparse
    annotation with its dense tensor."""
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    pkg()
    syn = pkg('synthetic')
    head = pkg('registry').build_head(dict(cases.vocc_head_cfg(), occ_weights=list(OCC_WEIGHTS))).eval()
    cw = head.code_weights.detach().clone()
    syn.load_seeded(head, 7)
    head.code_weights.data.copy_(cw)
    head = head.to(DEV).train()
    for m in head.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    w2p, org = syn.camera_batch(2, seed=1)
    feats = T(syn.vit_features(2, seed=0)).to(DEV).permute(1, 0, 2, 3).contiguous()
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        emb = head(feats, None, only_bev=True, world2pixel=T(w2p).to(DEV), origin=T(org).to(DEV))
    gts = annotation(np.random.default_rng(11), 2, head.voxel_num, 0.1)
    return head, emb.detach(), gts, head.occupancy_targets([[g] for g in gts], device=DEV)


def _loss_and_grads(head, emb, fn):
    head.zero_grad(set_to_none=True)
    x = emb.clone().requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        loss = fn(x)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in head.named_parameters() if p.grad is not None}
    grads['voxel_embed'] = x.grad.clone()
    return loss.detach(), grads


def _identical(a, b):
    print('loss %r against %r' % (float(a[0]), float(b[0])))
    assert set(a[1]) == set(b[1]) and len(a[1]) > 10
    for k in a[1]:
        d = float((a[1][k].float() - b[1][k].float()).abs().max())
        print('%-60s max |difference| %.3e of max |gradient| %.3e' % (k, d, float(b[1][k].float().abs().max())))
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


def test_targets_of_the_head_are_the_dense_chain(head_case):
    head, emb, gts, dense = head_case
    opl = pkg('dense_heads.occ_proj_lattice')
    OT = pkg('dense_heads.voxelformer_occupancy_head').OccupancyTargets
    t = head.occupancy_targets_device([[g] for g in gts], device=DEV)
    plan = head.occupancy_row_plan(t.labels.device)
    assert isinstance(t, OT) and t.order == 'rows' and t.plan is plan and plan is not None and t.bs == 2
    assert t.labels.dtype == torch.uint8 and t.count.dtype == torch.int32 and t.bad.tolist() == [0, 0]
    chain = opl.voxels_to_rows(dense.to(torch.uint8).reshape(2, head.occ_zdim, plan.rows).permute(0, 2, 1), plan, 2).reshape(-1)
    assert torch.equal(t.labels, chain) and t.count.tolist() == (dense < 16).sum(1).tolist() + [int((dense < 16).sum())]
    v = head.occupancy_targets_device(gts, rows=False, device=DEV)
    assert v.order == 'voxels' and torch.equal(v.labels.view(2, -1), dense.to(torch.uint8)) and torch.equal(v.count, t.count)
    assert torch.equal(v.ordered('rows', plan), t.labels) and torch.equal(t.ordered('voxels'), v.labels)
    # a packed annotation that is on the device already
    p = pkg('hipops').pack_occ_gts(gts).to(DEV)
    assert p.buffer.is_cuda and torch.equal(head.occupancy_targets_device(p).labels, t.labels)
    with pytest.raises(ValueError, match='one or the other'):
        head.occupancy_targets_device(p, invalid=[None, None])
    # one pack is outstanding per size class of the pinned staging buffer: an overwritten pack refuses to be copied
    first = pkg('hipops').pack_occ_gts(gts)
    second = pkg('hipops').pack_occ_gts([g[::-1] for g in gts])
    assert first.buffer.is_pinned() and first.buffer.data_ptr() == second.buffer.data_ptr()
    with pytest.raises(RuntimeError, match='packed again'):
        first.to(DEV)
    assert torch.equal(second.to(DEV).pairs.cpu(), T(np.concatenate([g[::-1] for g in gts])).to(torch.int32))
    own = pkg('hipops').pack_occ_gts(gts, pinned=False)
    pkg('hipops').pack_occ_gts(gts[::-1], pinned=False)
    assert torch.equal(own.to(DEV).pairs.cpu(), T(np.concatenate(gts)).to(torch.int32))
    # the evaluation form
    rng = np.random.default_rng(12)
    invalid = [rng.integers(0, head.voxel_num, 5000), None]
    e = head.occupancy_targets_device(gts, invalid=invalid, device=DEV)
    want = head.occupancy_eval_labels(gts, invalid, device=DEV)
    assert torch.equal(e.ordered('voxels').view(2, -1), want) and int((want == 255).sum()) > 4000


@pytest.mark.parametrize('weights', [None, True])
def test_loss_from_volume_is_bit_identical(head_case, weights):
    """``occupancy_loss_from_volume(voxel_embed, OccupancyTargets)`` against the same call with the dense tensor (the fused
    MLP + focal Function; ``weights``: with ``occ_weights``): the loss, d(voxel_embed) and EVERY parameter gradient, bit for
    bit -- the kernels receive the same bytes and the same count.  That needs a backward whose sums do not depend on the
    arrival order of the workgroups: ``ver_occ_mlp_backward_fused_slabs`` (the entries that add the MLP's parameter
    gradients with float atomics differed by 5e-7 ... 3e-6 between any two runs, the dense route against itself included)."""
    head, emb, gts, dense = head_case
    t = head.occupancy_targets_device(gts, device=DEV)
    a = _loss_and_grads(head, emb, lambda x: head.occupancy_loss_from_volume(x, t, class_weights=weights))
    b = _loss_and_grads(head, emb, lambda x: head.occupancy_loss_from_volume(x, dense, class_weights=weights))
    assert float(a[0]) > 0 and any(k.startswith('occ_branches.6.') for k in a[1])
    _identical(a, b)


@pytest.mark.parametrize('n', [100, 64 * 300 + 9])              # 2 workgroups; all 256, ragged last block
def test_mlp_backward_with_slabs_is_reproducible_and_equals_the_atomic_sums(n):
    """``ver_occ_mlp_backward_fused_slabs`` against ``ver_occ_mlp_backward_fused_stats`` on the same operands: the same d(x)
    (one kernel), parameter gradients that are the same sums in another order -- bound per element: 2 * slabs * 2^-24 * the
    sum of the |shares| the slabs hold, the worst case of re-ordering an fp32 sum of that many terms -- and the same bits
    from two calls."""
    hip = pkg('hipops')
    L = hip.lib()
    gen = torch.Generator(device='cpu').manual_seed(n)
    w2, w3 = (torch.randn(128, 128, generator=gen) * 0.12).to(DEV), (torch.randn(16, 128, generator=gen) * 0.12).to(DEV)
    vec = hip.occ_mlp_vectors(torch.zeros(128, device=DEV), *((torch.randn(128, generator=gen) * 0.3 + o).to(DEV) for o in (1, 0, 0, 1, 0)),
                              (torch.randn(16, generator=gen) * 0.3).to(DEV))
    x = (torch.randn(n, 128, generator=gen) * 1.5).bfloat16().to(DEV)
    gl = (torch.randn(n, 16, generator=gen) * 0.1).bfloat16().to(DEV)
    P = 6 * 128 + 16 * 128 + 16 + 128 * 128
    nbytes = L.ver_occ_mlp_backward_fused_slab_bytes(n)
    nslabs = min((n + 63) // 64, 256)
    assert nbytes == nslabs * P * 4 and L.ver_occ_mlp_backward_fused_slab_bytes(0) == 0
    runs = []
    for _ in range(2):
        gx, pg = torch.empty_like(x), torch.full((P,), float('nan'), device=DEV)
        slabs = torch.full((nbytes // 4,), float('nan'), device=DEV)
        assert L.ver_occ_mlp_backward_fused_slabs(hip._p(x), hip._p(gl), hip._p(w2), hip._p(w3), hip._p(vec), None, hip._p(gx), hip._p(pg),
                                                  hip._p(slabs), nbytes, n, 128, 16, 1e-5, None, 0, hip._stream()) == 0
        runs.append((gx, pg, slabs))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    gx, pg = torch.empty_like(x), torch.empty(P, device=DEV)
    assert L.ver_occ_mlp_backward_fused_stats(hip._p(x), hip._p(gl), hip._p(w2), hip._p(w3), hip._p(vec), None, hip._p(gx), hip._p(pg),
                                              n, 128, 16, 1e-5, None, 0, hip._stream()) == 0
    assert torch.equal(gx, runs[0][0]) and bool(torch.isfinite(pg).all()) and float(pg.abs().max()) > 0
    shares = runs[0][2].view(nslabs, P)
    assert bool((pg[256:384] == 0).all()) and bool((runs[0][1][256:384] == 0).all())        # (the unused row of the vectors stays zero in both)
    bound = 2 * nslabs * 2.0 ** -24 * shares.abs().double().sum(0)
    err = (runs[0][1].double() - pg.double()).abs()
    print('worst |difference| / bound: %.3f' % float((err / bound.clamp(min=1e-30)).max()))
    assert bool((err <= bound).all())
    with pytest.raises(RuntimeError, match='slabs'):                                       # a scratch buffer that is too small
        hip._check(L.ver_occ_mlp_backward_fused_slabs(hip._p(x), hip._p(gl), hip._p(w2), hip._p(w3), hip._p(vec), None, hip._p(gx),
                                                      hip._p(pg), hip._p(slabs), nbytes - 4, n, 128, 16, 1e-5, None, 0, hip._stream()), 'slabs')


def test_order_conversion_gives_the_same_loss(head_case):
    head, emb, gts, dense = head_case
    rows, vox = head.occupancy_targets_device(gts, device=DEV), head.occupancy_targets_device(gts, rows=False, device=DEV)
    assert rows.order == 'rows' and vox.order == 'voxels'
    a = _loss_and_grads(head, emb, lambda x: head.occupancy_loss_from_volume(x, vox))          # voxel order -> the row-order loss
    b = _loss_and_grads(head, emb, lambda x: head.occupancy_loss_from_volume(x, rows))
    _identical(a, b)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        logits = head.occupancy_from_volume(emb)                                               # the reference's voxel order
        want = head.occupancy_loss(logits, dense)
        assert torch.equal(head.occupancy_loss(logits, rows), want) and torch.equal(head.occupancy_loss(logits, vox), want)
        tup = head.occupancy_from_volume(emb, rows_only=True)                                  # the unfused row-order loss
        want = head.occupancy_loss(tup, dense)
        assert torch.equal(head.occupancy_loss(tup, rows), want) and torch.equal(head.occupancy_loss(tup, vox), want)


def test_loss_only_occupancy_with_occ_weights(head_case):
    head, emb, gts, dense = head_case
    t = head.occupancy_targets_device(gts, rows=False, device=DEV)
    logits = torch.randn(2, head.voxel_num, 16, generator=torch.Generator(device=DEV).manual_seed(3), device=DEV)
    res = []
    for gt in (t, dense):
        x = logits.clone().requires_grad_(True)
        out = head.loss_only_occupancy(None, None, gt, dict(occupancy_preds=x))
        out['loss_occupancy'].backward()
        res.append((out['loss_occupancy'].detach(), x.grad, out['loss_flow']))
    print('loss_only_occupancy %r against %r' % (float(res[0][0]), float(res[1][0])))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and float(res[0][2]) == 0.0
    head.occ_weights, kept = None, head.occ_weights
    try:
        assert not torch.equal(head.loss_only_occupancy(None, None, t, dict(occupancy_preds=logits))['loss_occupancy'], res[0][0])
    finally:
        head.occ_weights = kept


def test_confusion_histograms_are_identical(head_case):
    head, emb, gts, dense = head_case
    rng = np.random.default_rng(13)
    invalid = [rng.integers(0, head.voxel_num, 20000), rng.integers(0, head.voxel_num, 100)]
    t = head.occupancy_targets_device(gts, invalid=invalid, device=DEV)
    labels = head.occupancy_eval_labels(gts, invalid, device=DEV)
    thr = (0.25, 0.5)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        fused = head.occupancy_confusion_from_volume(emb, t, thr)
        assert torch.equal(fused, head.occupancy_confusion_from_volume(emb, labels, thr))
        tup = head.occupancy_from_volume(emb, rows_only=True)
        assert torch.equal(head.occupancy_confusion(tup, t, thr), head.occupancy_confusion(tup, labels, thr))
        logits = head.occupancy_from_volume(emb)
        assert torch.equal(head.occupancy_confusion(logits, t, thr), head.occupancy_confusion(logits, labels, thr))
    assert int(fused.sum()) == 2 * (2 * head.voxel_num - int((labels == 255).sum()))


def test_a_conflicting_annotation_raises_on_the_first_call(head_case, monkeypatch):
    head, emb, gts, dense = head_case
    losses = pkg('dense_heads.losses')
    v, c = int(gts[0][0, 0]), int(gts[0][0, 1])
    conflict = [np.concatenate([gts[0], [[v, (c + 1) % 16]]]), gts[1]]
    monkeypatch.setattr(losses, '_FOCAL_CHECK', 1)
    head.__dict__.pop('_occ_targets_checked', None)
    with pytest.raises(ValueError, match=r'bad\[1\] = 1'):
        head.occupancy_targets_device(conflict, device=DEV)
    t = head.occupancy_targets_device(conflict, device=DEV)                  # later calls do not read it ...
    with pytest.raises(ValueError, match=r'bad\[1\] = 1'):
        t.check()                                                            # ... unless asked
    monkeypatch.setattr(losses, '_FOCAL_CHECK', 2)
    with pytest.raises(ValueError, match=r'bad\[0\] = 2'):
        head.occupancy_targets_device([np.concatenate([gts[0], [[-1, 0], [5, 17]]]), gts[1]], device=DEV)
    monkeypatch.setattr(losses, '_FOCAL_CHECK', 0)
    head.__dict__.pop('_occ_targets_checked', None)
    assert head.occupancy_targets_device(conflict, device=DEV).bad.tolist() == [0, 1]


def test_detector_switch(tmp_path):
    """``VoxelFormer(device_occupancy_targets=True)`` in the bf16 row-order training form against the default detector.
    EQUAL loss dicts, bit for bit, where equality is defined: inside the detector's own ``head.loss`` call the loss is
    evaluated a second time on the SAME head outputs with the dense tensor the default detector would have built, and
    the targets' bytes are the dense tensor's pushed through ``voxels_to_rows``.  Two separate detector runs are
    compared as well, at the bounds of tests/test_detector_gpu.py only: ``k_sca_fwd_cs`` sums the cameras with float
    atomics, so two runs of the encoder agree to rounding, not in bits.  ``head.occupancy_targets`` is never called with the
    switch on (the loss routine the detector reaches still widens the bytes to int64: DESIGN.md 3.12).  And an evaluation
    whose label counts -- the row sums of the confusion matrices, which no prediction moves -- are equal."""
    torch.backends.cuda.matmul.allow_tf32 = False
    pkg()
    syn, reg = pkg('synthetic'), pkg('registry')
    OT = pkg('dense_heads.voxelformer_occupancy_head').OccupancyTargets
    det = reg.build_detector(dict(type='VoxelFormer', pts_bbox_head=cases.vocc_head_cfg(), train_cfg=dict(pts=cases.VOCC_TRAIN_CFG),
                                  autocast_dtype='bf16', occupancy_rows=True, device_occupancy_targets=True)).eval()
    assert det.device_occupancy_targets is True
    assert inspect.signature(type(det).__init__).parameters['device_occupancy_targets'].default is False       # opt-in
    head = det.pts_bbox_head
    cw = head.code_weights.detach().clone()
    syn.load_seeded(head, 7)
    head.code_weights.data.copy_(cw)
    det.to(DEV)
    names = ['scanA_vp0', 'scanA_vp1']
    store = _store(tmp_path, syn.vit_features(2, seed=0), names)
    gts = [cases.detection_gt(seed=40 + i, num_gt=3 + i) for i in range(2)]
    dense = np.random.default_rng(9).integers(0, 17, size=(2, 504000))
    metas = _metas(tmp_path, store, names, gts, [_sparse(d) for d in dense])
    inv = tmp_path / 'invalid_0.npy'
    np.save(str(inv), np.random.default_rng(10).integers(0, 504000, 3000))
    metas[0]['occ_invalid_path'] = str(inv)
    seen, exact, dense_calls = [], [], []
    loss, dense_targets = head.loss, head.occupancy_targets
    opl = pkg('dense_heads.occ_proj_lattice')

    def both(boxes, labels, gt_occupancy, outs):
        seen.append(gt_occupancy)
        got = loss(boxes, labels, gt_occupancy, outs)
        if isinstance(gt_occupancy, OT):                       # the same outputs against the default detector's dense tensor
            gt = dense_targets([[np.load(m['occ_gt_path'])] for m in metas], device=DEV)
            exact.append((got, loss(boxes, labels, gt, outs), gt))
        return got

    head.loss = both
    head.occupancy_targets = lambda *a, **k: (dense_calls.append(1), dense_targets(*a, **k))[1]
    res = {}
    for on in (True, False):
        det.device_occupancy_targets = on
        res[on] = {k: float(v) for k, v in det(return_loss=True, img_metas=metas).items()}
        assert len(dense_calls) == (0 if on else 1)
    assert isinstance(seen[0], OT) and seen[0].order == 'rows' and torch.is_tensor(seen[1]) and len(exact) == 1
    got, want, gt = exact[0]
    assert sorted(got) == sorted(want) and torch.equal(gt.cpu(), T(dense))
    for k in want:
        assert torch.equal(got[k], want[k]), (k, float(got[k]), float(want[k]))
    plan = seen[0].plan
    chain = opl.voxels_to_rows(gt.to(torch.uint8).reshape(2, head.occ_zdim, plan.rows).permute(0, 2, 1), plan, 2).reshape(-1)
    assert torch.equal(seen[0].labels, chain) and torch.equal(seen[1], gt) and seen[0].bad.tolist() == [0, 0]
    assert seen[0].count.tolist() == [int((d < 16).sum()) for d in dense] + [int((dense < 16).sum())]
    assert sorted(res[True]) == sorted(res[False]) and 'loss_occupancy' in res[True]
    for k in res[False]:
        print('%-20s %r against %r' % (k, res[True][k], res[False][k]))
    for k in res[False]:
        assert res[True][k] == pytest.approx(res[False][k], rel=1e-4, abs=1e-7), k
    hists = {}
    for on in (True, False):
        det.device_occupancy_targets = on
        hists[on] = det.evaluate_occupancy(metas, autocast_dtype='bf16', fused=on).hist
    assert torch.equal(hists[True].sum(-1), hists[False].sum(-1)) and int(hists[True].sum()) == 2 * 504000 - 3000 + (3000 - len(np.unique(np.load(str(inv)))))
