"""Occupancy targets from the sparse annotation, without a GPU: the numpy model of ``ver_occ_targets``
(``hipops.occ_targets_host``) against the head's dense ``occupancy_targets`` / ``occupancy_eval_labels`` and the plan's row
maps, the stated rules for repeated and rejected pairs, the host packer, the row table, the argument checks of the C ABI, and
the labels module's ``(gt, avg)`` of the occupancy loss for both label forms (``dense_heads/occupancy_labels.py``)."""
import ctypes
import types

import numpy as np
import pytest
import torch

from util import ROOT, pkg

CLASSES = 16
ROWS = 1920                                  # positions of the plan (16, 4, 40, 48)
T = torch.from_numpy


def _annotation(rng, bs, voxel_num, lo=0.03, hi=0.2, classes=CLASSES):
    """Per sample: [n, 2] int64 (distinct voxel, class), shuffled."""
    out = []
    for _ in range(bs):
        n = int(rng.integers(int(lo * voxel_num), int(hi * voxel_num) + 1))
        idx = rng.choice(voxel_num, n, replace=False)
        out.append(np.stack([idx, rng.integers(0, classes, n)], 1).astype(np.int64))
    return out


def _flat(gts):
    pairs = np.concatenate(gts) if gts else np.zeros((0, 2), np.int64)
    return pairs, np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int32)


def _head_stub(voxel_num):
    """What ``occupancy_targets`` / ``occupancy_eval_labels`` read of a head."""
    return types.SimpleNamespace(voxel_num=voxel_num, occupancy_classes=CLASSES, code_weights=torch.zeros(1))


@pytest.fixture(scope='module')
def plan():
    return pkg('dense_heads.occ_proj_lattice').get_plan(16, 4, 40, 48, 'cpu')


def test_voxel_order_is_the_heads_dense_target():
    hip = pkg('hipops')
    Head = pkg('dense_heads.voxelformer_occupancy_head').VoxelFormerOccupancyHead
    bs, voxel_num = 3, ROWS * 5
    gts = _annotation(np.random.default_rng(0), bs, voxel_num)
    gt = Head.occupancy_targets(_head_stub(voxel_num), [[g] for g in gts])          # the reference's nesting
    pairs, off = _flat(gts)
    labels, count, bad = hip.occ_targets_host(pairs, off, voxel_num, 5, CLASSES)
    assert labels.dtype == np.uint8 and count.dtype == np.int32 and bad.dtype == np.int32
    assert np.array_equal(labels.reshape(bs, voxel_num), gt.numpy().astype(np.uint8))
    assert np.array_equal(count[:bs], (gt < CLASSES).sum(1).numpy()) and count[bs] == int((gt < CLASSES).sum())
    assert bad.tolist() == [0, 0]
    # int32 pairs are the same annotation
    l32, c32, b32 = hip.occ_targets_host(pairs.astype(np.int32), off, voxel_num, 5, CLASSES)
    assert np.array_equal(l32, labels) and np.array_equal(c32, count) and b32.tolist() == [0, 0]


@pytest.mark.parametrize('Z', [5, 35])
def test_row_order_is_voxels_to_rows(plan, Z):
    hip, opl = pkg('hipops'), pkg('dense_heads.occ_proj_lattice')
    Head = pkg('dense_heads.voxelformer_occupancy_head').VoxelFormerOccupancyHead
    bs, voxel_num = 3, ROWS * Z
    gts = _annotation(np.random.default_rng(Z), bs, voxel_num)
    gt = Head.occupancy_targets(_head_stub(voxel_num), gts)
    want = opl.voxels_to_rows(gt.reshape(bs, Z, plan.rows).permute(0, 2, 1), plan, bs)
    pairs, off = _flat(gts)
    labels, count, bad = hip.occ_targets_host(pairs, off, voxel_num, Z, CLASSES, row_table=opl.row_table(plan))
    assert np.array_equal(labels, want.reshape(-1).numpy().astype(np.uint8))
    assert np.array_equal(count[:bs], (gt < CLASSES).sum(1).numpy()) and bad.tolist() == [0, 0]


def test_with_invalid_it_is_occupancy_eval_labels(plan):
    hip, opl = pkg('hipops'), pkg('dense_heads.occ_proj_lattice')
    Head = pkg('dense_heads.voxelformer_occupancy_head').VoxelFormerOccupancyHead
    rng = np.random.default_rng(3)
    bs, Z = 3, 5
    voxel_num = ROWS * Z
    gts = _annotation(rng, bs, voxel_num)
    invalid = [rng.choice(voxel_num, 700, replace=False), None, np.concatenate([gts[2][:50, 0], rng.choice(voxel_num, 9)])]
    want = Head.occupancy_eval_labels(_head_stub(voxel_num), gts, invalid)
    pairs, off = _flat(gts)
    inv = np.concatenate([np.zeros(0, np.int64) if i is None else i for i in invalid])
    ioff = np.concatenate([[0], np.cumsum([0 if i is None else len(i) for i in invalid])])
    labels, count, bad = hip.occ_targets_host(pairs, off, voxel_num, Z, CLASSES, invalid=inv, invalid_offsets=ioff)
    assert np.array_equal(labels.reshape(bs, voxel_num), want.numpy()) and int((labels == 255).sum()) > 700
    assert count[:bs].tolist() == [len(g) for g in gts] and bad.tolist() == [0, 0]        # the pairs' count: invalid voxels stay in it
    rows, _, _ = hip.occ_targets_host(pairs, off, voxel_num, Z, CLASSES, row_table=opl.row_table(plan), invalid=inv, invalid_offsets=ioff)
    assert np.array_equal(rows, opl.voxels_to_rows(want.reshape(bs, Z, plan.rows).permute(0, 2, 1), plan, bs).reshape(-1).numpy())


def test_repeated_listings():
    hip = pkg('hipops')
    rng = np.random.default_rng(4)
    voxel_num = 4099
    base = _annotation(rng, 2, voxel_num)
    pairs, off = _flat(base)
    labels, count, bad = hip.occ_targets_host(pairs, off, voxel_num, 1, CLASSES)
    # the same class again: nothing changes, nothing is counted
    again = [np.concatenate([g, g[:40], g[:7]]) for g in base]
    l2, c2, b2 = hip.occ_targets_host(*_flat(again), voxel_num, 1, CLASSES)
    assert np.array_equal(l2, labels) and np.array_equal(c2, count) and b2.tolist() == [0, 0]
    # other classes for 30 voxels of sample 0, two extra listings each: the largest class stays, every listing of another
    # class than the winner's lost -- whatever the order of the pairs
    v = base[0][:30, 0]
    c0 = base[0][:30, 1]
    c1, c2_ = (c0 + 1 + rng.integers(0, 7, 30)) % CLASSES, rng.integers(0, CLASSES, 30)
    conflict = np.concatenate([base[0], np.stack([v, c1], 1), np.stack([v, c2_], 1)])
    winner = np.maximum(np.maximum(c0, c1), c2_)
    lost = int((c0 != winner).sum() + (c1 != winner).sum() + (c2_ != winner).sum())
    assert lost >= 30
    want = labels.copy()
    want[v] = winner
    for seed in range(5):
        shuffled = conflict[np.random.default_rng(seed).permutation(len(conflict))]
        l3, c3, b3 = hip.occ_targets_host(*_flat([shuffled, base[1]]), voxel_num, 1, CLASSES)
        assert np.array_equal(l3, want) and np.array_equal(c3, count), seed            # the count stays exact
        assert b3.tolist() == [0, lost], seed


def test_rejected_pairs_and_the_empty_class():
    hip = pkg('hipops')
    voxel_num = 4099
    base = _annotation(np.random.default_rng(5), 2, voxel_num)
    labels, count, bad = hip.occ_targets_host(*_flat(base), voxel_num, 1, CLASSES)
    free = np.setdiff1d(np.arange(voxel_num), base[1][:, 0])[:3]
    junk = np.array([[-1, 3], [voxel_num, 3], [2 ** 40, 0], [free[0], -1], [free[1], CLASSES + 1], [free[2], 2 ** 35]])
    empty = np.array([[free[0], CLASSES], [free[1], CLASSES]])               # "empty" listed explicitly
    l2, c2, b2 = hip.occ_targets_host(*_flat([base[0], np.concatenate([junk[:3], base[1], empty, junk[3:]])]), voxel_num, 1, CLASSES)
    assert np.array_equal(l2, labels) and np.array_equal(c2, count) and b2.tolist() == [6, 0]
    # an empty label next to a class for the same voxel writes nothing and loses nothing
    both = np.concatenate([base[1], [[base[1][0, 0], CLASSES]]])
    l3, c3, b3 = hip.occ_targets_host(*_flat([base[0], both]), voxel_num, 1, CLASSES)
    assert np.array_equal(l3, labels) and np.array_equal(c3, count) and b3.tolist() == [0, 0]
    # out-of-range invalid voxels
    _, _, b4 = hip.occ_targets_host(*_flat(base), voxel_num, 1, CLASSES, invalid=np.array([-1, 5, voxel_num]), invalid_offsets=[0, 2, 3])
    assert b4.tolist() == [2, 0]
    for kw in (dict(voxel_num=4099, zdim=2), dict(voxel_num=4100, zdim=2, classes=255)):
        with pytest.raises(ValueError):
            hip.occ_targets_host(*_flat(base), kw['voxel_num'], kw['zdim'], kw.get('classes', CLASSES))
    with pytest.raises(ValueError, match='ascend'):
        hip.occ_targets_host(np.zeros((4, 2), np.int64), [0, 5, 4], voxel_num, 1, CLASSES)


def test_empty_and_full_samples():
    hip = pkg('hipops')
    voxel_num = 960
    rng = np.random.default_rng(6)
    full = np.stack([rng.permutation(voxel_num), rng.integers(0, CLASSES, voxel_num)], 1)
    gts = [_annotation(rng, 1, voxel_num)[0], np.zeros((0, 2), np.int64), full]
    labels, count, bad = hip.occ_targets_host(*_flat(gts), voxel_num, 5, CLASSES)
    labels = labels.reshape(3, voxel_num)
    assert (labels[1] == CLASSES).all() and count.tolist() == [len(gts[0]), 0, voxel_num, len(gts[0]) + voxel_num]
    assert np.array_equal(labels[2][full[:, 0]], full[:, 1]) and bad.tolist() == [0, 0]
    l0, c0, b0 = hip.occ_targets_host(np.zeros((0, 2), np.int32), [0, 0, 0], voxel_num, 5, CLASSES)
    assert (l0 == CLASSES).all() and l0.size == 2 * voxel_num and c0.tolist() == [0, 0, 0] and b0.tolist() == [0, 0]
    l0, c0, _ = hip.occ_targets_host(np.zeros((0, 2), np.int32), [0], voxel_num, 5, CLASSES)          # no sample at all
    assert l0.size == 0 and c0.tolist() == [0]


def test_pack_occ_gts():
    hip = pkg('hipops')
    rng = np.random.default_rng(7)
    gts = _annotation(rng, 3, 5000)
    gts[1] = np.zeros((0, 2), np.int64)
    mixed = [[gts[0]], gts[1].astype(np.int32), (T(gts[2]),)]                # nesting, an empty sample, int32, a tensor
    p = hip.pack_occ_gts(mixed, pinned=False)
    pairs, off = _flat(gts)
    assert p.bs == 3 and p.n_total == len(pairs) and p.n_invalid == 0 and p.invalid is None and p.invalid_offsets is None
    assert p.pairs.dtype == torch.int32 and p.offsets.dtype == torch.int32 and p.buffer.dim() == 1
    assert np.array_equal(p.pairs.numpy(), pairs) and np.array_equal(p.offsets.numpy(), off)
    assert p.pairs.data_ptr() % 8 == 0                                         # one (index, class) pair: the kernel's vector load
    assert p.pairs.data_ptr() == p.buffer.data_ptr() + 4 * 2 * (p.bs + 1)      # views of the one buffer that is copied
    invalid = [rng.integers(0, 5000, 11), None, rng.integers(0, 5000, 4).astype(np.int32)]
    q = hip.pack_occ_gts(gts, invalid, pinned=False)
    assert q.n_invalid == 15 and q.invalid_offsets.tolist() == [0, 11, 11, 15]
    assert np.array_equal(q.invalid.numpy(), np.concatenate([invalid[0], invalid[2]])) and np.array_equal(q.pairs.numpy(), pairs)
    # values outside int32 stay out of range instead of wrapping into it
    wide = hip.pack_occ_gts([np.array([[2 ** 32 + 5, 3], [-2 ** 40, 1], [7, 2 ** 33]])], pinned=False)
    assert wide.pairs.tolist() == [[2 ** 31 - 1, 3], [-2 ** 31, 1], [7, 2 ** 31 - 1]]
    none = hip.pack_occ_gts([], pinned=False)
    assert none.bs == 0 and none.offsets.tolist() == [0] and none.pairs.shape == (0, 2)
    with pytest.raises(ValueError):
        hip.pack_occ_gts([np.zeros((3, 3), np.int64)], pinned=False)
    with pytest.raises(TypeError):
        hip.pack_occ_gts([np.zeros((3, 2), np.float32)], pinned=False)
    with pytest.raises(ValueError):
        hip.pack_occ_gts(gts, invalid[:2], pinned=False)
    # on the host ``to`` is a copy, not the staging buffer itself
    assert q.to('cpu').buffer.data_ptr() != q.buffer.data_ptr() and torch.equal(q.to('cpu').pairs, q.pairs)


def test_abi_without_a_gpu():
    hip = pkg('hipops')
    text = open(ROOT + '/include/ver_ops.h').read()
    assert 'int ver_occ_targets(' in text and 'the evaluation never reads it' in text
    assert 'ver_occ_targets' in hip.SYMBOLS
    lib = hip.lib()
    handle = ctypes.CDLL(hip.LIB_PATH)
    assert hasattr(handle, 'ver_occ_targets') and lib.ver_abi_version() == hip.ABI_VERSION
    ret, params = hip.prototypes()['ver_occ_targets']
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert ret is I and params == [P, I, P, L, P, I, P, L, P, P, P, P, L, I, I, I, P]
    assert list(lib.ver_occ_targets.argtypes) == params
    buf = (ctypes.c_int * 64)()
    call = lambda pairs=buf, off=buf, n=4, inv=None, ioff=None, ni=0, lab=buf, cnt=buf, bad=buf, voxels=40, z=5, classes=16, bs=2, dt=0: (
        lib.ver_occ_targets(pairs, dt, off, n, inv, 0, ioff, ni, None, lab, cnt, bad, voxels, z, classes, bs, None))
    for kw in (dict(pairs=None), dict(off=None), dict(lab=None), dict(cnt=None), dict(bad=None), dict(ni=3), dict(inv=buf, ni=3)):
        assert call(**kw) == -1 and b'null' in lib.ver_last_error(), kw
    assert call(classes=255) == -2 and b'255' in lib.ver_last_error()
    assert call(voxels=41) == -2 and b'multiple of zdim' in lib.ver_last_error()
    assert call(voxels=2 ** 30, z=1) == -2 and b'2^31' in lib.ver_last_error()
    assert call(voxels=2 ** 30 - 1, z=1, bs=3) == -2 and b'2^31' in lib.ver_last_error()
    assert call(bs=0) == 0 and call(bs=0, pairs=None, off=None, lab=None, cnt=None, bad=None) == 0
    assert call(bs=-1) == -1 and call(z=0) == -1 and call(dt=2) == -1 and call(n=-1) == -1
    off = ctypes.cast(ctypes.addressof(buf) + 4, ctypes.c_void_p)
    assert call(pairs=off) == -1 and b'aligned' in lib.ver_last_error()
    assert call(lab=ctypes.cast(ctypes.addressof(buf) + 1, ctypes.c_void_p)) == -1 and b'aligned' in lib.ver_last_error()


def test_row_table_of_the_vocc_plan():
    """One table for every batch size: (offset, n_rows, index) of the 120 x 120 positions reproduce ``_row_index``."""
    opl = pkg('dense_heads.occ_proj_lattice')
    plan = opl.lattice_plan(128, 4, 60, 60, 'cpu')
    assert plan is opl.get_plan(128, 4, 120, 120, 'cpu') and plan.rows == 14400
    table = opl.row_table(plan)
    assert table.shape == (14400, 3) and table.dtype == np.int32 and opl.row_table(plan) is table
    assert torch.equal(opl.row_table(plan, 'cpu'), T(table)) and opl.row_table(plan, 'cpu') is opl.row_table(plan, 'cpu')
    q = np.arange(plan.rows)
    for bs in (1, 3):
        fwd = opl._row_index(plan, bs, 'cpu')[0].numpy().reshape(bs, plan.rows)
        got = bs * table[q, 0][None, :] + np.arange(bs)[:, None] * table[q, 1][None, :] + table[q, 2][None, :]
        assert np.array_equal(got, fwd)


def test_targets_object_converts_between_the_orders(plan):
    """``OccupancyTargets.ordered``: the bytes as they are in their own order, the row maps once otherwise -- both ways."""
    hip, opl = pkg('hipops'), pkg('dense_heads.occ_proj_lattice')
    OT = pkg('dense_heads.voxelformer_occupancy_head').OccupancyTargets
    bs, Z = 2, 5
    voxel_num = ROWS * Z
    pairs, off = _flat(_annotation(np.random.default_rng(8), bs, voxel_num))
    vox = OT(*(T(a) for a in hip.occ_targets_host(pairs, off, voxel_num, Z, CLASSES)), 'voxels', bs, None, Z)
    row = OT(*(T(a) for a in hip.occ_targets_host(pairs, off, voxel_num, Z, CLASSES, row_table=opl.row_table(plan))), 'rows', bs, plan, Z)
    assert vox.ordered('voxels') is vox.labels and row.ordered('rows', plan) is row.labels
    assert torch.equal(vox.ordered('rows', plan), row.labels) and torch.equal(row.ordered('voxels'), vox.labels)
    assert vox.check() is vox
    bad = OT(vox.labels, vox.count, torch.tensor([2, 0], dtype=torch.int32), 'voxels', bs, None, Z)
    with pytest.raises(ValueError, match=r'bad\[0\] = 2'):
        bad.check()
    lost = OT(vox.labels, vox.count, torch.tensor([0, 5], dtype=torch.int32), 'voxels', bs, None, Z)
    with pytest.raises(ValueError, match=r'bad\[1\] = 5'):
        lost.check()
    with pytest.raises(ValueError):
        OT(vox.labels, vox.count, vox.bad, 'rows', bs, None, Z)


def test_loss_labels_of_a_dense_tensor_and_of_targets_are_the_same_pairs(plan):
    """``occupancy_labels.loss_labels``, the one place where the occupancy loss gets ``(gt, avg)``: the dense int64 tensor
    and the ``OccupancyTargets`` of the same sparse pairs give identical bytes in identical positions and equal counts, for
    logits in the voxel order and in the plan's row order; the count of a mask whose length is no multiple of 8 (the
    ``.sum()`` branch) equals the word-sum count of the same labels padded with empty ones; -1 and 300 leave the narrowing
    step as 255."""
    hip, opl, ol = pkg('hipops'), pkg('dense_heads.occ_proj_lattice'), pkg('dense_heads.occupancy_labels')
    Head = pkg('dense_heads.voxelformer_occupancy_head').VoxelFormerOccupancyHead
    bs, Z = 2, 5
    voxel_num = ROWS * Z
    gts = _annotation(np.random.default_rng(9), bs, voxel_num)
    dense = Head.occupancy_targets(_head_stub(voxel_num), gts)
    pairs, off = _flat(gts)
    vox = ol.OccupancyTargets(*(T(a) for a in hip.occ_targets_host(pairs, off, voxel_num, Z, CLASSES)), 'voxels', bs, None, Z)
    row = ol.OccupancyTargets(*(T(a) for a in hip.occ_targets_host(pairs, off, voxel_num, Z, CLASSES, row_table=opl.row_table(plan))),
                              'rows', bs, plan, Z)
    in_rows = opl.voxels_to_rows(dense.reshape(bs, Z, plan.rows).permute(0, 2, 1), plan, bs).reshape(-1)
    assert not torch.equal(in_rows, dense.reshape(-1))
    for logit_plan, want in ((None, dense.reshape(-1)), (plan, in_rows)):
        for as_bytes in (False, True):
            gt, avg = ol.loss_labels(dense, CLASSES, logit_plan, bs, Z, as_bytes=as_bytes)
            assert gt.dtype == torch.int64 and torch.equal(gt, want)           # (a CPU tensor is never narrowed)
            assert avg.dtype == torch.float32 and float(avg) == len(pairs)
            for targets in (vox, row):
                got, count = ol.loss_labels(targets, CLASSES, logit_plan, bs, Z, as_bytes=as_bytes)
                assert got.dtype == (torch.uint8 if as_bytes else torch.int64) and got.shape == want.shape
                assert torch.equal(got.to(torch.uint8), want.to(torch.uint8))
                assert count.dtype == torch.float32 and float(count) == float(avg)
    assert torch.equal(ol.labels_in_rows(row, plan, bs, Z), ol.labels_in_rows(dense, plan, bs, Z, dtype=torch.uint8))
    assert ol.labels_in_voxels(dense) is dense and ol.labels_in_voxels(vox) is vox.labels
    # the count: 19197 labels take the plain sum, the same labels padded with three empty ones the word sum
    cut = in_rows[:bs * voxel_num - 3].to(torch.uint8)
    padded = torch.cat([cut, torch.full((3,), CLASSES, dtype=torch.uint8)])
    assert cut.numel() % 8 == 5 and padded.numel() % 8 == 0
    short, long_ = ol.count_occupied(cut < CLASSES), ol.count_occupied(padded < CLASSES)
    assert float(short) == float(long_) == float(ol.count_occupied(padded < CLASSES, by_words=False)) == int((cut < CLASSES).sum())
    assert 0 < float(short) < len(pairs) + 1 and short.dtype == long_.dtype == torch.float32
    # the narrowing step, forced on a CPU tensor: out-of-range labels stay out of range as bytes
    odd = torch.tensor([-1, 300, 0, CLASSES, 255, 256, -7, 2 ** 40, 254])
    assert ol.narrow_labels(odd).tolist() == [255, 255, 0, CLASSES, 255, 255, 255, 255, 254]
    spoiled = dense.clone()
    spoiled[0, 17], spoiled[1, 4321] = -1, 300
    narrowed = ol.narrow_labels(spoiled)
    assert narrowed.dtype == torch.uint8 and narrowed[0, 17] == 255 and narrowed[1, 4321] == 255
    keep = torch.ones_like(spoiled, dtype=torch.bool)
    keep[0, 17] = keep[1, 4321] = False
    assert torch.equal(narrowed[keep], dense[keep].to(torch.uint8))
    through = ol.labels_in_rows(narrowed, plan, bs, Z).reshape(-1)
    assert int((through == 255).sum()) == 2 and int((through != in_rows.to(torch.uint8)).sum()) == 2


def test_reproducible_mlp_backward_entry_without_a_gpu():
    """``ver_occ_mlp_backward_fused_slabs`` / ``_slab_bytes``: declared, exported, argument checks before any launch."""
    hip = pkg('hipops')
    lib = hip.lib()
    P = 6 * 128 + 16 * 128 + 16 + 128 * 128
    assert {'ver_occ_mlp_backward_fused_slabs', 'ver_occ_mlp_backward_fused_slab_bytes'} <= set(hip.SYMBOLS)
    assert hip.prototypes()['ver_occ_mlp_backward_fused_slab_bytes'] == (ctypes.c_long, [ctypes.c_long])
    assert [lib.ver_occ_mlp_backward_fused_slab_bytes(n) for n in (0, 1, 64, 65, 64 * 256, 10 ** 8)] == [0, P * 4, P * 4, 2 * P * 4, 256 * P * 4, 256 * P * 4]
    buf = (ctypes.c_float * 64)()
    call = lambda slabs=buf, nbytes=P * 4, n=4, x=buf, width=128, flags=0: lib.ver_occ_mlp_backward_fused_slabs(
        x, buf, buf, buf, buf, None, buf, buf, slabs, nbytes, n, width, 16, 1e-5, None, flags, None)
    assert call(slabs=None) == -1 and b'null slabs' in lib.ver_last_error()
    assert call(nbytes=P * 4 - 4) == -1 and b'needed' in lib.ver_last_error()
    assert call(width=64) == -2 and call(flags=8) == -1 and call(n=-1) == -1
    assert lib.ver_occ_mlp_backward_fused_slabs(None, None, None, None, None, None, None, None, None, 0, 4, 128, 16, 1e-5, None, 0, None) == -1
