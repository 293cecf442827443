"""Occupancy pairs from byte labels, without a GPU: the numpy model of ``ver_occ_pairs`` (``hipops.occ_pairs_host``) against
the plain ``np.nonzero`` statement in both label orders, the round trip through ``occ_targets_host``, offsets clamping and the
overflow word, the flat-index flag, and the library's argument validation (which never touches the device)."""
import ctypes

import numpy as np
import pytest
import torch

from occ_pairs_helper import CLASSES, expected, group_table, in_rows, volume
from util import pkg


def _same(got, want, dtype=np.int32):
    pairs, offsets, count = got
    kept, woff, wcount = want
    assert pairs.dtype == dtype and offsets.dtype == np.int32 and count.dtype == np.int32
    assert np.array_equal(offsets, woff) and np.array_equal(count, wcount)
    assert np.array_equal(pairs[:offsets[-1]], kept) and not pairs[offsets[-1]:].any()


@pytest.mark.parametrize('zdim,rows', [(1, 1023), (5, 205), (35, 30), (1, 1)])
@pytest.mark.parametrize('bs', [1, 3])
def test_host_model_is_the_nonzero_statement_in_both_orders(zdim, rows, bs):
    hip = pkg('hipops')
    rng = np.random.default_rng(zdim + bs)
    voxel_num = zdim * rows
    vol = volume(rng, bs, voxel_num, 0.2, empty=1, full=2)
    want = expected(vol, bs * voxel_num)
    got = hip.occ_pairs_host(vol.reshape(-1), bs, voxel_num, zdim, CLASSES)
    _same(got, want)
    assert got[0].shape == (bs * voxel_num, 2) and got[2][bs + 1] == 0
    table = group_table(rng, rows)
    _same(hip.occ_pairs_host(in_rows(vol, table, zdim), bs, voxel_num, zdim, CLASSES, row_table=table, dtype=torch.int64), want, np.int64)


@pytest.mark.parametrize('with_table', [False, True])
def test_round_trip_through_the_targets_model(with_table):
    hip = pkg('hipops')
    rng = np.random.default_rng(5)
    bs, zdim, rows = 3, 5, 41
    voxel_num = zdim * rows
    vol = volume(rng, bs, voxel_num, 0.3, empty=0, full=1, specials=False)
    table = group_table(rng, rows) if with_table else None
    labels = in_rows(vol, table, zdim) if with_table else vol.reshape(-1)
    pairs, offsets, count = hip.occ_pairs_host(labels, bs, voxel_num, zdim, CLASSES, row_table=table)
    back, back_count, bad = hip.occ_targets_host(pairs[:offsets[-1]], offsets, voxel_num, zdim, CLASSES, row_table=table)
    assert np.array_equal(back, labels) and np.array_equal(back_count, count[:bs + 1]) and bad.tolist() == [0, 0]


def test_offsets_are_clamped_and_the_overflow_word_is_written():
    hip = pkg('hipops')
    rng = np.random.default_rng(6)
    bs, voxel_num = 3, 300
    vol = volume(rng, bs, voxel_num, 0.3)
    total = int((vol < CLASSES).sum())
    first = int((vol[0] < CLASSES).sum())
    for capacity in (0, first, first + 1, total - 1, total, total + 5):
        got = hip.occ_pairs_host(vol.reshape(-1), bs, voxel_num, 1, CLASSES, capacity=capacity)
        _same(got, expected(vol, capacity))
        pairs, offsets, count = got
        assert pairs.shape == (capacity, 2) and offsets.max() <= capacity and offsets[-1] == min(total, capacity)
        assert count[bs] == total and count[bs + 1] == int(total > capacity) and (np.diff(offsets) >= 0).all()


def test_flat_indices_are_those_of_the_flattened_batch():
    hip = pkg('hipops')
    rng = np.random.default_rng(7)
    bs, voxel_num = 3, 200
    vol = volume(rng, bs, voxel_num, 0.25)
    pairs, offsets, count = hip.occ_pairs_host(vol.reshape(-1), bs, voxel_num, 1, CLASSES, flat=True, dtype=torch.int64)
    _same((pairs, offsets, count), expected(vol, bs * voxel_num, flat=True), np.int64)
    flat = torch.from_numpy(vol.reshape(-1))
    idx, = torch.where(flat < CLASSES)                      # head.occupancy_pairs_from_classes
    assert torch.equal(torch.from_numpy(pairs[:offsets[-1]]), torch.stack([idx, flat[idx].long()], dim=-1))
    with pytest.raises(ValueError, match='2\\^31'):
        hip.occ_pairs_host(np.zeros(0, np.uint8), 2, 2 ** 30, 1, CLASSES, capacity=0, flat=True)


def test_host_model_refuses_bad_arguments():
    hip = pkg('hipops')
    lab = np.zeros(12, np.uint8)
    for kwargs in (dict(zdim=5), dict(classes=255), dict(classes=0), dict(capacity=-1), dict(dtype=torch.int16)):
        args = dict(dict(bs=2, voxel_num=6, zdim=1, classes=CLASSES), **kwargs)
        with pytest.raises((ValueError, TypeError)):
            hip.occ_pairs_host(lab, **args)
    with pytest.raises(ValueError):
        hip.occ_pairs_host(lab[:11], 2, 6, 1, CLASSES)
    with pytest.raises(ValueError):
        hip.occ_pairs_host(lab, 2, 6, 2, CLASSES, row_table=np.zeros((2, 3), np.int32))


def test_gts_view_and_gpu_only_entry():
    hip = pkg('hipops')
    pairs, offsets = torch.zeros(7, 2, dtype=torch.int32), torch.tensor([0, 2, 5], dtype=torch.int32)
    view = hip.OccPairsGts(pairs, offsets)
    assert isinstance(view, hip.PackedOccGts) and view.bs == 2 and view.n_total == 7 and not view.has_invalid
    assert view.pairs is pairs and view.offsets is offsets and view.invalid is None
    with pytest.raises(TypeError):
        hip.OccPairsGts(pairs.float(), offsets)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        hip.occ_pairs(torch.zeros(12, dtype=torch.uint8), 2, 6, 1, CLASSES)


def test_library_validates_arguments_without_a_gpu():
    hip = pkg('hipops')
    lib = hip.lib()
    i, l, ptr = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    assert hip.PROTOTYPES['ver_occ_pairs'] == (i, [ptr] * 3 + [i] + [ptr] * 3 + [l, l, i, i, i, i, ptr])
    assert hip.PROTOTYPES['ver_occ_pairs_blocks'] == (l, [i, l]) and hip.PROTOTYPES['ver_occ_pairs_block_size'] == (l, [])
    block = lib.ver_occ_pairs_block_size()
    assert block == hip.occ_pairs_block_size() and block >= 64
    assert [lib.ver_occ_pairs_blocks(*a) for a in ((0, 100), (3, 0), (-1, 5), (1, 1), (1, block), (1, block + 1), (3, 2 * block + 1))] \
        == [0, 0, 0, 1, 1, 2, 9]
    buf = (ctypes.c_int64 * 8)()                              # a 16-byte aligned host address: the checks only look at pointer
    a = (ctypes.addressof(buf) + 15) & ~15                    # values, and every call below is refused before any launch

    def call(bs=2, voxel_num=70, zdim=35, classes=16, capacity=8, dtype=0, flags=0, labels=a, pairs=a, offsets=a, count=a,
             work=a, table=None):
        return lib.ver_occ_pairs(labels, table, pairs, dtype, offsets, count, work, capacity, voxel_num, zdim, classes, bs, flags, None)

    OK, EINVAL, EUNSUPPORTED = 0, -1, -2
    # zero sizes launch nothing and look at no pointer
    assert call(bs=0, labels=None, pairs=None, offsets=None, count=None, work=None) == OK
    assert call(voxel_num=0, labels=None, pairs=None, offsets=None, count=None, work=None) == OK
    for bad in (dict(bs=-1), dict(voxel_num=-1), dict(zdim=0), dict(classes=0), dict(capacity=-1), dict(dtype=2), dict(flags=2)):
        assert call(**bad) == EINVAL, bad
    assert b'ver_occ_pairs' in lib.ver_last_error()
    for bad in (dict(classes=255), dict(voxel_num=71), dict(bs=4, voxel_num=35 * 2 ** 25), dict(voxel_num=35 * 2 ** 27),
                dict(bs=2, voxel_num=2 ** 30, zdim=1, flags=1), dict(bs=65536, voxel_num=35), dict(capacity=2 ** 31)):
        assert call(**bad) == EUNSUPPORTED, bad
    for bad in (dict(labels=None), dict(offsets=None), dict(count=None), dict(work=None), dict(pairs=None),
                dict(pairs=a + 4), dict(pairs=a + 8, dtype=1), dict(offsets=a + 2), dict(count=a + 1), dict(work=a + 2), dict(table=a + 2)):
        assert call(**bad) == EINVAL, bad
