"""``ver_occ_pairs`` on the GPU against its numpy model (``hipops.occ_pairs_host``): pairs inside the offsets, offsets and
counts as integers, bit for bit; nothing written behind ``offsets[bs]``.

Sizes: a workgroup covers ``occ_pairs_block_size()`` (B) consecutive voxels of one sample, so per ``zdim`` the voxel counts
are the multiples of ``zdim`` nearest to B - 1 from below, B where ``zdim`` divides it, and nearest to B + 1 from above
(``zdim`` = 1 hits all three exactly), plus vocc.py's 14 400 x 35.  Row tables: the plans of ``occ_proj_lattice`` exist for
even lattices only, so the block-edge sizes use ``occ_pairs_helper.group_table`` (the same (offset, n_rows, index)
construction over a random partition); the vocc.py size uses the real plan's table, obtained as ``tests/occ_targets_helper.py``
obtains it."""
import numpy as np
import pytest
import torch

from occ_pairs_helper import CLASSES, expected, group_table, in_rows, volume
from occ_targets_helper import ROWS, Z
from util import pkg

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda'
GUARD = -7


def _check(vol, zdim, table=None, capacity=None, dtype=torch.int32, flat=False, out=None, classes=CLASSES):
    """One kernel call on ``vol`` [bs, voxel_num] (voxel order; moved into row order with ``table``) against the model."""
    hip = pkg('hipops')
    bs, voxel_num = vol.shape
    labels = vol.reshape(-1) if table is None else in_rows(vol, table, zdim)
    want = hip.occ_pairs_host(labels, bs, voxel_num, zdim, classes, table, capacity, flat, dtype)
    dev_table = None if table is None else T(table).to(DEV)
    guarded = out is None
    if out is None:
        cap = bs * voxel_num if capacity is None else capacity
        out = hip.occ_pairs(T(labels).to(DEV), bs, voxel_num, zdim, classes, dev_table, capacity, flat, dtype)
        assert out[0].shape == (cap, 2) and out[0].dtype == dtype
        out[0].fill_(GUARD)                                    # the same call again into guarded buffers
    got = hip.occ_pairs(T(labels).to(DEV), bs, voxel_num, zdim, classes, dev_table, capacity, flat, dtype, out=out)
    assert all(g is o for g, o in zip(got, out))
    torch.cuda.synchronize()
    pairs, offsets, count = (t.cpu().numpy() for t in got)
    assert np.array_equal(offsets, want[1]) and np.array_equal(count, want[2]), (offsets, want[1], count, want[2])
    n = int(offsets[-1])
    assert pairs.dtype == want[0].dtype and np.array_equal(pairs[:n], want[0][:n])
    assert not guarded or (pairs[n:] == GUARD).all()           # nothing behind offsets[bs] was touched
    return got, n


def _edge_sizes(zdim):
    block = pkg('hipops').occ_pairs_block_size()
    sizes = [(block - 1) // zdim * zdim, -(-(block + 1) // zdim) * zdim]
    return sizes + ([block] if block % zdim == 0 else [])


@pytest.mark.parametrize('bs', [1, 3])
@pytest.mark.parametrize('zdim', [1, 5, 35])
def test_block_edges_densities_orders_and_capacities(zdim, bs):
    rng = np.random.default_rng(10 * zdim + bs)
    block = pkg('hipops').occ_pairs_block_size()
    sizes = _edge_sizes(zdim)
    assert min(sizes) < block < max(sizes) and (zdim != 1 or sorted(sizes) == [block - 1, block, block + 1])
    for voxel_num in sizes + [3 * sizes[1]]:                  # (the last: more than two blocks per sample)
        table = group_table(rng, voxel_num // zdim)
        for density in (0.0, 0.02, 1.0):
            vol = volume(rng, bs, voxel_num, density, empty=1, full=2 if density else None, specials=density < 1.0)
            assert density == 1.0 or ((vol == CLASSES).any() and (vol == 255).any())
            total = int((vol < CLASSES).sum())
            for t in (None, table):
                _, n = _check(vol, zdim, t)
                assert n == total
                for capacity in sorted({0, max(total - 1, 0), total}):
                    got, n = _check(vol, zdim, t, capacity=capacity)
                    assert n == capacity and int(got[2][bs + 1]) == int(total > capacity)
            _check(vol, zdim, table, dtype=torch.int64, flat=True)
            _check(vol, zdim, None, dtype=torch.int32, flat=True)
            _check(vol, zdim, None, dtype=torch.int64)


def test_nothing_is_written_past_the_capacity_or_behind_the_offsets():
    hip = pkg('hipops')
    rng = np.random.default_rng(3)
    bs, voxel_num = 3, 2500
    dense, sparse = volume(rng, bs, voxel_num, 0.5), volume(rng, bs, voxel_num, 0.02, empty=0)
    total = int((dense < CLASSES).sum())
    for dtype in (torch.int32, torch.int64):
        # a buffer with room behind the capacity: the kernel sees only the leading `capacity` pairs
        big = torch.full((total + 64, 2), GUARD, dtype=dtype, device=DEV)
        capacity = total - 40
        meta = hip.occ_pairs(T(dense.reshape(-1)).to(DEV), bs, voxel_num, 1, CLASSES, capacity=capacity, dtype=dtype, out=None)[1:]
        got, n = _check(dense, 1, capacity=capacity, dtype=dtype, out=(big[:capacity],) + tuple(meta))
        assert n == capacity and int(got[2][bs + 1]) == 1 and bool((big[capacity:] == GUARD).all())
        # reuse after a call with more pairs: the stale pairs stay where they were, behind offsets[bs]
        out = hip.occ_pairs(T(dense.reshape(-1)).to(DEV), bs, voxel_num, 1, CLASSES, dtype=dtype)
        before = out[0].clone()
        got, n = _check(sparse, 1, dtype=dtype, out=out)
        assert 0 < n < total and torch.equal(got[0][n:], before[n:]) and int(got[2][bs + 1]) == 0
        assert int(got[1][0]) == int(got[1][1]) == 0          # the empty first sample owns an empty slice


@pytest.mark.parametrize('bs', [1, 3])
def test_vocc_size_with_the_plan_table(bs):
    opl = pkg('dense_heads.occ_proj_lattice')
    plan = opl.lattice_plan(128, 4, 60, 60, torch.device(DEV, torch.cuda.current_device()))
    table = opl.row_table(plan)
    assert table.shape == (ROWS, 3)
    rng = np.random.default_rng(bs)
    vol = volume(rng, bs, ROWS * Z, 0.02, empty=1)
    for t, flat, dtype in ((table, False, torch.int32), (table, True, torch.int64), (None, False, torch.int64)):
        _, n = _check(vol, Z, t, flat=flat, dtype=dtype)
        assert n == int((vol < CLASSES).sum())
    got, n = _check(vol, Z, table, capacity=1000)
    assert n == 1000 and int(got[2][bs + 1]) == 1


def test_zero_sizes_and_refusals():
    hip = pkg('hipops')
    empty = torch.zeros(0, dtype=torch.uint8, device=DEV)
    for bs, voxel_num in ((0, 70), (2, 0)):
        pairs, offsets, count = hip.occ_pairs(empty, bs, voxel_num, 35, CLASSES, capacity=4)
        assert pairs.shape == (4, 2) and offsets.tolist() == [0] * (bs + 1) and count.tolist() == [0] * (bs + 2)
    lab = torch.zeros(70, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        hip.occ_pairs(lab, 2, 36, 1, CLASSES)
    with pytest.raises(TypeError):
        hip.occ_pairs(lab.int(), 2, 35, 35, CLASSES)
    with pytest.raises(ValueError):
        hip.occ_pairs(lab, 2, 35, 35, CLASSES, row_table=torch.zeros(2, 3, dtype=torch.int32, device=DEV))
    out = hip.occ_pairs(lab, 2, 35, 35, CLASSES)
    with pytest.raises(ValueError):
        hip.occ_pairs(lab, 2, 35, 35, CLASSES, dtype=torch.int64, out=out)
    with pytest.raises(ValueError, match='2\\^31'):
        hip.occ_pairs(lab, 2, 2 ** 30, 1, CLASSES, capacity=8, flat=True)


def test_capture_and_two_replays_with_different_labels():
    hip = pkg('hipops')
    rng = np.random.default_rng(4)
    bs, zdim, rows = 3, 5, 700
    voxel_num = zdim * rows
    table = group_table(rng, rows)
    vols = [volume(rng, bs, voxel_num, d, empty=e) for d, e in ((0.3, 0), (0.05, 2))]
    labels = torch.empty(bs * voxel_num, dtype=torch.uint8, device=DEV)
    dev_table = T(table).to(DEV)
    labels.copy_(T(in_rows(vols[0], table, zdim)))
    hip.occ_pairs(labels, bs, voxel_num, zdim, CLASSES, dev_table)                # library and allocator warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip.occ_pairs(labels, bs, voxel_num, zdim, CLASSES, dev_table)
    for vol in vols + vols[:1]:
        labels.copy_(T(in_rows(vol, table, zdim)))
        graph.replay()
        torch.cuda.synchronize()
        kept, offsets, count = expected(vol, bs * voxel_num)
        assert np.array_equal(out[1].cpu().numpy(), offsets) and np.array_equal(out[2].cpu().numpy(), count)
        assert np.array_equal(out[0][:int(offsets[-1])].cpu().numpy(), kept)


@pytest.mark.parametrize('with_table', [False, True])
@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_round_trip_through_ver_occ_targets(with_table, dtype):
    hip = pkg('hipops')
    rng = np.random.default_rng(5)
    bs, zdim, rows = 3, 35, 59
    voxel_num = zdim * rows
    vol = volume(rng, bs, voxel_num, 0.2, empty=1, full=2, specials=False)
    table = group_table(rng, rows) if with_table else None
    dev_table = T(table).to(DEV) if with_table else None
    labels = T(in_rows(vol, table, zdim) if with_table else vol.reshape(-1).copy()).to(DEV)
    pairs, offsets, count = hip.occ_pairs(labels, bs, voxel_num, zdim, CLASSES, dev_table, dtype=dtype)
    pairs[int(offsets[-1]):] = GUARD                            # what lies behind offsets[bs] belongs to no sample
    gts = hip.OccPairsGts(pairs, offsets)
    back, back_count, bad = hip.occ_targets(gts.pairs, gts.offsets, voxel_num, zdim, CLASSES, dev_table)
    assert torch.equal(back, labels) and torch.equal(back_count, count[:bs + 1]) and bad.tolist() == [0, 0]
