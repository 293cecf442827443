"""Shared by tests/test_occ_pairs_cpu.py and tests/test_occ_pairs_gpu.py: label volumes, group-major row tables of any row
count, and the plain ``np.nonzero`` statement of the pairs."""
import numpy as np

CLASSES = 16


def group_table(rng, rows, groups=3):
    """int32 [rows, 3] = (group offset, group n_rows, index within the group), built as ``occ_proj_lattice.row_table`` builds
    it from a plan's groups -- here from a random partition of the ``rows`` positions into ``groups`` groups (one may be
    empty), so that any row count has a table, not only the even lattices a plan exists for."""
    cuts = np.sort(rng.integers(0, rows + 1, groups - 1))
    members = np.split(rng.permutation(rows), cuts)
    table = np.empty((rows, 3), dtype=np.int32)
    offset = 0
    for m in members:
        table[m, 0], table[m, 1], table[m, 2] = offset, len(m), np.arange(len(m))
        offset += len(m)
    return table


def volume(rng, bs, voxel_num, density, classes=CLASSES, empty=None, full=None, specials=True):
    """uint8 [bs, voxel_num] in voxel order: ``density`` of the voxels occupied with random classes, the rest ``classes``
    (empty); with ``specials`` a few voxels are 255 (invalid) or a byte between the two; sample ``empty`` has no occupied
    voxel, sample ``full`` only occupied ones."""
    vol = np.full((bs, voxel_num), classes, dtype=np.uint8)
    occupied = rng.random((bs, voxel_num)) < density
    vol[occupied] = rng.integers(0, classes, int(occupied.sum()))
    if specials and voxel_num:
        other = rng.random((bs, voxel_num)) < 0.01
        vol[other] = rng.choice(np.array([255, classes + 1, 254], dtype=np.uint8), int(other.sum()))
        vol[:, 0] = np.where(np.arange(bs) % 2 == 0, 255, vol[:, 0])
    if empty is not None and empty < bs:
        vol[empty] = np.where(vol[empty] < classes, classes, vol[empty])
    if full is not None and full < bs:
        vol[full] = rng.integers(0, classes, voxel_num)
    return vol


def in_rows(vol, table, zdim):
    """The bytes of ``vol`` [bs, voxel_num] where the row order puts them (the formula of ``ver_occ_targets``), flat."""
    bs, voxel_num = vol.shape
    rows = voxel_num // zdim
    z, q = np.divmod(np.arange(voxel_num, dtype=np.int64), rows)
    t = table.astype(np.int64)
    where = ((bs * t[q, 0])[None] + np.arange(bs, dtype=np.int64)[:, None] * t[q, 1][None] + t[q, 2][None]) * zdim + z[None]
    out = np.empty(bs * voxel_num, dtype=np.uint8)
    out[where.reshape(-1)] = vol.reshape(-1)
    return out


def plain_pairs(vol, classes=CLASSES, flat=False):
    """The pairs as the reference states them, per sample: ``idx = nonzero(cls < C); stack(idx, cls[idx])``."""
    out = []
    for b, v in enumerate(vol):
        idx, = np.nonzero(v < classes)
        out.append(np.stack([idx + (b * vol.shape[1] if flat else 0), v[idx].astype(np.int64)], axis=1))
    return out


def expected(vol, capacity, classes=CLASSES, flat=False):
    """(kept pairs [min(total, capacity), 2] int64, offsets, count) from ``plain_pairs``."""
    per = plain_pairs(vol, classes, flat)
    n = np.array([len(p) for p in per], dtype=np.int64)
    total = int(n.sum())
    kept = (np.concatenate(per) if per else np.zeros((0, 2), np.int64))[:capacity]
    offsets = np.minimum(np.concatenate([[0], np.cumsum(n)]), capacity).astype(np.int32)
    count = np.concatenate([n, [total, int(total > capacity)]]).astype(np.int32)
    return kept, offsets, count
