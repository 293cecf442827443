"""Occupancy labels of the head, in one place: the two forms they come in (a dense tensor in the reference's (Z, X, Y)
voxel order, or an ``OccupancyTargets``), the one permutation between that order and the row order of the occupancy GEMMs,
the ``(labels, normaliser)`` pair the occupancy loss takes, the dense builder behind ``occupancy_targets`` /
``occupancy_eval_labels``, and the classification rule of ``get_occupancy_prediction`` as torch ops."""
import torch

from .occ_proj_lattice import rows_to_voxels, voxels_to_rows


class OccupancyTargets:
    """Occupancy targets of a batch in static shapes, as ``VoxelFormerOccupancyHead.occupancy_targets_device`` builds them
    from the sparse annotation in one launch sequence (``hipops.occ_targets``); accepted wherever the dense ``[bs,
    voxel_num]`` tensor is.  ``labels`` uint8 [bs * voxel_num]: ``classes`` = empty, 255 = not evaluated; ``order`` says where
    a voxel's byte sits: ``'voxels'`` = the reference's (Z, X, Y) order per sample, ``'rows'`` = the group-major row order
    of the occupancy GEMMs of ``plan`` (the bytes the loss kernels read next to the logit rows, as they are).  ``count``
    int32 [bs + 1]: occupied voxels per sample and their total (``count[-1]`` is the losses' ``avg_factor``); ``bad`` int32
    [2]: rejected pairs, and listings of a voxel that lost to a larger class."""

    def __init__(self, labels, count, bad, order, bs, plan=None, zdim=1):
        if order not in ('rows', 'voxels') or (order == 'rows' and plan is None):
            raise ValueError("OccupancyTargets: order is 'voxels', or 'rows' with the plan the rows belong to")
        self.labels, self.count, self.bad, self.order, self.bs, self.plan, self.zdim = labels, count, bad, order, bs, plan, zdim

    def check(self):
        """Read ``bad`` on the host (a device -> host synchronisation) and raise ``ValueError`` when a counter is set."""
        rejected, lost = (int(v) for v in self.bad.tolist())
        if rejected or lost:
            what = []
            if rejected:
                what.append('bad[0] = %d: pairs or invalid voxels with an index or a class out of range were skipped '
                            '(the reference raises on them)' % rejected)
            if lost:
                what.append('bad[1] = %d: listings of a voxel that lost to a larger class of the same voxel' % lost)
            raise ValueError('occupancy annotation: ' + '; '.join(what))
        return self

    def ordered(self, order, plan=None):
        """``labels`` (uint8 [bs * voxel_num]) in ``order``: as they are when that is their order, else permuted once with
        the plan's row maps -- the only place where targets of this kind change their order."""
        if order == self.order and (order == 'voxels' or plan is self.plan):
            return self.labels
        voxels = self.labels
        if self.order == 'rows':
            voxels = rows_to_voxels(self.labels.view(-1, self.zdim), self.plan, self.bs).permute(0, 2, 1).reshape(-1)
        if order == 'voxels':
            return voxels
        return labels_in_rows(voxels, plan, self.bs, self.zdim).reshape(-1)


def labels_in_rows(labels, plan, bs, zdim, dtype=None):
    """Labels in the row order of ``plan``, [bs * plan.rows, zdim] next to logit rows [bs * plan.rows, zdim, classes]:
    ``labels`` is a dense tensor of bs * zdim * plan.rows voxels in the reference's (Z, X, Y) order per sample, or an
    ``OccupancyTargets``.  The one statement of that permutation.  ``dtype``: dense labels are cast to it before their
    rows are gathered (an ``OccupancyTargets`` holds bytes)."""
    if isinstance(labels, OccupancyTargets):
        return labels.ordered('rows', plan).view(-1, zdim)
    gt = labels.reshape(bs, zdim, plan.rows).permute(0, 2, 1)                  # (Z, X, Y) order -> [bs, X*Y, Z]
    return voxels_to_rows(gt if dtype is None else gt.to(dtype), plan, bs)


def labels_in_voxels(labels):
    """Labels in the reference's (Z, X, Y) voxel order: a dense tensor as it is, an ``OccupancyTargets`` through ``ordered``."""
    return labels.ordered('voxels') if isinstance(labels, OccupancyTargets) else labels


def narrow_labels(labels):
    """int64 labels -> bytes for a head with fewer than 255 classes: clamped into [-1, 255] before the narrowing cast, so
    that an out-of-range value stays out of range as a byte (-1 -> 255, >= 256 -> 255: both reach the loss kernel's own
    check as invalid labels) instead of wrapping into a valid class."""
    return labels.clamp(-1, 255).to(torch.uint8)


def count_occupied(occupied, by_words=True):
    """Number of set entries of a bool mask, as an fp32 scalar tensor (the occupancy loss's ``avg_factor``)."""
    if by_words and occupied.numel() % 8 == 0:
        # the count of a 0/1 byte mask, eight bytes at a time: (word * 0x0101...01) >> 56 is the sum of the word's bytes
        # (exact; the reduction kernel reads a bool tensor one byte per lane: 0.46 ms for 97 M labels against 0.05)
        words = occupied.view(torch.uint8).view(torch.int64)
        return ((words * 0x0101010101010101) >> 56).sum() * 1.0
    return occupied.sum() * 1.0


def loss_labels(labels, classes, plan=None, bs=None, zdim=1, as_bytes=False):
    """``(gt, avg)`` of the occupancy loss: one label per logit row, flat, and the number of occupied voxels.  ``labels``: a
    dense tensor in the reference's voxel order or an ``OccupancyTargets``; ``plan``: the logits are in that plan's row order
    (``bs`` samples of ``zdim`` layers), None: in the voxel order.  ``as_bytes``: for a consumer whose kernels read byte
    labels as they are -- the fused MLP + focal-loss Function (ver_focal_loss_forward_grad_u8), and ``FocalLoss`` on the GPU
    for the labels of an ``OccupancyTargets`` (ver_focal_loss_forward_u8 / _backward_u8); otherwise for the torch formulas
    of the registered loss (``F.one_hot``), which index with int64 -- the bytes of an ``OccupancyTargets`` are widened."""
    if isinstance(labels, OccupancyTargets):
        # byte labels in either order and the occupied count: nothing to clamp, narrow or reduce
        gt = labels.ordered('rows' if plan is not None else 'voxels', plan)
        return (gt if as_bytes else gt.long()), labels.count[-1] * 1.0
    # the labels are permuted into the GEMMs' row order and counted as BYTES (17 classes): int64 labels made the permutation
    # and the count three passes over 0.77 GB each at 192 viewpoints (1.4 ms; now 0.3 with the narrowing copy)
    narrow = as_bytes and labels.is_cuda and labels.dtype == torch.int64 and classes < 255
    gt = narrow_labels(labels) if narrow else labels
    if plan is not None:
        gt = labels_in_rows(gt, plan, bs, zdim)
    gt = gt.reshape(-1)
    return gt, count_occupied(gt < classes, by_words=narrow)


def dense_labels(occ_gts, invalid, dtype, classes, voxel_num, device):
    """The sparse annotation as a dense ``dtype`` [bs, voxel_num] tensor on ``device`` in the reference's voxel order:
    ``occ_gts[b]`` is an ``[n, 2]`` array of (flat voxel index, class) pairs of the occupied voxels (or the reference's
    one-element list around it), every other voxel gets ``classes`` = empty; the voxels of ``invalid[b]`` (``invalid`` or
    an entry may be None) get 255 = not evaluated."""
    gt = torch.full((len(occ_gts), voxel_num), classes, dtype=dtype, device=device)
    for b, pairs in enumerate(occ_gts):
        if isinstance(pairs, (list, tuple)):                   # occ_gts[bs][queue_index]
            pairs = pairs[0]
        pairs = torch.as_tensor(pairs).long().to(device)
        if pairs.numel():
            gt[b, pairs[:, 0]] = pairs[:, 1].to(dtype)
        skipped = invalid[b] if invalid is not None else None
        if skipped is not None:
            skipped = torch.as_tensor(skipped).long().reshape(-1).to(device)
            if skipped.numel():
                gt[b, skipped] = 255
    return gt


def classify(logits, threshold):
    """The prediction rule of the reference's ``get_occupancy_prediction`` (head:1505-1540, focal-loss branch) on logits
    [N, classes]: fp32 sigmoid, the threshold as an extra "empty" column, arg-max -> int64 [N], ``classes`` = empty."""
    p = logits.float().sigmoid()
    return torch.cat((p, torch.full_like(p[:, :1], threshold)), dim=-1).argmax(dim=-1)
