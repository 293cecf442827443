"""Detection mAP / mAR in the indoor protocol: what the reference's ``MP3DDataset.evaluate``
(mp3docc_dataset.py:304-384) gets from datasets/indoor_eval.py:196 with ``iou_thr = (0.10, 0.25, 0.5, 0.75)``, restated here
on plain arrays -- boxes are [n, 7] = (x, y, z_bottom, dx, dy, dz, yaw), the format of ``head._to_box_type`` and of
``LiDARInstance3DBoxes(..., origin=(0.5, 0.5, 0))``.

Host side (numpy, float64): ``box3d_overlaps_host`` (mmdet3d's ``overlaps(mode='iou')``: height overlap times the area of
the clipped BEV polygon), ``det_match_host`` (the per-image loop of ``eval_det_cls``, indoor_eval.py:54-143),
``average_precision``, ``eval_det`` and ``indoor_eval``.  ``DeviceDetMetrics``: the same statistics from records matched
on the device (``hipops.det_match`` on the boxes of ``head.get_bboxes_padded``), one device->host copy per evaluation.
``det_decode_host``: the host statement of the fused decoding in front of the matcher (``hipops.det_decode``), with its
order on equal scores.

Where this differs from the reference by choice: equal scores are ordered by arrival (image, then slot) -- the reference's
``np.argsort(-confidence)`` leaves ties in no particular order; AP is float64 (the reference rounds it to float32); a box
with a non-finite entry or a dimension <= 0 overlaps nothing.  There is no table printing."""
import collections

import numpy as np

DEFAULT_IOU_THR = (0.10, 0.25, 0.5, 0.75)
_SLOTS = 10            # vertices kept per clipped polygon (a rectangle cut by four half planes has at most 8)

DetRecords = collections.namedtuple('DetRecords', 'scores labels tp_bits npos')
DetRecords.__doc__ = """What AP is computed from: ``scores`` [n], ``labels`` [n] and ``tp_bits`` [n] (bit t: a true positive at
threshold t) of every kept prediction in arrival order, ``npos`` {label: ground truths of that class}."""


def _as_array(x, dtype=None):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


def _corners(boxes):
    """[n, 7] -> BEV corners [n, 4, 2], counter-clockwise, in the dtype of ``boxes``."""
    dt = boxes.dtype
    half = dt.type(0.5)
    c, s = np.cos(boxes[:, 6]), np.sin(boxes[:, 6])
    lx = (boxes[:, 3] * half)[:, None] * np.array([1, -1, -1, 1], dtype=dt)
    ly = (boxes[:, 4] * half)[:, None] * np.array([1, 1, -1, -1], dtype=dt)
    px = boxes[:, 0, None] + c[:, None] * lx - s[:, None] * ly
    py = boxes[:, 1, None] + s[:, None] * lx + c[:, None] * ly
    return np.stack([px, py], -1)


def _clip(poly, cnt, c0, c1):
    """One Sutherland-Hodgman step for N polygons at once: keep the side of the line c0 -> c1 [N, 2] to its left.
    poly [N, _SLOTS, 2] with ``cnt`` [N] live vertices -> the same."""
    m = poly.shape[1]
    slot = np.arange(m)[None, :]
    live = slot < cnt[:, None]
    before = np.where(slot == 0, np.maximum(cnt[:, None] - 1, 0), slot - 1)
    e = c1 - c0
    d_cur = e[:, None, 0] * (poly[..., 1] - c0[:, None, 1]) - e[:, None, 1] * (poly[..., 0] - c0[:, None, 0])
    d_prev = np.take_along_axis(d_cur, before, 1)
    prev = np.take_along_axis(poly, before[..., None], 1)
    in_cur, in_prev = d_cur >= 0, d_prev >= 0
    crosses = live & (in_cur != in_prev)
    den = np.where(crosses, d_prev - d_cur, poly.dtype.type(1))
    t = np.where(crosses, d_prev / den, poly.dtype.type(0))
    cut = prev + t[..., None] * (poly - prev)
    emit = np.stack([cut, poly], 2).reshape(poly.shape[0], 2 * m, 2)          # per edge: the cut point, then its end point
    keep = np.stack([crosses, live & in_cur], 2).reshape(poly.shape[0], 2 * m)
    order = np.argsort(~keep, axis=1, kind='stable')[:, :m]
    return np.take_along_axis(emit, order[..., None], 1), np.minimum(keep.sum(1), m)


def _bev_intersection(ca, cb):
    """Areas [N] of the intersections of N pairs of convex counter-clockwise quadrilaterals [N, 4, 2]."""
    n = ca.shape[0]
    poly = np.zeros((n, _SLOTS, 2), dtype=ca.dtype)
    poly[:, :4] = ca
    cnt = np.full(n, 4)
    for k in range(4):
        poly, cnt = _clip(poly, cnt, cb[:, k], cb[:, (k + 1) % 4])
    slot = np.arange(_SLOTS)[None, :]
    nxt = np.where(slot + 1 >= cnt[:, None], 0, slot + 1)
    q = np.take_along_axis(poly, nxt[..., None], 1)
    terms = np.where(slot < cnt[:, None], poly[..., 0] * q[..., 1] - q[..., 0] * poly[..., 1], poly.dtype.type(0))
    return np.abs(terms.sum(1)) * poly.dtype.type(0.5)


def _usable(boxes):
    return np.isfinite(boxes).all(1) & (boxes[:, 3:6] > 0).all(1)


def box3d_overlaps_host(a, b, dtype=np.float64):
    """IoU [n, m] of the rotated boxes a [n, 7] and b [m, 7] (mmdet3d ``overlaps(mode='iou')``, indoor_eval.py:102):
    ``o = bev * h`` with ``h = max(0, min(za + dza, zb + dzb) - max(za, zb))`` and ``bev`` the area of the Sutherland-Hodgman
    clip of the two BEV rectangles; ``iou = o / max(va + vb - o, 1e-8)``.  A box with a non-finite entry or a dimension
    <= 0 gives 0.  ``dtype``: the arithmetic's precision (float32 runs the same model in single precision, the yardstick
    of the kernel's rounding)."""
    dt = np.dtype(dtype)
    a, b = _as_array(a, dt).reshape(-1, 7), _as_array(b, dt).reshape(-1, 7)
    n, m = a.shape[0], b.shape[0]
    if n == 0 or m == 0:
        return np.zeros((n, m), dtype=dt)
    ok_a, ok_b = _usable(a), _usable(b)
    unit = np.array([0, 0, 0, 1, 1, 1, 0], dtype=dt)
    a, b = np.where(ok_a[:, None], a, unit), np.where(ok_b[:, None], b, unit)
    ia, ib = np.repeat(np.arange(n), m), np.tile(np.arange(m), n)
    bev = _bev_intersection(_corners(a)[ia], _corners(b)[ib]).reshape(n, m)
    top = np.minimum((a[:, 2] + a[:, 5])[:, None], (b[:, 2] + b[:, 5])[None, :])
    h = np.maximum(top - np.maximum(a[:, 2, None], b[None, :, 2]), dt.type(0))
    o = bev * h
    vol = (a[:, 3] * a[:, 4] * a[:, 5])[:, None] + (b[:, 3] * b[:, 4] * b[:, 5])[None, :]
    iou = o / np.maximum(vol - o, dt.type(1e-8))
    return np.where(ok_a[:, None] & ok_b[None, :], iou, dt.type(0))


def det_match_host(pred_boxes, pred_labels, pred_scores, pred_valid, gt_boxes, gt_labels, ngt, thresholds, num_classes=None,
                   dtype=np.float64):
    """The per-image loop of ``eval_det_cls`` on padded arrays (the host statement of ``ver_det_match``): pred_* [S, P(, 7)],
    gt_* [S, G(, 7)], ngt [S] -> (iou_max float64 [S, P], gt_index int32 [S, P], tp_bits uint8 [S, P], {label: valid ground
    truths}).  Every sample's valid predictions are visited in (score descending, slot ascending) order; each takes the
    same-class ground truth of its sample with the largest IoU (the first of equal ones) and is a true positive at threshold
    t when that IoU is above it and no earlier prediction has marked that ground truth as detected at t -- it never falls back
    to a second best.  ``pred_valid == 0`` or a label outside [0, num_classes) (``None``: no upper end): matches nothing."""
    pred_boxes, gt_boxes = _as_array(pred_boxes), _as_array(gt_boxes)
    pred_labels, gt_labels = _as_array(pred_labels).astype(np.int64), _as_array(gt_labels).astype(np.int64)
    pred_scores, pred_valid, ngt = _as_array(pred_scores), _as_array(pred_valid), _as_array(ngt)
    s_count, p_cap = pred_labels.shape
    g_cap = gt_labels.shape[1]
    thr = [float(t) for t in thresholds]

    def in_range(lab):
        return (lab >= 0) & ((lab < num_classes) if num_classes is not None else True)

    iou_max = np.zeros((s_count, p_cap))
    gt_index = np.full((s_count, p_cap), -1, dtype=np.int32)
    tp_bits = np.zeros((s_count, p_cap), dtype=np.uint8)
    npos = collections.Counter()
    for s in range(s_count):
        n = int(min(max(int(ngt[s]), 0), g_cap))
        glab = gt_labels[s, :n]
        g_ok = in_range(glab)
        npos.update(glab[g_ok].tolist())
        live = (pred_valid[s] != 0) & in_range(pred_labels[s])
        if not n or not live.any():
            continue
        iou = box3d_overlaps_host(pred_boxes[s], gt_boxes[s, :n], dtype)
        detected = np.zeros((len(thr), n), dtype=bool)
        for d in np.argsort(-pred_scores[s], kind='stable'):
            if not live[d]:
                continue
            best, jmax = -np.inf, -1
            for j in np.nonzero(g_ok & (glab == pred_labels[s, d]))[0]:
                if iou[d, j] > best:
                    best, jmax = iou[d, j], j
            if jmax < 0:
                continue
            iou_max[s, d], gt_index[s, d] = best, jmax
            for t, value in enumerate(thr):
                if best > value and not detected[t, jmax]:
                    detected[t, jmax] = True
                    tp_bits[s, d] |= 1 << t
    return iou_max, gt_index, tp_bits, dict(npos)


def det_decode_host(cls, box, center_range, score_threshold=None, bottom_center=True, k=None):
    """The host statement of ``ver_det_decode`` (``hipops.det_decode``), float64 numpy: cls [B, Q, C] logits (any float
    dtype; a torch bf16 tensor is widened exactly) or None (the layout form: every query in order, scores and labels 0),
    box [B, Q, 8 | 10] normalised codes, ``center_range`` six numbers and ``score_threshold`` (both rounded to float32 first:
    that is what the kernel and torch's comparison of a float32 tensor with a Python number see).
    -> (boxes float64 [B, K, 7 | 9], scores float64 [B, K], labels int32, valid uint8, query int32 [B, K]).
    Slot j is the j-th entry of the flattened [Q * C] logits in (logit descending, flat index ascending) order -- a stable
    argsort of the negated logits, which leaves a NaN after every number and -0.0 equal to +0.0.  ``valid``: the gravity
    centre inside the range (inclusive), the score above the threshold, the logit not a NaN."""
    if hasattr(box, 'detach'):
        box = box.detach().double().cpu().numpy()
    box = np.asarray(box, np.float64)
    if box.ndim != 3 or box.shape[-1] not in (8, 10):
        raise ValueError('det_decode_host: box must be [B, Q, 8 | 10] normalised codes, got %s' % (box.shape,))
    bs, nq, codes = box.shape
    if cls is not None:
        if hasattr(cls, 'detach'):
            cls = cls.detach().double().cpu().numpy()
        logits = np.asarray(cls, np.float64).reshape(bs, nq, -1)
        ncls = logits.shape[2]
        flat = logits.reshape(bs, nq * ncls)
        k = min(nq * ncls, 1024) if k is None else int(k)
        if not 1 <= k <= nq * ncls:
            raise ValueError('det_decode_host: k=%d of %d logits' % (k, nq * ncls))
        index = np.argsort(-flat, axis=1, kind='stable')[:, :k]
        picked = np.take_along_axis(flat, index, 1)
        with np.errstate(over='ignore'):
            scores = 1.0 / (1.0 + np.exp(-picked))
        labels, query = index % ncls, index // ncls
        number = ~np.isnan(picked)
    else:
        k = nq if k is None else int(k)
        if k != nq:
            raise ValueError('det_decode_host: the layout form decodes every query: k=%d, Q=%d' % (k, nq))
        query = np.tile(np.arange(nq), (bs, 1))
        labels, scores, number = np.zeros((bs, nq), np.int64), np.zeros((bs, nq)), np.ones((bs, nq), bool)
    rows = np.take_along_axis(box, query[..., None], 1)
    with np.errstate(over='ignore', invalid='ignore'):
        dims = np.exp(rows[..., [2, 3, 5]])
        yaw = np.arctan2(rows[..., 6], rows[..., 7])
    centre = rows[..., [0, 1, 4]]
    rng = np.asarray([float(v) for v in center_range], np.float32).astype(np.float64)
    with np.errstate(invalid='ignore'):
        valid = number & (centre >= rng[:3]).all(-1) & (centre <= rng[3:]).all(-1)
        if score_threshold is not None:
            valid &= scores > float(np.float32(score_threshold))
    z = centre[..., 2] - 0.5 * dims[..., 2] if bottom_center else centre[..., 2]
    parts = [centre[..., 0], centre[..., 1], z, dims[..., 0], dims[..., 1], dims[..., 2], yaw]
    if codes == 10:
        parts += [rows[..., 8], rows[..., 9]]
    return np.stack(parts, -1), scores, labels.astype(np.int32), valid.astype(np.uint8), query.astype(np.int32)


def average_precision(recalls, precisions, mode='area'):
    """AP of a recall / precision curve ([n] or [curves, n]) -> float64 [curves].  'area': the area under the precision
    envelope (precision made non-increasing from the right) between recall 0 and 1; '11points': the mean of the best
    precision at recall >= 0, 0.1, ..., 1."""
    recalls, precisions = np.atleast_2d(np.asarray(recalls, dtype=np.float64)), np.atleast_2d(np.asarray(precisions, dtype=np.float64))
    if recalls.shape != precisions.shape or recalls.ndim != 2:
        raise ValueError('average_precision: recalls %s and precisions %s' % (recalls.shape, precisions.shape))
    ap = np.zeros(recalls.shape[0])
    if mode == 'area':
        for i, (rec, pre) in enumerate(zip(recalls, precisions)):
            mrec = np.concatenate([[0.0], rec, [1.0]])
            mpre = np.maximum.accumulate(np.concatenate([[0.0], pre, [0.0]])[::-1])[::-1]
            step = np.nonzero(mrec[1:] != mrec[:-1])[0]
            ap[i] = np.sum((mrec[step + 1] - mrec[step]) * mpre[step + 1])
    elif mode == '11points':
        for i, (rec, pre) in enumerate(zip(recalls, precisions)):
            for level in np.arange(0, 1 + 1e-3, 0.1):
                above = pre[rec >= level]
                ap[i] += above.max() if above.size else 0.0
            ap[i] /= 11
    else:
        raise ValueError('Unrecognized mode, only "area" and "11points" are supported')
    return ap


def _annos_to_records(gt_annos, dt_annos, iou_thr):
    """Match every image of the two lists (``det_match_host``, one image at a time) -> ``DetRecords``."""
    if len(gt_annos) != len(dt_annos):
        raise ValueError('%d ground-truth and %d detection annotations' % (len(gt_annos), len(dt_annos)))
    scores, labels, bits, npos = [], [], [], collections.Counter()
    for gt, dt in zip(gt_annos, dt_annos):
        pb = _as_array(dt['boxes_3d'], np.float64).reshape(-1, 7)
        pl = _as_array(dt['labels_3d']).astype(np.int64).reshape(-1)
        ps = _as_array(dt['scores_3d']).reshape(-1)
        gl = _as_array(gt['class']).astype(np.int64).reshape(-1) if gt.get('gt_num', 1) != 0 else np.zeros(0, np.int64)
        gb = _as_array(gt['gt_boxes_upright_depth'], np.float64).reshape(-1, 7)[:len(gl)] if len(gl) else np.zeros((0, 7))
        if (pl < 0).any() or (gl < 0).any():
            raise ValueError('indoor_eval: negative class label')
        if len(pl):
            _, _, tp, count = det_match_host(pb[None], pl[None], ps[None], np.ones((1, len(pl)), np.uint8), gb[None], gl[None],
                                             [len(gl)], iou_thr)
            bits.append(tp[0])
        else:
            count = collections.Counter(gl.tolist())
        npos.update(count)
        scores.append(ps)
        labels.append(pl)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)   # noqa: E731
    return DetRecords(cat(scores, np.float64), cat(labels, np.int64), cat(bits, np.uint8), dict(npos))


def eval_det(records_or_lists, iou_thr=DEFAULT_IOU_THR):
    """Recall, precision and AP per class and threshold: {label: [(recall [n], precision [n], ap float64 [1]) per
    threshold]} from ``DetRecords`` or from the pair of lists ``(gt_annos, dt_annos)`` of ``indoor_eval``.  The classes are
    the union of the predicted and the ground-truth labels (indoor_eval.py:237-244).  A class nobody predicted gets recall,
    precision and AP 0 (``np.zeros(1)``); a class with predictions and NO ground truth gets NaN recall and AP through the
    same numpy expressions as the reference's (``tp / 0``)."""
    rec = records_or_lists if isinstance(records_or_lists, DetRecords) else _annos_to_records(*records_or_lists, iou_thr)
    scores, labels, bits = np.asarray(rec.scores, np.float64), np.asarray(rec.labels, np.int64), np.asarray(rec.tp_bits)
    out = {}
    for label in sorted(set(labels.tolist()) | {int(c) for c, n in rec.npos.items() if n > 0}):
        pick = np.nonzero(labels == label)[0]
        if not len(pick):
            out[label] = [(np.zeros(1), np.zeros(1), np.zeros(1)) for _ in iou_thr]
            continue
        pick = pick[np.argsort(-scores[pick], kind='stable')]                      # score descending, then arrival
        npos = float(rec.npos.get(label, 0))
        out[label] = []
        for t in range(len(iou_thr)):
            hit = ((bits[pick] >> t) & 1).astype(np.float64)
            tp, fp = np.cumsum(hit), np.cumsum(1.0 - hit)
            with np.errstate(divide='ignore', invalid='ignore'):
                recall = tp / npos
            precision = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
            out[label].append((recall, precision, average_precision(recall, precision)))
    return out


def _result_dict(per_class, iou_thr, label2cat):
    name = (lambda c: label2cat[c]) if label2cat is not None else str
    ret = {}
    for t, value in enumerate(iou_thr):
        aps, recs = [], []
        for label, curves in per_class.items():
            recall, _, ap = curves[t]
            ret['%s_AP_%.2f' % (name(label), value)] = float(ap[0])
            ret['%s_rec_%.2f' % (name(label), value)] = float(recall[-1])
            aps.append(float(ap[0]))
            recs.append(float(recall[-1]))
        ret['mAP_%.2f' % value] = float(np.mean(aps)) if aps else float('nan')
        ret['mAR_%.2f' % value] = float(np.mean(recs)) if recs else float('nan')
    return ret


def indoor_eval(gt_annos, dt_annos, metric=DEFAULT_IOU_THR, label2cat=None):
    """The reference's ``indoor_eval`` (datasets/indoor_eval.py:196) on plain arrays.  ``gt_annos[i]``: dict(gt_num,
    gt_boxes_upright_depth [n, 7], class [n]); ``dt_annos[i]``: dict(boxes_3d [k, 7], scores_3d [k], labels_3d [k]) of the
    same image; ``metric``: the IoU thresholds; ``label2cat``: {label: name} (``None``: the label's number).
    -> {'<cat>_AP_<thr>', '<cat>_rec_<thr>', 'mAP_<thr>', 'mAR_<thr>'} with thr as '%.2f'; recall is the last point of the
    class's recall curve.  NaN for a class with predictions and no ground truth (``eval_det``)."""
    return _result_dict(eval_det((gt_annos, dt_annos), metric), metric, label2cat)


class DeviceDetMetrics:
    """Detection mAP / mAR of a validation run with the matching done where the head's outputs are.  ``add`` queues launches
    only: ``head.get_bboxes_padded`` (one top-k for the batch) and ``hipops.det_match`` (one workgroup per sample), keeps
    the batch's (scores, labels, valid, tp_bits) on the device and accumulates ``npos`` there.  ``get_stats`` makes ONE
    device->host copy, drops the invalid slots, orders each class by (score descending, arrival) and computes AP in float64
    with the host functions above -> the dict of ``indoor_eval``.  ``state`` / ``merge`` combine shards (``gather``: over the
    ranks of a process group).  CPU tensors: the same plumbing with ``det_match_host`` in place of the kernel."""

    def __init__(self, num_classes, iou_thr=DEFAULT_IOU_THR, device=None):
        import torch
        self.num_classes = int(num_classes)
        self.iou_thr = tuple(float(t) for t in iou_thr)
        if not 1 <= len(self.iou_thr) <= 8:
            raise ValueError('DeviceDetMetrics: %d thresholds (1..8: one bit each)' % len(self.iou_thr))
        self.npos = torch.zeros(self.num_classes, dtype=torch.int64, device=device)
        self._parts = []               # in arrival order: device tuples (scores, labels, valid, tp_bits) | host states

    def add(self, head, preds_dicts, gts, fused=False):
        """Count one batch: the head's ``preds_dicts`` against ``gts``, a ``PaddedGts`` (``head.pad_gts``) whose boxes are
        (x, y, z_bottom, dx, dy, dz, yaw[, ...]).  ``fused``: decode with ``hipops.det_decode`` -- decoder outputs to
        records in two launches of ours, equal scores in a stated order (``head.get_bboxes_padded(fused=True)``)."""
        boxes, scores, labels, valid = head.get_bboxes_padded(preds_dicts, fused=True) if fused else head.get_bboxes_padded(preds_dicts)
        return self.add_padded(boxes, scores, labels, valid, gts)

    def add_padded(self, boxes, scores, labels, valid, gts):
        import torch
        with torch.no_grad():
            pb, gb = boxes[..., :7].float().contiguous(), gts.boxes[..., :7].float().contiguous()
            pl, gl, ps = labels.to(torch.int32), gts.labels.to(torch.int32), scores.float()
            if self.npos.device != pb.device:
                self.npos = self.npos.to(pb.device)
            if pb.is_cuda:
                from .hipops import det_match
                _, _, bits = det_match(pb, pl, ps, valid, gb, gl, gts.counts, self.iou_thr, self.npos)
            else:
                _, _, bits, count = det_match_host(pb, pl, ps, valid, gb, gl, gts.counts, self.iou_thr, self.num_classes)
                bits = torch.from_numpy(bits)
                for label, n in count.items():
                    self.npos[label] += n
            self._parts.append((ps.reshape(-1), pl.reshape(-1), valid.reshape(-1), bits.reshape(-1)))
        return self

    def state(self):
        """Everything counted so far on the host (one device->host copy): dict(scores float64 [n], labels int64 [n], tp_bits
        uint8 [n] of the VALID slots in arrival order, npos int64 [num_classes])."""
        import torch
        dev = [p for p in self._parts if isinstance(p, tuple)]
        flat = torch.cat([torch.stack([t.double() for t in p], 1).reshape(-1) for p in dev] + [self.npos.double()])
        flat = flat.cpu().numpy()                      # scores, labels, flags and counts are all exact in float64
        at, rows, npos = 0, [], flat[len(flat) - self.num_classes:].astype(np.int64)
        for p in self._parts:
            if isinstance(p, tuple):
                n = p[0].numel()
                block = flat[at:at + 4 * n].reshape(n, 4)
                at += 4 * n
                rows.append(block[block[:, 2] != 0][:, [0, 1, 3]])
            else:
                rows.append(np.stack([p['scores'], p['labels'].astype(np.float64), p['tp_bits'].astype(np.float64)], 1))
                npos = npos + p['npos']
        rows = np.concatenate(rows) if rows else np.zeros((0, 3))
        return dict(scores=rows[:, 0].copy(), labels=rows[:, 1].astype(np.int64), tp_bits=rows[:, 2].astype(np.uint8), npos=npos)

    def merge(self, state):
        """Append the records of another shard (its ``state()``) after what was counted here so far."""
        if len(state['npos']) != self.num_classes:
            raise ValueError('merge: a state of %d classes into %d' % (len(state['npos']), self.num_classes))
        self._parts.append({k: np.asarray(v) for k, v in state.items()})
        return self

    def gather(self, group=None):
        """Collect the records of every rank of ``group`` on every rank, in rank order (``all_gather_object`` of the CPU
        states, at the end of an evaluation); a no-op without a process group."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            states = [None] * dist.get_world_size(group)
            dist.all_gather_object(states, self.state(), group=group)
            self.reset()
            for st in states:
                self.merge(st)
        return self

    def records(self):
        st = self.state()
        bad = (st['labels'] < 0) | (st['labels'] >= self.num_classes)
        if bad.any():
            raise ValueError('DeviceDetMetrics: predicted label %d outside [0, %d)' % (int(st['labels'][bad][0]), self.num_classes))
        return DetRecords(st['scores'], st['labels'], st['tp_bits'], {c: int(n) for c, n in enumerate(st['npos']) if n})

    def get_stats(self, label2cat=None):
        """The dict of ``indoor_eval`` for everything added or merged so far."""
        return _result_dict(eval_det(self.records(), self.iou_thr), self.iou_thr, label2cat)

    def reset(self):
        self.npos.zero_()
        self._parts = []
