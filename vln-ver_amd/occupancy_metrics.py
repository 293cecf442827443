"""Occupancy post-processing metrics ("next" row 4 of SURVEY.md 8f): confusion-matrix IoU / mIoU
as the reference's datasets/occupancy_metrics.py:3-90 (``SSCMetrics``; class ``n_classes-1``... the
LAST row/column of the histogram is the empty class).  ``DeviceSSCMetrics``: the same statistics from histograms
counted on the device (ver_occ_confusion), for several thresholds, summed over DDP ranks."""
import numpy as np


class SSCMetrics:
    def __init__(self, n_classes=17):
        self.n_classes = n_classes
        self.empty_label = n_classes
        self.hist = np.zeros((n_classes, n_classes))

    @staticmethod
    def hist_info(n_cl, pred, gt):
        """rows = reference label, cols = prediction; labels outside [0, n_cl) are ignored."""
        assert pred.shape == gt.shape
        k = (gt >= 0) & (gt < n_cl)
        hist = np.bincount(n_cl * gt[k].astype(int) + pred[k].astype(int), minlength=n_cl ** 2)
        return hist.reshape(n_cl, n_cl), int(np.sum(pred[k] == gt[k])), int(np.sum(k))

    def add_batch(self, y_pred, y_true, visible_mask=None):
        y_pred, y_true = np.asarray(y_pred).flatten(), np.asarray(y_true).flatten()
        if visible_mask is not None:
            keep = np.asarray(visible_mask).flatten() == 1
            y_pred, y_true = y_pred[keep], y_true[keep]
        self.hist = self.hist + self.hist_info(self.n_classes, y_pred, y_true)[0]

    def get_stats(self):
        d = np.diag(self.hist)
        miou = d / (self.hist.sum(1) + self.hist.sum(0) - d + 1e-6) * 100.0
        tp = np.sum(self.hist[:-1, :-1])
        fp = np.sum(self.hist[-1, :-1])
        fn = np.sum(self.hist[:-1, -1])
        if tp != 0:
            precision, recall, iou = tp / (tp + fp), tp / (tp + fn), tp / (tp + fp + fn) * 100.0
        else:
            precision, recall, iou = 0, 0, 0
        iou_ssc = miou[:self.n_classes - 1]
        return dict(iou=iou, precision=precision, recall=recall, iou_ssc=iou_ssc, miou=np.mean(iou_ssc))

    def reset(self):
        self.hist = np.zeros((self.n_classes, self.n_classes))


def dense_labels(sparse_pred, num_voxels, empty_label):
    """(index, class) pairs of ``get_occupancy_prediction`` -> dense label vector."""
    out = np.full(num_voxels, empty_label, dtype=np.int64)
    sp = np.asarray(sparse_pred)
    out[sp[:, 0]] = sp[:, 1]
    return out


class DeviceSSCMetrics:
    """``SSCMetrics`` whose histogram lives on the device and is filled by ``head.occupancy_confusion`` (one
    ``ver_occ_confusion`` pass per batch, no host round trip per viewpoint), for several occupancy thresholds at once.
    ``hist``: int64 [T, n_classes, n_classes] (the LAST row / column is the empty class); ``last``: the per-sample
    histograms [bs, T, n_classes, n_classes] of the latest ``add``.  ``all_reduce`` sums the histograms over the ranks
    of a process group; ``get_stats`` returns ``SSCMetrics.get_stats`` of the summed histogram (float64)."""

    def __init__(self, n_classes=17, thresholds=(0.25,), device=None):
        import torch
        self.n_classes = n_classes
        self.thresholds = tuple(float(t) for t in thresholds)
        self.hist = torch.zeros((len(self.thresholds), n_classes, n_classes), dtype=torch.int64, device=device)
        self.last = None

    def add(self, head, occupancy_preds, labels):
        """Count one batch: ``occupancy_preds`` as ``head.occupancy_confusion`` takes them (reference-order logits or
        the row-order tuple), ``labels`` uint8 [bs, voxel_num] of ``head.occupancy_eval_labels``."""
        return self.add_hist(head.occupancy_confusion(occupancy_preds, labels, self.thresholds))

    def add_volume(self, head, voxel_embed, labels):
        """Count one batch from the encoder output itself: ``head.occupancy_confusion_from_volume`` (no logits where the
        fused MLP applies, the same histograms everywhere)."""
        return self.add_hist(head.occupancy_confusion_from_volume(voxel_embed, labels, self.thresholds))

    def add_hist(self, hist):
        """Add histograms [T, K, K] or per-sample [bs, T, K, K] (kept as ``last``)."""
        if hist.dim() == 4:
            self.last = hist
            hist = hist.sum(0)
        self.hist += hist.to(self.hist.device)
        return self

    def all_reduce(self, group=None):
        """Sum the histograms over the ranks of ``group`` (torch.distributed; a no-op without a process group)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.hist, op=dist.ReduceOp.SUM, group=group)
        return self

    def _stats(self, hist):
        m = SSCMetrics(self.n_classes)
        m.hist = hist.cpu().numpy().astype(np.float64)
        return m.get_stats()

    def get_stats(self, threshold_index=0):
        """The dict of ``SSCMetrics.get_stats`` (iou, precision, recall, iou_ssc, miou) at one threshold."""
        return self._stats(self.hist[threshold_index])

    def sample_stats(self, b, threshold_index=0):
        """``get_stats`` of sample ``b`` of the latest batch alone."""
        return self._stats(self.last[b, threshold_index])

    def reset(self):
        self.hist.zero_()
        self.last = None
