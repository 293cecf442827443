"""Box (de)normalisation and NMS-free decoding ("next" row 2): same maths as the reference's
core/bbox/util.py:4-55 and core/bbox/coders/nms_free_coder.py:9-122, layout_coder.py."""
import torch

from ..registry import BBOX_CODERS


def normalize_bbox(bboxes, pc_range=None):
    """(cx,cy,cz,w,l,h,rot[,vx,vy]) -> (cx,cy,log w,log l,cz,log h,sin,cos[,vx,vy])."""
    cx, cy, cz = bboxes[..., 0:1], bboxes[..., 1:2], bboxes[..., 2:3]
    w, l, h = bboxes[..., 3:4].log(), bboxes[..., 4:5].log(), bboxes[..., 5:6].log()
    rot = bboxes[..., 6:7]
    parts = [cx, cy, w, l, cz, h, rot.sin(), rot.cos()]
    if bboxes.size(-1) > 7:
        parts += [bboxes[..., 7:8], bboxes[..., 8:9]]
    return torch.cat(parts, dim=-1)


def denormalize_bbox(nb, pc_range=None):
    rot = torch.atan2(nb[..., 6:7], nb[..., 7:8])
    cx, cy, cz = nb[..., 0:1], nb[..., 1:2], nb[..., 4:5]
    w, l, h = nb[..., 2:3].exp(), nb[..., 3:4].exp(), nb[..., 5:6].exp()
    parts = [cx, cy, cz, w, l, h, rot]
    if nb.size(-1) > 8:
        parts += [nb[:, 8:9], nb[:, 9:10]]
    return torch.cat(parts, dim=-1)


class _TopKCoder:
    def __init__(self, pc_range, voxel_size=None, post_center_range=None, max_num=100,
                 score_threshold=None, num_classes=10):
        self.pc_range = pc_range
        self.voxel_size = voxel_size
        self.post_center_range = post_center_range
        self.max_num = max_num
        self.score_threshold = score_threshold
        self.num_classes = num_classes

    def encode(self):
        pass

    def decode_single(self, cls_scores, bbox_preds):
        """cls_scores [num_query, C] logits; bbox_preds [num_query, 10] normalised."""
        cls_scores = cls_scores.sigmoid()
        scores, indexs = cls_scores.view(-1).topk(min(self.max_num, cls_scores.numel()))
        labels = indexs % self.num_classes
        bbox_index = indexs // self.num_classes
        boxes = denormalize_bbox(bbox_preds[bbox_index], self.pc_range)
        thresh = None
        if self.score_threshold is not None:
            thresh = scores > self.score_threshold
        if self.post_center_range is None:
            raise NotImplementedError('Need to reorganize output as a batch, only '
                                      'support post_center_range is not None for now!')
        rng = torch.tensor(self.post_center_range, device=scores.device)
        mask = (boxes[..., :3] >= rng[:3]).all(1) & (boxes[..., :3] <= rng[3:]).all(1)
        if thresh is not None:
            mask &= thresh
        return dict(bboxes=boxes[mask], scores=scores[mask], labels=labels[mask])

    def decode(self, preds_dicts):
        all_cls = preds_dicts['all_cls_scores'][-1]
        all_box = preds_dicts['all_bbox_preds'][-1]
        return [self.decode_single(all_cls[i], all_box[i]) for i in range(all_cls.size(0))]

    def _decode_fused(self, cls, box, k, bottom_center):
        """``ver_det_decode`` on GPU tensors (one launch, a stated order on ties), its float64 host model
        (``detection_metrics.det_decode_host``) on CPU tensors -> (boxes, scores, labels int32, valid uint8, query int32)."""
        if self.post_center_range is None:
            raise NotImplementedError('Need to reorganize output as a batch, only '
                                      'support post_center_range is not None for now!')
        if box.is_cuda:
            from ..hipops import det_decode
            if cls is not None and cls.dtype not in (torch.float32, torch.bfloat16):
                cls = cls.float()
            return det_decode(cls, box.float(), self.post_center_range, self.score_threshold if cls is not None else None,
                              bottom_center, k)
        from ..detection_metrics import det_decode_host
        out = det_decode_host(cls, box, self.post_center_range, self.score_threshold if cls is not None else None,
                              bottom_center, k)
        dtype = box.dtype if box.dtype in (torch.float32, torch.float64) else torch.float32
        return tuple(torch.from_numpy(a).to(dtype) if a.dtype == 'float64' else torch.from_numpy(a) for a in out)


@BBOX_CODERS.register_module(force=True)
class NMSFreeCoder(_TopKCoder):

    def decode_padded(self, preds_dicts, fused=False, bottom_center=False, with_query=False):
        """The batched, fixed-shape twin of ``decode``: one ``topk`` over [bs, Nq * C] of the last decoder layer ->
        (boxes [bs, K, box_dim], scores [bs, K], labels int64 [bs, K], valid uint8 [bs, K]), K = min(max_num, Nq * C).
        ``valid``: the centre lies inside ``post_center_range`` and the score is above ``score_threshold`` -- the slots
        ``decode`` keeps, with the same values in the same order.  No boolean indexing, no host synchronisation.
        ``fused``: the whole chain in one launch of ours (``hipops.det_decode``; on CPU tensors its host model) with the
        order (logit descending, flat index ascending) where ``topk`` leaves equal scores in no stated order -- the same
        slots wherever the scores are distinct; labels are int32 then, a NaN logit is never valid, and ``bottom_center``
        asks for z = cz - h / 2 directly, ``with_query`` for the query index of every slot as a fifth result."""
        if fused:
            out = self._decode_fused(preds_dicts['all_cls_scores'][-1], preds_dicts['all_bbox_preds'][-1],
                                     min(self.max_num, preds_dicts['all_cls_scores'][-1][0].numel()), bottom_center)
            return out if with_query else out[:4]
        if bottom_center or with_query:
            raise ValueError('decode_padded: bottom_center / with_query belong to fused=True')
        cls_scores = preds_dicts['all_cls_scores'][-1].sigmoid()
        bbox_preds = preds_dicts['all_bbox_preds'][-1]
        bs, nq, nc = cls_scores.shape
        scores, indexs = cls_scores.reshape(bs, nq * nc).topk(min(self.max_num, nq * nc), dim=1)
        labels = indexs % self.num_classes
        bbox_index = indexs // self.num_classes
        picked = bbox_preds.gather(1, bbox_index[..., None].expand(-1, -1, bbox_preds.shape[-1]))
        boxes = denormalize_bbox(picked.reshape(-1, picked.shape[-1]), self.pc_range).reshape(bs, picked.shape[1], -1)
        if self.post_center_range is None:
            raise NotImplementedError('Need to reorganize output as a batch, only '
                                      'support post_center_range is not None for now!')
        rng = [float(v) for v in self.post_center_range]       # compared as scalars: no host-built tensor to copy over
        valid = torch.ones_like(scores, dtype=torch.bool)
        for axis in range(3):
            valid = valid & (boxes[..., axis] >= rng[axis]) & (boxes[..., axis] <= rng[3 + axis])
        if self.score_threshold is not None:
            valid &= scores > self.score_threshold
        return boxes, scores, labels, valid.to(torch.uint8)


@BBOX_CODERS.register_module(force=True)
class LayoutCoder(_TopKCoder):
    """core/bbox/coders/layout_coder.py: no scores -- every layout query of the last decoder layer is
    de-normalised and kept when its centre lies inside ``post_center_range``."""

    def decode_single(self, layout_preds):
        boxes = denormalize_bbox(layout_preds, self.pc_range)
        if self.post_center_range is None:
            raise NotImplementedError('Need to reorganize output as a batch, only '
                                      'support post_center_range is not None for now!')
        rng = torch.as_tensor(self.post_center_range, device=boxes.device, dtype=boxes.dtype)
        mask = (boxes[..., :3] >= rng[:3]).all(1) & (boxes[..., :3] <= rng[3:]).all(1)
        return dict(layouts=boxes[mask])

    def decode(self, preds_dicts):
        last = preds_dicts['all_layout_preds'][-1]
        return [self.decode_single(last[i]) for i in range(last.size(0))]

    def decode_padded(self, preds_dicts, fused=False, bottom_center=False):
        """``decode`` in fixed shapes: (layouts [bs, Nq, box_dim], valid uint8 [bs, Nq]) -- every layout query of the last
        decoder layer in order, ``valid`` where its centre lies inside ``post_center_range``: the rows ``decode`` keeps.
        ``fused``: one launch of ours (the layout form of ``hipops.det_decode``; its host model on CPU tensors), which can
        write the bottom-centre z (``bottom_center``) directly."""
        last = preds_dicts['all_layout_preds'][-1]
        if fused:
            boxes, _, _, valid, _ = self._decode_fused(None, last, last.shape[1], bottom_center)
            return boxes, valid
        if bottom_center:
            raise ValueError('decode_padded: bottom_center belongs to fused=True')
        boxes = denormalize_bbox(last.reshape(-1, last.shape[-1]), self.pc_range).reshape(last.shape[0], last.shape[1], -1)
        if self.post_center_range is None:
            raise NotImplementedError('Need to reorganize output as a batch, only '
                                      'support post_center_range is not None for now!')
        rng = [float(v) for v in self.post_center_range]
        valid = torch.ones(boxes.shape[:2], dtype=torch.bool, device=boxes.device)
        for axis in range(3):
            valid = valid & (boxes[..., axis] >= rng[axis]) & (boxes[..., axis] <= rng[3 + axis])
        return boxes, valid.to(torch.uint8)
