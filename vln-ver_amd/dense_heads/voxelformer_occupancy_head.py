"""VoxelFormerOccupancyHead: voxel queries -> VERFormer encoder -> coarse-to-fine occupancy
logits (+ the detection branches when a decoder is configured).

Mirrors the reference's bevformer/dense_heads/voxelformer_occupancy_head.py (constructor
kwargs :44-178 incl. the mmdet ``DETRHead`` ones it forwards, layer names :180-266, forward
branches :282-640, init :269-279) so that ``model['pts_bbox_head']`` of vocc.py builds unchanged
and a reference checkpoint loads with ``strict=True``.

What differs is how the occupancy branch is evaluated:
* the three ConvTranspose3d layers run on the even lattice (``upsample.py``: 3.5x fewer MACs,
  bit-compatible semantics incl. the bias-only odd rows/cols);
* the raw ``.view`` re-interpretations of :558 and :564 are kept exactly (they are part of the
  reference's results), per sample, so any batch size works (the reference is bs=1 only).
"""
import collections
import contextlib
import copy
import math
import os

import torch
import torch.nn as nn

from ..modules.bricks import BaseModule, const_tensor, lowp_view
from ..modules.voxel_decoder import inverse_sigmoid
from ..registry import (HEADS, build_bbox_coder, build_loss, build_positional_encoding,
                        build_transformer)
from . import coders, losses  # noqa: F401  (registers NMSFreeCoder / FocalLoss / ...)
from .assigner import SamplingResult, build_assigner
from .coders import normalize_bbox
from ..ddp import reduce_mean
from .occ_proj_lattice import lattice_plan, occ_proj_from_lattice, row_table, rows_to_voxels
from .occupancy_labels import OccupancyTargets, classify, dense_labels, labels_in_rows, labels_in_voxels, loss_labels
from .row_linear import row_linear
from .upsample import full_volume, is_reference_geometry, upsample_lattice


def _mean_over_ranks(value, like):
    """``reduce_mean(like.new_tensor([value]))`` of the reference's loss normalisers (head:954, :964) as a Python float.
    Without a process group the mean over ranks is the value itself: no tensor is built, nothing is copied to the device
    and read back (two stream synchronisations per decoder layer otherwise)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return float(value)
    return float(reduce_mean(like.new_tensor([float(value)])))


# Ground truth of a batch in static shapes (``VoxelFormerOccupancyHead.pad_gts``), all on the device: boxes [bs, cap, 9]
# (gravity centre, dims, yaw, zero velocity; rows >= counts[b] are padding), labels int64 [bs, cap], counts int32 [bs].
PaddedGts = collections.namedtuple('PaddedGts', 'boxes labels counts')

# What ``VoxelFormerOccupancyHead.infer`` returns, all on the device and in shapes that depend on nothing a viewpoint holds:
# volume [bs, Nq, C] (the encoder output); boxes [bs, K, box_dim] (bottom-centre z), scores [bs, K], labels int32 [bs, K], valid
# uint8 [bs, K] as ``get_bboxes_padded(fused=True)`` gives them; classes uint8 [bs * voxel_num] in the order of ``plan`` (the
# GEMMs' row order; None: the reference's voxel order); occ_pairs int32 [capacity, 2] (voxel index within the sample, class),
# occ_offsets int32 [bs + 1], occ_count int32 [bs + 2] as ``hipops.occ_pairs`` gives them.
InferenceOutputs = collections.namedtuple('InferenceOutputs', 'volume boxes scores labels valid classes plan occ_pairs occ_offsets occ_count')


def inference_results(head, outs, img_metas=None):
    """``InferenceOutputs`` -> what ``VoxelFormer.simple_test`` returns, ``(volume [Nq, bs, C] on the device, [dict(pts_bbox=
    dict(boxes_3d, scores_3d, labels_3d))] per sample, dict(occupancy_preds, flow_preds=None))``, with ONE device -> host copy:
    every table travels as 32-bit words of one buffer and is cut apart on the host.  ``occupancy_preds``: int64 [K_b, 2]
    (voxel index within the sample, class) per sample -- a list, or for a single viewpoint the reference's single tensor."""
    bs, k, dim = outs.boxes.shape
    as_words = lambda t: t.contiguous().view(torch.int32).reshape(-1)
    parts = [as_words(outs.boxes.float()), as_words(outs.scores.float()), outs.labels.to(torch.int32).reshape(-1),
             outs.valid.to(torch.int32).reshape(-1), outs.occ_pairs.reshape(-1), outs.occ_offsets, outs.occ_count]
    sizes = [p.numel() for p in parts]
    host = torch.cat(parts).cpu()
    boxes, scores, labels, valid, pairs, offsets, count = host.split(sizes)
    boxes, scores = boxes.view(torch.float32).view(bs, k, dim), scores.view(torch.float32).view(bs, k)
    labels, valid, pairs = labels.view(bs, k), valid.view(bs, k), pairs.view(-1, 2)
    bbox_list = []
    for b, meta in zip(range(bs), img_metas or [None] * bs):
        keep = valid[b] != 0
        box_type = (meta or {}).get('box_type_3d')
        kept = boxes[b][keep]
        bbox_list.append(dict(pts_bbox=dict(boxes_3d=box_type(kept, dim) if box_type is not None else kept,
                                            scores_3d=scores[b][keep], labels_3d=labels[b][keep].long())))
    if int(count[bs + 1]):
        raise RuntimeError('inference: %d occupied voxels do not fit the pair capacity %d (pair_capacity=); the pairs '
                           'behind it were not written' % (int(count[bs]), pairs.shape[0]))
    off = offsets.tolist()
    occ = [pairs[off[b]:off[b + 1]].long() for b in range(bs)]
    return outs.volume.permute(1, 0, 2), bbox_list, dict(occupancy_preds=occ[0] if bs == 1 else occ, flow_preds=None)


def _to_device_async(t, dev):
    """Host tensor -> ``dev`` without making the host wait for the stream (pinned staging + asynchronous copy); the
    plain ``.to(dev)`` of a pageable tensor blocks until every launch queued before it has run."""
    if torch.device(dev).type != 'cuda':
        return t.to(dev)
    return t.pin_memory().to(dev, non_blocking=True)


def _confusion(logits, labels, samples, thresholds, hist):
    """hist[s, t] += confusion matrix of sample s under threshold t (``VoxelFormerOccupancyHead.occupancy_confusion``):
    logits [samples * rows, C], labels one per row in the same order.  ``ver_occ_confusion`` on the GPU; for CPU tensors
    or a class count the kernel is not built for, the same counts as torch ops (the reference's prediction of
    ``get_occupancy_prediction`` -- fp32 sigmoid, the threshold column, ``argmax`` -- and ``bincount`` over
    ``gt * K + pred`` for ``gt < K``)."""
    c = logits.shape[-1]
    logits = logits.reshape(-1, c)
    labels = labels.reshape(-1)
    if logits.is_cuda and c % 8 == 0 and 8 <= c <= 32:
        from ..hipops import occ_confusion
        return occ_confusion(logits, labels.to(torch.uint8), thresholds, samples, hist)
    k = c + 1
    gt = labels.long().view(samples, -1)
    keep = gt < k
    first = torch.arange(samples, device=gt.device)[:, None] * k + gt           # (sample, label) row of the histogram
    for t, thr in enumerate(thresholds):
        pred = classify(logits, thr).view(samples, -1)
        counts = torch.bincount((first * k + pred)[keep], minlength=samples * k * k)
        hist[:, t] += counts.view(samples, k, k).to(hist.device)
    return hist


def bias_init_with_prob(prior_prob):
    return float(-math.log((1 - prior_prob) / prior_prob))


@HEADS.register_module(force=True)
class VoxelFormerOccupancyHead(BaseModule):

    def __init__(self, *args, with_box_refine=True, as_two_stage=False, transformer=None,
                 bbox_coder=None, num_cls_fcs=2, code_weights=None, bev_h=120, bev_w=120, bev_z=4,
                 num_layout_query=10, getbev=None, occupancy_size=[0.1, 0.1, 0.1],
                 point_cloud_range=[-6.0, -6.0, -1.5, 6.0, 6.0, 2.0], loss_layout=None,
                 loss_occupancy=None, loss_flow=None, flow_gt_dimension=2, occ_dims=16,
                 det_dims=None, num_occ_fcs=2, occupancy_classes=1, only_occ=False, only_det=False,
                 add_layout=False, with_occupancy_flow=False, with_color_render=False,
                 occ_weights=None, flow_weights=None, occ_loss_type='focal_loss',
                 occ_head_type='mlp', occ_head_network=None, refine_occ=False,
                 # ---- mmdet DETRHead kwargs
                 num_classes=None, in_channels=None, num_query=100, num_reg_fcs=2,
                 sync_cls_avg_factor=False, positional_encoding=None, loss_cls=None,
                 loss_bbox=None, loss_iou=None, train_cfg=None, test_cfg=None, init_cfg=None,
                 **kwargs):
        super().__init__(init_cfg)
        if args:
            raise TypeError('VoxelFormerOccupancyHead takes keyword arguments only')
        if occ_head_type != 'mlp' or with_color_render or with_occupancy_flow:
            raise NotImplementedError('only the mlp occupancy head of vocc.py is built')
        self.bev_h, self.bev_w, self.bev_z = bev_h, bev_w, bev_z
        self.fp16_enabled = False
        self.only_occ, self.only_det, self.add_layout = only_occ, only_det, add_layout
        self.occ_loss_type = occ_loss_type
        self.refine_occ = refine_occ
        self.num_layout_query = num_layout_query
        # room-layout branch (head:96-105): its own, fixed range and coder
        self.layout_range = [-50.0, -50.0, -5.0, 50.0, 50.0, 5.0]
        self.layout_coder = build_bbox_coder(dict(type='LayoutCoder', post_center_range=[-50, -50, -5.0, 50, 50, 5.0],
                                                  pc_range=self.layout_range, max_num=10, num_classes=1))
        self.getbev = getbev
        self._volume_writer = None
        self.with_box_refine, self.as_two_stage = with_box_refine, as_two_stage
        if as_two_stage:
            raise NotImplementedError('as_two_stage=True is not used by vocc.py (:98)')
        self.code_size = kwargs.get('code_size', 10)
        code_weights = code_weights if code_weights is not None else \
            [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0]
        self.occ_weights = occ_weights
        self.bbox_coder = build_bbox_coder(bbox_coder) if bbox_coder is not None else None
        self.pc_range = self.bbox_coder.pc_range if self.bbox_coder is not None else point_cloud_range
        self.real_w = self.pc_range[3] - self.pc_range[0]
        self.real_h = self.pc_range[4] - self.pc_range[1]
        self.real_z = self.pc_range[5] - self.pc_range[2]
        self.num_cls_fcs = num_cls_fcs - 1
        self.occupancy_size = occupancy_size
        self.point_cloud_range = point_cloud_range
        self.occ_xdim = int((point_cloud_range[3] - point_cloud_range[0]) / occupancy_size[0])
        self.occ_ydim = int((point_cloud_range[4] - point_cloud_range[1]) / occupancy_size[1])
        self.occ_zdim = int((point_cloud_range[5] - point_cloud_range[2]) / occupancy_size[2])
        self.occ_dims = occ_dims
        self.num_occ_fcs = num_occ_fcs
        self.occupancy_classes = occupancy_classes
        self.voxel_num = self.occ_xdim * self.occ_ydim * self.occ_zdim
        self.bev_num = bev_h * bev_w * bev_z
        transformer = copy.deepcopy(transformer)
        if only_occ:
            transformer['decoder'] = None
        # ---- DETRHead part
        self.bg_cls_weight = 0
        self.sync_cls_avg_factor = sync_cls_avg_factor
        self.num_query, self.num_classes, self.in_channels = num_query, num_classes, in_channels
        self.num_reg_fcs = num_reg_fcs
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.assigner = None
        if train_cfg:                                   # mmdet DETRHead: assigner + PseudoSampler
            assert 'assigner' in train_cfg, 'assigner should be provided when train_cfg is set.'
            assert loss_cls['loss_weight'] == train_cfg['assigner']['cls_cost']['weight'], \
                'The classification weight for loss and matcher should be exactly the same.'
            assert loss_bbox['loss_weight'] == train_cfg['assigner']['reg_cost']['weight'], \
                'The regression L1 weight for loss and matcher should be exactly the same.'
            self.assigner = build_assigner(train_cfg['assigner'])
        self.loss_cls = build_loss(loss_cls) if loss_cls is not None else None
        self.loss_bbox = build_loss(loss_bbox) if loss_bbox is not None else None
        self.loss_iou = build_loss(loss_iou) if loss_iou is not None else None
        use_sigmoid = self.loss_cls.use_sigmoid if self.loss_cls is not None else True
        self.cls_out_channels = num_classes if use_sigmoid else num_classes + 1
        self.positional_encoding = build_positional_encoding(positional_encoding)
        self.transformer = build_transformer(transformer)
        self.embed_dims = self.transformer.embed_dims
        assert positional_encoding['num_feats'] * 2 == self.embed_dims, \
            'embed_dims should be exactly 2 times of num_feats.'
        self._init_layers()
        self.code_weights = nn.Parameter(torch.tensor(code_weights), requires_grad=False)
        self.loss_occupancy = build_loss(loss_occupancy) if loss_occupancy is not None else None
        self.loss_flow = None
        self.predict_flow = False
        if only_occ:
            self.loss_cls = None
            self.loss_bbox = None
        if add_layout:                                  # head:176-177
            if loss_layout is None:
                raise TypeError('add_layout=True needs a loss_layout config (the reference builds it unconditionally)')
            self.loss_layout = build_loss(loss_layout)

    def _init_layers(self):
        """Same module tree / names as head:180-266."""
        c = self.embed_dims
        if self.transformer.decoder is not None:
            cls_branch = []
            for _ in range(self.num_reg_fcs):
                cls_branch += [nn.Linear(c, c), nn.LayerNorm(c), nn.ReLU(inplace=True)]
            cls_branch.append(nn.Linear(c, self.cls_out_channels))
            fc_cls = nn.Sequential(*cls_branch)

            def reg_like():
                layers = []
                for _ in range(self.num_reg_fcs):
                    layers += [nn.Linear(c, c), nn.ReLU()]
                layers.append(nn.Linear(c, self.code_size))
                return nn.Sequential(*layers)

            num_pred = self.transformer.decoder.num_layers

            def clones(m):
                if self.with_box_refine:
                    return nn.ModuleList([copy.deepcopy(m) for _ in range(num_pred)])
                return nn.ModuleList([m for _ in range(num_pred)])

            self.cls_branches = clones(fc_cls)
            self.reg_branches = clones(reg_like())
            self.layout_branches = clones(reg_like())
            self.voxel_embedding = nn.Embedding(self.bev_num, c)
            self.query_embedding = nn.Embedding(self.num_query, c * 2)
            self.query_layout_embedding = nn.Embedding(self.num_layout_query, c * 2)
        else:
            self.voxel_embedding = nn.Embedding(self.bev_num, c)
        if self.bev_z == self.occ_zdim:
            self.occ_proj = nn.Linear(c, self.occ_dims)
        else:
            self.occ_proj = nn.Linear(self.bev_z * c, self.occ_dims * self.occ_zdim)
        occ_branch = []
        for _ in range(self.num_occ_fcs):
            occ_branch += [nn.Linear(self.occ_dims, self.occ_dims), nn.LayerNorm(self.occ_dims),
                           nn.ReLU(inplace=True)]
        occ_branch.append(nn.Linear(self.occ_dims, self.occupancy_classes))
        self.occ_branches = nn.Sequential(*occ_branch)
        if self.refine_occ:
            geom = dict(stride=(1, 2, 2), padding=(2, 4, 4), dilation=(2, 2, 2), output_padding=(0, 1, 1))
            self.up_sample = nn.Sequential(*[nn.ConvTranspose3d(768, 768, (3, 5, 5), **geom)
                                             for _ in range(3)])

    def init_weights(self):
        """head:269-279."""
        self.transformer.init_weights()
        if self.loss_cls is not None and self.loss_cls.use_sigmoid:
            for m in self.cls_branches:
                nn.init.constant_(m[-1].bias, bias_init_with_prob(0.01))
        if self.loss_occupancy is not None and self.loss_occupancy.use_sigmoid:
            nn.init.constant_(self.occ_branches[-1].bias, bias_init_with_prob(0.01))

    # ------------------------------------------------------------------ occupancy branch
    def _upsample(self, x):
        convs = list(self.up_sample)
        if all(is_reference_geometry(m) for m in convs) and len(convs) == 3:
            e, b = upsample_lattice(x, [m.weight for m in convs], [m.bias for m in convs])
            return full_volume(e, b)
        return self.up_sample(x)

    def class_weight_table(self, class_weights, device):
        """The class-weight argument of the occupancy losses -> fp32 [occupancy_classes + 1] on ``device``, or None.
        ``class_weights``: None (unweighted), True (``self.occ_weights``; unweighted when that is None), a sequence of
        numbers or a tensor.  A sequence is validated on the host -- exactly occupancy_classes + 1 finite numbers -- and
        becomes a constant that is created once per (values, device): no host -> device copy per step (the reference makes
        one, head:1419), so a step with weights can be captured after one eager warm-up; reassigning ``self.occ_weights``
        gives other values and with them another table.  It is no parameter and no buffer: the state dict is the
        reference's.  A tensor is the caller's own (it may overwrite it in place between steps)."""
        if class_weights is True:
            class_weights = self.occ_weights
        if class_weights is None or class_weights is False:
            return None
        n = self.occupancy_classes + 1
        if torch.is_tensor(class_weights):
            if tuple(class_weights.shape) != (n,):
                raise ValueError('occupancy class weights must be [%d] (one per label in [0, %d]), got %s'
                                 % (n, n - 1, tuple(class_weights.shape)))
            return class_weights.detach().to(device=device, dtype=torch.float32)
        try:
            values = tuple(float(v) for v in class_weights)
        except TypeError:
            raise ValueError('occ_weights must be a sequence of %d numbers, got %r' % (n, class_weights)) from None
        if len(values) != n or not all(math.isfinite(v) for v in values):
            raise ValueError('occ_weights must be %d finite numbers (one per label in [0, %d], the last for the empty '
                             'label), got %r' % (n, n - 1, class_weights))
        return const_tensor(values, device, torch.float32)

    def occupancy_loss_from_volume(self, voxel_embed, gt_occupancy, class_weights=None):
        """``occupancy_loss(occupancy_from_volume(voxel_embed), gt_occupancy, class_weights)`` for training steps that need the loss
        and not the logits: on the lattice path the logits stay in the row order the GEMMs left them in and the
        TARGETS are brought into that order instead (an int64 per voxel instead of 16 logits, and no permutation in
        the backward pass).  The loss is a sum over (logit row, target) pairs -- the same pairs, the same value."""
        table = self.class_weight_table(class_weights, voxel_embed.device)
        res = self.occupancy_from_volume(voxel_embed, rows_only=True, loss_targets=gt_occupancy, loss_class_weight=table)
        if torch.is_tensor(res) and res.dim() == 0:
            return res                              # the fused MLP + focal-loss path evaluated the loss itself
        return self.occupancy_loss(res, gt_occupancy, table)

    fuse_occ_mlp_loss = True          # (class switch for tests / A-B runs: 0 = logits, then the loss as a separate op)

    def _fused_loss_applies(self):
        """The occupancy term is mmdet's sigmoid FocalLoss with mean reduction (vocc.py:190-195): the form the fused
        MLP + focal-loss Function evaluates."""
        from .losses import FocalLoss
        lo = self.loss_occupancy
        return self.fuse_occ_mlp_loss and isinstance(lo, FocalLoss) and lo.use_sigmoid and lo.reduction == 'mean'

    def _volume_input(self, voxel_embed):
        """The encoder output as the occupancy branch reads it: the bf16 side copy where there is one, contiguous."""
        # under bf16 autocast the encoder's last LayerNorm wrote the bf16 copy of its output next to the fp32 one
        # (bricks.residual_layer_norm): the lattice path would make exactly that copy again (and widen its gradient)
        lowp = lowp_view(voxel_embed)
        if lowp is not voxel_embed and lowp.shape == voxel_embed.shape and lowp.is_contiguous():
            voxel_embed = lowp
        return voxel_embed.contiguous()

    def _lattice_geometry(self):
        """The head's geometry takes the lattice path: three reference-geometry ConvTranspose3d layers to 8x the query grid."""
        convs = list(self.up_sample) if self.refine_occ else []
        return (self.refine_occ and self.bev_z != self.occ_zdim and len(convs) == 3
                and all(is_reference_geometry(m) for m in convs)
                and 8 * self.bev_h == self.occ_xdim and 8 * self.bev_w == self.occ_ydim)

    def occupancy_row_plan(self, device):
        """The plan whose row order ``occupancy_from_volume(..., rows_only=True)`` leaves its logits in on ``device``, or None
        where the head takes the dense path: the lattice after the three upsampling layers is [C, bev_z, 4 bev_h, 4 bev_w],
        and ``lattice_plan`` is the call ``occ_proj_from_lattice`` makes for it."""
        if not self._lattice_geometry():
            return None
        return lattice_plan(self.embed_dims, self.bev_z, 4 * self.bev_h, 4 * self.bev_w, device)

    def _occ_rows_from_lattice(self, voxel_embed):
        """The lattice path of ``occupancy_from_volume`` up to the rows ``occ_branches`` reads: voxel_embed as
        ``_volume_input`` returns it -> ``(rows [bs*X*Y, Z*occ_dims] in group-major GEMM order, plan, fold)``, or None
        when the head's geometry takes the dense path.  ``fold``: ``occ_branches[0]`` was folded, centred, into
        ``occ_proj`` -- the rows are ITS output and the MLP kernels start at the first LayerNorm."""
        if not self.refine_occ:
            return None
        bs = voxel_embed.shape[0]
        c = self.embed_dims
        x = voxel_embed.view(bs, c, self.bev_z, self.bev_h, self.bev_w)          # raw view :558
        convs = list(self.up_sample)
        if self._lattice_geometry():
            # lattice path: neither the dense volume nor its 3/4 constant columns are formed
            e, b_up = upsample_lattice(x, [m.weight for m in convs], [m.bias for m in convs])
            # ``occ_proj`` (:571) is followed by ``occ_branches[0]`` = Linear(128, 128) on every 128-slice of
            # its output (:580) with nothing in between: on the fused bf16 path the two compose into ONE Linear,
            # W' = (I_35 (x) W1) W_proj, b' = (I_35 (x) W1) b_proj + b1 (3.5 GFLOP per step, autograd maps the
            # gradient of W' back onto both parameters), and the MLP kernels start at the first LayerNorm.
            fold = self.fold_first_occ_linear and e.is_cuda and self._occ_mlp_runs_fused(e)
            w_proj, b_proj = self.occ_proj.weight, self.occ_proj.bias
            if fold:
                l1 = self.occ_branches[0]
                with torch.autocast('cuda', enabled=False):
                    # ... and the Linear that feeds a LayerNorm is CENTRED over its output axis on the way
                    # (W1 <- P W1, b1 <- P b1, P = I - 11^T/128): LN(Wx + b) = LN(PWx + Pb) exactly, the rows the
                    # MLP kernel loads then have zero mean by construction and its LayerNorm skips the mean pass
                    # (a quarter of the forward kernel's VALU work); autograd maps the gradients back through P
                    w1c, b1c = self._centered(l1.weight.float(), l1.bias.float())
                    # (a batched product over the 35 z-slices: ``matmul`` of a matrix with a 3-D tensor goes through
                    #  transposed contiguous copies of the whole [35, 128, 3072] weight, forward and backward)
                    w_proj = torch.bmm(w1c.expand(self.occ_zdim, *w1c.shape).contiguous(),
                                       w_proj.float().view(self.occ_zdim, self.occ_dims, -1)).view_as(w_proj)
                    b_proj = torch.addmm(b1c, b_proj.float().view(self.occ_zdim, self.occ_dims), w1c.t()).view(-1)
            res = occ_proj_from_lattice(e, convs[-1].bias, w_proj, b_proj)
            if res is not None:
                return res[0], res[1], fold
        return None

    def occupancy_from_volume(self, voxel_embed, rows_only=False, loss_targets=None, loss_class_weight=None):
        """voxel_embed [bs, Nq, C] (per-sample contiguous Nq*C buffer = the reference's
        ``bev_embed`` at bs=1) -> occupancy logits [bs, X*Y*Z, classes]   (head:554-580).
        ``rows_only`` (lattice path): return ``(logits [bs*X*Y, Z, classes] in GEMM row order, plan, bs)`` instead."""
        bs = voxel_embed.shape[0]
        c = self.embed_dims
        voxel_embed = self._volume_input(voxel_embed)
        lattice = self._occ_rows_from_lattice(voxel_embed)
        if lattice is not None:
            # ``occ_branches`` is row-wise: run it on the rows as the GEMMs left them
            # (group-major) and bring only the 8x narrower logits into the reference's
            # (Z, X, Y) voxel order (:572-579)
            rows, plan, fold = lattice
            if (loss_targets is not None and fold and self._fused_loss_applies()
                    and self.occupancy_classes == 16 and torch.is_grad_enabled()):
                # training loss only: the MLP kernel's logits go straight into the focal-loss pass, which leaves
                # the unscaled gradient in their place; the MLP backward reads it with the loss's scalar factor
                # (hipops.OccMLPFocalLossFunction) -- no focal backward pass over the [N, 16] tensor
                return self._occ_mlp_focal_loss(rows.view(-1, self.occ_dims), loss_targets, plan, bs, loss_class_weight)
            logits = self._occ_mlp(rows.view(rows.shape[0], self.occ_zdim, self.occ_dims), first_folded=fold)
            if rows_only:
                return logits, plan, bs
            logits = rows_to_voxels(logits, plan, bs)                       # [bs, X*Y, Z, classes]
            return logits.permute(0, 2, 1, 3).reshape(bs, -1, logits.shape[-1])
        if self.refine_occ:
            x = voxel_embed.view(bs, c, self.bev_z, self.bev_h, self.bev_w)          # raw view :558
            x = self._upsample(x).contiguous()
            x = x.view(bs, self.bev_z, self.occ_xdim, self.occ_ydim, c)              # raw view :564
            ox, oy = self.occ_xdim, self.occ_ydim
        else:
            x = voxel_embed.view(bs, self.bev_z, self.bev_h, self.bev_w, c)
            ox, oy = self.bev_h, self.bev_w
        return self._occ_from_grid(x, bs, ox, oy)

    def _occ_from_grid(self, x, bs, ox, oy):
        """``occ_proj`` + ``occ_branches`` on a [bs, bev_z, ox, oy, C] view (head:566-580, :338-350) -> logits
        [bs, ox*oy*occ_zdim, classes] in the reference's (Z, X, Y) order."""
        if self.bev_z == self.occ_zdim:
            occ = self.occ_proj(x)
        else:
            x = x.permute(0, 2, 3, 1, 4).flatten(3)
            occ = self.occ_proj(x)
            occ = occ.view(bs, ox, oy, self.occ_zdim, self.occ_dims).permute(0, 3, 1, 2, 4)
        return self._occ_mlp(occ.reshape(bs, -1, self.occ_dims))

    @staticmethod
    def _occ_mlp_is_fusable(mods):
        """[Linear(128,128), LayerNorm, ReLU] x2 + Linear(128,16) -- the vocc.py occupancy MLP."""
        if len(mods) != 7:
            return False
        kinds = (nn.Linear, nn.LayerNorm, nn.ReLU, nn.Linear, nn.LayerNorm, nn.ReLU, nn.Linear)
        if not all(isinstance(m, k) for m, k in zip(mods, kinds)):
            return False
        l1, n1, _, l2, n2, _, l3 = mods
        return (tuple(l1.weight.shape) == (128, 128) and tuple(l2.weight.shape) == (128, 128)
                and tuple(l3.weight.shape) == (16, 128) and all(m.bias is not None for m in (l1, l2, l3))
                and all(tuple(m.normalized_shape) == (128,) and m.elementwise_affine and m.bias is not None
                        for m in (n1, n2)) and n1.eps == n2.eps)

    fold_first_occ_linear = True      # (class switch for tests: compare against the unfolded fused path)

    @staticmethod
    def _centered(weight, bias):
        """(P W, P b), P = I - 11^T/n over the OUTPUT axis of an nn.Linear: the pre-activations get zero mean over the
        features without changing LayerNorm(W x + b)."""
        return weight - weight.mean(0, keepdim=True), bias - bias.mean()

    def _centered_second_linear(self):
        """``_centered`` (W2, b2) of ``occ_branches[3]`` in fp32, whatever the autocast state: what the fused MLP kernels
        take with ``centered=True`` after a folded, centred first Linear."""
        l2 = self.occ_branches[3]
        with torch.autocast('cuda', enabled=False):
            return self._centered(l2.weight.float(), l2.bias.float())

    def _occ_mlp_runs_fused(self, x):
        """True when ``_occ_mlp`` will take the fused MFMA kernels for this input (bf16 arithmetic)."""
        return x.is_cuda and self._occ_mlp_is_fusable(list(self.occ_branches)) and (
            x.dtype == torch.bfloat16 or (torch.is_autocast_enabled('cuda') and
                                          torch.get_autocast_dtype('cuda') == torch.bfloat16))

    def _occ_mlp_focal_loss(self, x, gt_occupancy, plan, bs, class_weight=None):
        """``occupancy_loss`` of the fused bf16 path with a folded (and centred) first Linear, evaluated as ONE autograd
        Function: x [N, 128] rows in GEMM order, gt_occupancy in the reference's (Z, X, Y) voxel order.  ``class_weight``:
        the table of ``class_weight_table`` -- indexed by label VALUE, so the row permutation of the labels leaves it alone."""
        from ..hipops import occ_mlp_focal_loss_sum
        _, n1, _, _, n2, _, l3 = list(self.occ_branches)
        lo = self.loss_occupancy
        if torch.is_tensor(gt_occupancy):
            # (the same first-call host check as FocalLoss.forward; it only runs on a module's first call, so the labels are
            #  clamped before they are narrowed to bytes all the same: occupancy_labels.narrow_labels)
            lo.check_label_range(gt_occupancy, self.occupancy_classes)
        gt, avg = loss_labels(gt_occupancy, self.occupancy_classes, plan, bs, self.occ_zdim, as_bytes=True)
        w2c, b2c = self._centered_second_linear()
        with torch.autocast('cuda', enabled=False):
            s = occ_mlp_focal_loss_sum(x.to(torch.bfloat16), n1.weight, n1.bias, w2c, b2c, n2.weight, n2.bias,
                                       l3.weight, l3.bias, gt, n1.eps, lo.gamma, lo.alpha, centered=True,
                                       class_weight=class_weight)
        return torch.nan_to_num(lo.loss_weight * (s / avg))

    def _occ_mlp(self, x, first_folded=False):
        """``occ_branches`` (head:241-248).  On the GPU each LayerNorm(128)+ReLU pair is one fused
        HIP pass (``ver_ln_relu_*``); Linear layers are hipBLASLt GEMMs with a split-K weight
        gradient (``row_linear``).  Under bf16 autocast the vocc.py shape of the Sequential runs as
        the fused MFMA kernels ``ver_occ_mlp_forward/backward`` instead.  ``first_folded``: x is already the
        output of ``occ_branches[0]`` (folded into ``occ_proj`` by the caller; fused path only)."""
        mods = list(self.occ_branches)
        if self._occ_mlp_runs_fused(x):
            # bf16 arithmetic (autocast): the whole Sequential is one MFMA kernel each way
            from ..hipops import occ_mlp
            l1, n1, _, l2, n2, _, l3 = mods
            with torch.autocast('cuda', enabled=False):
                if first_folded:                 # the caller centred Linear 1 in the fold; Linear 2 here
                    w2c, b2c = self._centered_second_linear()
                    return occ_mlp(x.to(torch.bfloat16), None, None, n1.weight, n1.bias, w2c, b2c,
                                   n2.weight, n2.bias, l3.weight, l3.bias, n1.eps, centered=True)
                return occ_mlp(x.to(torch.bfloat16), l1.weight, l1.bias, n1.weight, n1.bias, l2.weight, l2.bias,
                               n2.weight, n2.bias, l3.weight, l3.bias, n1.eps)
        assert not first_folded, 'only the fused occupancy MLP takes a folded first Linear'
        i = 0
        while i < len(mods):
            m = mods[i]
            if (isinstance(m, nn.LayerNorm) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                    and x.is_cuda and tuple(m.normalized_shape) == (128,) and m.elementwise_affine):
                from ..hipops import layer_norm_relu
                x = layer_norm_relu(x, m.weight, m.bias, m.eps)
                i += 2
            elif isinstance(m, nn.Linear) and x.is_cuda:
                x = row_linear(x, m.weight, m.bias)
                i += 1
            else:
                x = m(x)
                i += 1
        return x

    # ------------------------------------------------------------------ forward
    def forward(self, mlvl_feats, img_metas, prev_bev=None, only_bev=False, occupancy_rows=False, targets_for=None, **kwargs):
        """mlvl_feats [Ncam, bs, Nk, C] (the detector's (6,1,196,768)); img_metas: per-sample
        meta dicts (``sample_idx`` -> camera files, or inline ``world2pixel``/``origin``).
        Extra kwargs (``world2pixel``, ``origin`` device tensors) bypass the metas.
        Returns the reference's dict (head:615-625).  ``occupancy_rows`` (training steps that only feed ``loss``):
        ``occupancy_preds`` may come back as ``(logits in GEMM row order, plan, bs)``, which ``occupancy_loss`` takes
        as it is (targets permuted instead of logits, see ``occupancy_loss_from_volume``)."""
        num_cam, bs = mlvl_feats.shape[:2]
        dtype = mlvl_feats.dtype
        voxel_queries = self.voxel_embedding.weight.to(dtype)
        voxel_mask = torch.zeros((bs, self.bev_z, self.bev_h, self.bev_w), device=voxel_queries.device,
                                 dtype=dtype)
        voxel_pos = self.positional_encoding(voxel_mask).to(dtype)
        grid_length = (self.real_h / self.bev_h, self.real_w / self.bev_w)
        common = dict(grid_length=grid_length, bev_pos=voxel_pos, img_metas=img_metas,
                      prev_bev=prev_bev, **kwargs)
        if only_bev or self.only_occ:
            with self._encoder_params(voxel_queries, bs):
                voxel_embed = self.transformer.get_voxel_features(
                    mlvl_feats, voxel_queries, self.bev_z, self.bev_h, self.bev_w, **common)
            if only_bev:
                return voxel_embed
            self._dump_volumes(voxel_embed, img_metas)
            return dict(bev_embed=voxel_embed, all_cls_scores=None, all_bbox_preds=None,
                        all_layout_preds=None, occupancy_preds=self._only_occ(voxel_embed),
                        flow_preds=None, enc_cls_scores=None, enc_bbox_preds=None,
                        enc_occupancy_preds=None)
        object_query_embeds = self.query_embedding.weight.to(dtype)
        with self._encoder_params(voxel_queries, bs):
            voxel_embed = self.transformer.get_voxel_features(
                mlvl_feats, voxel_queries, self.bev_z, self.bev_h, self.bev_w, **common)
        # (the detection half -- decoder, cls / reg branches, Hungarian cost matrices -- only reads the encoder output, and so
        #  does the occupancy head.  Running the former on a second HIP stream was measured in round 5: its ~1 500 small
        #  launches per direction do execute beside the occupancy head's GEMMs, but those fill every CU, the small kernels
        #  stretch 2x and the 64-viewpoint step gains 0.7 % (480 -> 483 viewpoints/s); one traced run with the second
        #  stream never finished.  One stream.)
        out = self.detect_from_volume(voxel_embed, object_query_embeds, targets_for=targets_for, img_metas=img_metas, **kwargs)
        bev_embed, all_cls, all_box, layouts, pending = out
        if self.only_det:
            occupancy = None
        elif self.add_layout:
            # head:458-474: the layout branch of the reference never upsamples -- plain [bs,Z,H,W,C] view,
            # occ_proj, occ_branches on the coarse grid (X*Y = bev_h*bev_w cells, occ_zdim layers)
            occupancy = self._only_occ(voxel_embed)
        else:
            # (the encoder output itself, [bs,Nq,C]: the tensor object that carries the bf16 side copy of the last LayerNorm
            #  -- bev_embed.permute(1,0,2) is the same memory but a fresh view without it)
            occupancy = self.occupancy_from_volume(voxel_embed, rows_only=occupancy_rows)
        self._dump_volumes(voxel_embed, img_metas)
        out = dict(bev_embed=bev_embed, all_cls_scores=all_cls, all_bbox_preds=all_box,
                   all_layout_preds=torch.stack(layouts) if self.add_layout else None,
                   occupancy_preds=occupancy, flow_preds=None, enc_cls_scores=None,
                   enc_bbox_preds=None, enc_occupancy_preds=None)
        if pending is not None:
            out['pending_targets'] = pending
        return out

    # viewpoints per call up to which the encoder's 36 Linear parameters are lent as bf16 copies (one multi-tensor cast each
    # way instead of ~70 launches of a few KB): the small-batch steps are bound by launch count, not by bytes
    # (config.latency); larger batches keep the split weight gradient of bricks.tall_linear
    lowp_encoder_max_batch = 16

    def _encoder_params(self, like, bs):
        """Under bf16 autocast in a training step at a small batch: the encoder's Linear parameters as bf16 copies made by one
        multi-tensor cast (modules/lowp_params.py), like the detection half's."""
        if bs > self.lowp_encoder_max_batch or os.environ.get('VER_LOWP_PARAMS', '1') != '1':
            return contextlib.nullcontext()
        lowp = getattr(self, '_lowp_encoder', None)
        if lowp is None:
            from ..modules.lowp_params import LowpParams
            lowp = self.__dict__['_lowp_encoder'] = LowpParams([self.transformer.encoder])
        return lowp.lent() if lowp.applies(like) else contextlib.nullcontext()

    def _detection_params(self, like):
        """Under bf16 autocast in a training step: the Linear parameters of the decoder and of the cls / reg branches as
        bf16 copies made by one multi-tensor cast (modules/lowp_params.py) instead of one cast per parameter and call."""
        lowp = getattr(self, '_lowp_detection', None)
        if lowp is None:
            from ..modules.lowp_params import LowpParams
            roots = [self.transformer.decoder, self.cls_branches, self.reg_branches]
            if hasattr(self.transformer, 'reference_points'):
                roots.append(self.transformer.reference_points)
            lowp = self.__dict__['_lowp_detection'] = LowpParams([r for r in roots if r is not None])
        on = os.environ.get('VER_LOWP_PARAMS', '1') == '1'            # (0: autocast's own per-call casts, for A/B runs)
        return lowp.lent() if (on and lowp.applies(like)) else contextlib.nullcontext()

    def detect_from_volume(self, voxel_embed, object_query_embeds=None, targets_for=None, img_metas=None, **kwargs):
        """The detection half of ``forward`` on an encoder output ``voxel_embed`` [bs, Nq, C] (``forward(..., only_bev=True)``):
        decoder, cls / reg (/ layout) branches and box de-normalisation of every decoder layer, under the lent bf16 parameter
        copies where they apply -> (bev_embed [Nq, bs, C], all_cls [L, bs, Nq, classes], all_box [L, bs, Nq, code], layouts,
        pending).  ``object_query_embeds``: None = the head's query embedding in the volume's dtype.  The statements
        ``forward`` runs between its encoder pass and its occupancy branch, so the two halves can be called one by one."""
        if object_query_embeds is None:
            object_query_embeds = self.query_embedding.weight.to(voxel_embed.dtype)
        with self._detection_params(voxel_embed):
            return self._detection_half(voxel_embed, object_query_embeds, targets_for, img_metas, kwargs)

    def _detection_half(self, voxel_embed, object_query_embeds, targets_for, img_metas, kwargs):
        """Decoder + cls / reg (/ layout) branches on the encoder output [bs,Nq,C] (head:584-613), and the start of the
        Hungarian assignment when ``targets_for`` is given.  -> (bev_embed [Nq,bs,C], all_cls, all_box, layouts, pending)."""
        bev_embed, hs, init_reference, inter_references = self.transformer.decode(
            voxel_embed, object_query_embeds, self.bev_z, self.bev_h, self.bev_w,
            reg_branches=self.reg_branches if self.with_box_refine else None,
            cls_branches=None, img_metas=img_metas, **kwargs)
        # bev_embed [Nq,bs,C] is a permuted view of the contiguous [bs,Nq,C] encoder output
        hs = hs.permute(0, 2, 1, 3)
        # head:584-613 evaluates the branches layer by layer and de-normalises each layer's boxes on its own; the branch
        # outputs of all L layers are stacked here and de-normalised in one pass (the same elementwise arithmetic on
        # [L,bs,Nq,.] instead of L times on [bs,Nq,.]: a sixth of the launches, forward and backward)
        nl = hs.shape[0]
        states = hs.unbind(0)           # (one backward node for the L layers instead of a zero-filled [L,...] buffer per use)
        all_cls = torch.stack([self.cls_branches[lvl](states[lvl]) for lvl in range(nl)])
        # with box refinement the decoder has evaluated reg_branches[lvl] on these very states already (its reference-point
        # update, detached there): the same values, now with the graph the reference builds by evaluating them again
        taken = self.transformer.decoder.take_branch_outputs() if self.with_box_refine else None
        if taken is None or len(taken) != nl:
            taken = [self.reg_branches[lvl](states[lvl]) for lvl in range(nl)]
        tmp = torch.stack(taken)
        reference = init_reference[None] if nl == 1 else torch.cat([init_reference[None], inter_references[:nl - 1]])
        assert reference.shape[-1] == 3
        reference = inverse_sigmoid(reference)
        all_box = self._denormalize(tmp, reference, self.pc_range)
        layouts = []
        if self.add_layout:
            # head:501-513: the room layout is regressed from the SAME decoder states by its own branch and
            # de-normalised into the (fixed, 100 m) layout range
            lay = torch.stack([self.layout_branches[lvl](hs[lvl]) for lvl in range(nl)])
            layouts = list(self._denormalize(lay, reference, self.layout_range).unbind(0))
        # (the branches above only read the decoder states: they run BEFORE the occupancy head -- the reference runs them
        #  after it, head:584-613, same results -- so that a training step can start its Hungarian assignment early:
        #  ``targets_for=(gt_bboxes_list, gt_labels_list)`` queues the cost matrices and their device -> host copy here, the
        #  host solves them while the GPU is busy with the occupancy head below, and ``loss`` picks the result up; with the
        #  assigner's solver='device' there is nothing to start early: ``loss`` only queues launches)
        pending = None
        if targets_for is not None and not self.add_layout and not self._device_solver() \
                and not torch.cuda.is_current_stream_capturing():
            pending = self._targets_begin(all_cls, all_box, list(targets_for[0]), list(targets_for[1]))
            if pending is not None:
                pending['key'] = tuple(id(g) for g in targets_for[0])      # (the caller's box tensors: loss() checks them)
        return bev_embed, all_cls, all_box, layouts, pending

    @staticmethod
    def _denormalize(tmp, reference, rng):
        """Branch output [..., 10] + inverse-sigmoid reference [..., 3] -> box code with metric centre (head:590-606):
        (cx, cy) and cz go through a sigmoid into ``rng`` = (x0, y0, z0, x1, y1, z1), the other entries stay as they are.
        Written over whole rows (the reference slices columns 0:2 and 4:5 out and concatenates): the three columns see the
        same operations in the same order, and the backward is five elementwise passes instead of a zero-filled buffer
        per slice."""
        dev, width = tmp.device, tmp.shape[-1]
        cols = const_tensor([0, 1, 0, 0, 2, 0, 0, 0, 0, 0][:width], dev, torch.long)
        span = const_tensor([rng[3] - rng[0], rng[4] - rng[1], 0, 0, rng[5] - rng[2], 0, 0, 0, 0, 0][:width], dev, torch.float32)
        low = const_tensor([rng[0], rng[1], 0, 0, rng[2], 0, 0, 0, 0, 0][:width], dev, torch.float32)
        centre = const_tensor([1, 1, 0, 0, 1, 0, 0, 0, 0, 0][:width], dev, torch.bool)
        ref = reference.index_select(-1, cols)          # (x, y, z) of the reference under columns 0, 1, 4 (the rest is unused)
        metric = (tmp + ref).sigmoid() * span + low     # fp32 whenever the reference is (type promotion, as in the reference)
        return torch.where(centre, metric, tmp)

    def _only_occ(self, voxel_embed):
        """head:338-350: the only_occ branch never upsamples (plain [bs,Z,H,W,C] view)."""
        bs = voxel_embed.shape[0]
        x = voxel_embed.reshape(bs, self.bev_z, self.bev_h, self.bev_w, self.embed_dims)
        return self._occ_from_grid(x, bs, self.bev_h, self.bev_w)

    def occupancy_loss(self, occupancy_preds, gt_occupancy, class_weights=None):
        """Occupancy term of ``loss_single`` (head:977-989): sigmoid focal loss over
        [N, classes] logits with integer targets in [0, classes] (``classes`` = empty voxel),
        normalised by the number of occupied voxels, NaN-guarded.  ``class_weights`` (``class_weight_table``): every row
        times the factor of its label, as ``loss_only_occupancy`` does with ``occ_weights`` (head:1417-1425); the
        normaliser stays the unweighted count.
        An ``OccupancyTargets`` brings its labels in the order of the logits and ``count[-1]`` as the normaliser: no
        compare, no reduction over the labels -- and on the GPU no widening: ``FocalLoss`` reads the bytes."""
        plan = bs = None
        if isinstance(occupancy_preds, tuple):                         # (logits in GEMM row order, plan, bs)
            occupancy_preds, plan, bs = occupancy_preds               # [bs*X*Y, Z, classes], group-major rows
        preds = occupancy_preds.reshape(-1, self.occupancy_classes)
        if not (preds.is_cuda and preds.dtype == torch.bfloat16):     # the fused loss reads bf16 as is
            preds = preds.float()
        gt, avg = loss_labels(gt_occupancy, self.occupancy_classes, plan, bs, self.occ_zdim,
                              as_bytes=isinstance(gt_occupancy, OccupancyTargets) and preds.is_cuda)
        gt, avg = gt.to(preds.device), avg.to(preds.device)
        table = self.class_weight_table(class_weights, preds.device)
        if table is None:
            return torch.nan_to_num(self.loss_occupancy(preds, gt, avg_factor=avg))
        return torch.nan_to_num(self.loss_occupancy(preds, gt, avg_factor=avg, class_weight=table))

    # ------------------------------------------------------------------ detection losses
    def _get_target_single(self, cls_score, bbox_pred, gt_labels, gt_bboxes):
        """head:642-705 for one sample."""
        num_bboxes = bbox_pred.size(0)
        gt_c = gt_bboxes.shape[-1]
        if gt_bboxes.dim() == 1:
            gt_bboxes = gt_bboxes[None]
        assign_result = self.assigner.assign(bbox_pred, cls_score, gt_bboxes, gt_labels, None)
        sr = SamplingResult(assign_result, bbox_pred, gt_bboxes)
        labels = gt_bboxes.new_full((num_bboxes,), self.num_classes, dtype=torch.long)
        labels[sr.pos_inds] = gt_labels if gt_labels.dim() < 1 else gt_labels[sr.pos_assigned_gt_inds]
        label_weights = gt_bboxes.new_ones(num_bboxes)
        bbox_targets = torch.zeros_like(bbox_pred)[..., :gt_c]
        bbox_weights = torch.zeros_like(bbox_pred)
        bbox_weights[sr.pos_inds] = 1.0
        bbox_targets[sr.pos_inds] = sr.pos_gt_bboxes
        return labels, label_weights, bbox_targets, bbox_weights, sr.pos_inds, sr.neg_inds

    def loss_single(self, cls_scores, bbox_preds, occupancy_preds, gt_bboxes_list, gt_labels_list,
                    gt_occupancy=None):
        """One decoder layer's losses (head:903-990): Hungarian targets, sigmoid focal loss with
        the (all-reduced) positive count as normaliser, code-weighted L1 on normalised boxes with
        non-finite targets dropped, occupancy focal loss; NaN-guarded.
        cls_scores [bs,Nq,C], bbox_preds [bs,Nq,10]; gt_bboxes_list / gt_labels_list per sample."""
        num_imgs = cls_scores.size(0)
        out = [self._get_target_single(cls_scores[i], bbox_preds[i], gt_labels_list[i], gt_bboxes_list[i])
               for i in range(num_imgs)]
        labels = torch.cat([o[0] for o in out], 0)
        label_weights = torch.cat([o[1] for o in out], 0)
        bbox_targets = torch.cat([o[2] for o in out], 0)
        bbox_weights = torch.cat([o[3] for o in out], 0)
        num_total_pos = sum(o[4].numel() for o in out)
        num_total_neg = sum(o[5].numel() for o in out)
        cls_scores = cls_scores.reshape(-1, self.cls_out_channels)
        cls_avg_factor = num_total_pos * 1.0 + num_total_neg * self.bg_cls_weight
        if self.sync_cls_avg_factor:
            cls_avg_factor = _mean_over_ranks(cls_avg_factor, cls_scores)
        cls_avg_factor = max(cls_avg_factor, 1)
        loss_cls = self.loss_cls(cls_scores, labels, label_weights, avg_factor=cls_avg_factor)
        num_total_pos = max(_mean_over_ranks(num_total_pos, loss_cls), 1.0)
        bbox_preds = bbox_preds.reshape(-1, bbox_preds.size(-1))
        normalized = normalize_bbox(bbox_targets, self.pc_range)
        isnotnan = torch.isfinite(normalized).all(dim=-1)
        bbox_weights = bbox_weights * self.code_weights
        loss_bbox = self.loss_bbox(bbox_preds[isnotnan, :10], normalized[isnotnan, :10],
                                   bbox_weights[isnotnan, :10], avg_factor=num_total_pos)
        loss_occ = self._occupancy_term(occupancy_preds, gt_occupancy, loss_cls)
        return torch.nan_to_num(loss_cls), torch.nan_to_num(loss_bbox), loss_occ

    def _occupancy_term(self, occupancy_preds, gt_occupancy, like):
        """``occupancy_loss`` without class weights, or a zero like ``like`` for a head that predicted no occupancy."""
        return self.occupancy_loss(occupancy_preds, gt_occupancy) if occupancy_preds is not None else torch.zeros_like(like)

    def loss(self, gt_bboxes_list, gt_labels_list, gt_occupancy, preds_dicts):
        """Loss dict of the reference (head:1251-1384): last decoder layer -> ``loss_cls``,
        ``loss_bbox``, ``loss_occupancy``, ``loss_flow`` (zero); earlier layers -> ``d{i}.loss_*``.
        gt_bboxes_list: per sample [G, 7..9] boxes (gravity centre + dims + yaw [+ vel]);
        gt_occupancy: int64 [bs, voxel_num] with ``occupancy_classes`` = empty.
        With the assigner's ``solver='device'`` or ``'fused'``, ``gt_bboxes_list`` may be a ``PaddedGts`` (``pad_gts``;
        ``gt_labels_list`` is then unused): the static-shape form, with which nothing between the predictions and the loss
        dict touches the host; the two lists are padded here otherwise.  ``'fused'`` forms costs, targets, losses and their
        gradients in the set-loss kernels (``_set_loss_fused``) instead of the torch chain."""
        occ = preds_dicts['occupancy_preds']
        terms, lo = self._detection_terms(preds_dicts['all_cls_scores'], preds_dicts['all_bbox_preds'], gt_bboxes_list,
                                          gt_labels_list, pending=preds_dicts.get('pending_targets'), occ=occ,
                                          gt_occupancy=gt_occupancy,
                                          padded_error="loss: a PaddedGts needs train_cfg.assigner.solver = 'device'")
        if lo is None:
            lo = self._occupancy_term(occ, gt_occupancy, terms[-1][0])
        return self._loss_dict(terms, loss_occupancy=lo, loss_flow=torch.zeros_like(terms[-1][0]))

    def _detection_terms(self, all_cls, all_box, gts, gt_labels, pending=None, batched=True, padded_error=None, occ=None,
                         gt_occupancy=None):
        """``(loss_cls, loss_bbox)`` of every decoder layer, by the one route the assigner's solver and the form of the
        ground truth select -> (list of L pairs, occupancy term or None).  ``gts``: per-sample boxes or a ``PaddedGts``
        (``gt_labels`` is then unused; ``padded_error``: what the ``ValueError`` says when the solver cannot take one).
        * solver 'fused': the set-loss kernels (``_set_loss_fused``);
        * solver 'device' (``batched`` only): the torch chain on targets solved on the device (``_targets_device``);
        * ``pending``: targets ``forward`` started for these very box tensors (``_targets_finish``);
        * ``batched``: all layers and samples in one round trip to the host solver (``_batched_targets``);
        * else, or when there was nothing to batch: ``loss_single`` per layer, whose last call also evaluates the occupancy
          term of ``occ`` -- the only route that returns one.
        ``batched=False`` (``loss_only_detection``, ``loss_addlayout``): 'fused' or ``loss_single``, nothing in between."""
        on_device = self._device_solver() if batched else self._fused_solver()
        targets = None
        if isinstance(gts, PaddedGts) or on_device:
            if not on_device:
                raise ValueError(padded_error)
            if not isinstance(gts, PaddedGts):
                gts = self.pad_gts(gts, gt_labels)
            if self._fused_solver():
                return list(zip(*self._set_loss_fused(all_cls, all_box, gts, self.loss_bbox))), None
            targets = self._targets_device(all_cls, all_box, gts)
        elif batched and pending is not None and pending.get('key') == tuple(id(g) for g in gts):
            targets = self._targets_finish(pending)         # started in forward(), solved under the occupancy head
        elif batched:
            targets = self._batched_targets(all_cls, all_box, *self._prepare_gts(gts, gt_labels, all_box.device))
        if targets is not None:
            # every decoder layer's classification / box terms in one pass over [L * bs * Nq] rows
            return list(zip(*self._losses_from_targets(all_cls, all_box, *targets))), None
        boxes, labels = self._prepare_gts(gts, gt_labels, all_box.device)
        last = len(all_cls) - 1
        out = [self.loss_single(all_cls[lvl], all_box[lvl], occ if lvl == last else None, boxes, labels,
                                gt_occupancy if lvl == last else None) for lvl in range(last + 1)]
        return [o[:2] for o in out], out[-1][2]

    @staticmethod
    def _loss_dict(terms, **last):
        """The reference's loss dict from the (loss_cls, loss_bbox) of every decoder layer: ``d{i}.loss_*`` of the earlier
        layers, then the last layer's pair and its further terms ``last``, in that order (callers sum the values in it)."""
        losses = {}
        for lvl, (lc, lb) in enumerate(terms[:-1]):
            losses['d%d.loss_cls' % lvl] = lc
            losses['d%d.loss_bbox' % lvl] = lb
        losses.update(loss_cls=terms[-1][0], loss_bbox=terms[-1][1], **last)
        return losses

    @staticmethod
    def _prepare_gts(gt_bboxes_list, gt_labels_list, device):
        """Boxes padded with zero velocity columns (head:1316-1317), labels as int64 tensors, on ``device``."""
        boxes = [VoxelFormerOccupancyHead._boxes_as_tensor(g, device) for g in gt_bboxes_list]
        return boxes, [torch.as_tensor(x, device=device).long() for x in gt_labels_list]

    def occupancy_targets(self, occ_gts, device=None):
        """The dataset's sparse occupancy annotation -> the dense target ``loss`` takes (head:1322-1326, :1404-1408):
        ``occ_gts[b]`` is an ``[n, 2]`` array of (flat voxel index, class) pairs of the occupied voxels (or the
        reference's one-element list around it); every other voxel gets ``occupancy_classes`` = empty.
        -> int64 [bs, voxel_num]."""
        device = device if device is not None else self.code_weights.device
        return dense_labels(occ_gts, None, torch.long, self.occupancy_classes, self.voxel_num, device)

    def occupancy_targets_device(self, occ_gts, invalid=None, rows=None, device=None):
        """``occupancy_targets`` (and, with ``invalid``, ``occupancy_eval_labels``) without the dense int64 volume and the
        per-sample copies: ``occ_gts`` / ``invalid`` as those two take them -- or a ``hipops.PackedOccGts`` a loader packed
        (and perhaps copied) ahead of time -- go to the device as ONE asynchronous copy and become an ``OccupancyTargets``
        in one ``ver_occ_targets`` call.  ``rows``: None = the GEMMs' row order exactly when the head's geometry has a
        lattice plan (``occupancy_row_plan``), the reference's voxel order otherwise; False = the voxel order; True = the
        row order where there is a plan.  On a CPU ``device`` the same contract in numpy (``hipops.occ_targets_host``).
        ``bad`` is read on the host on a module's first call only (VER_FOCAL_CHECK=2: every call, 0: never; never under
        stream capture), as ``FocalLoss.check_label_range`` reads its labels; ``OccupancyTargets.check()`` reads it on demand."""
        from .. import hipops
        from .losses import _FOCAL_CHECK
        device = torch.device(device if device is not None else self.code_weights.device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if isinstance(occ_gts, hipops.PackedOccGts) and invalid is not None:
            raise ValueError('occupancy_targets_device: a PackedOccGts carries its invalid voxels (pack_occ_gts(occ_gts, invalid)); '
                             'pass one or the other')
        packed = occ_gts if isinstance(occ_gts, hipops.PackedOccGts) else hipops.pack_occ_gts(occ_gts, invalid, pinned=device.type == 'cuda')
        plan = self.occupancy_row_plan(device) if rows is not False else None
        z, classes = self.occ_zdim, self.occupancy_classes
        if device.type == 'cuda':
            p = packed if packed.buffer.is_cuda else packed.to(device)
            labels, count, bad = hipops.occ_targets(p.pairs, p.offsets, self.voxel_num, z, classes,
                                                    row_table(plan, device) if plan is not None else None,
                                                    p.invalid, p.invalid_offsets)
        else:
            p = packed if not packed.buffer.is_cuda else packed.to('cpu')
            labels, count, bad = (torch.from_numpy(a) for a in hipops.occ_targets_host(
                p.pairs.numpy(), p.offsets.numpy(), self.voxel_num, z, classes, row_table(plan) if plan is not None else None,
                None if p.invalid is None else p.invalid.numpy(), None if p.invalid is None else p.invalid_offsets.numpy()))
        targets = OccupancyTargets(labels, count, bad, 'rows' if plan is not None else 'voxels', packed.bs, plan, z)
        capturing = device.type == 'cuda' and torch.cuda.is_current_stream_capturing()
        if not capturing and (_FOCAL_CHECK >= 2 or (_FOCAL_CHECK == 1 and not self.__dict__.get('_occ_targets_checked'))):
            self.__dict__['_occ_targets_checked'] = True
            targets.check()
        return targets

    def occupancy_eval_labels(self, occ_gts, occ_invalid=None, device=None):
        """The evaluation labels of ``MP3DDataset.evaluate_occ_iou`` (mp3docc_dataset.py:500-514) as bytes: ``occ_gts`` as
        in ``occupancy_targets``; ``occ_invalid[b]`` (or None) the voxel indices of the ``occ_invalid_path`` file, whose
        voxels leave the visible mask.  -> uint8 [bs, voxel_num] in the reference's voxel order: ``occupancy_classes`` =
        empty, 255 = not evaluated (``occupancy_confusion`` ignores every label above ``occupancy_classes``)."""
        device = device if device is not None else self.code_weights.device
        return dense_labels(occ_gts, occ_invalid, torch.uint8, self.occupancy_classes, self.voxel_num, device)

    def occupancy_confusion(self, occupancy_preds, labels, thresholds=(0.25,), hist=None):
        """Confusion matrices of the occupancy prediction of ``get_occupancy_prediction`` at every threshold against
        ``labels`` (``occupancy_eval_labels``), per sample: -> int64 [bs, T, K, K], K = classes + 1, row = label,
        column = prediction (the histogram ``SSCMetrics.add_batch`` accumulates); ``hist`` of that shape: accumulated into.
        ``occupancy_preds``: the reference-order logits [bs, N, classes] of ``forward``, or the row-order tuple of
        ``occupancy_rows=True`` / ``occupancy_from_volume(..., rows_only=True)``, whose LABELS are brought into the
        logits' row order (a histogram does not depend on the order of its pairs).  GPU logits with a class count the
        kernel is built for: one ``ver_occ_confusion`` pass per row block; otherwise the same counts in torch."""
        thresholds = tuple(float(t) for t in thresholds)
        nc = self.occupancy_classes
        if isinstance(occupancy_preds, tuple):                         # (logits in GEMM row order, plan, bs)
            logits, plan, bs = occupancy_preds                         # [bs*X*Y, Z, classes], group-major rows
            gt = labels_in_rows(labels, plan, bs, self.occ_zdim)
            if hist is None:
                hist = torch.zeros((bs, len(thresholds), nc + 1, nc + 1), dtype=torch.int64, device=logits.device)
            # the rows of sample b in group g are contiguous (row bs*offset_g + b*n_g + i): one call per group
            for g in plan.groups:
                sl = slice(bs * g.offset, bs * (g.offset + g.n_rows))
                _confusion(logits[sl], gt[sl], bs, thresholds, hist)
            return hist
        bs = occupancy_preds.shape[0] if occupancy_preds.dim() == 3 else 1
        labels = labels_in_voxels(labels).to(occupancy_preds.device)
        if hist is None:
            hist = torch.zeros((bs, len(thresholds), nc + 1, nc + 1), dtype=torch.int64, device=occupancy_preds.device)
        return _confusion(occupancy_preds, labels, bs, thresholds, hist)

    # ------------------------------------------------------------------ evaluation without logits
    def _fused_eval_rows(self, voxel_embed):
        """``(x bf16 [rows, 128], plan, bs)`` when the classifying MLP launches apply to this volume -- the lattice path
        with the folded, centred first Linear (bf16 autocast on the GPU), 16 classes, no autograd -- else None."""
        if torch.is_grad_enabled() or self.occupancy_classes != 16:
            return None
        lattice = self._occ_rows_from_lattice(self._volume_input(voxel_embed))
        if lattice is None or not lattice[2]:
            return None
        rows, plan, _ = lattice
        return rows.view(-1, self.occ_dims).to(torch.bfloat16), plan, voxel_embed.shape[0]

    def _fused_eval_params(self):
        """(image, vectors, eps) of the classifying MLP launches for the folded, centred chain: what ``OccMLPFunction``
        packs for ``_occ_mlp(first_folded=True)`` (W2 in W1's image section, b1 = 0)."""
        from ..hipops import occ_mlp_pack, occ_mlp_vectors
        _, n1, _, _, n2, _, l3 = list(self.occ_branches)
        w2c, b2c = self._centered_second_linear()
        with torch.autocast('cuda', enabled=False):
            image = occ_mlp_pack(w2c, w2c, l3.weight)
            vec = occ_mlp_vectors(torch.zeros(128, device=w2c.device), n1.weight, n1.bias, b2c, n2.weight, n2.bias,
                                  l3.bias)
        return image, vec, n1.eps

    def occupancy_confusion_from_volume(self, voxel_embed, labels, thresholds=(0.25,), hist=None):
        """``occupancy_confusion(occupancy_from_volume(voxel_embed, rows_only=True), labels, thresholds, hist)`` -- the
        same int64 [bs, T, K, K] histograms -- without the logits where the fused MLP applies (bf16 autocast on the GPU,
        the lattice path, no autograd): the forward kernel classifies every row in its epilogue and counts the
        (label, prediction) pairs itself, one ``ver_occ_mlp_confusion`` launch per row group.  Everywhere else (CPU
        tensors, fp32, an ``occ_branches`` the kernel is not built for, gradients enabled) the two existing functions are
        composed."""
        thresholds = tuple(float(t) for t in thresholds)
        nc = self.occupancy_classes

        fused = self._fused_eval_rows(voxel_embed) if 1 <= len(thresholds) <= 8 else None
        if fused is None:
            preds = self.occupancy_from_volume(voxel_embed, rows_only=True)
            return self.occupancy_confusion(preds, labels, thresholds, hist)
        from ..hipops import occ_mlp_confusion
        x, plan, bs = fused
        image, vec, eps = self._fused_eval_params()
        gt = labels_in_rows(labels, plan, bs, self.occ_zdim, dtype=torch.uint8)
        if hist is None:
            hist = torch.zeros((bs, len(thresholds), nc + 1, nc + 1), dtype=torch.int64, device=x.device)
        z = self.occ_zdim
        # the rows of sample b in group g are contiguous (GEMM row bs*offset_g + b*n_g + i, Z voxels each): one launch per group
        for g in plan.groups:
            lo, hi = bs * g.offset, bs * (g.offset + g.n_rows)
            occ_mlp_confusion(x[lo * z:hi * z], image, vec, gt[lo:hi], thresholds, bs, hist, eps,
                              first_linear=False, centered=True)
        return hist

    def _classes_from_logits(self, logits, threshold):
        """uint8 class per row of logits [..., classes] under ``get_occupancy_prediction``'s rule; ``classes`` = empty."""
        nc = self.occupancy_classes
        lead = logits.shape[:-1]
        flat = logits.reshape(-1, nc)
        if flat.is_cuda and nc % 8 == 0:
            from ..hipops import occ_predict
            pairs = occ_predict(flat, threshold)
            cls = torch.full((flat.shape[0],), nc, dtype=torch.uint8, device=flat.device)
            cls[pairs[:, 0]] = pairs[:, 1].to(torch.uint8)
            return cls.view(lead)
        return classify(flat, threshold).to(torch.uint8).view(lead)

    def occupancy_classes_from_volume(self, voxel_embed, threshold=0.25):
        """The dense class map of ``get_occupancy_prediction``: uint8 [bs, X*Y*Z] in the reference's (Z, X, Y) voxel
        order, ``occupancy_classes`` = empty.  Where the fused MLP applies (see ``occupancy_confusion_from_volume``) one
        ``ver_occ_mlp_classes`` launch writes a byte per voxel and no logits; otherwise the classes of
        ``occupancy_from_volume``'s logits."""
        fused = self._fused_eval_rows(voxel_embed)
        if fused is None:
            return self._classes_from_logits(self.occupancy_from_volume(voxel_embed).detach(), threshold)
        from ..hipops import occ_mlp_classes
        x, plan, bs = fused
        image, vec, eps = self._fused_eval_params()
        cls = occ_mlp_classes(x, image, vec, threshold, eps=eps, first_linear=False, centered=True)
        cls = rows_to_voxels(cls.view(-1, self.occ_zdim), plan, bs)                   # [bs, X*Y, Z]
        return cls.permute(0, 2, 1).reshape(bs, -1)

    def occupancy_pairs_from_classes(self, classes):
        """Class map (``occupancy_classes_from_volume``) -> the sparse pairs of ``get_occupancy_prediction``: int64 [K, 2]
        (voxel index over the flattened batch, class), ascending voxel index."""
        flat = classes.reshape(-1)
        occ_index, = torch.where(flat < self.occupancy_classes)
        return torch.stack([occ_index, flat[occ_index].long()], dim=-1)

    # ------------------------------------------------------------------ inference in fixed shapes
    def _check_infer(self):
        who = 'VoxelFormerOccupancyHead.infer'
        if self.training:
            raise RuntimeError('%s: the head is in training mode; inference runs in eval mode (head.eval())' % who)
        if self.add_layout:
            raise NotImplementedError('%s: add_layout=True: the room-layout terms are not part of the captured step' % who)
        if self.only_occ or self.only_det:
            raise NotImplementedError('%s covers the default multi-task branch of the head (only_occ / only_det are set)' % who)
        if getattr(self, 'getbev', None) is not None:
            raise NotImplementedError('%s: a head built with getbev=<store> writes volumes to the host inside forward (device '
                                      '-> host copies and file I/O), which cannot be captured' % who)

    def _infer_classes(self, voxel_embed, occ_threshold):
        """(class bytes uint8 [bs * voxel_num], plan): in the GEMMs' row order of ``plan`` where the head takes the lattice
        path -- from the classifying MLP launch without logits where ``_fused_eval_rows`` applies, from the row-order logits
        under ``get_occupancy_prediction``'s rule otherwise -- and in the reference's voxel order (plan None) on the dense path."""
        fused = self._fused_eval_rows(voxel_embed)
        if fused is not None:
            from ..hipops import occ_mlp_classes
            x, plan, _ = fused
            image, vec, eps = self._fused_eval_params()
            return occ_mlp_classes(x, image, vec, occ_threshold, eps=eps, first_linear=False, centered=True).reshape(-1), plan
        preds = self.occupancy_from_volume(voxel_embed, rows_only=True)
        logits, plan = (preds[0], preds[1]) if isinstance(preds, tuple) else (preds, None)
        flat = logits.reshape(-1, self.occupancy_classes)
        if flat.is_cuda and self.occupancy_classes % 8 == 0:
            from ..hipops import occ_predict_classes
            return occ_predict_classes(flat, occ_threshold), plan
        return classify(flat, occ_threshold).to(torch.uint8), plan

    @torch.no_grad()
    def infer(self, feats, world2pixel, origin, occ_threshold=0.25, pair_capacity=None, autocast_dtype=torch.bfloat16, out=None):
        """One inference step in fixed shapes and without a host read: feats [Ncam, bs, Nk, C], world2pixel [bs, Ncam, 4, 4],
        origin [bs, 3] -> ``InferenceOutputs``.  ONE encoder pass; the detection half on its output (``detect_from_volume``)
        and the fused decode of the last decoder layer (``get_bboxes_padded(fused=True)``); occupancy as class bytes in the
        GEMMs' row order -- one ``ver_occ_mlp_classes`` launch and no logits under bf16 autocast, the row-order logits
        classified by ``get_occupancy_prediction``'s kernels in fp32 (``autocast_dtype=None``) -- and ``ver_occ_pairs`` with
        the plan's row table: per-sample (voxel index, class) pairs with offsets, at most ``pair_capacity`` of them (None:
        ``bs * voxel_num``, which cannot overflow; ``occ_count[bs + 1]`` reports an overflow).  No logits in voxel order, no
        permuting copy, no pair count on the host: every call launches the same work, so it can be captured
        (``graphs.GraphedInference``).  ``out``: the ``InferenceOutputs`` of an earlier call with the same shapes to write
        into.  Eval mode, the default multi-task branch, no ``getbev``."""
        from .. import hipops
        self._check_infer()
        bs = feats.shape[1]
        on = autocast_dtype is not None and feats.is_cuda
        with torch.autocast('cuda', dtype=autocast_dtype or torch.bfloat16, enabled=on, cache_enabled=False):
            voxel_embed = self.forward(feats, None, only_bev=True, world2pixel=world2pixel, origin=origin)
            _, all_cls, all_box, _, _ = self.detect_from_volume(voxel_embed, self.query_embedding.weight.to(feats.dtype),
                                                                world2pixel=world2pixel, origin=origin)
            decoded = self.get_bboxes_padded(dict(all_cls_scores=all_cls, all_bbox_preds=all_box), fused=True)
            classes, plan = self._infer_classes(voxel_embed, occ_threshold)
        z, nc = self.occ_zdim, self.occupancy_classes
        if out is not None:
            for dst, src in zip(out[:6], (voxel_embed,) + tuple(decoded) + (classes,)):
                dst.copy_(src)
            voxel_embed, decoded, classes = out.volume, tuple(out[1:5]), out.classes
        if classes.is_cuda:
            table = row_table(plan, classes.device) if plan is not None else None
            pairs = hipops.occ_pairs(classes, bs, self.voxel_num, z, nc, table, pair_capacity,
                                     out=None if out is None else (out.occ_pairs, out.occ_offsets, out.occ_count))
        else:
            pairs = tuple(torch.from_numpy(a) for a in hipops.occ_pairs_host(
                classes.numpy(), bs, self.voxel_num, z, nc, row_table(plan) if plan is not None else None, pair_capacity))
            if out is not None:
                for dst, src in zip(out[7:], pairs):
                    dst.copy_(src)
                pairs = tuple(out[7:])
        return InferenceOutputs(voxel_embed, *decoded, classes, plan, *pairs)

    def get_occupancy_prediction_from_volume(self, voxel_embed, occ_threshold=0.25):
        """``get_occupancy_prediction`` of ``occupancy_from_volume(voxel_embed)`` -- the same pairs -- through the class map."""
        classes = self.occupancy_classes_from_volume(voxel_embed, occ_threshold)
        return dict(occupancy_preds=self.occupancy_pairs_from_classes(classes), flow_preds=None)

    def loss_only_occupancy(self, gt_bboxes_list, gt_labels_list, gt_occupancy, preds_dicts):
        """``only_occ`` detectors (head:1387-1447): the occupancy focal loss alone, weighted per class by ``occ_weights``
        when the config sets them (head:1417-1425; ``loss`` / ``loss_addlayout`` do not read them, there as here), plus
        the zero ``loss_flow``."""
        lo = self.occupancy_loss(preds_dicts['occupancy_preds'], gt_occupancy, class_weights=True)
        return dict(loss_occupancy=lo, loss_flow=torch.zeros_like(lo))

    def loss_only_detection(self, gt_bboxes_list, gt_labels_list, preds_dicts):
        """``only_det`` detectors (head:1619-1700): classification and box terms of every decoder layer, no
        occupancy term."""
        all_cls, all_box = preds_dicts['all_cls_scores'], preds_dicts['all_bbox_preds']
        if not isinstance(gt_bboxes_list, PaddedGts):
            if not isinstance(gt_bboxes_list, (list, tuple)):
                gt_bboxes_list, gt_labels_list = [gt_bboxes_list], [gt_labels_list]
            gt_bboxes_list, gt_labels_list = self._prepare_gts(gt_bboxes_list, gt_labels_list, all_box.device)
        terms, _ = self._detection_terms(all_cls, all_box, gt_bboxes_list, gt_labels_list, batched=False,
                                         padded_error="loss_only_detection: a PaddedGts needs train_cfg.assigner.solver = 'fused'")
        return self._loss_dict(terms)

    # ------------------------------------------------------------------ room-layout branch (add_layout=True)
    def _layout_targets_single(self, layout_pred, gt_layout):
        """Layout half of ``_get_target_layout_single`` (head:760-841): Hungarian matching on the L1 cost of the
        normalised box alone (``assign(..., layout=True)``; all layout boxes carry label 0), matched queries get
        weight 1 and their ground-truth box as target.  -> (targets [Nq,9], weights [Nq,10], #pos, #neg)."""
        if gt_layout.dim() == 1:
            gt_layout = gt_layout[None]
        zeros = torch.zeros(gt_layout.shape[0], dtype=torch.long, device=layout_pred.device)
        res = self.assigner.assign(layout_pred, None, gt_layout, zeros, None, layout=True)
        sr = SamplingResult(res, layout_pred, gt_layout)
        targets = torch.zeros_like(layout_pred)[..., :gt_layout.shape[-1]]
        weights = torch.zeros_like(layout_pred)
        weights[sr.pos_inds] = 1.0
        targets[sr.pos_inds] = sr.pos_gt_bboxes.to(targets.dtype)
        return targets, weights, sr.pos_inds.numel(), sr.neg_inds.numel()

    def loss_single_layout(self, cls_scores, bbox_preds, layout_preds, occupancy_preds, gt_bboxes_list,
                           gt_labels_list, gt_layout_list, gt_occupancy=None):
        """One decoder layer's losses with the layout term (head:992-1104): ``loss_single`` plus a code-weighted L1
        on the layout boxes normalised like detection boxes, averaged over the (all-reduced) number of matched
        layout queries.  -> (loss_cls, loss_bbox, loss_layout, loss_occupancy)."""
        loss_cls, loss_bbox, loss_occ = self.loss_single(cls_scores, bbox_preds, occupancy_preds, gt_bboxes_list,
                                                         gt_labels_list, gt_occupancy)
        return loss_cls, loss_bbox, self._layout_term(layout_preds, gt_layout_list, loss_cls), loss_occ

    def _layout_term(self, layout_preds, gt_layout_list, loss_cls):
        """The layout term of ``loss_single_layout`` (head:1060-1104) for one decoder layer's layout boxes [bs, Nq, 10]."""
        out = [self._layout_targets_single(layout_preds[i], gt_layout_list[i]) for i in range(layout_preds.size(0))]
        layout_targets = torch.cat([o[0] for o in out], 0)
        layout_weights = torch.cat([o[1] for o in out], 0)
        num_layout_pos = sum(o[2] for o in out)
        num_layout_pos = max(_mean_over_ranks(num_layout_pos, loss_cls), 1.0)
        layout_preds = layout_preds.reshape(-1, layout_preds.size(-1))
        normalized = normalize_bbox(layout_targets, self.layout_range)
        ok = torch.isfinite(normalized).all(dim=-1)
        layout_weights = layout_weights * self.code_weights
        loss_layout = self.loss_layout(layout_preds[ok, :10], normalized[ok, :10], layout_weights[ok, :10],
                                       avg_factor=num_layout_pos)
        return torch.nan_to_num(loss_layout)

    @staticmethod
    def _boxes_as_tensor(b, device):
        """mmdet3d box object (``gravity_center`` + ``tensor``, head:1181-1186) or plain [G, 7..9] tensor -> [G, 9]
        (gravity centre, dims, yaw, zero-padded velocity)."""
        if hasattr(b, 'gravity_center'):
            b = torch.cat((b.gravity_center, b.tensor[:, 3:]), dim=1)
        b = torch.as_tensor(b).to(device)
        if b.dim() == 1:
            b = b[None]
        if b.shape[-1] < 9:
            b = torch.cat([b, b.new_zeros(b.shape[0], 9 - b.shape[-1])], dim=1)
        return b

    def loss_addlayout(self, gt_bboxes_list, gt_labels_list, gt_layout_list, gt_occupancy, preds_dicts):
        """Loss dict of the layout-enabled head (head:1106-1248): every decoder layer contributes its detection
        terms (``d{i}.loss_cls`` / ``d{i}.loss_bbox``), the last layer additionally ``loss_layout``,
        ``loss_occupancy`` and the zero ``loss_flow``.  Lists are per sample (the reference is bs=1 and takes the
        single sample's box objects directly: those are accepted too)."""
        all_cls, all_box = preds_dicts['all_cls_scores'], preds_dicts['all_bbox_preds']
        all_layout, occ = preds_dicts['all_layout_preds'], preds_dicts['occupancy_preds']
        dev = all_box.device
        if not isinstance(gt_bboxes_list, (list, tuple)):
            gt_bboxes_list, gt_labels_list, gt_layout_list = [gt_bboxes_list], [gt_labels_list], [gt_layout_list]
        boxes, labels = self._prepare_gts(gt_bboxes_list, gt_labels_list, dev)
        layouts = [self._boxes_as_tensor(b, dev) for b in gt_layout_list]
        last = len(all_cls) - 1
        terms, lo = self._detection_terms(all_cls, all_box, boxes, labels, batched=False, occ=occ, gt_occupancy=gt_occupancy)
        if self._fused_solver() and all_box.is_cuda:
            # 'fused': the last layer's layout term through the same kernels without class logits (cost, solve and loss
            # of L = 1), its normaliser all-reduced on the device
            room = self.pad_gts(layouts, [g.new_zeros(g.shape[0], dtype=torch.long) for g in layouts])
            ll = self._set_loss_fused(None, all_layout[last:], room, self.loss_layout)[1][0]
        else:
            ll = self._layout_term(all_layout[last], layouts, terms[last][0])
        if lo is None:
            lo = self._occupancy_term(occ, gt_occupancy, terms[last][0])
        return self._loss_dict(terms, loss_occupancy=lo, loss_flow=torch.zeros_like(terms[last][0]), loss_layout=ll)

    def _to_box_type(self, boxes, img_meta):
        """head:1466-1471: bottom centre + the dataset's box class when the meta carries one."""
        boxes = boxes.clone()
        boxes[:, 2] = boxes[:, 2] - boxes[:, 5] * 0.5
        box_type = (img_meta or {}).get('box_type_3d')
        return box_type(boxes, boxes.shape[-1]) if box_type is not None else boxes

    def get_bboxes(self, preds_dicts, img_metas=None, rescale=False):
        """head:1450-1476: NMS-free top-k decoding of the last decoder layer."""
        preds = self.bbox_coder.decode(preds_dicts)
        metas = img_metas or [None] * len(preds)
        return [[self._to_box_type(p['bboxes'], m), p['scores'], p['labels']] for p, m in zip(preds, metas)]

    def get_bboxes_padded(self, preds_dicts, fused=False):
        """``get_bboxes`` in fixed shapes (``bbox_coder.decode_padded``): (boxes [bs, K, box_dim] with bottom-centre z as
        ``_to_box_type`` makes it, scores [bs, K], labels [bs, K], valid uint8 [bs, K]); the slots with ``valid`` set are
        ``get_bboxes``' boxes in the same order.  Launches only -- what ``DeviceDetMetrics.add`` feeds to the matcher.
        ``fused``: one launch (``hipops.det_decode``) that writes the bottom-centre boxes directly; labels are int32 and equal
        scores are ordered by (query, class) -- the same slots wherever the scores are distinct."""
        if fused:
            return self.bbox_coder.decode_padded(preds_dicts, fused=True, bottom_center=True)
        boxes, scores, labels, valid = self.bbox_coder.decode_padded(preds_dicts)
        boxes = boxes.clone()
        boxes[..., 2] = boxes[..., 2] - boxes[..., 5] * 0.5
        return boxes, scores, labels, valid

    def get_layouts(self, preds_dicts, img_metas=None):
        """head:1478-1502: layout boxes of the last decoder layer inside the layout range."""
        preds = self.layout_coder.decode(preds_dicts)
        metas = img_metas or [None] * len(preds)
        return [[self._to_box_type(p['layouts'], m)] for p, m in zip(preds, metas)]

    def get_layouts_padded(self, preds_dicts, fused=False):
        """``get_layouts`` in fixed shapes (``layout_coder.decode_padded``): (layouts [bs, Nq, box_dim] with bottom-centre z,
        valid uint8 [bs, Nq]); the rows with ``valid`` set are ``get_layouts``' boxes in the same order.  ``fused``: one
        launch of ours instead of the torch chain."""
        if fused:
            return self.layout_coder.decode_padded(preds_dicts, fused=True, bottom_center=True)
        boxes, valid = self.layout_coder.decode_padded(preds_dicts)
        boxes = boxes.clone()
        boxes[..., 2] = boxes[..., 2] - boxes[..., 5] * 0.5
        return boxes, valid

    # ---- Hungarian targets of all decoder layers and samples with ONE device->host round trip
    def _batched_targets(self, all_cls, all_box, gt_boxes, gt_labels):
        """``_get_target_single`` (head:642-705) for every (layer, sample) at once: the cost matrices
        [L,bs,Nq,Gmax] are formed on the device (same formulas as ``HungarianAssigner3D.assign``),
        copied to the host in one piece, solved there (scipy, as in the reference) and the matched
        indices come back in one piece.  Returns (labels [L,bs,Nq], bbox_targets [L,bs,Nq,9],
        positive mask [L,bs,Nq], positives per layer) or None when there is nothing to batch."""
        return self._targets_finish(self._targets_begin(all_cls, all_box, gt_boxes, gt_labels))

    def _targets_begin(self, all_cls, all_box, gt_boxes, gt_labels):
        """First half of ``_batched_targets``: cost matrices on the device and their ASYNCHRONOUS copy into pinned host
        memory (an event marks its end).  Nothing here waits for the device."""
        from .assigner import linear_sum_assignment
        if linear_sum_assignment is None or not self._restated_costs():
            return None
        counts = [int(g.shape[0]) for g in gt_boxes]
        gmax = max(counts) if counts else 0
        if gmax == 0:
            return None
        gt_pad, lab_pad = self._pad_tables(gt_boxes, gt_labels, counts, gmax, all_box.dtype, all_box.device)
        with torch.no_grad():
            cost = self._assignment_costs(all_cls, all_box, gt_pad, lab_pad)
            event = None
            if cost.is_cuda:
                host = torch.empty(cost.shape, dtype=cost.dtype, pin_memory=True)
                host.copy_(cost, non_blocking=True)
                event = torch.cuda.Event()
                event.record()
            else:
                host = cost
        return dict(host=host, event=event, counts=counts, gt_pad=gt_pad, lab_pad=lab_pad)

    def _restated_costs(self):
        """The assigner's costs are ``FocalLossCost`` + ``BBox3DL1Cost``: the pair ``_assignment_costs`` and the kernels restate."""
        from .assigner import BBox3DL1Cost, FocalLossCost
        a = self.assigner
        return a is not None and isinstance(a.cls_cost, FocalLossCost) and isinstance(a.reg_cost, BBox3DL1Cost)

    def _pad_tables(self, gt_boxes, gt_labels, counts, gmax, dtype, dev):
        """The per-sample gt lists as padded tables on ``dev``: boxes ``dtype`` [bs, gmax, 9] (velocity columns zero,
        head:1316-1317) and labels int64 [bs, gmax]; rows past a sample's count stay zero."""
        bs = len(counts)
        gt_pad = torch.zeros(bs, gmax, 9, dtype=dtype, device=dev)
        lab_pad = torch.zeros(bs, gmax, dtype=torch.long, device=dev)
        widths = {int(g.shape[-1]) for g in gt_boxes}
        if len(widths) == 1 and all(torch.is_tensor(g) and g.device == dev for g in gt_boxes) \
                and all(torch.is_tensor(x) and x.device == dev for x in gt_labels):
            # the usual case (every sample's boxes on the device, one width): the padded [bs, Gmax] tables are one
            # concatenation and one indexed copy each, whatever the batch size (velocity columns stay zero, head:1316-1317)
            width = min(widths.pop(), 9)
            slots = self._gt_slots(tuple(counts), gmax, dev)
            gt_pad.view(bs * gmax, 9)[:, :width].index_copy_(0, slots, torch.cat(list(gt_boxes))[:, :width].to(dtype))
            lab_pad.view(-1).index_copy_(0, slots, torch.cat([x.reshape(-1) for x in gt_labels]).long())
        else:
            gt_boxes, gt_labels = self._prepare_gts(gt_boxes, gt_labels, dev)
            for i, (g, lab) in enumerate(zip(gt_boxes, gt_labels)):
                if counts[i]:
                    gt_pad[i, :counts[i]] = g.to(dtype)
                    lab_pad[i, :counts[i]] = lab.reshape(-1)
        return gt_pad, lab_pad

    def _assignment_costs(self, all_cls, all_box, gt_pad, lab_pad):
        """Cost matrices fp32 [L, bs, Nq, Gmax] of every (layer, sample) against the padded gt tables: the formulas of
        ``HungarianAssigner3D.assign`` (``FocalLossCost`` + ``BBox3DL1Cost`` on the normalised box).  Call under no_grad."""
        a = self.assigner
        nl, bs, nq, _ = all_cls.shape
        gmax = gt_pad.shape[1]
        c = a.cls_cost
        p = all_cls.float().sigmoid()
        neg = -(1 - p + c.eps).log() * (1 - c.alpha) * p.pow(c.gamma)
        pos = -(p + c.eps).log() * c.alpha * (1 - p).pow(c.gamma)
        cls_cost = ((pos - neg) * c.weight).gather(3, lab_pad[None, :, None, :].expand(nl, bs, nq, gmax))
        gt_norm = normalize_bbox(gt_pad.view(-1, 9), a.pc_range).view(bs, gmax, -1)[..., :8]
        # padded gts hold log(0): keep them finite, their columns are never handed to the solver
        gt_norm = torch.nan_to_num(gt_norm, nan=0.0, posinf=0.0, neginf=0.0)
        reg_cost = (all_box.float()[..., None, :8] - gt_norm[None, :, None]).abs().sum(-1) * a.reg_cost.weight
        return cls_cost + reg_cost

    def _targets_from_match(self, idx_t, gt_pad, lab_pad):
        """Matched gt index per query, int64 [L, bs, Nq] (-1: background) -> (labels, bbox_targets, positive mask)."""
        nl, bs, nq = idx_t.shape
        gmax = gt_pad.shape[1]
        pos_mask = idx_t >= 0
        safe = idx_t.clamp(min=0)
        labels = torch.where(pos_mask, lab_pad[None].expand(nl, bs, gmax).gather(2, safe),
                             torch.full_like(safe, self.num_classes))
        bbox_targets = gt_pad[None].expand(nl, bs, gmax, 9).gather(2, safe[..., None].expand(nl, bs, nq, 9))
        return labels, bbox_targets, pos_mask

    def _targets_finish(self, ctx):
        """Second half: wait for the copy (only), solve the assignments on the host, build the targets on the device."""
        if ctx is None:
            return None
        if ctx['event'] is not None:
            ctx['event'].synchronize()
        gt_pad, lab_pad = ctx['gt_pad'], ctx['lab_pad']
        idx = self._solve_on_host(ctx['host'].numpy(), ctx['counts'])
        num_pos = (idx >= 0).reshape(idx.shape[0], -1).sum(1).tolist()
        idx_t = _to_device_async(torch.from_numpy(idx), gt_pad.device)
        return self._targets_from_match(idx_t, gt_pad, lab_pad) + (num_pos,)

    # ---- the same targets without the round trip (train_cfg.assigner.solver = 'device')
    def _device_solver(self):
        return getattr(self.assigner, 'solver', 'host') in ('device', 'fused')

    def _fused_solver(self):
        return getattr(self.assigner, 'solver', 'host') == 'fused'

    def _set_loss_fused(self, all_cls, all_box, gts, loss_box_module):
        """The classification and box terms of all L decoder layers from a ``PaddedGts`` in four launches of ours
        (train_cfg.assigner.solver = 'fused'): ``det_costs`` -> ``lsa_solve`` -> ``_device_normalisers`` -> ``det_set_loss``,
        whose backward is the fourth.  Costs, targets, per-element terms and their gradients are what ``_assignment_costs``,
        ``_targets_from_match`` and ``_losses_from_targets`` state; nothing is copied to the host, so the call can be captured.
        ``all_cls`` None: the room-layout form (regression cost and L1 term alone, ``loss_box_module`` = ``loss_layout``).
        -> (loss_cls per layer, loss_bbox per layer).  CPU tensors: the torch formulas of ``solver='device'``."""
        a = self.assigner
        if (not self._restated_costs() or not isinstance(self.loss_cls, losses.FocalLoss)
                or not isinstance(loss_box_module, losses.L1Loss)):
            raise NotImplementedError("solver='fused' is built for FocalLossCost + BBox3DL1Cost assigners with FocalLoss + L1Loss")
        if not all_box.is_cuda:
            return self._losses_from_targets(all_cls, all_box, *self._targets_device(all_cls, all_box, gts))
        from ..hipops import AssignmentFlag, det_costs, det_set_loss, lsa_solve
        nl, bs, nq = all_box.shape[:3]
        tables = (gts.boxes.float(), gts.labels, gts.counts)
        c = a.cls_cost
        flag = AssignmentFlag.of(all_box.device)
        flag.poll()                                          # a problem of an EARLIER step is reported here
        with torch.no_grad():
            cost = det_costs(all_cls, all_box, tables, c.weight, c.alpha, c.gamma, c.eps, a.reg_cost.weight)
            match = lsa_solve(cost, gts.counts[None].expand(nl, bs), bad=flag.dev)
            # (``preset_normalisers``: set by ``graphs.GraphedTrainStep(exchange=)`` around its capture alone -- the static
            #  [2, L] rows it fills before every replay, because the all-reduce below cannot be captured)
            norm = getattr(self, 'preset_normalisers', None) if all_cls is not None else None
            if norm is None:
                norm = self._device_normalisers((match >= 0).sum((1, 2)), bs * nq)
            elif tuple(norm.shape) != (2, nl):
                raise ValueError('preset_normalisers %s for %d decoder layers' % (tuple(norm.shape), nl))
        loss_cls, loss_box, _ = det_set_loss(all_cls, all_box, match, tables, self.code_weights, norm,
                                             (self.loss_cls.loss_weight, loss_box_module.loss_weight), self.loss_cls.alpha,
                                             self.loss_cls.gamma, bad=flag.dev)
        flag.mirror(None)
        return loss_cls.unbind(0), loss_box.unbind(0)

    def pad_gts(self, gt_bboxes_list, gt_labels_list, capacity=None):
        """The per-sample gt lists -> ``PaddedGts`` on the head's device, ``capacity`` boxes per sample (default: the
        largest count): shapes that do not change with the counts, which a captured step needs -- new ground truth is
        copied into the same three tensors."""
        counts = [int(g.shape[0]) for g in gt_bboxes_list]
        largest = max(counts) if counts else 0
        cap = largest if capacity is None else int(capacity)
        if largest > cap:
            raise ValueError('pad_gts: a sample holds %d boxes, the capacity is %d' % (largest, cap))
        dev = self.code_weights.device
        boxes, labels = self._pad_tables(list(gt_bboxes_list), list(gt_labels_list), counts, cap, torch.float32, dev)
        return PaddedGts(boxes, labels, _to_device_async(torch.tensor(counts, dtype=torch.int32), dev))

    def _targets_device(self, all_cls, all_box, gts):
        """``_batched_targets`` from a ``PaddedGts`` with the assignment solved where the costs are: the same cost matrices
        [L, bs, Nq, cap], ``hipops.lsa_solve`` with every sample's count as its column bound (repeated per layer), the same
        gathers.  Only launches are queued -- no copy to the host, no synchronisation, no host-built tensor -- so the call
        can be captured.  -> (labels, bbox_targets, pos_mask, positives per layer as an int64 DEVICE tensor [L]).  A
        problem scipy would raise on leaves its queries unmatched and is reported by a later call (``AssignmentFlag``).
        CPU tensors: the same plumbing with scipy in place of the kernel."""
        if not self._restated_costs():
            raise NotImplementedError("solver='device' is built for FocalLossCost + BBox3DL1Cost assigners")
        nl, bs, nq, _ = all_cls.shape
        gt_pad, lab_pad, counts = gts.boxes.to(all_box.dtype), gts.labels, gts.counts
        if gt_pad.shape[1] == 0:                             # no box anywhere: one padding column keeps the gathers well-formed
            gt_pad, lab_pad = gt_pad.new_zeros(bs, 1, 9), lab_pad.new_zeros(bs, 1)
        ncols = counts[None].expand(nl, bs)
        with torch.no_grad():
            if all_box.is_cuda:
                from ..hipops import AssignmentFlag, lsa_solve
                cost = self._assignment_costs(all_cls, all_box, gt_pad, lab_pad)
                flag = AssignmentFlag.of(cost.device)
                flag.poll()                                  # a problem of an EARLIER step is reported here
                idx_t = lsa_solve(cost, ncols, bad=flag.dev).long()
                flag.mirror(None)
            else:
                cost = self._assignment_costs(all_cls, all_box, gt_pad, lab_pad)
                idx_t = torch.from_numpy(self._solve_on_host(cost.numpy(), counts.tolist()))
        labels, bbox_targets, pos_mask = self._targets_from_match(idx_t, gt_pad, lab_pad)
        # positives per layer, counted from the match like the host path: sum_b min(Nq, counts[b]) whenever every problem
        # was solved, and still the number of rows with a target when a flagged problem left its queries unmatched
        return labels, bbox_targets, pos_mask, pos_mask.sum((1, 2))

    @staticmethod
    def _solve_on_host(cost, counts):
        """The assignments on the host, as in the reference: scipy on ``cost[l, b, :, :counts[b]]`` of a numpy cost array
        [L, bs, Nq, G] for a list of counts -> numpy int64 [L, bs, Nq], -1 = unmatched."""
        from .assigner import linear_sum_assignment
        import numpy as np
        nl, bs, nq, _ = cost.shape
        idx = np.full((nl, bs, nq), -1, dtype=np.int64)
        for lvl in range(nl):
            for i, n in enumerate(counts):
                if n:
                    rows, cols = linear_sum_assignment(cost[lvl, i, :, :n])
                    idx[lvl, i, rows] = cols
        return idx

    def _device_normalisers(self, num_pos, per_layer):
        """``_losses_from_targets``' two normalisers fp32 [2, L] from the positives per layer as a device tensor: formed in
        fp64 and rounded to fp32 once, as the Python path does with its doubles (bit-identical on one rank).  With a process
        group the rounded rows are divided by the world size and summed in fp32 -- ``reduce_mean``'s own arithmetic on the
        Python path's ``new_tensor([value])``, so the two agree to the bit for any ``bg_cls_weight`` and world size -- in
        ONE all-reduce for both rows, and stay on the device: no ``float(reduce_mean(...))`` round trip per decoder layer."""
        import torch.distributed as dist
        n = num_pos.to(torch.float64)
        rows = torch.stack([n * 1.0 + (per_layer - n) * self.bg_cls_weight, n]).to(torch.float32)
        if dist.is_available() and dist.is_initialized():
            mean = rows / dist.get_world_size()
            dist.all_reduce(mean, op=dist.ReduceOp.SUM)
            rows = torch.stack([mean[0] if self.sync_cls_avg_factor else rows[0], mean[1]])
        return rows.clamp(min=1.0)

    _GT_SLOTS = {}

    @classmethod
    def _gt_slots(cls, counts, gmax, dev):
        """Rows of the padded [bs * Gmax] gt tables that hold a box, for this step's gt counts (int64 on ``dev``; the
        last few count patterns are kept: a fixed dataset order repeats them every epoch, a synthetic step every step)."""
        key = (counts, gmax, str(dev))
        hit = cls._GT_SLOTS.get(key)
        if hit is None:
            if len(cls._GT_SLOTS) >= 64:
                cls._GT_SLOTS.clear()
            rows = [i * gmax + j for i, c in enumerate(counts) for j in range(c)]
            hit = cls._GT_SLOTS[key] = _to_device_async(torch.tensor(rows, dtype=torch.long), dev)
        return hit

    def _losses_from_targets(self, all_cls, all_box, labels, bbox_targets, pos_mask, num_pos):
        """The detection terms of ``loss_single`` (head:903-976, applied per layer by multi_apply) for all L decoder layers
        at once, from precomputed targets -> (loss_cls [L], loss_bbox [L]): the same per-element terms, summed per layer and
        divided by that layer's normaliser.  Rows the reference drops by boolean indexing (non-finite normalised targets)
        get weight 0 instead, so nothing here synchronises with the host."""
        nl = all_cls.shape[0]
        per_layer = pos_mask[0].numel()
        if torch.is_tensor(num_pos):                     # (``_targets_device``: the counts never left the device)
            norm = self._device_normalisers(num_pos, per_layer)
        else:
            cls_avg, pos_avg = [], []
            for lvl in range(nl):
                f = num_pos[lvl] * 1.0 + (per_layer - num_pos[lvl]) * self.bg_cls_weight
                if self.sync_cls_avg_factor:
                    f = _mean_over_ranks(f, all_cls)
                cls_avg.append(max(f, 1))
                pos_avg.append(max(_mean_over_ranks(num_pos[lvl], all_cls), 1.0))
            norm = _to_device_async(torch.tensor([cls_avg, pos_avg], dtype=torch.float32), all_cls.device)
        cls_scores = all_cls.reshape(-1, self.cls_out_channels)
        elem = self.loss_cls(cls_scores, labels.reshape(-1), None, reduction_override='none')
        loss_cls = elem.reshape(nl, -1).sum(1) / norm[0]
        bbox_preds = all_box.reshape(-1, all_box.size(-1))
        pos = pos_mask.reshape(-1)
        normalized = normalize_bbox(bbox_targets.reshape(-1, bbox_targets.size(-1)), self.pc_range)
        keep = (torch.isfinite(normalized).all(dim=-1) & pos).to(bbox_preds.dtype)
        weights = keep[:, None] * self.code_weights
        target = torch.nan_to_num(normalized[:, :10], nan=0.0, posinf=0.0, neginf=0.0) * keep[:, None]
        elem = self.loss_bbox(bbox_preds[:, :10] * keep[:, None], target, weights[:, :10], reduction_override='none')
        loss_bbox = elem.reshape(nl, -1).sum(1) / norm[1]
        return torch.nan_to_num(loss_cls).unbind(0), torch.nan_to_num(loss_bbox).unbind(0)

    def get_occupancy_prediction(self, occ_results, occ_threshold=0.25):
        """head:1505-1540 (focal-loss branch): sigmoid, threshold as an extra "empty" column,
        arg-max -> sparse ``(voxel index, class)`` pairs of the occupied voxels."""
        logits = occ_results['occupancy_preds'].reshape(-1, self.occupancy_classes)
        if logits.is_cuda and self.occupancy_classes % 8 == 0:
            # on the device: one classification + ordered compaction (ver_occ_predict).  The kernel evaluates the sigmoid
            # in fp32 whatever the logits' dtype: the reference's pairs bit for bit on fp32 logits; on bf16 logits it is
            # the classification of `logits.float()` (a bf16 sigmoid would round the probabilities to 8 bits before
            # the threshold compare and the arg-max, and flip rows near the threshold or with near-equal classes)
            from ..hipops import occ_predict
            occ_results['occupancy_preds'] = occ_predict(logits, occ_threshold)
            occ_results['flow_preds'] = None
            return occ_results
        occ_class = classify(logits, occ_threshold)      # fp32 like the kernel and the (fp32) reference
        occ_index, = torch.where(occ_class < self.occupancy_classes)
        occ_results['occupancy_preds'] = torch.stack([occ_index, occ_class[occ_index]], dim=-1)
        occ_results['flow_preds'] = None
        return occ_results

    def _dump_volumes(self, voxel_embed, img_metas):
        """``getbev=<path>`` (head:627-638, the export run of projects/configs/verformer/get_occ.py): every forward
        appends the encoder output of its viewpoints to the volume store under ``img_metas[b]['sample_idx']`` -- float64,
        gzip, the raw ``(C, Z, H, W)`` view of the query-major ``[Nq, C]`` buffer.  The reference writes
        ``img_metas[0]`` only (bs = 1); a batched call writes one volume per sample.  voxel_embed: [bs, Nq, C]."""
        if self.getbev is None:
            return
        if not img_metas or len(img_metas) != voxel_embed.shape[0]:
            raise ValueError('getbev needs one img_meta with a sample_idx per viewpoint to name the volumes')
        if self._volume_writer is None:
            from ..volume_io import VolumeWriter
            self._volume_writer = VolumeWriter(self.getbev)
        for b, meta in enumerate(img_metas):
            self.export_volume(self._volume_writer, meta['sample_idx'], voxel_embed[b])

    def export_volume(self, writer, key, voxel_embed_sample):
        """``getbev`` dump of head:627-638 for one sample ([Nq,C] encoder output)."""
        return writer.write(key, voxel_embed_sample, (self.bev_z, self.bev_h, self.bev_w), self.embed_dims)

    def lift(self, mlvl_feats, img_metas=None, **kwargs):
        """The lifting path alone (encoder + occupancy branch, no detection decoder):
        -> (voxel_embed [bs,Nq,C], occupancy logits [bs, X*Y*Z, classes])."""
        voxel_embed = self.forward(mlvl_feats, img_metas, only_bev=True, **kwargs)
        return voxel_embed, self.occupancy_from_volume(voxel_embed)
