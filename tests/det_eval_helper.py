"""Inputs shared by test_det_eval_cpu.py and test_det_eval_gpu.py: room-scale random boxes, screened detection batches and
random outputs of the vocc detection head."""
import numpy as np
import torch

import cases
from util import pkg

THR = (0.10, 0.25, 0.5, 0.75)
THR8 = (0.05, 0.10, 0.25, 0.35, 0.5, 0.6, 0.75, 0.9)
MARGIN = 1e-4


def random_boxes(rng, n):
    """[n, 7] fp32: centres in the vocc.py range, dimensions 0.1 - 4 m, any yaw (more than one turn either way)."""
    lo, hi = np.array(cases.PC_RANGE[:3]), np.array(cases.PC_RANGE[3:])
    return np.concatenate([rng.uniform(lo, hi, (n, 3)), rng.uniform(0.1, 4.0, (n, 3)), rng.uniform(-7.0, 7.0, (n, 1))],
                          1).astype(np.float32)


def draw_sample(rng, pcap, gcap, ng, classes=cases.CLASS_NUM):
    """One image: ``ng`` ground truths in ``gcap`` slots (the rest filled with boxes that must not be read as valid),
    ``pcap`` predictions = jittered copies of ground truths (same label) followed by random boxes, scores in random order."""
    gb, gl = random_boxes(rng, gcap), rng.integers(0, classes, gcap)
    pb, pl = random_boxes(rng, pcap), rng.integers(0, classes, pcap)
    if ng:
        src = rng.integers(0, ng, pcap)
        copy = rng.random(pcap) < 0.6
        jitter = gb[src] + rng.normal(0, 1, (pcap, 7)).astype(np.float32) * np.array([.15, .15, .1, .1, .1, .1, .2], np.float32)
        jitter[:, 3:6] = np.maximum(jitter[:, 3:6], 0.05)
        pb = np.where(copy[:, None], jitter, pb).astype(np.float32)
        pl = np.where(copy, gl[src], pl)
    ps = rng.random(pcap).astype(np.float32)
    return dict(pb=pb, pl=pl.astype(np.int32), ps=ps, pv=np.ones(pcap, np.uint8), gb=gb, gl=gl.astype(np.int32), ng=ng)


def needs_redraw(sample, thresholds, margin=MARGIN):
    """The float64 host model decides: a same-class pair within ``margin`` of a threshold, a prediction whose two best
    same-class IoUs lie within ``margin`` of each other, or two equal scores.  Two best IoUs that are both EXACTLY 0 in the
    model (disjoint boxes: the separating-axis case, where kernel and model both return a true zero and both keep the first
    candidate) are no near-tie -- with 17 classes nearly every image has a prediction with two disjoint same-class ground
    truths, and the rule would otherwise redraw them all."""
    dm = pkg('detection_metrics')
    ng = sample['ng']
    if len(np.unique(sample['ps'])) != len(sample['ps']):
        return True
    if not ng:
        return False
    iou = dm.box3d_overlaps_host(sample['pb'], sample['gb'][:ng])
    same = sample['pl'][:, None] == sample['gl'][None, :ng]
    if any((np.abs(iou[same] - float(np.float32(t))) < margin).any() for t in thresholds):
        return True
    top = np.sort(np.where(same, iou, -1.0), 1)[:, ::-1]
    if ng >= 2:
        two = (top[:, 1] >= 0) & (top[:, 0] - top[:, 1] < margin) & (top[:, 0] > 0)
        if two.any():
            return True
    return False


def screened_batch(seed, s, pcap, gcap, thresholds, counts=None):
    """-> (dict of stacked arrays pb [S, P, 7], pl, ps, pv, gb [S, G, 7], gl, ngt [S]; number of redrawn samples)."""
    rng = np.random.default_rng(seed)
    samples, redrawn = [], 0
    for i in range(s):
        ng = int(counts[i]) if counts is not None else int(rng.integers(0, gcap + 1))
        bad = False
        for _ in range(20):
            smp = draw_sample(rng, pcap, gcap, ng)
            if not needs_redraw(smp, thresholds):
                break
            bad = True
        else:
            raise AssertionError('no screened sample in 20 draws')
        redrawn += bad
        samples.append(smp)
    out = {k: np.stack([smp[k] for smp in samples]) for k in ('pb', 'pl', 'ps', 'pv', 'gb', 'gl')}
    out['ngt'] = np.array([smp['ng'] for smp in samples], np.int32)
    return out, redrawn


def build_head(device='cpu'):
    pkg()
    torch.manual_seed(3)
    return pkg('registry').build_head(dict(cases.vocc_head_cfg(), train_cfg=cases.VOCC_TRAIN_CFG)).eval().to(device)


def random_head_outputs(seed, bs, layers=2):
    """``preds_dicts`` of the detection branch with random content: logits [L, bs, Nq, C], normalised boxes [L, bs, Nq, 10]
    = (cx, cy, log w, log l, cz, log h, sin, cos, vx, vy) spread over (and a little beyond) the coder's centre range."""
    g = torch.Generator().manual_seed(seed)
    nq, nc = cases.QUERY_NUM, cases.CLASS_NUM
    cls = torch.randn(layers, bs, nq, nc, generator=g) * 2.0
    box = torch.randn(layers, bs, nq, 10, generator=g)
    box[..., 0:2] *= 5.5
    box[..., 4] = box[..., 4] * 2.0
    box[..., [2, 3, 5]] = box[..., [2, 3, 5]] * 0.6
    return dict(all_cls_scores=cls, all_bbox_preds=box)


def gts_near(head_boxes, seed, take):
    """Ground truths for one image from its own decoded boxes ``[boxes [k, >=7] bottom-centre, scores, labels]``: ``take``
    of them, jittered, with the prediction's label -> (boxes fp32 [take, 7], labels int64 [take])."""
    boxes, _, labels = head_boxes
    g = torch.Generator().manual_seed(seed)
    take = min(take, boxes.shape[0])
    pick = torch.randperm(boxes.shape[0], generator=g)[:take]
    gb = boxes[pick, :7].detach().cpu().float().clone()
    gb += torch.randn(take, 7, generator=g) * torch.tensor([.1, .1, .05, .05, .05, .05, .1])
    gb[:, 3:6] = gb[:, 3:6].clamp(min=0.05)
    return gb, labels[pick].detach().cpu().long()


def head_batches(head, seeds_and_sizes=((11, 2), (12, 3), (13, 1))):
    """-> [(preds_dicts, PaddedGts, gt boxes list, gt labels list, get_bboxes lists)] per batch."""
    out = []
    for seed, bs in seeds_and_sizes:
        preds = {k: v.to(head.code_weights.device) for k, v in random_head_outputs(seed, bs).items()}
        lists = head.get_bboxes(preds)
        takes = [(7 * seed + 3 * i) % 9 for i in range(bs)]                              # 0..8 ground truths, some images none
        gts = [gts_near(lists[i], 100 * seed + i, takes[i]) for i in range(bs)]
        gb, gl = [g[0] for g in gts], [g[1] for g in gts]
        out.append((preds, head.pad_gts(gb, gl, capacity=8), gb, gl, lists))
    return out


def lists_to_annos(batches):
    gt_annos, dt_annos = [], []
    for _, _, gb, gl, lists in batches:
        for i in range(len(gb)):
            gt_annos.append(dict(gt_num=len(gl[i]), gt_boxes_upright_depth=gb[i].cpu().numpy(), **{'class': gl[i].cpu().numpy()}))
            dt_annos.append(dict(boxes_3d=lists[i][0][:, :7], scores_3d=lists[i][1], labels_3d=lists[i][2]))
    return gt_annos, dt_annos
