"""Shared by tests/test_infer_gpu.py and tests/test_infer_graph_gpu.py: vocc.py's head with seeded weights on the GPU (built
once per process) and synthetic viewpoints, as tests/test_train_graph_gpu.py builds them."""
import numpy as np
import torch

import cases
from util import pkg

T = torch.from_numpy
DEV = torch.device('cuda', 0)
_CACHE = {}


def head():
    if 'head' not in _CACHE:
        torch.backends.cuda.matmul.allow_tf32 = False
        torch.backends.cudnn.allow_tf32 = False
        pkg()
        h = pkg('registry').build_head(dict(cases.vocc_head_cfg(), train_cfg=cases.VOCC_TRAIN_CFG)).eval()
        code_weights = h.code_weights.detach().clone()
        pkg('synthetic').load_seeded(h, 7)
        h.code_weights.data.copy_(code_weights)          # (the seeded fill also hits this fixed, non-trainable loss-weight vector)
        _CACHE['head'] = h.to(DEV)
    return _CACHE['head']


def threshold():
    """An occupancy threshold at which about half of the voxels of viewpoint 0 are occupied: with seeded weights every
    voxel clears the default 0.25, and a test of the compaction wants both kinds.  The median of the best class
    probability of the fp32 logits (an fp32 value, handed on as it is); computed once."""
    if 'thr' not in _CACHE:
        h = head()
        with torch.no_grad():
            volume = h(viewpoints(1)[0], None, only_bev=True, world2pixel=viewpoints(1)[1], origin=viewpoints(1)[2])
            best = h.occupancy_from_volume(volume).float().sigmoid().amax(-1)
        _CACHE['thr'] = float(best.flatten().median())
    return _CACHE['thr']


def viewpoints(n, first=0):
    """(feats [6, n, 196, 768], world2pixel [n, 6, 4, 4], origin [n, 3]) of synthetic viewpoints first .. first + n - 1."""
    syn = pkg('synthetic')
    w2p, org = syn.camera_batch(first + n, seed=1)
    feats = T(syn.vit_features(first + n, seed=0)).to(DEV)
    return (feats[first:].permute(1, 0, 2, 3).contiguous(), T(w2p[first:]).to(DEV).contiguous(), T(org[first:]).to(DEV).contiguous())


def model_pairs(h, outs):
    """``occ_pairs_host`` of the step's own class bytes: (pairs, offsets, count) as numpy."""
    hip, opl = pkg('hipops'), pkg('dense_heads.occ_proj_lattice')
    bs = outs.volume.shape[0]
    table = opl.row_table(outs.plan) if outs.plan is not None else None
    return hip.occ_pairs_host(outs.classes.cpu().numpy(), bs, h.voxel_num, h.occ_zdim, h.occupancy_classes, table,
                              outs.occ_pairs.shape[0])


def same_as_model(h, outs):
    """The step's pairs, offsets and counts equal the model's, bit for bit; -> (live pairs as numpy, offsets)."""
    pairs, offsets, count = model_pairs(h, outs)
    got = [t.cpu().numpy() for t in (outs.occ_pairs, outs.occ_offsets, outs.occ_count)]
    assert np.array_equal(got[1], offsets) and np.array_equal(got[2], count), (got[1], offsets, got[2], count)
    n = int(offsets[-1])
    assert got[0].dtype == pairs.dtype and np.array_equal(got[0][:n], pairs[:n])
    return got[0][:n], offsets


def flat_pairs(outs, voxel_num):
    """The per-sample pairs as int64 [K, 2] over the flattened batch: what ``occupancy_pairs_from_classes`` returns."""
    off = outs.occ_offsets.cpu().tolist()
    pairs = outs.occ_pairs.cpu().long()
    out = []
    for b in range(len(off) - 1):
        p = pairs[off[b]:off[b + 1]].clone()
        p[:, 0] += b * voxel_num
        out.append(p)
    return torch.cat(out)
