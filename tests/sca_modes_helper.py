"""Case builders of the fused-gather tests.  ``random_sca_case``: the hit table of the synthetic cameras over a voxel grid with
random value / offsets / logits / grad rows (tests/test_hip_ops_gpu.py, tests/test_sca_backward_forms_gpu.py).  ``case``
(test_sca_gather_samples_outside_the_map): a gather case at the 14x14 map with random offsets or the reference's initial ring
of offsets."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import cases  # noqa: E402


def random_sca_case(seed, B, grid, heads, hd, P, map_hw=(14, 14), D=1):
    """hit table (device) and numpy fp32 value [B,6,Nk,heads,hd], offsets [B,Nq,heads,P,2] (pixels, 3 sigma), logits
    [B,Nq,heads,P], grad rows [B,Nq,heads*hd]."""
    syn = importlib.import_module('vln-ver_amd.synthetic')
    hip = importlib.import_module('vln-ver_amd.hipops')
    rng = np.random.default_rng(seed)
    z, h, w = grid
    nq = z * h * w
    nk = map_hw[0] * map_hw[1]
    w2p, org = syn.camera_batch(B, seed=1)
    hit = hip.project_points(torch.from_numpy(w2p).to('cuda'), torch.from_numpy(org).to('cuda'), cases.PC_RANGE, z, h, w)
    value = rng.standard_normal((B, 6, nk, heads, hd)).astype(np.float32)
    offsets = (rng.standard_normal((B, nq, heads, P, 2)) * 3.0).astype(np.float32)
    logits = rng.standard_normal((B, nq, heads, P)).astype(np.float32)
    gslots = rng.standard_normal((B, nq, heads * hd)).astype(np.float32)
    return hit, value, offsets, logits, gslots


def case(seed, B, grid, heads, hd, ring):
    syn = importlib.import_module('vln-ver_amd.synthetic')
    hip = importlib.import_module('vln-ver_amd.hipops')
    rng = np.random.default_rng(seed)
    z, h, w = grid
    nq = z * h * w
    w2p, org = syn.camera_batch(B, seed=1)
    hit = hip.project_points(torch.from_numpy(w2p).cuda(), torch.from_numpy(org).cuda(), cases.PC_RANGE, z, h, w)
    value = torch.from_numpy(rng.standard_normal((B, 6, 196, heads, hd)).astype(np.float32)).cuda()
    logits = torch.from_numpy(rng.standard_normal((B, nq, heads, 8)).astype(np.float32)).cuda()
    if ring:        # the reference's initial offsets (spatial_cross_attention.py:255-270): many samples miss the map
        th = torch.arange(heads, dtype=torch.float32) * (2.0 * np.pi / heads)
        d = torch.stack([th.cos(), th.sin()], -1)
        d = d / d.abs().max(-1, keepdim=True)[0]
        ring_o = d[:, None, :] * torch.arange(1, 9, dtype=torch.float32)[None, :, None]
        offsets = ring_o.cuda()[None, None].expand(B, nq, heads, 8, 2).contiguous()
    else:
        offsets = torch.from_numpy((rng.standard_normal((B, nq, heads, 8, 2)) * 3.0).astype(np.float32)).cuda()
    return hip, hit, value, offsets, logits
