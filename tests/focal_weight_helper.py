"""The model of the class-weighted occupancy focal loss shared by tests/test_focal_weight_cpu.py and _gpu.py: the formula
of ``oracle.ver_oracle.focal_loss`` restated in float64, times ``class_weight[target][:, None]`` (mmdet's
``loss * weight.view(-1, 1)`` with the reference's ``weight = weights[gt_occupancy]``, head:1417-1425)."""
import numpy as np
import torch
import torch.nn.functional as F


def model_elements(logits, target, class_weight, gamma=2.0, alpha=0.25):
    """float64 [N, C]: the elementwise weighted focal loss (differentiable w.r.t. ``logits`` when it requires grad)."""
    x = logits.double()
    c = x.shape[1]
    t = F.one_hot(target.long(), c + 1)[:, :c].double()
    p = x.sigmoid()
    pt = (1 - p) * t + p * (1 - t)
    w = (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma)
    loss = F.binary_cross_entropy_with_logits(x, t, reduction='none') * w
    return loss * class_weight.double()[target.long()][:, None]


def weights_for(classes, seed):
    """[0.25, 4] per class, one class exactly 0, the empty class 0.5."""
    w = torch.from_numpy(np.random.default_rng(seed).uniform(0.25, 4.0, classes + 1).astype(np.float32))
    w[3] = 0.0
    w[classes] = 0.5
    return w
