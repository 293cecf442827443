"""The float64 model of ``optim.ClipAdamW`` shared by tests/test_optim_model_cpu.py and tests/test_optim_graph_gpu.py: the
arithmetic stated at the top of csrc/ver_optim.hip in plain torch, one statement per line of that comment.  The model
holds the parameters, both moments and the update counts itself, so a test drives it with the gradient sequence it gives
the optimizer.  tests/test_optim_model_cpu.py pins it to ``clip_grad_norm_`` + ``torch.optim.AdamW`` in float64."""
import torch


class AdamWModel:
    """``groups``: [dict(params=[tensors], lr=, betas=, eps=, weight_decay=)] (the keys default like ClipAdamW's); the
    tensors are copied to float64 on the CPU, in the order of the groups.  ``step(grads)`` takes one gradient (or None: the
    tensor is skipped and its count does not move) per tensor in that order and returns the unclipped norm, a float64 scalar."""

    def __init__(self, groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=0.0):
        self.max_norm = float(max_norm)
        self.groups, self.p, self.group_of = [], [], []
        for gi, group in enumerate(groups):
            self.groups.append(dict(lr=group.get('lr', lr), betas=tuple(group.get('betas', betas)), eps=group.get('eps', eps),
                                    weight_decay=group.get('weight_decay', weight_decay)))
            for t in group['params']:
                self.p.append(t.detach().cpu().double().clone())
                self.group_of.append(gi)
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.k = [0] * len(self.p)

    def step(self, grads):
        assert len(grads) == len(self.p)
        grads = [None if g is None else g.detach().cpu().double() for g in grads]
        have = [g for g in grads if g is not None]
        if not have:
            return torch.zeros((), dtype=torch.float64)
        norm = torch.sqrt(sum((g * g).sum() for g in have))
        factor = torch.ones((), dtype=torch.float64)
        if self.max_norm > 0:
            factor = torch.clamp(self.max_norm / (norm + 1e-6), max=1.0)          # (torch.clamp hands a NaN on)
        for i, g in enumerate(grads):
            if g is None:
                continue
            h = self.groups[self.group_of[i]]
            lr, (b1, b2), eps, wd = h['lr'], h['betas'], h['eps'], h['weight_decay']
            self.k[i] += 1
            k = self.k[i]
            g = g.reshape(self.p[i].shape) * factor
            self.p[i] *= 1 - lr * wd
            self.m[i] = b1 * self.m[i] + (1 - b1) * g
            self.v[i] = b2 * self.v[i] + (1 - b2) * g * g
            self.p[i] -= (lr / (1 - b1 ** k)) * self.m[i] / (self.v[i].sqrt() / (1 - b2 ** k) ** 0.5 + eps)
        return norm
