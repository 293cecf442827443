"""The float64 model of ``optim.ClipAdamW`` (tests/optim_model_helper.py), which tests/test_optim_graph_gpu.py holds the
HIP kernels to, pinned to ``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.AdamW`` run in float64 on the CPU."""
import pytest
import torch

from optim_model_helper import AdamWModel


@pytest.mark.parametrize('max_norm', [0.7, 1e9, 0.0])             # clipping active (on most steps), inactive, off
def test_adamw_model_equals_clip_grad_norm_plus_torch_adamw_in_float64(max_norm):
    """Six steps, two parameter groups with their own lr / weight decay / eps under one clip norm, a parameter whose first
    gradient arrives two steps late (its own bias corrections), one step with gradients ten times as large.  torch forms
    the first moment as a lerp and the step as ``addcdiv``: the same real-number arithmetic, a few double roundings apart,
    so parameters and moments agree to 1e-12 of max |.| and the norm to 1e-12 relative."""
    gen = torch.Generator().manual_seed(5)
    shapes = [(1,), (5,), (33, 7), (1031,), (257,)]
    base = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]

    def groups(ps):
        return [dict(params=ps[:3], lr=3e-3, weight_decay=0.05), dict(params=ps[3:], lr=3e-4, weight_decay=0.0, eps=1e-6)]
    ref = [torch.nn.Parameter(b.clone()) for b in base]
    opt = torch.optim.AdamW(groups(ref), betas=(0.9, 0.99))
    model = AdamWModel(groups(base), betas=(0.9, 0.99), max_norm=max_norm)
    worst, clipped = 0.0, 0
    for it in range(6):
        grads = [None if (i == 2 and it < 2) else torch.randn(s, generator=gen, dtype=torch.float64) * (10.0 if it == 3 else 0.005 if it == 4 else 1.0)
                 for i, s in enumerate(shapes)]
        for q, g in zip(ref, grads):
            q.grad = None if g is None else g.clone()
        with_grad = [q for q in ref if q.grad is not None]
        want_norm = torch.linalg.vector_norm(torch.cat([q.grad.reshape(-1) for q in with_grad]))
        if max_norm > 0:
            clipped += int(float(torch.nn.utils.clip_grad_norm_(with_grad, max_norm)) > max_norm)
        opt.step()
        norm = model.step(grads)
        assert norm.dtype == torch.float64 and abs(float(norm) - float(want_norm)) <= 1e-12 * float(want_norm)
        for i, q in enumerate(ref):
            pairs = [(model.p[i], q.detach())]
            if grads[i] is not None or it >= 2 or i != 2:
                st = opt.state[q]
                pairs += [(model.m[i], st['exp_avg']), (model.v[i], st['exp_avg_sq'])]
                assert model.k[i] == int(st['step'])
            for got, want in pairs:
                d = float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)
                worst = max(worst, d)
                assert d <= 1e-12, (it, i, d)
    assert model.k == [6, 6, 4, 6, 6]
    if max_norm == 0.7:
        assert 0 < clipped < 6                                          # (the small step stays under the bound)
    print('fp64 AdamW model vs torch, max_norm %g: worst distance %.2e of max |.| (bound 1e-12)' % (max_norm, worst))
