"""Float64 model of ver_mha_forward / _backward (include/ver_ops.h): the softmax attention of nn.MultiheadAttention between
the input projections and out_proj, forward and the three gradients from the formulas of the header, with an explicit keep
mask for the dropout on the probabilities.  The yardstick of tests/test_mha_cpu.py and tests/test_mha_gpu.py."""
import numpy as np
import torch


def _heads(t, heads):
    """[N, B, heads*hd] -> [B, heads, N, hd] (float64)."""
    n, b, c = t.shape
    return t.double().reshape(n, b, heads, c // heads).permute(1, 2, 0, 3)


def _rows(t):
    """[B, heads, N, hd] -> [N, B, heads*hd]."""
    b, h, n, hd = t.shape
    return t.permute(2, 0, 1, 3).reshape(n, b, h * hd)


def model(q, k, v, heads, grad_out=None, keep=None, p_drop=0.0):
    """q [Nq, B, C], k, v [Nk, B, C], grad_out [Nq, B, C] or None, keep bool [B, heads, Nq, Nk] or None (everything kept)
    -> dict(out, lse [B, heads, Nq]) and, with grad_out, grad_q, grad_k, grad_v.  Everything float64."""
    qh, kh, vh = _heads(q, heads), _heads(k, heads), _heads(v, heads)
    hd = qh.shape[-1]
    s = qh @ kh.transpose(-1, -2) / float(np.sqrt(hd))
    mx = s.max(-1, keepdim=True)[0]
    e = (s - mx).exp()
    p = e / e.sum(-1, keepdim=True)
    m = torch.ones_like(p) if keep is None else torch.as_tensor(keep).to(torch.float64)
    m = m / (1.0 - p_drop)
    pd = p * m
    res = dict(out=_rows(pd @ vh), lse=(mx + e.sum(-1, keepdim=True).log()).squeeze(-1))
    if grad_out is not None:
        do = _heads(grad_out, heads)
        dv = pd.transpose(-1, -2) @ do
        dp = (do @ vh.transpose(-1, -2)) * m
        ds = p * (dp - (dp * p).sum(-1, keepdim=True))
        res.update(grad_q=_rows(ds @ kh / float(np.sqrt(hd))), grad_k=_rows(ds.transpose(-1, -2) @ qh / float(np.sqrt(hd))),
                   grad_v=_rows(dv))
    return res


def keep_indices(B, heads, Nq, Nk):
    """idx = ((b*heads + h)*Nq + i)*Nk + j as an int64 array [B, heads, Nq, Nk]."""
    return np.arange(B * heads * Nq * Nk, dtype=np.int64).reshape(B, heads, Nq, Nk)


def make_inputs(seed, B, heads, hd, Nq, Nk, quant=None):
    """Seeded standard-normal q, k, v, grad_out in the kernels' layout ([N, B, heads*hd], float64); ``quant`` rounds them to the
    operand format first (the bf16 cases are judged on the rounded inputs)."""
    rng = np.random.default_rng(seed)
    quant = quant or (lambda t: t)
    f = lambda n: quant(torch.from_numpy(rng.standard_normal((n, B, heads * hd)).astype(np.float32))).double()
    return dict(q=f(Nq), k=f(Nk), v=f(Nk), grad_out=f(Nq))


def f32_bound(want):
    """fp32 precision contract as the issue states it: 1e-4 of the model's largest magnitude, per tensor."""
    return 1e-4 * float(want.abs().max())


def check_f32(got, want, what):
    d = float((got.detach().double().cpu() - want).abs().max())
    bound = f32_bound(want)
    print('%-10s max|delta| %.3e  bound %.3e  max|ref| %.3e' % (what, d, bound, float(want.abs().max())))
    assert bool(torch.isfinite(got).all()), what
    assert d <= bound, (what, d, bound)


def check_bf16(got, want, what):
    """bf16 contract: relative L2 <= 1e-2 against the float64 model on the bf16-rounded inputs."""
    g = got.detach().double().cpu()
    nrm = float(want.norm())
    r = float((g - want).norm()) / nrm if nrm > 0 else float(g.abs().max())
    print('%-10s rel L2 %.3e  |ref| %.3e' % (what, r, nrm))
    assert bool(torch.isfinite(got).all()), what
    assert r <= 1e-2, (what, r)
