"""Float64 restatement of the detection decoder's deformable attention between its input Linears and output_proj, and
the input generators of tests/test_dattn3d_cpu.py / test_dattn3d_gpu.py.

The reference is torch in float64: softmax over the (level, point) logits of a (query, head), loc = ref + offsets /
(W, H, D), then the package's ``voxel_decoder.voxel_multi_scale_deformable_attn`` (the grid_sample form pinned to the
reference's vectors by test_oracle_golden.py).  Gradients come from autograd on it.

Trilinear gradients jump where a sampling coordinate loc*size - 0.5 is an integer.  That is a condition on the INPUTS, not
a tolerance: ``keep_off_the_lattice`` moves an offending offset by 0.01 of a cell (offsets are in cells) until every
coordinate is at least ``MIN_DIST`` away from an integer, and ``lattice_distance`` is what the tests assert it with."""
import numpy as np
import torch

from util import pkg

MIN_DIST = 1e-3
BF16_EPS = 2.0 ** -8          # one bf16 rounding, relative (8 significand bits, round to nearest)


def sizes_whd(shapes, dtype=torch.float64):
    """[L, 3] = (W, H, D) of every level: what the (x, y, z) offsets are divided by."""
    s = torch.as_tensor(np.asarray(shapes, dtype=np.int64).reshape(-1, 3))
    return torch.stack([s[:, 2], s[:, 1], s[:, 0]], -1).to(dtype)


def level_start(shapes):
    s = np.asarray(shapes, dtype=np.int64).reshape(-1, 3)
    n = s[:, 0] * s[:, 1] * s[:, 2]
    return torch.from_numpy(np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64))


def locations(shapes, ref, offsets):
    """float64 loc [B, Nq, heads, L, P, 3]: the division first, then the add."""
    whd = sizes_whd(shapes)
    return ref.double()[:, :, None, :, None, :] + offsets.double() / whd[None, None, None, :, None, :]


def lattice_distance(shapes, ref, offsets):
    """Smallest distance of a sampling coordinate loc*size - 0.5 to an integer, over every sample and axis (float64)."""
    pix = locations(shapes, ref, offsets) * sizes_whd(shapes)[None, None, None, :, None, :] - 0.5
    return float((pix - pix.round()).abs().min())


def keep_off_the_lattice(shapes, ref, offsets, quant=lambda t: t):
    """``offsets`` with every offending entry moved by the first multiple of 0.01 of a cell that puts its coordinate at least
    MIN_DIST (with a margin for the rounding of ``quant``, e.g. to bf16) away from an integer.  No sample is dropped."""
    whd = sizes_whd(shapes)[None, None, None, :, None, :]
    base = offsets.clone()
    out = quant(base)
    for k in range(1, 400):
        pix = (ref.double()[:, :, None, :, None, :] + out.double() / whd) * whd - 0.5
        bad = (pix - pix.round()).abs() < 2 * MIN_DIST
        if not bool(bad.any()):
            break
        out = torch.where(bad, quant(base + 0.01 * k), out)
    assert lattice_distance(shapes, ref, out) >= MIN_DIST
    return out


def make_inputs(seed, batch, shapes, heads, head_dim, num_query, points, lo=-0.2, hi=1.2, quant=lambda t: t):
    """float32 operands: ref in [0, 1], offsets such that loc spans [lo, hi], standard-normal value / logits / grad_out.
    ``quant`` rounds value, offsets and logits (the bf16 cases); the lattice condition holds for the rounded offsets."""
    rng = np.random.default_rng(seed)
    shp = np.asarray(shapes, dtype=np.int64).reshape(-1, 3)
    nlev = shp.shape[0]
    nk = int((shp[:, 0] * shp[:, 1] * shp[:, 2]).sum())
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    value = quant(f32(rng.standard_normal((batch, nk, heads, head_dim))))
    ref = f32(rng.uniform(0.0, 1.0, (batch, num_query, nlev, 3)))
    loc = torch.from_numpy(rng.uniform(lo, hi, (batch, num_query, heads, nlev, points, 3)))
    offsets = ((loc - ref.double()[:, :, None, :, None, :]) * sizes_whd(shp)[None, None, None, :, None, :]).float()
    offsets = keep_off_the_lattice(shp, ref, offsets, quant)
    logits = quant(f32(rng.standard_normal((batch, num_query, heads, nlev * points))))
    grad_out = f32(rng.standard_normal((batch, num_query, heads * head_dim)))
    return dict(value=value, shapes=torch.from_numpy(shp), level_start=level_start(shp), ref=ref, offsets=offsets,
                logits=logits, grad_out=grad_out)


def from_msda3d(c):
    """Operands of ``cases.msda3d_inputs`` (loc, softmax weights w) as operands of the fused op: ref = 0, offsets = loc *
    (W, H, D), logits = log(w).  float64, so that the mapping adds nothing of its own."""
    shp = np.asarray(c['shapes'], dtype=np.int64).reshape(-1, 3)
    loc = torch.from_numpy(c['loc']).double()
    b, nq, heads, nlev, npt, _ = loc.shape
    return dict(value=torch.from_numpy(c['value']), shapes=torch.from_numpy(shp), level_start=level_start(shp),
                ref=torch.zeros(b, nq, nlev, 3, dtype=torch.float64),
                offsets=loc * sizes_whd(shp)[None, None, None, :, None, :],
                logits=torch.from_numpy(c['w']).double().reshape(b, nq, heads, nlev * npt).log(),
                grad_out=torch.from_numpy(c['grad_out']))


def reference(c, want_grads=True):
    """float64 on the CPU: dict(out, grad_value, grad_offsets, grad_logits, grad_ref) of the operands ``c``."""
    dec = pkg('modules.voxel_decoder')
    value = c['value'].detach().double().cpu().requires_grad_(want_grads)
    ref = c['ref'].detach().double().cpu().requires_grad_(want_grads)
    offsets = c['offsets'].detach().double().cpu().requires_grad_(want_grads)
    logits = c['logits'].detach().double().cpu().requires_grad_(want_grads)
    shapes = [[int(v) for v in row] for row in c['shapes'].tolist()]
    b, nq, heads, nlev, npt, _ = offsets.shape
    w = logits.softmax(-1).view(b, nq, heads, nlev, npt)
    loc = ref[:, :, None, :, None, :] + offsets / sizes_whd(shapes)[None, None, None, :, None, :]
    out = dec.voxel_multi_scale_deformable_attn(value, shapes, loc, w)
    res = dict(out=out.detach())
    if want_grads:
        out.backward(c['grad_out'].detach().double().cpu())
        res.update(grad_value=value.grad, grad_offsets=offsets.grad, grad_logits=logits.grad, grad_ref=ref.grad)
    return res


def softmax_backward(w, grad_w):
    """d(logits) of d(softmax weights): w * (g - sum(w * g)) over the last axis, float64."""
    w, grad_w = w.double(), grad_w.double()
    return w * (grad_w - (w * grad_w).sum(-1, keepdim=True))


def f32_bound(want):
    """README, "Precision contract": max |delta| <= 1e-4 * max(1, max |reference|) per tensor."""
    return 1e-4 * max(1.0, float(want.abs().max()))


def check_f32(got, want, what):
    d = float((got.detach().double().cpu() - want).abs().max())
    bound = f32_bound(want)
    print('%-14s max|delta| %.3e  bound %.3e  max|ref| %.3e' % (what, d, bound, float(want.abs().max())))
    assert d <= bound, (what, d, bound)


def check_bf16_stored(got, want, what):
    """An output stored as bf16: the fp32 bound plus one bf16 rounding of the reference, elementwise."""
    d = (got.detach().double().cpu() - want).abs()
    bound = f32_bound(want) + BF16_EPS * want.abs()
    print('%-14s max|delta| %.3e  worst delta/bound %.3f' % (what, float(d.max()), float((d / bound).max())))
    assert bool((d <= bound).all()), (what, float((d / bound).max()))
