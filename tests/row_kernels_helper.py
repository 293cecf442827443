"""fp64 references, fp32 models and bounds for the three row-wise streaming kernels (test_row_kernels_cpu.py,
test_row_kernels_gpu.py): ``ver_add_ln_*`` and ``ver_relu_dropout_*`` (csrc/ver_addln.hip), ``ver_ln_relu_*`` (csrc/ver_mlp.hip).
Pure torch / numpy on the CPU; nothing here ever sees a kernel's output when a bound is formed.

Per kernel:
  * the EXACT chain: the operation in fp64 on the dtype-rounded inputs (``*_eval(..., torch.float64)``; the backward pass is
    written out, test_row_kernels_cpu.py holds it against autograd of torch.nn.functional);
  * two fp32 models of the kernel's arithmetic: the same formulas in plain torch fp32, and ``*_ordered``, which follows the
    order read off the kernel -- per-lane partial sums (add_ln: lane l of 64 owns elements 4 (l + 64 k) .. + 3, the four of a
    k added pairwise; ln_relu: lane l of 16 owns 8 consecutive channels), the 64- / 16-lane butterfly of ver_common.h group_sum
    (every step adds a lane's value to its partner's, so every lane ends with the balanced tree over neighbouring lanes:
    ``tree``), mean first and the variance from the centred values, 1 / C as an fp32 factor, the parameter sums per lane over
    the rows of the grid-stride loop, then over the waves / row slots of a workgroup, then over the workgroups (float
    atomics: any order; the model takes them in turn).  bf16 outputs are the fp32 model rounded to nearest even once.  A
    model of WHERE the arithmetic happens, not of bits: the compiler's fused multiply-adds and the hardware reciprocal
    square root are left to the factor below;
  * the keep mask: ``hipops.dropout_keep_host`` on the flat element index;
  * ``distances``: relative L2 over the whole tensor (``all``), over the worst column (``col``) and the worst row (``row``),
    each slice norm in a denominator floored at the tensor's RMS slice norm, and the largest absolute difference (``maxabs``);
    for 1/std and the element-wise kernel also the largest relative difference of an element (``relmax``);
  * ``bounds``: ``4 d_ref + floor`` per statistic, d_ref the larger distance of the two fp32 models from the exact chain on
    the same inputs.  The floor is 16 ulps at the tensor's largest magnitude for ``maxabs`` and 16 * 2^-23 for the relative
    statistics.  The ulp is fp32's for bf16 outputs too: their one rounding is inside d_ref already, and 16 bf16 ulps would
    be 6 % of the largest element -- the smaller floor only asks more.

Ceilings (``CEILINGS``): no bound may exceed what the op tests of test_hip_ops_gpu.py grant the quantity -- 2e-5 for a forward
fp32 output, 1e-4 (+ 1e-4 relative) for d(residual) / d(a) / d(x) in fp32, 2e-3 (+ 1e-4 relative) for a parameter gradient; a
larger one means the inputs are wrong.  Those figures were granted on rows of mean 0.  On the batches with edge rows
(``edge=True``: rows of mean 100, whose fp32 INPUTS have an ulp of 7.6e-6 so that the fp32 mean alone moves y by 1e-5)
the element-wise ceilings are held by the whole-tensor statistic instead of ``maxabs``; everywhere else by both.

ln_relu runs on GATE-STABLE rows (``ln_relu_rows``): a candidate row is kept iff every pre-ReLU value of the exact chain is
further from 0 than ``MARGIN`` = 1e-3; the helper asserts that MARGIN >= 4 x the largest move of a pre-ReLU value between a
model and the exact chain, that every model has the exact chain's gates on every row, and that N rows came from at most 2 N
candidates.

Denormal and non-finite inputs of relu_dropout: the exact chain maps a product beyond the output type's range to inf, as the
fp32 multiply does.  Positions holding a denormal x are left out of the statistics (``denormal``: whether a device keeps or
flushes them is its denormal mode, see include/ver_ops.h); the GPU test checks them on their own.
"""
import functools
import importlib
import math

import numpy as np
import torch

EPS = float(np.float32(1e-5))            # what the kernels receive as `float eps`
FACTOR = 4.0
ULPS = 16
MARGIN = 1e-3
EDGE_ROWS = 41                           # rows of add_ln's edge batch: 36 random rows around the five edge rows
SEEDS = (0, 1, 2 ** 62 - 1, -1, 0x9E3779B97F4A7C15 - 2 ** 64)
# launch constants of the launchers (csrc/ver_addln.hip, csrc/ver_mlp.hip): workgroups at most, rows per workgroup
ADD_LN_FWD_GRID, ADD_LN_BWD_GRID, ADD_LN_ROWS = 8192, 2048, 4
RELU_DROPOUT_GRID, RELU_DROPOUT_PER_WG = 16384, 256 * 4
LN_RELU_GRID, LN_RELU_ROWS = 4096, 16
# quantity -> (absolute, relative) ceiling of a bound (module docstring)
CEILINGS = {'y': (2e-5, 0.0), 'd_a': (1e-4, 1e-4), 'd_res': (1e-4, 1e-4), 'd_x': (1e-4, 1e-4),
            'd_gamma': (2e-3, 1e-4), 'd_beta': (2e-3, 1e-4)}
BF16_CEILING = (2e-2, 2e-2)              # d(a) of a bf16 `a`, as test_add_dropout_layer_norm_fused grants it


def hipops():
    return importlib.import_module('vln-ver_amd.hipops')


def f32(v):
    return float(np.float32(v))


def keep_mask(shape, seed, p_drop, index=None):
    """bool tensor of ``shape``: the host rule on the flat element index (or on ``index``, an integer array of that shape)."""
    n = int(np.prod(shape))
    if p_drop <= 0.0:
        return torch.ones(shape, dtype=torch.bool)
    idx = np.arange(n, dtype=np.uint64) if index is None else np.asarray(index)
    return torch.from_numpy(hipops().dropout_keep_host(idx, seed, p_drop).reshape(shape))


def scale_of(p_drop, dtype):
    """1 / (1 - p) of the fp32 p the kernels receive: in fp64 for the exact chain, as the kernels' fp32 quotient else."""
    if p_drop <= 0.0:
        return 1.0
    if dtype == torch.float64:
        return 1.0 / (1.0 - f32(p_drop))
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p_drop)))


def tree(v):
    """group_sum over the last axis (64 or 16 lanes): the balanced tree over neighbouring lanes, in v's dtype."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def to_out(t, dtype):
    """a model's fp32 result in the kernel's output type: bf16 is one rounding to nearest even."""
    return t.bfloat16() if dtype == torch.bfloat16 else t


def _in_turn(parts):
    """sum of the leading axis one slice after the other (a grid-stride loop, the workgroups' atomics)."""
    acc = torch.zeros_like(parts[0])
    for t in range(parts.shape[0]):
        acc = acc + parts[t]
    return acc


def _slot_sums(terms, slots):
    """[slots, C]: per row slot of the grid, the rows it visits in the grid-stride loop added in turn."""
    n, c = terms.shape
    trips = (n + slots - 1) // slots
    pad = torch.zeros(trips * slots, c, dtype=terms.dtype)
    pad[:n] = terms
    return _in_turn(pad.view(trips, slots, c))


# ------------------------------------------------------------------------------------------------------------ add_ln
def add_ln_inputs(n, c, adtype, seed=31, edge=False, a_scale=1.0):
    """a [n,c] (adtype), residual, gamma, beta, grad_y fp32 and grad_y_bf16, the distribution of
    test_add_dropout_layer_norm_fused (``a_scale``: a = a_scale randn; add_ln_reference takes 1 - p for p > 0.5, so that the
    kept elements, times 1 / (1 - p), stay O(1) and |y| stays in the range the forward ceiling was granted for).  ``edge`` (n >= 8) writes the edge rows: 1 a = 0 and residual = 4 (a constant power of
    two), 2 and n-1 mean 100 / std 1, 3 all zero, 4 magnitudes up to 1e15."""
    gen = torch.Generator(device='cpu').manual_seed(seed + 7 * c)
    a = torch.randn(n, c, generator=gen) * a_scale
    res = torch.randn(n, c, generator=gen)
    gamma, beta = torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen) * 0.1
    gy = torch.randn(n, c, generator=gen)
    gy16 = (torch.randn(n, c, generator=gen) * 0.5).bfloat16()
    if edge:
        assert n >= 8
        a[1], res[1] = 0.0, 4.0
        for r in (2, n - 1):
            a[r] *= 0.1
            res[r] = 100.0 + torch.randn(c, generator=gen)
        a[3], res[3] = 0.0, 0.0
        mag = 10.0 ** (torch.rand(c, generator=gen) * 15.0)
        a[4], res[4] = a[4] * mag, res[4] * mag
    return dict(a=a.to(adtype), res=res, gamma=gamma, beta=beta, gy=gy, gy16=gy16, edge=edge)


def add_ln_eval(inp, keep, p_drop, dtype, use_gy16=True, one_pass=False, no_scale_in_da=False):
    """The operation and its backward pass, every step in ``dtype``: fp64 = the exact chain, fp32 = the plain-torch model.
    ``one_pass`` (a planted fault): variance as E[x^2] - mean^2.  ``no_scale_in_da`` (another): d(a) without 1 / (1 - p)."""
    a, res, g, b = (inp[k].to(dtype) for k in ('a', 'res', 'gamma', 'beta'))
    scale = scale_of(p_drop, dtype)
    x = res + torch.where(keep, a * scale, torch.zeros((), dtype=dtype))
    mu = x.mean(1, keepdim=True)
    xc = x - mu
    var = (x * x).mean(1, keepdim=True) - mu * mu if one_pass else (xc * xc).mean(1, keepdim=True)
    rs = torch.rsqrt(var + EPS)
    xh = xc * rs
    out = dict(y=xh * g + b, mean=mu[:, 0], rstd=rs[:, 0])
    go = inp['gy'].to(dtype) + (inp['gy16'].to(dtype) if use_gy16 else 0.0)
    gg = go * g
    dx = (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True)) * rs
    out.update(d_res=dx, d_a=torch.where(keep, dx * (1.0 if no_scale_in_da else scale), torch.zeros((), dtype=dtype)),
               d_gamma=(go * xh).sum(0), d_beta=go.sum(0))
    return out


def add_ln_ordered(inp, keep, p_drop, use_gy16=True):
    """fp32 in the kernels' order (module docstring; k_add_ln_fwd / k_add_ln_bwd)."""
    f = torch.float32
    a, res, g, b = inp['a'].float(), inp['res'], inp['gamma'], inp['beta']
    n, c = res.shape
    K = c // 256
    inv_c = float(np.float32(1.0) / np.float32(c))
    scale = scale_of(p_drop, f)
    lanes = lambda t: t.reshape(n, K, 64, 4)
    x = res + torch.where(keep, a * scale, torch.zeros((), dtype=f))
    xl = lanes(x)
    s = torch.zeros(n, 64)
    for k in range(K):
        s = s + ((xl[:, k, :, 0] + xl[:, k, :, 1]) + (xl[:, k, :, 2] + xl[:, k, :, 3]))
    mu = (tree(s) * inv_c)[:, None]
    xc = x - mu
    xcl = lanes(xc)
    q = torch.zeros(n, 64)
    for k in range(K):
        for i in range(4):
            q = q + xcl[:, k, :, i] * xcl[:, k, :, i]
    rs = torch.rsqrt(tree(q) * inv_c + np.float32(EPS))[:, None]
    out = dict(y=xc * rs * g + b, mean=mu[:, 0], rstd=rs[:, 0])
    go = inp['gy'] + inp['gy16'].float() if use_gy16 else inp['gy']
    xh = (x - mu) * rs
    gg = go * g
    ggl, ggxl = lanes(gg), lanes(gg * xh)
    s1, s2 = torch.zeros(n, 64), torch.zeros(n, 64)
    for k in range(K):
        for i in range(4):
            s1 = s1 + ggl[:, k, :, i]
            s2 = s2 + ggxl[:, k, :, i]
    m1, m2 = (tree(s1) * inv_c)[:, None], (tree(s2) * inv_c)[:, None]
    dx = (gg - m1 - xh * m2) * rs
    out.update(d_res=dx, d_a=torch.where(keep, dx * scale, torch.zeros((), dtype=f)))
    grid = min((n + ADD_LN_ROWS - 1) // ADD_LN_ROWS, ADD_LN_BWD_GRID)
    for name, terms in (('d_gamma', go * xh), ('d_beta', go)):
        w = _slot_sums(terms, grid * ADD_LN_ROWS).view(grid, ADD_LN_ROWS, c)
        out[name] = _in_turn((w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3]))
    return out


def _finish_add_ln(r, adtype):
    r['d_a'] = to_out(r['d_a'], adtype)
    return r


@functools.lru_cache(maxsize=None)
def add_ln_reference(n, c, adtype, p_drop, seed, use_gy16=True, edge=False):
    """Inputs, keep mask, exact chain, both fp32 models, d_ref and the bounds of one case; computed once, shared, not to be
    modified."""
    inp = add_ln_inputs(n, c, adtype, edge=edge, a_scale=1.0 - p_drop if p_drop > 0.5 else 1.0)
    keep = keep_mask((n, c), seed, p_drop)
    exact = add_ln_eval(inp, keep, p_drop, torch.float64, use_gy16)
    models = [_finish_add_ln(add_ln_eval(inp, keep, p_drop, torch.float32, use_gy16), adtype),
              _finish_add_ln(add_ln_ordered(inp, keep, p_drop, use_gy16), adtype)]
    ceil = dict(CEILINGS)
    if adtype == torch.bfloat16:
        ceil['d_a'] = BF16_CEILING
    d_ref, bound = bounds(models, exact, ceil, edge)
    return dict(inp=inp, keep=keep, exact=exact, models=models, d_ref=d_ref, bound=bound, p_drop=p_drop, seed=seed)


# ------------------------------------------------------------------------------------------------------ relu_dropout
def relu_dropout_inputs(n, dtype, seed=33, special=True):
    """x and grad_y [n] in ``dtype`` (no element of grad_y is 0).  ``special`` (n >= 1020) writes, from element 100 on: +0, -0,
    the smallest positive normal, a positive and a negative denormal, +inf, the largest finite value; and the same again in
    the last 16 elements."""
    gen = torch.Generator(device='cpu').manual_seed(seed)
    x = torch.randn(n, generator=gen).to(dtype)
    gy = torch.randn(n, generator=gen).to(dtype)
    gy = torch.where(gy == 0, torch.ones((), dtype=dtype), gy)
    if special and n >= 1020:
        fi = torch.finfo(dtype)
        denorm = fi.tiny / 4.0                               # (representable in both types: 2 bits below the normal range)
        vals = torch.tensor([0.0, -0.0, fi.tiny, denorm, -denorm, float('inf'), fi.max], dtype=torch.float64).to(dtype)
        for at in (100, n - 16):
            x[at:at + len(vals)] = vals
    return dict(x=x, gy=gy)


def relu_dropout_eval(inp, keep, p_drop, dtype, divide=False):
    """y = keep and x > 0 ? x * scale : 0, d(x) = y != 0 ? d(y) * scale : 0, every step in ``dtype`` (fp64: the exact chain, with
    a product beyond the output type's range mapped to inf).  ``divide``: the plain model, x / (1 - p) instead of x * scale.
    Works on any device.  Also returns ``denormal``: where x is a denormal (module docstring)."""
    x, gy = inp['x'], inp['gy']
    out_t = x.dtype
    fi = torch.finfo(out_t)
    xs, gs = x.to(dtype), gy.to(dtype)
    zero = torch.zeros((), dtype=dtype, device=x.device)
    if divide and p_drop > 0.0:
        q = float(np.float32(1.0) - np.float32(p_drop))
        ys, gsc = xs / q, gs / q
    else:
        scale = scale_of(p_drop, dtype)
        ys, gsc = xs * scale, gs * scale
    gate = keep.to(x.device) & (xs > 0)
    y = torch.where(gate, ys, zero)
    dx = torch.where(gate, gsc, zero)
    if dtype == torch.float64:
        limit = float(fi.max) * (1.0 + fi.eps / 4.0)
        y = torch.where(y.abs() > limit, torch.sign(y) * float('inf'), y)
    denormal = (xs != 0) & (xs.abs() < float(fi.tiny))
    if dtype == torch.float64:
        return dict(y=y, d_x=dx, denormal=denormal)
    return dict(y=to_out(y, out_t), d_x=to_out(dx, out_t), denormal=denormal, y32=y, d_x32=dx)   # (*32: before the rounding)


def relu_dropout_reference(n, dtype, p_drop, seed, device='cpu'):
    """As add_ln_reference (not cached: the large case is large).  The models run on ``device``; the mask is the host rule."""
    inp = {k: v.to(device) for k, v in relu_dropout_inputs(n, dtype).items()}
    keep = keep_mask((n,), seed, p_drop).to(device)
    exact = relu_dropout_eval(inp, keep, p_drop, torch.float64)
    models = [relu_dropout_eval(inp, keep, p_drop, torch.float32, divide=True),
              relu_dropout_eval(inp, keep, p_drop, torch.float32)]
    skip = exact.pop('denormal')
    for m in models:
        m.pop('denormal')
    d_ref, bound = bounds(models, exact, {}, True, skip={'y': skip, 'd_x': skip}, relmax=('y', 'd_x'))
    return dict(inp=inp, keep=keep, exact=exact, models=models, d_ref=d_ref, bound=bound, denormal=skip, p_drop=p_drop,
                seed=seed, skip={'y': skip, 'd_x': skip}, relmax=('y', 'd_x'))


def one_rounding(got, model32):
    """bool per element: a bf16 ``got`` is the round-to-nearest-even of the fp32 model value or of an fp32 value within 4 ulps
    of it (0 and non-finite values: equal)."""
    m = model32.double()
    lo, hi = (m * (1.0 - 2.0 ** -21)).float().bfloat16().double(), (m * (1.0 + 2.0 ** -21)).float().bfloat16().double()
    g = got.double()
    inside = (g >= torch.minimum(lo, hi)) & (g <= torch.maximum(lo, hi))
    return torch.where(torch.isfinite(m) & (m != 0), inside, g == m.float().bfloat16().double())


# ----------------------------------------------------------------------------------------------------------- ln_relu
def ln_relu_params(seed=8):
    """gamma = rand + 0.5 (away from 0: a feature with gamma near 0 rejects every row), beta = 0.2 randn pushed to |beta| >= 0.01
    (the gates of a constant row are the signs of beta)."""
    gen = torch.Generator(device='cpu').manual_seed(seed)
    gamma = torch.rand(128, generator=gen) + 0.5
    beta = torch.randn(128, generator=gen) * 0.2
    beta = torch.where(beta.abs() < 0.01, torch.where(beta < 0, -0.01, 0.01), beta)
    return gamma, beta


def ln_relu_eval(x, gamma, beta, gy, dtype, gate_from_xhat=False):
    """As add_ln_eval.  ``gate_from_xhat`` (a planted fault): the backward gate from the normalised value."""
    xs, g, b = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    mu = xs.mean(1, keepdim=True)
    xc = xs - mu
    rs = torch.rsqrt((xc * xc).mean(1, keepdim=True) + EPS)
    xh = xc * rs
    pre = xh * g + b
    out = dict(y=torch.relu(pre), mean=mu[:, 0], rstd=rs[:, 0], pre=pre)
    if gy is not None:
        dz = torch.where((xh if gate_from_xhat else pre) > 0, gy.to(dtype), torch.zeros((), dtype=dtype))
        gg = dz * g
        out.update(d_x=(gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True)) * rs,
                   d_gamma=(dz * xh).sum(0), d_beta=dz.sum(0))
    return out


def ln_relu_ordered(x, gamma, beta, gy):
    """fp32 in the kernels' order (k_ln_relu_fwd / k_ln_relu_bwd)."""
    xs = x.float()
    n = xs.shape[0]
    inv_w = float(np.float32(1.0) / np.float32(128))
    lanes = lambda t: t.reshape(n, 16, 8)

    def lane_sum(t):
        tl, s = lanes(t), torch.zeros(n, 16)
        for j in range(8):
            s = s + tl[:, :, j]
        return tree(s)

    mu = (lane_sum(xs) * inv_w)[:, None]
    xc = xs - mu
    rs = torch.rsqrt(lane_sum(xc * xc) * inv_w + np.float32(EPS))[:, None]
    xh = xc * rs
    pre = xh * gamma + beta
    out = dict(y=torch.relu(pre), mean=mu[:, 0], rstd=rs[:, 0], pre=pre)
    dz = torch.where(pre > 0, gy.float(), torch.zeros(()))
    gg = dz * gamma
    m1, m2 = (lane_sum(gg) * inv_w)[:, None], (lane_sum(gg * xh) * inv_w)[:, None]
    out['d_x'] = rs * (gg - m1 - xh * m2)
    grid = min(max((n + LN_RELU_ROWS - 1) // LN_RELU_ROWS, 1), LN_RELU_GRID)
    for name, terms in (('d_gamma', dz * xh), ('d_beta', dz)):
        w = _slot_sums(terms, grid * LN_RELU_ROWS).view(grid, LN_RELU_ROWS, 128)
        out[name] = _in_turn(_in_turn(w.transpose(0, 1).contiguous()))
    return out


def _stable(x, gamma, beta):
    with torch.no_grad():
        pre = ln_relu_eval(x, gamma, beta, None, torch.float64)['pre']
    return x[(pre.abs() > MARGIN).all(1)]


def ln_relu_rows(n, dtype, gamma, beta, seed=8):
    """n gate-stable rows of x = 2 randn + 0.3 in ``dtype`` from 2 n candidates.  From 15 rows on, rows 3
    and n-1 have mean 100 and std 1 (selected the same way) and row 7 is the constant 4."""
    gen = torch.Generator(device='cpu').manual_seed(seed + n)
    cand = (torch.randn(2 * n, 128, generator=gen) * 2 + 0.3).to(dtype)
    rows = _stable(cand, gamma, beta)
    assert rows.shape[0] >= n, '%d gate-stable rows in %d candidates' % (rows.shape[0], cand.shape[0])
    rows = rows[:n].clone()
    if n >= 15:
        far = _stable((100.0 + torch.randn(4, 128, generator=gen)).to(dtype), gamma, beta)
        assert far.shape[0] >= 2, 'mean-100 rows: %d of 4 gate-stable' % far.shape[0]
        rows[3], rows[n - 1] = far[0], far[1]
        rows[7] = 4.0
    return rows


def _finish_ln_relu(r, dtype):
    for k in ('y', 'd_x'):
        r[k] = to_out(r[k], dtype)
    return r


@functools.lru_cache(maxsize=None)
def ln_relu_reference(n, dtype):
    gamma, beta = ln_relu_params()
    x = ln_relu_rows(n, dtype, gamma, beta)
    gen = torch.Generator(device='cpu').manual_seed(4000 + n)
    gy = torch.randn(n, 128, generator=gen).to(dtype)
    exact = ln_relu_eval(x, gamma, beta, gy, torch.float64)
    models = [ln_relu_eval(x, gamma, beta, gy, torch.float32), ln_relu_ordered(x, gamma, beta, gy)]
    pre = exact.pop('pre')
    assert float(pre.abs().min()) > MARGIN
    for m in models:
        mp = m.pop('pre').double()
        move = float((mp - pre).abs().max())
        assert MARGIN >= 4.0 * move, 'a pre-ReLU value moves by %.3e between a model and the exact chain' % move
        assert bool(((mp > 0) == (pre > 0)).all()), 'a model has other gates than the exact chain'
        _finish_ln_relu(m, dtype)
    ceil = dict(CEILINGS) if dtype == torch.float32 else {}
    d_ref, bound = bounds(models, exact, ceil, n >= 15)
    return dict(x=x, gy=gy, gamma=gamma, beta=beta, exact=exact, models=models, d_ref=d_ref, bound=bound, gates=pre > 0)


# -------------------------------------------------------------------------------------------------- the comparator
def _rel(diff, ref, dim):
    """worst relative L2 of the slices along ``dim``, each denominator floored at the RMS slice norm."""
    num, den = diff.norm(dim=1 - dim), ref.norm(dim=1 - dim)
    floor = den.pow(2).mean().sqrt()
    return float((num / torch.maximum(den, floor).clamp(min=1e-300)).max())


def _stats(g, r, skip=None, relmax=False):
    g, r = g.detach().double(), r.detach().double().to(g.device)
    assert g.shape == r.shape, (g.shape, r.shape)
    if skip is not None:
        keep = ~skip.to(g.device)
        g, r = torch.where(keep, g, 0.0), torch.where(keep, r, 0.0)
    fin = torch.isfinite(r)
    names = ['all', 'maxabs'] + (['col', 'row'] if r.dim() == 2 else []) + (['relmax'] if relmax else [])
    if not bool(fin.all()):                                # a non-finite reference value is met exactly or not at all
        if not bool((fin | (g == r)).all()):
            return {s: float('inf') for s in names}
        g, r = torch.where(fin, g, 0.0), torch.where(fin, r, 0.0)
    if not bool(torch.isfinite(g).all()):
        return {s: float('inf') for s in names}
    d = g - r
    rn, dn = float(r.norm()), float(d.norm())
    out = {'all': dn / rn if rn > 0 else (0.0 if dn == 0 else float('inf')), 'maxabs': float(d.abs().max())}
    if r.dim() == 2:
        out['col'], out['row'] = _rel(d, r, 1), _rel(d, r, 0)
    if relmax:
        nz = r != 0
        miss = torch.where(d != 0, float('inf'), 0.0)                  # (a value where the reference has an exact 0)
        out['relmax'] = float(torch.where(nz, d.abs() / r.abs().clamp(min=1e-300), miss).max())
    return out


def distances(got, ref, skip=None, relmax=('rstd',)):
    """{quantity: {statistic: distance}} of ``got`` from ``ref`` for every quantity both hold (module docstring)."""
    skip = skip or {}
    return {k: _stats(got[k], ref[k], skip.get(k), k in relmax) for k in ref if k in got and got[k] is not None}


def measure(r, got):
    """the distances of ``got`` from the exact chain of the reference ``r``, as its bounds were formed."""
    return distances(got, r['exact'], r.get('skip'), r.get('relmax', ('rstd',)))


def ulp32(m):
    return 2.0 ** (math.floor(math.log2(m)) - 23) if m >= 2.0 ** -126 else 2.0 ** -149


def bounds(models, exact, ceilings, edge, skip=None, relmax=('rstd',)):
    """(d_ref, bound): {(quantity, statistic): value} (module docstring).  Only the references enter."""
    ds = [distances(m, exact, skip, relmax) for m in models]
    d_ref, bound = {}, {}
    for k, stats in ds[0].items():
        r = exact[k].detach().double()
        if skip and k in skip:
            r = torch.where(skip[k].to(r.device), 0.0, r)
        top = float(torch.where(torch.isfinite(r), r.abs(), 0.0).max())
        for s in stats:
            v = max(d[k][s] for d in ds)
            floor = ULPS * ulp32(top) if s == 'maxabs' else ULPS * 2.0 ** -23
            d_ref[(k, s)], bound[(k, s)] = v, FACTOR * v + floor
        if k in ceilings:
            ca, cr = ceilings[k]
            rms = max(float(r.pow(2).mean().sqrt()), 1e-300)
            for s in (['all'] if edge else ['all', 'maxabs']):
                limit = (ca + cr * top) / (rms if s == 'all' else 1.0)
                assert bound[(k, s)] <= limit, 'bound %.3e of %s/%s exceeds the ceiling %.3e: the inputs are wrong' % (
                    bound[(k, s)], k, s, limit)
    return d_ref, bound


def violations(d_got, bound):
    """[(quantity, statistic, distance, bound)] of every bound exceeded (a NaN distance exceeds its bound)."""
    return [(k, s, d_got[k][s], b) for (k, s), b in bound.items() if k in d_got and not d_got[k][s] <= b]


def table(title, d_ref, d_got, bound):
    """the three columns docs/HISTORY.md records: d_ref, the measured distance, the bound."""
    lines = ['%s' % title, '  %-8s %-9s %10s %10s %10s' % ('quantity', 'statistic', 'd_ref', 'measured', 'bound')]
    for (k, s), b in bound.items():
        got = ('%10.3e' % d_got[k][s]) if d_got is not None and k in d_got else '%10s' % '-'
        lines.append('  %-8s %-9s %10.3e %s %10.3e' % (k, s, d_ref[(k, s)], got, b))
    return '\n'.join(lines)
