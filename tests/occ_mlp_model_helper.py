"""fp64 references of the fused occupancy MLP (csrc/ver_occ_mlp.hip) on GATE-STABLE rows, and the per-feature comparator
built on them (test_occ_mlp_gates_cpu.py, test_occ_mlp_gates_gpu.py).

On random rows a few ReLU gates flip between any two bf16 evaluations of the chain and every flip replaces its gradient
element, so a whole-tensor bound of 6-9 % is all random rows allow.  Here the flips are taken out of the INPUTS: rows are
kept only where every pre-ReLU value of both layers is a margin away from zero (``stable_rows``), and then two fp64 chains
-- an exact one and a model that rounds to bf16 where a kernel hands values on -- are a fraction of a per cent apart per
feature.  That distance, ``d_ref``, defines the bound a kernel has to meet: ``4 d_ref + 2^-8`` (``bounds``).

Rounding points of the kernels, as ``chain(..., rounded=<kernel>)`` models them (line numbers of csrc/ver_occ_mlp.hip):

``'forward'`` (k_occ_mlp_fwd)
  * h1, h2: ``relu_packed(pack8(y))`` at the end of ln_relu_nat (235) / ln_relu_tile (161); the normalised values stay fp32;
  * the logits: ``pack4`` at the store (440).
``'row_split'`` (k_occ_mlp_bwd, also ``rounded=True``)
  * the normalised values of both layers: ``pack8`` in ln_relu_nat<KEEP> (214) / ln_relu_keep (544), the pre-ReLU value is
    formed from the ROUNDED one (230, 552) and so is the gate of the backward (580);
  * h1, h2: ``pack8`` (235, 554);
  * d(beta) sums ``pack8(dz)``, d(gamma) sums ``pack8(dz * n)`` (592-598, selector MFMAs);
  * d(a2), d(a1) / d(x): ``pack8`` at the end of ln_relu_bwd (611); d(b2) / d(b1) are sums of those packed values (616);
    d(W2) / d(W1) are products of the packed tensors (hipops._rows_tn), each chunk of 8 000 rows leaving its bf16 GEMM
    rounded to bf16;
  * d(x) of the unfolded chain: ``pack8`` at the store (771).
``'wave_spec'`` (k_occ_mlp_bwd_ws), everything the row-split kernel rounds (214, 235 or ln_fwd4 1206-1211; 1023 / 1274) and
what crosses between its two views through LDS tiles:
  * a2: ``pack4`` at the end of rows_product (1524);
  * d(h2): ``pack4`` (1539); d(h1): ``pack4`` (1524 again, into T4);
  * d(z) is therefore bf16 already where d(beta) / d(gamma) are summed (1013 / 1241; the d(gamma) product with the bf16 n is
    exact in the MFMA, 1561 / 1578);
  * d(logits) times a device scalar: ``pack8`` (1285 / 1389).
The LayerNorm backward of both backward kernels subtracts the gradient mean in every mode (606-610, 1018-1022, 1265-1274),
and uses the rounded normalised values.
This is a model of WHERE rounding happens, not of bits: fp32 accumulation order and the hardware reciprocal square root are
left out on purpose; the factor 4 of the bound and the margin of the row selection cover them.

Modes: ``unfolded`` (flags bit 0: the chain starts with Linear 1), ``folded`` (x is the first Linear's output) and
``folded_centered`` (VER_OCC_MLP_CENTERED: the hidden Linears are centred over their output axis, x = bf16(x0 W1c^T + b1c),
and BOTH LayerNorms are evaluated WITHOUT the mean pass in both references -- the arithmetic the flag states).  In the
centred mode the gradients are those of the UNcentred W2 / b2 (autograd maps them back through the projection, as
test_occ_mlp_centered_equals_plain_and_the_fp64_chain does), and d(x) is compared with its row mean removed: the producer's
centred Linear annihilates the all-ones direction of d(x), and off the centred rows the two functions "LayerNorm" and
"LayerNorm without the mean pass" have different gradients along exactly that direction.
"""
import functools

import torch

EPS = 1e-5
MODES = ('unfolded', 'folded', 'folded_centered')
KERNELS = ('forward', 'row_split', 'wave_spec')
POOL = 2048                      # gate-stable rows kept per (mode, seed, scale)
CHUNK = 20000                    # candidates per selection chunk
MAX_CANDIDATES = 400000
MAX_BOUND = 5e-2                 # no bound may exceed this: a larger one means the inputs are wrong
PER_FEATURE_ROWS = 2048          # per-column / per-row-of-matrix statistics from this many data rows on
ROWS_TN_CHUNK = 8000             # hipops._rows_tn
KEYS = ('w1', 'b1', 'g1', 'be1', 'w2', 'b2', 'g2', 'be2', 'w3', 'b3')
FOLDED_KEYS = KEYS[2:]


def bf16(t):
    return t.bfloat16().double()


class _Ste(torch.autograd.Function):
    """bf16 rounding of a value hand-off, straight through for the gradient."""

    @staticmethod
    def forward(ctx, t):
        return bf16(t)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGrad(torch.autograd.Function):
    """identity whose gradient is rounded to bf16: a gradient hand-off."""

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return bf16(g)


class _NormKept(torch.autograd.Function):
    """LayerNorm without its affine part as the backward kernels run it: the normalised values are kept as bf16 and the
    backward uses those, and subtracts the gradient mean whether or not the forward skipped the mean pass."""

    @staticmethod
    def forward(ctx, a, centered):
        v = a if centered else a - a.mean(1, keepdim=True)
        rs = torch.rsqrt(v.pow(2).mean(1, keepdim=True) + EPS)
        raw = v * rs
        n = bf16(raw)
        ctx.save_for_backward(n, rs)
        ctx.mark_non_differentiable(raw, rs)
        return n, raw, rs

    @staticmethod
    def backward(ctx, g, _raw, _rs):
        n, rs = ctx.saved_tensors
        return (g - g.mean(1, keepdim=True) - n * (g * n).mean(1, keepdim=True)) * rs, None


class _AffineSums(torch.autograd.Function):
    """y = n gamma + beta with the parameter sums formed from packed bf16 values (``pack_product``: the row-split kernel
    packs dz * n; the wave-specialised one multiplies the packed dz with the packed n)."""

    @staticmethod
    def forward(ctx, n, gamma, beta, pack_product):
        ctx.save_for_backward(n, gamma)
        ctx.pack_product = pack_product
        return n * gamma + beta

    @staticmethod
    def backward(ctx, dz):
        n, gamma = ctx.saved_tensors
        dgam = bf16(dz * n) if ctx.pack_product else bf16(dz) * n
        return dz * gamma, dgam.sum(0), bf16(dz).sum(0), None


class _LinearRowsTN(torch.autograd.Function):
    """Linear whose weight gradient is hipops._rows_tn: bf16 GEMMs over chunks of 8 000 rows, each result rounded to bf16."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return x @ w.t() + b

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        n = x.shape[0]
        main = n // ROWS_TN_CHUNK * ROWS_TN_CHUNK
        dw = torch.zeros_like(w)
        for lo in range(0, main, ROWS_TN_CHUNK):
            dw += bf16(g[lo:lo + ROWS_TN_CHUNK].t() @ x[lo:lo + ROWS_TN_CHUNK])
        if main < n:
            dw += bf16(g[main:].t() @ x[main:])
        return g @ w, dw, g.sum(0)


def params(seed=12):
    """The distribution of test_hip_ops_gpu._occ_mlp_params, with about a quarter of the LayerNorm gammas negated so that
    both gate signs occur.  fp32, as the kernels' callers hold them."""
    gen = torch.Generator(device='cpu').manual_seed(seed)
    p = dict(w1=torch.randn(128, 128, generator=gen) * 0.12, b1=torch.randn(128, generator=gen) * 0.3,
             g1=torch.randn(128, generator=gen) * 0.3 + 1.0, be1=torch.randn(128, generator=gen) * 0.3,
             w2=torch.randn(128, 128, generator=gen) * 0.12, b2=torch.randn(128, generator=gen) * 0.3,
             g2=torch.randn(128, generator=gen) * 0.3 + 1.0, be2=torch.randn(128, generator=gen) * 0.3,
             w3=torch.randn(16, 128, generator=gen) * 0.12, b3=torch.randn(16, generator=gen) * 0.3)
    for k in ('g1', 'g2'):
        p[k] = torch.where(torch.rand(128, generator=gen) < 0.25, -p[k], p[k])
    return p


def center(w, b):
    """the hidden Linear centred over its OUTPUT axis (what the head passes with ``centered=True``)."""
    return w - w.mean(0, keepdim=True), b - b.mean()


def keys_of(mode):
    return KEYS if mode == 'unfolded' else FOLDED_KEYS


def chain(x, p, mode, rounded=False, gy=None, gscale=None):
    """The chain in fp64.  ``x`` [n,128] (bf16 values), ``p`` the fp32 parameters; weights are used as
    ``bfloat16().double()``, vectors as ``.double()``.  ``rounded``: False = exact; a name of KERNELS (True = 'row_split') =
    that kernel's rounding points (module docstring).  With ``gy`` [n,16] (bf16 values; times the fp32 scalar ``gscale``) the
    backward pass runs as well (autograd).  Returns a dict: ``logits``, ``rstd`` [n,2], ``pre`` = the two pre-ReLU tensors,
    ``xhat`` = the two normalised tensors before their own rounding, and with ``gy``: ``x`` = d(x) and the gradient of
    every parameter of ``keys_of(mode)``."""
    assert mode in MODES
    kern = 'row_split' if rounded is True else (rounded or None)
    assert kern is None or kern in KERNELS
    bwd = kern in ('row_split', 'wave_spec')
    ws = kern == 'wave_spec'
    centered = mode == 'folded_centered'
    keys = keys_of(mode)
    want_grad = gy is not None
    leaf = {k: p[k].double().requires_grad_(want_grad) for k in keys}
    xl = x.double().requires_grad_(want_grad)
    w2, b2 = center(leaf['w2'], leaf['b2']) if centered else (leaf['w2'], leaf['b2'])
    w2, w3 = _Ste.apply(w2), _Ste.apply(leaf['w3'])                 # (bf16 operands: exact chain and model alike)
    linear = _LinearRowsTN.apply if kern == 'row_split' else (lambda t, w, b: t @ w.t() + b)
    hand_g = _RoundGrad.apply if bwd else (lambda t: t)             # a gradient hand-off both backward kernels have
    hand_g_ws = _RoundGrad.apply if ws else (lambda t: t)           # ... and one only the wave-specialised kernel has

    def norm_relu(a, gamma, beta):
        if bwd:
            n, raw, rs = _NormKept.apply(a, centered)
            pre = _AffineSums.apply(n, gamma, beta, not ws)
        else:
            v = a if centered else a - a.mean(1, keepdim=True)
            rs = torch.rsqrt(v.pow(2).mean(1, keepdim=True) + EPS)
            raw = v * rs
            pre = raw * gamma + beta
        h = torch.relu(pre)
        return (_Ste.apply(h) if kern else h), pre.detach(), raw.detach(), rs.detach()

    a1 = hand_g(xl)
    if mode == 'unfolded':
        a1 = hand_g(linear(a1, _Ste.apply(leaf['w1']), leaf['b1']))
    h1, pre1, raw1, rs1 = norm_relu(a1, leaf['g1'], leaf['be1'])
    a2 = hand_g(linear(hand_g_ws(h1), w2, b2))
    if ws:
        a2 = _Ste.apply(a2)
    h2, pre2, raw2, rs2 = norm_relu(a2, leaf['g2'], leaf['be2'])
    logits = hand_g_ws(h2) @ w3.t() + leaf['b3']
    out = dict(logits=bf16(logits.detach()) if kern == 'forward' else logits.detach(), rstd=torch.cat([rs1, rs2], 1),
               pre=(pre1, pre2), xhat=(raw1, raw2))
    if want_grad:
        g = gy.double()
        if gscale is not None:
            g = g * float(gscale)
            if kern:
                g = bf16(g)
        logits.backward(g)
        out['x'] = xl.grad
        for k in keys:
            out[k] = leaf[k].grad
    return finish(out, mode)


def finish(out, mode):
    """what is compared of a result (reference or kernel): in the centred mode d(x) without its row mean (module docstring)."""
    if mode == 'folded_centered' and 'x' in out:
        gx = out['x'].double()
        out['x'] = gx - gx.mean(1, keepdim=True)
    return out


def same_gates(a, b):
    return all(bool(((pa > 0) == (pb > 0)).all()) for pa, pb in zip(a['pre'], b['pre']))


def candidates(p, mode, n, gen, scale=1.0):
    """n candidate rows of x (bf16): 1.5 randn, as the existing tests draw them; in the centred mode the output of the centred
    first Linear on such rows.  ``scale`` moves the rows' 1/std."""
    x0 = torch.randn(n, 128, generator=gen) * 1.5
    if mode == 'folded_centered':
        w1c, b1c = center(p['w1'].double(), p['b1'].double())
        x0 = x0.double() @ w1c.t() + b1c
    return (x0 * scale).bfloat16()


def margin_ok(exact, p, E):
    """|pre_l[f]| > 2 (E_l |gamma_l[f]| + 2^-8 |beta_l[f]|) + 1e-3 for both layers and every feature: E_l |gamma| is what the
    roundings upstream of the layer can move the pre-ReLU value by, 2^-8 |beta| covers the layer's own rounding of the
    normalised value (it moves n gamma = pre - beta by 2^-9 relative)."""
    keep = None
    for l, (g, b) in enumerate((('g1', 'be1'), ('g2', 'be2'))):
        m = 2.0 * (E[l] * p[g].double().abs() + 2.0 ** -8 * p[b].double().abs()) + 1e-3
        ok = (exact['pre'][l].abs() > m).all(1)
        keep = ok if keep is None else keep & ok
    return keep


@functools.lru_cache(maxsize=None)
def _pool(mode, seed, scale):
    p = params(seed)
    gen = torch.Generator(device='cpu').manual_seed(1000 + seed)
    kept, seen, E = [], 0, None
    while sum(k.shape[0] for k in kept) < POOL:
        assert seen + CHUNK <= MAX_CANDIDATES, '%s: %d gate-stable rows in %d candidates' % (
            mode, sum(k.shape[0] for k in kept), seen)
        x = candidates(p, mode, CHUNK, gen, scale)
        seen += CHUNK
        with torch.no_grad():
            exact = chain(x, p, mode)
            if E is None:            # the largest move of a normalised value by the roundings upstream of it, any kernel
                E = [0.0, 0.0]
                for kern in KERNELS:
                    r = chain(x, p, mode, kern)
                    for l in range(2):
                        E[l] = max(E[l], float((r['xhat'][l] - exact['xhat'][l]).abs().max()))
                if mode != 'unfolded':
                    assert E[0] == 0.0
        kept.append(x[margin_ok(exact, p, E)])
    rows = torch.cat(kept)[:POOL]
    with torch.no_grad():
        exact = chain(rows, p, mode)
        for kern in KERNELS:         # the condition the selection exists for
            assert same_gates(chain(rows, p, mode, kern), exact), (mode, kern)
    return rows, tuple(E), seen


def stable_rows(mode, count, seed=12, scale=1.0):
    """``count`` gate-stable rows of x (bf16 [count,128]) for the parameters ``params(seed)``: the first rows of a pool of POOL
    selected rows (cached per mode, seed and scale); more rows than the pool holds are the pool indexed at random."""
    rows, _, _ = _pool(mode, seed, float(scale))
    if count <= rows.shape[0]:
        return rows[:count]
    gen = torch.Generator(device='cpu').manual_seed(2000 + seed + count)
    return rows[torch.randint(0, rows.shape[0], (count,), generator=gen)]


def pool_stats(mode, seed=12, scale=1.0):
    """(E_1, E_2), candidates drawn."""
    _, E, seen = _pool(mode, seed, float(scale))
    return E, seen


def grad_logits(n, seed=12):
    """d(logits), drawn per row: no two rows have the same gradient even where their x repeats."""
    gen = torch.Generator(device='cpu').manual_seed(3000 + seed + n)
    return (torch.randn(n, 16, generator=gen) * 0.1).bfloat16()


# ---------------------------------------------------------------------------------------------------- the comparator
def _rel(diff, ref, dim):
    """worst relative L2 of the slices along ``dim`` (norms over the other axis), each denominator floored at the RMS norm."""
    other = 1 - dim
    num = diff.norm(dim=other)
    den = ref.norm(dim=other)
    floor = den.pow(2).mean().sqrt()
    return float((num / torch.maximum(den, floor).clamp(min=1e-300)).max())


def distances(got, ref):
    """{name: {statistic: distance}} of ``got`` from ``ref`` for the logits, d(x), every parameter gradient and rstd -- those
    both hold.  Statistics: ``all`` the whole-tensor relative L2; for 2-D quantities ``col`` the worst relative L2 of a
    feature column and, for a parameter matrix, ``row`` that of a row; for d(x) and the logits ``data_row`` the worst of a
    data row.  Each column / row norm in a denominator is floored at the tensor's RMS column / row norm.
    rstd has one more, ``bias``: the worst column's |mean over the rows of the relative deviation|.  The rounding of h1 moves
    1/std of the second LayerNorm by 4e-4 relative L2, at random per row, so the L2 bound of that column is 1.6e-3 and a
    1/std that is off by 1e-3 in EVERY row passes it; the mean deviation of the model is 1e-5 and does not."""
    out = {}
    for k in ('logits', 'x') + KEYS + ('rstd',):
        if k not in got or k not in ref or got[k] is None:
            continue
        g, r = got[k].detach().double().cpu(), ref[k].detach().double().cpu()
        assert g.shape == r.shape, (k, g.shape, r.shape)
        d = {'all': float((g - r).norm() / r.norm().clamp(min=1e-300))}
        if r.dim() == 2:
            d['col'] = _rel(g - r, r, 1)
            if k == 'rstd':
                d['bias'] = float(((g - r) / r).mean(0).abs().max())
            else:
                d['data_row' if k in ('logits', 'x') else 'row'] = _rel(g - r, r, 0)
        out[k] = d
    return out


def bounds(d_ref, n):
    """bound = 4 d_ref + floor per statistic in use at ``n`` data rows.  The factor 4 covers what the model omits (fp32
    summation order, the hardware reciprocal square root, the one or two extra bf16 roundings in the parameter sums); the
    floor, 2^-8, is one bf16 rounding, for the quantities where the model distance is exactly zero (d(beta2), d(b3)).  From
    PER_FEATURE_ROWS rows on every statistic counts; below, the per-data-row one for d(x) and the logits and whole tensors
    for the parameter gradients, with a floor of 2^-7.  rstd (fp32) has a floor of 1e-5.  No bound may exceed MAX_BOUND."""
    out = {}
    for k, stats in d_ref.items():
        for s, v in stats.items():
            if k == 'rstd':
                floor = 1e-5
            elif n >= PER_FEATURE_ROWS:
                floor = 2.0 ** -8
            elif k in ('logits', 'x'):
                if s != 'data_row':
                    continue
                floor = 2.0 ** -8
            else:
                if s != 'all':
                    continue
                floor = 2.0 ** -7
            b = 4.0 * v + floor
            assert b <= MAX_BOUND, 'bound %.3e of %s/%s exceeds %.0e: the inputs are wrong' % (b, k, s, MAX_BOUND)
            out[(k, s)] = b
    return out


def violations(d_got, bound):
    """[(name, statistic, distance, bound)] of every bound exceeded (a NaN distance exceeds its bound)."""
    bad = []
    for (k, s), b in bound.items():
        if k in d_got and not d_got[k][s] <= b:
            bad.append((k, s, d_got[k][s], b))
    return bad


def table(title, d_ref, d_got, bound):
    """the three columns docs/HISTORY.md records: d_ref, the measured distance, the bound."""
    lines = ['%s' % title, '  %-8s %-9s %10s %10s %10s' % ('quantity', 'statistic', 'd_ref', 'measured', 'bound')]
    for (k, s), b in bound.items():
        got = ('%10.3e' % d_got[k][s]) if d_got is not None and k in d_got else '%10s' % '-'
        lines.append('  %-8s %-9s %10.3e %s %10.3e' % (k, s, d_ref[k][s], got, b))
    return '\n'.join(lines)


@functools.lru_cache(maxsize=None)
def reference(mode, n, kernel, seed=12, scale=1.0, gscale=None):
    """The inputs and both references of one case, computed once and shared (do not modify): dict(x, gy, p, exact, model,
    d_ref, bound).  ``kernel`` = 'forward': logits and rstd; a backward kernel: d(x) and the parameter gradients."""
    p = params(seed)
    x = stable_rows(mode, n, seed, scale)
    gy = None if kernel == 'forward' else grad_logits(n, seed)
    exact = chain(x, p, mode, False, gy, gscale)
    model = chain(x, p, mode, kernel, gy, gscale)
    assert same_gates(model, exact)
    if n > PER_FEATURE_ROWS:                 # (the large cases stay cached for the whole session: keep what is compared)
        for r in (exact, model):
            del r['pre'], r['xhat']
    if kernel != 'forward':                  # (the logits and rstd are the forward kernel's)
        for r in (exact, model):
            del r['logits'], r['rstd']
    d_ref = distances(model, exact)
    return dict(x=x, gy=gy, p=p, exact=exact, model=model, d_ref=d_ref, bound=bounds(d_ref, n))
