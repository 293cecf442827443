"""The four general-shape sampling kernels of csrc/ver_msda.hip -- ``k_msda_fwd`` / ``k_msda_bwd`` (the mmcv drop-in) and
``k_msda3d_fwd`` / ``k_msda3d_bwd`` (the detection decoder's default path) -- against the fp64 model of
tests/msda_forms_helper.py: every lane form of ``dispatch_group`` both ways, exact cell edges and padding borders, atomics
colliding on one key, non-finite and far-away locations in the backward pass, the buffer contract of the C ABI and the
wrappers' dtype / stride handling.  Bounds: forward ``maxdiff < 2e-5``, gradients ``util.close``, as everywhere for these ops;
test_msda_forms_cpu.py holds the fp32 CPU oracle under a quarter of each on the same inputs.  Every comparison prints the
worst ratio to each bound (``RATIO ...``; run with ``-s``)."""
import pytest
import torch

import msda_forms_helper as H
from util import close, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
VER_OK, VER_EINVAL, VER_EUNSUPPORTED = 0, -1, -2


def _apply(dim, value, shapes, lsi, loc, attn):
    hip = pkg('hipops')
    if dim == 2:
        return hip.MultiScaleDeformableAttnFunction_fp32.apply(value, shapes, lsi, loc, attn, 64)
    return hip.voxel_msda(value, shapes, lsi, loc, attn)


def _run(c, loc=None, attn=None, grad_out=None):
    """forward + backward through the autograd wrapper; the four results on the CPU."""
    v = c['value'].to(DEV).requires_grad_(True)
    l = (c['loc'] if loc is None else loc).to(DEV).requires_grad_(True)
    a = (c['attn'] if attn is None else attn).to(DEV).requires_grad_(True)
    out = _apply(c['dim'], v, c['shapes'].to(DEV), c['level_start'].to(DEV), l, a)
    out.backward((c['grad_out'] if grad_out is None else grad_out).to(DEV))
    torch.cuda.synchronize()
    return dict(out=out.detach().cpu(), grad_value=v.grad.cpu(), grad_loc=l.grad.cpu(), grad_attn=a.grad.cpu())


def _check(title, got, want):
    r = H.ratios(got, want)
    print('RATIO %s %s' % (title, ' '.join('%s=%.4f' % kv for kv in r.items())))
    for k in H.QUANTITIES:
        assert got[k].dtype == torch.float32 and bool(torch.isfinite(got[k]).all()), k
        assert r[k] < 1.0, (title, k, r[k])
    assert close(got['grad_value'], want['grad_value']) and close(got['grad_loc'], want['grad_loc'])
    assert close(got['grad_attn'], want['grad_attn'])


def _nontrivial(got, want):
    """an all-zero result cannot pass on the absolute tolerance: each norm is within 1 % of the model's, which is not small"""
    for k in H.QUANTITIES:
        n, m = float(got[k].double().norm()), float(want[k].norm())
        assert m > 0.1 and abs(n - m) <= 0.01 * m, (k, n, m)


# ------------------------------------------------------------------------------------- 1: every form, both ops, both passes
@pytest.mark.parametrize('hd', H.WIDTHS)
@pytest.mark.parametrize('dim', [2, 3])
def test_every_lane_form_forward_and_backward(dim, hd):
    c = H.random_case(dim, hd)
    got = _run(c)
    _check('random dim=%d hd=%d form=G%d,NC%d' % ((dim, hd) + H.form(hd)), got, c['model'])
    _nontrivial(got, c['model'])


# ------------------------------------------------------------------------------------------------------------ 2: cell edges
@pytest.mark.parametrize('hd', H.EDGE_WIDTHS)
@pytest.mark.parametrize('dim', [2, 3])
def test_cell_edges_borders_and_gate_values(dim, hd):
    c = H.edge_case(dim, hd)
    got = _run(c)
    _check('edge dim=%d hd=%d' % (dim, hd), got, c['model'])
    _nontrivial(got, c['model'])
    outside = ~c['gate']
    assert int(outside.sum()) > 0
    assert float(got['grad_loc'][outside].abs().max()) == 0.0 and float(got['grad_attn'][outside].abs().max()) == 0.0
    # a corner of weight 0 with a non-zero gradient: integer coordinates strictly inside the map
    inner = H.interior_integer(c)
    assert int(inner.sum()) > 0 and float(got['grad_loc'][inner].abs().max()) > 1e-3
    assert close(got['grad_loc'][inner], c['model']['grad_loc'][inner])


# ------------------------------------------------------------------------------------------------------------ 3: collisions
@pytest.mark.parametrize('dim', [2, 3])
def test_atomics_colliding_on_one_key(dim):
    c = H.collide_case(dim)
    got = _run(c)
    _check('collide dim=%d' % dim, got, c['model'])
    _nontrivial(got, c['model'])


# ------------------------------------------------------------------------------ 4: non-finite and far locations, both passes
BAD = (float('nan'), float('inf'), float('-inf'), 1e30)


@pytest.mark.parametrize('dim', [2, 3])
def test_nonfinite_and_far_locations_in_the_backward(dim):
    """Query 5 of batch 0 gets NaN, +inf, -inf and 1e30 in turn over its coordinates (so every sample of it holds at least one,
    in every position).  Its samples' grad_loc / grad_attn are exactly 0, its output rows are 0, everything is finite, every
    other query's results are those of the untouched run bit for bit.  grad_value: the overwritten query no longer adds to
    it, so it is compared (``close``; atomic order is free) with the model and with a run in which that query's attention
    weights are zero -- the untouched run minus that query."""
    c = H.random_case(dim, 33)
    base = _run(c)
    loc = c['loc'].clone()
    n = loc[0, 5].numel()
    loc[0, 5] = torch.tensor([BAD[i % 4] for i in range(n)]).view(loc[0, 5].shape)
    if dim == 2:                                                         # (an even count of coordinates: shift every other sample)
        loc[0, 5, :, :, 1::2] = torch.tensor([BAD[(i + 1) % 4] for i in range(n // 2)]).view(loc[0, 5, :, :, 1::2].shape)
    loc[0, 5, 0, 0, 0] = 1e30                                            # far away on every axis, nothing non-finite
    loc[0, 5, 0, 1, 1] = c['loc'][0, 5, 0, 1, 1]                         # one NaN beside coordinates inside the map
    loc[0, 5, 0, 1, 1, 0] = float('nan')
    keep = torch.ones(c['loc'].shape[:2], dtype=torch.bool)
    keep[0, 5] = False
    assert not bool(H.in_gate(dim, c['shapes'], loc)[0, 5].any()) and torch.equal(loc[keep], c['loc'][keep])
    got = _run(c, loc=loc)
    for k in H.QUANTITIES:
        assert bool(torch.isfinite(got[k]).all()), k
    assert float(got['grad_loc'][0, 5].abs().max()) == 0.0 and float(got['grad_attn'][0, 5].abs().max()) == 0.0
    assert float(got['out'][0, 5].abs().max()) == 0.0
    for k in ('out', 'grad_loc', 'grad_attn'):
        assert torch.equal(got[k][keep], base[k][keep]), k
        assert float(base[k][0, 5].abs().max()) > 0.0, k
    attn0 = c['attn'].clone()
    attn0[0, 5] = 0.0
    without = _run(c, attn=attn0)
    assert close(got['grad_value'], without['grad_value'])
    want = H.model(dim, c['value'], c['shapes'], c['loc'], attn0, c['grad_out'])
    assert close(got['grad_value'], want['grad_value'])
    assert float((got['grad_value'] - base['grad_value']).abs().max()) > 1e-2      # (the query did contribute)


def test_nonfinite_and_far_locations_in_the_3d_forward():
    c = H.random_case(3, 33)
    args = (c['value'].to(DEV), c['shapes'].to(DEV), c['level_start'].to(DEV))
    attn = c['attn'].to(DEV)
    for bad in BAD + (7.5, -7.5):
        out = _apply(3, *args, torch.full_like(c['loc'], bad).to(DEV), attn)
        assert out.shape == (2, 13, 3 * 33) and float(out.abs().max()) == 0.0, bad
    assert float(_apply(3, *args, c['loc'].to(DEV), attn).abs().max()) > 0.1


# --------------------------------------------------------------------------------------------- 5: buffers of the C ABI
def _entries(dim):
    L = pkg('hipops').lib()
    if dim == 2:
        return (lambda *a: L.ver_msda_forward(*a[:-1], 64, a[-1])), (lambda *a: L.ver_msda_backward(*a[:-1], 64, a[-1]))
    return L.ver_msda3d_forward, L.ver_msda3d_backward


def _sizes(c):
    bsz, nk, heads, hd = c['value'].shape
    _, nq, _, nlev, npt, _ = c['loc'].shape
    return [bsz, nk, heads, hd, nlev, npt, nq]


@pytest.mark.parametrize('dim', [2, 3])
def test_gradient_buffers_accumulate_and_overwrite(dim):
    """grad_value is accumulated into (1.0 comes back as 1 + gradient); grad_loc / grad_attn_w are written for every sample,
    those outside the map included, which get 0 (7.0 does not survive anywhere)."""
    hip = pkg('hipops')
    p, st = hip._p, hip._stream()
    c = H.edge_case(dim, 32)
    _, bwd = _entries(dim)
    v, sh, ls, l, a, go = (c[k].to(DEV).contiguous() for k in ('value', 'shapes', 'level_start', 'loc', 'attn', 'grad_out'))
    gv, gl, ga = torch.full_like(v, 1.0), torch.full_like(l, 7.0), torch.full_like(a, 7.0)
    rc = bwd(p(v), p(sh), p(ls), p(l), p(a), p(go), p(gv), p(gl), p(ga), *_sizes(c), st)
    assert rc == VER_OK, hip.lib().ver_last_error()
    torch.cuda.synchronize()
    m = c['model']
    assert close(gv.cpu() - 1.0, m['grad_value']) and float((gv - 1.0).abs().max()) > 0.1
    assert close(gl.cpu(), m['grad_loc']) and close(ga.cpu(), m['grad_attn'])
    outside = ~c['gate']
    assert float(gl.cpu()[outside].abs().max()) == 0.0 and float(ga.cpu()[outside].abs().max()) == 0.0
    assert not bool((gl == 7.0).any()) and not bool((ga == 7.0).any())


@pytest.mark.parametrize('dim', [2, 3])
def test_argument_checks_of_the_entries(dim):
    hip = pkg('hipops')
    p, st = hip._p, hip._stream()
    fwd, bwd = _entries(dim)
    c = H.random_case(dim, 8)
    bsz, nk, heads, hd, nlev, npt, nq = _sizes(c)
    # an empty query set: VER_OK with null data pointers, both ways
    for b0, q0 in ((0, nq), (bsz, 0), (0, 0)):
        assert fwd(None, None, None, None, None, None, b0, nk, heads, hd, nlev, npt, q0, st) == VER_OK
        assert bwd(None, None, None, None, None, None, None, None, None, b0, nk, heads, hd, nlev, npt, q0, st) == VER_OK
    v, sh, ls, l, a, go = (c[k].to(DEV).contiguous() for k in ('value', 'shapes', 'level_start', 'loc', 'attn', 'grad_out'))
    out = torch.full_like(go, 3.0)
    gv, gl, ga = torch.zeros_like(v), torch.zeros_like(l), torch.zeros_like(a)
    # head_dim 257: refused before any launch, nothing written
    assert fwd(p(v), p(sh), p(ls), p(l), p(a), p(out), bsz, nk, heads, 257, nlev, npt, nq, st) == VER_EUNSUPPORTED
    assert b'head_dim 257' in hip.lib().ver_last_error()
    assert bwd(p(v), p(sh), p(ls), p(l), p(a), p(go), p(gv), p(gl), p(ga), bsz, nk, heads, 257, nlev, npt, nq, st) == VER_EUNSUPPORTED
    # a null grad_out, heads = 0
    assert bwd(p(v), p(sh), p(ls), p(l), p(a), None, p(gv), p(gl), p(ga), bsz, nk, heads, hd, nlev, npt, nq, st) == VER_EINVAL
    assert bwd(p(v), p(sh), p(ls), p(l), p(a), p(go), p(gv), p(gl), p(ga), bsz, nk, 0, hd, nlev, npt, nq, st) == VER_EINVAL
    assert fwd(p(v), p(sh), p(ls), p(l), p(a), p(out), bsz, nk, 0, hd, nlev, npt, nq, st) == VER_EINVAL
    assert fwd(p(v), p(sh), p(ls), p(l), p(a), None, bsz, nk, heads, hd, nlev, npt, nq, st) == VER_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and float(gv.abs().max()) == 0.0 and float(gl.abs().max()) == 0.0
    # the wrappers raise
    wide = torch.zeros(1, nk, 1, 257, device=DEV)
    loc1, attn1 = torch.zeros(1, 2, 1, nlev, npt, dim, device=DEV), torch.zeros(1, 2, 1, nlev, npt, device=DEV)
    with pytest.raises(RuntimeError, match='head_dim 257'):
        _apply(dim, wide, sh, ls, loc1, attn1)
    # ... and the entries still work afterwards
    assert fwd(p(v), p(sh), p(ls), p(l), p(a), p(out), bsz, nk, heads, hd, nlev, npt, nq, st) == VER_OK
    torch.cuda.synchronize()
    assert float((out.cpu().double() - c['model']['out']).abs().max()) < 2e-5


# ------------------------------------------------------------------------------------------------------------ 6: wrappers
def test_2d_wrapper_under_autocast_takes_bf16_value():
    hip = pkg('hipops')
    assert hip.MultiScaleDeformableAttnFunction_fp16 is hip.MultiScaleDeformableAttnFunction_fp32
    c = H.random_case(2, 33)
    sh, ls, l, a = (c[k].to(DEV) for k in ('shapes', 'level_start', 'loc', 'attn'))
    v16 = c['value'].bfloat16().to(DEV)
    with torch.autocast('cuda', torch.bfloat16):
        out = _apply(2, v16, sh, ls, l, a)
    want = _apply(2, v16.float(), sh, ls, l, a)
    assert out.dtype == torch.float32 and torch.equal(out, want) and float(out.abs().max()) > 0.1


@pytest.mark.parametrize('dim', [2, 3])
def test_wrappers_take_strided_operands(dim):
    """A permuted-view ``loc`` and the stride-0 ``grad_output`` of ``out.sum().backward()`` give the contiguous call's grad_loc /
    grad_attn bit for bit and its grad_value within ``close`` (atomic order is free)."""
    c = H.random_case(dim, 33)
    ones = torch.ones_like(c['grad_out'])
    base = _run(c, grad_out=ones)
    sh, ls = c['shapes'].to(DEV), c['level_start'].to(DEV)
    # loc stored as [B, heads, Nq, ...] and handed over as the [B, Nq, heads, ...] view of it
    stored = c['loc'].to(DEV).transpose(1, 2).contiguous().requires_grad_(True)
    view = stored.transpose(1, 2)
    assert not view.is_contiguous()
    v, a = c['value'].to(DEV).requires_grad_(True), c['attn'].to(DEV).requires_grad_(True)
    out = _apply(dim, v, sh, ls, view, a)
    out.sum().backward()                                                 # (grad_output: an expanded scalar, every stride 0)
    assert torch.equal(out.detach().cpu(), base['out'])
    assert torch.equal(stored.grad.transpose(1, 2).cpu(), base['grad_loc']) and torch.equal(a.grad.cpu(), base['grad_attn'])
    assert close(v.grad.cpu(), base['grad_value'])
    want = H.model(dim, c['value'], c['shapes'], c['loc'], c['attn'], ones)
    _check('strided dim=%d' % dim, dict(out=out.detach().cpu(), grad_value=v.grad.cpu(),
                                        grad_loc=stored.grad.transpose(1, 2).cpu(), grad_attn=a.grad.cpu()), want)
