"""Keeps the fp64 model and the bounds of tests/msda_forms_helper.py honest, without a GPU:
  * the model is the oracle's fp64 autograd everywhere except ``grad_loc`` of samples with a pixel coordinate of exactly -1, and
    in 3-D the oracle's unmasked fp64 autograd is ``F.grid_sample``'s -- so the kernels' documented exception to "5-D grid_sample
    semantics" (include/ver_ops.h) is exactly that one point per axis;
  * on every input the GPU tests use, the fp32 CPU oracle stays under a quarter of each bound against the model, so that a
    kernel that misses a bound is wrong and not unlucky;
  * the model reproduces the recorded reference results (tests/golden) to the same bounds."""
import pytest
import torch
import torch.nn.functional as F

import cases
import msda_forms_helper as H
from util import close, golden, maxdiff

T = torch.from_numpy
RANDOM = [(dim, hd) for dim in (2, 3) for hd in H.WIDTHS]
EDGE = [(dim, hd) for dim in (2, 3) for hd in H.EDGE_WIDTHS]


def _raw(c):
    return H.autograd(c['dim'], c['value'], c['shapes'], c['loc'], c['attn'], c['grad_out'], torch.float64)


def test_forms_and_widths():
    """WIDTHS holds the last width of every form and the first of the next; 78 groups give every form a ragged last block."""
    forms = [H.form(w) for w in H.WIDTHS]
    assert sorted(set(forms)) == sorted({(8, 1), (16, 1), (32, 1), (64, 1), (32, 3), (64, 2), (64, 3), (64, 4)})
    tops = (8, 16, 32, 64, 96, 128, 192, 256)
    assert set(H.WIDTHS) == {1} | set(tops) | {t + 1 for t in tops[:-1]}
    for t in tops[:-1]:
        assert H.form(t) != H.form(t + 1)
    c = H.random_case(2, 8)
    groups = c['loc'].shape[0] * c['loc'].shape[1] * c['loc'].shape[2]
    assert groups == 78 and c['loc'].shape[0] == 2
    for g, _ in set(forms):
        per_block = 256 // g
        assert groups > 2 * per_block and groups % per_block != 0, g


@pytest.mark.parametrize('dim', [2, 3])
def test_random_inputs_are_gate_stable(dim):
    for hd in (1, 33, 256):
        c = H.random_case(dim, hd)
        pix = H.pixels(dim, c['shapes'], c['loc'])
        frac = pix - torch.floor(pix)
        assert float(frac.min()) >= H.MARGIN and float(frac.max()) <= 1.0 - H.MARGIN
        assert c['moved'] < 0.05 * c['loc'].numel()
        assert min(int(c['gate'].sum()), int((~c['gate']).sum())) >= 20    # both sides of the gate are populated
        assert float(c['loc'].min()) < 0.0 and float(c['loc'].max()) > 1.0


@pytest.mark.parametrize('dim', [2, 3])
def test_edge_inputs_hold_every_edge(dim):
    c = H.edge_case(dim)
    pix, size = c['pix'], H.sizes_of(dim, c['shapes'])
    for lvl in range(size.shape[0]):
        for ax in range(dim):
            p, n = pix[:, :, :, lvl, :, ax], float(size[lvl, ax])
            for t in (-1.25, -1.0, -0.5, 0.0, 0.25, n - 1.0, n - 0.5, n, n + 0.25):
                assert bool((p == t).any()), (lvl, ax, t)
    assert bool((size == 1).any())                                      # the one-pixel axes
    assert int(H.interior_integer(c).sum()) > 0
    assert bool(c['gate'].any()) and bool((~c['gate']).any())
    cc = H.collide_case(dim)
    assert cc['value'].shape[1] == 1 and bool(cc['gate'].all())


@pytest.mark.parametrize('dim', [2, 3])
def test_model_is_the_oracle_except_at_minus_one(dim):
    """Both halves: equality wherever no coordinate is exactly -1, and a non-zero oracle gradient at some of those points."""
    c = H.edge_case(dim)
    raw, m = _raw(c), c['model']
    for k in ('out', 'grad_value', 'grad_attn'):
        assert torch.equal(raw[k], m[k]), k
    at_minus_one = (c['pix'] == -1.0).any(-1)
    differs = (raw['grad_loc'] != m['grad_loc']).any(-1)
    assert not bool((differs & ~at_minus_one).any())
    assert int(differs.sum()) > 0 and float(raw['grad_loc'][at_minus_one].abs().max()) > 1e-3
    assert float(m['grad_loc'][at_minus_one].abs().max()) == 0.0
    # outside the gate everything else is zero both ways: out / grad_value / grad_attn of a sample that is alone in its query
    assert float(raw['grad_attn'][~c['gate']].abs().max()) == 0.0
    for hd in (5, 64):                                                   # no such point among the random inputs
        r = H.random_case(dim, hd)
        assert torch.equal(_raw(r)['grad_loc'], r['model']['grad_loc'])


def _grid_sample_op(value, shapes, loc, attn):
    """The 3-D op as the decoder's reference function composes it: per level one 5-D ``F.grid_sample`` (trilinear, zeros,
    align_corners=False) of value_l [B*heads, hd, D, H, W] on grid = 2 loc - 1, weighted by attn and summed."""
    bsz, _, heads, hd = value.shape
    _, nq, _, nlev, npt, _ = loc.shape
    grids = 2.0 * loc - 1.0
    start, parts = 0, []
    for lvl, (d, h, w) in enumerate(shapes):
        v = value[:, start:start + d * h * w].flatten(2).transpose(1, 2).reshape(bsz * heads, hd, d, h, w)
        start += d * h * w
        g = grids[:, :, :, lvl].transpose(1, 2).flatten(0, 1)[:, :, :, None, :]                  # [B*heads, Nq, P, 1, 3]
        parts.append(F.grid_sample(v, g, mode='bilinear', padding_mode='zeros', align_corners=False)[..., 0])
    a = attn.transpose(1, 2).reshape(bsz * heads, 1, nq, nlev * npt)
    out = (torch.stack(parts, -2).flatten(-2) * a).sum(-1).view(bsz, heads * hd, nq)
    return out.transpose(1, 2)


def test_unmasked_3d_gradient_is_grid_sample():
    c = H.edge_case(3)
    raw = _raw(c)
    v, l, a = (c[k].double().requires_grad_(True) for k in ('value', 'loc', 'attn'))
    out = _grid_sample_op(v, c['shapes'].tolist(), l, a)
    out.backward(c['grad_out'].double())
    assert maxdiff(out.detach(), raw['out']) < 1e-12
    assert maxdiff(v.grad, raw['grad_value']) < 1e-12
    assert maxdiff(a.grad, raw['grad_attn']) < 1e-12
    assert maxdiff(l.grad, raw['grad_loc']) < 1e-11
    at_minus_one = (c['pix'] == -1.0).any(-1)
    assert float(l.grad[at_minus_one].abs().max()) > 1e-3               # grid_sample's non-zero gradient where the kernel gives 0
    assert maxdiff(l.grad[~at_minus_one], c['model']['grad_loc'][~at_minus_one]) < 1e-11


def _quarter(c):
    got = H.gated(c['dim'], c['shapes'], c['loc'],
                  H.autograd(c['dim'], c['value'], c['shapes'], c['loc'], c['attn'], c['grad_out'], torch.float32))
    r = H.ratios(got, c['model'])
    print('fp32 oracle / bound:', ' '.join('%s %.3f' % kv for kv in r.items()))
    for k, v in r.items():
        assert v <= 0.25, (k, v)
    for k in H.QUANTITIES:
        assert float(c['model'][k].norm()) > 0.1, k


@pytest.mark.parametrize('dim,hd', RANDOM)
def test_fp32_oracle_within_a_quarter_of_the_bounds_random(dim, hd):
    _quarter(H.random_case(dim, hd))


@pytest.mark.parametrize('dim,hd', EDGE)
def test_fp32_oracle_within_a_quarter_of_the_bounds_edge(dim, hd):
    _quarter(H.edge_case(dim, hd))


@pytest.mark.parametrize('dim', [2, 3])
def test_fp32_oracle_within_a_quarter_of_the_bounds_collide(dim):
    _quarter(H.collide_case(dim))


def test_model_equals_the_golden_files():
    c = cases.msda_inputs(**cases.MSDA_CASES['small_2lvl'])
    g = golden('msda_core_small_2lvl')
    m = H.model(2, T(c['value']), T(c['shapes']), T(c['loc']), T(c['w']), T(c['grad_out']))
    assert maxdiff(m['out'], g['out']) < 2e-5
    assert close(m['grad_value'], g['grad_value']) and close(m['grad_loc'], g['grad_loc']) and close(m['grad_attn'], g['grad_w'])
    c = cases.msda3d_inputs(**cases.MSDA3D_CASES['two_levels'])
    g = golden('msda3d_core_two_levels')
    m = H.model(3, T(c['value']), T(c['shapes']), T(c['loc']), T(c['w']), T(c['grad_out']))
    assert maxdiff(m['out'], g['out']) < 2e-5
    assert close(m['grad_value'][:, ::3], g['grad_value']) and close(m['grad_loc'], g['grad_loc'])
    assert close(m['grad_attn'], g['grad_w'])
