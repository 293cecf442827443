"""row_kernels_helper without a GPU: the exact chains are torch's fp64 autograd, the fp32 models meet every bound and every
ceiling, the gate-stable rows deliver what the ln_relu bounds rest on, and each fault a row kernel of this kind can have --
planted into a model's output -- exceeds the bound of the quantity it is planted in (test_row_kernels_gpu.py holds the
kernels to the same bounds)."""
import numpy as np
import pytest
import torch

import row_kernels_helper as H

F32, BF16 = torch.float32, torch.bfloat16
F = torch.nn.functional


def _mutated(r, base=1, **changes):
    got = dict(r['models'][base])
    got.update(changes)
    return H.violations(H.measure(r, got), r['bound'])


def _hit(bad):
    return {v[:2] for v in bad}


def _big():
    """8 197 rows of 768 channels, bf16 a, p = 0.1: the training step's instantiation, the backward's second trip."""
    return H.add_ln_reference(H.ADD_LN_BWD_GRID * H.ADD_LN_ROWS + 5, 768, BF16, 0.1, 2 ** 62 - 1)


def test_exact_chains_are_torch_autograd_in_fp64():
    r = H.add_ln_reference(H.EDGE_ROWS, 768, BF16, 0.1, 1, True, True)
    inp, keep = r['inp'], r['keep']
    a, res, g, b = (inp[k].double().requires_grad_(True) for k in ('a', 'res', 'gamma', 'beta'))
    x = res + torch.where(keep, a / (1.0 - H.f32(0.1)), torch.zeros((), dtype=torch.float64))
    y = F.layer_norm(x, (768,), g, b, H.EPS)
    y.backward(inp['gy'].double() + inp['gy16'].double())
    want = dict(y=y.detach(), d_a=a.grad, d_res=res.grad, d_gamma=g.grad, d_beta=b.grad)
    for k, v in want.items():
        err = float((r['exact'][k] - v).abs().max() / v.abs().max())
        assert err < 1e-12, (k, err)
    q = H.ln_relu_reference(17, F32)
    x, g, b = (q[k].double().requires_grad_(True) for k in ('x', 'gamma', 'beta'))
    y = torch.relu(F.layer_norm(x, (128,), g, b, H.EPS))
    y.backward(q['gy'].double())
    for k, v in dict(y=y.detach(), d_x=x.grad, d_gamma=g.grad, d_beta=b.grad).items():
        err = float((q['exact'][k] - v).abs().max() / v.abs().max())
        assert err < 1e-12, (k, err)


def test_models_meet_every_bound():
    """the unmutated fp32 models pass (the ceilings are asserted where the bounds are formed); the three grid-stride cases
    print their d_ref and bounds."""
    cases = [_big(), H.add_ln_reference(H.EDGE_ROWS, 256, F32, 0.1, 1, True, True), H.add_ln_reference(5, 512, F32, 0.999, 1),
             H.add_ln_reference(5, 1024, BF16, 1e-8, 1), H.ln_relu_reference(H.LN_RELU_GRID * H.LN_RELU_ROWS + 17, BF16),
             H.ln_relu_reference(17, F32), H.relu_dropout_reference(1028, F32, 0.1, -1),
             H.relu_dropout_reference(1028, BF16, 0.5, 0)]
    for r in cases:
        for base in (0, 1):
            assert not _mutated(r, base)
        assert r['bound'] and all(np.isfinite(v) for v in r['bound'].values())
    print(H.table('add_ln 8197 x 768', cases[0]['d_ref'], None, cases[0]['bound']))
    print(H.table('ln_relu 65553', cases[4]['d_ref'], None, cases[4]['bound']))


def test_constant_rows_are_exact_in_the_models():
    """a = 0, residual = 4: the fp32 mean is 4 (768 x 4 x fl(1/768) rounds to 4), the centred values are 0 and y == beta bit
    for bit, in the order the kernel takes too."""
    for c in (256, 768):
        r = H.add_ln_reference(H.EDGE_ROWS, c, F32, 0.1, 1, True, True)
        for m in r['models']:
            for row in (1, 3):
                assert float(m['mean'][row]) == float(r['inp']['res'][row, 0])
                assert torch.equal(m['y'][row].view(torch.int32), r['inp']['beta'].view(torch.int32))


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_gate_stable_rows(dtype):
    """N rows from 2 N candidates (asserted in the helper, as are the margin against the models' moves and the equality of the
    gates); the recipe keeps about 90 %; both gate signs occur in every feature."""
    gamma, beta = H.ln_relu_params()
    assert float(gamma.min()) >= 0.5 and float(beta.abs().min()) >= H.f32(0.01)
    gen = torch.Generator(device='cpu').manual_seed(5)
    cand = (torch.randn(4096, 128, generator=gen) * 2 + 0.3).to(dtype)
    kept = H._stable(cand, gamma, beta).shape[0] / 4096.0
    print('%s: %.1f %% of the candidates are gate-stable' % (dtype, 100 * kept))
    assert kept > 0.75
    r = H.ln_relu_reference(H.LN_RELU_GRID * H.LN_RELU_ROWS + 17, dtype)
    assert bool(r['gates'].any(0).all()) and bool((~r['gates']).any(0).all())
    assert torch.equal(r['gates'][7], r['beta'] > 0)                       # the constant row
    assert abs(float(r['x'][3].float().mean()) - 100.0) < 0.5 and abs(float(r['x'][-1].float().mean()) - 100.0) < 0.5


def test_rows_of_the_last_trip_missing_from_the_parameter_gradients():
    r = _big()
    inp = dict(r['inp'])
    for k in ('gy', 'gy16'):
        inp[k] = inp[k].clone()
        inp[k][-5:] = 0
    short = H.add_ln_eval(inp, r['keep'], 0.1, F32)
    bad = _hit(_mutated(r, 0, d_gamma=short['d_gamma'], d_beta=short['d_beta']))
    print('5 of %d rows missing: %s' % (inp['gy'].shape[0], sorted(bad)))
    assert {('d_gamma', 'maxabs'), ('d_gamma', 'all'), ('d_beta', 'maxabs'), ('d_beta', 'all')} <= bad
    q = H.ln_relu_reference(H.LN_RELU_GRID * H.LN_RELU_ROWS + 17, F32)
    gy = q['gy'].clone()
    gy[-17:] = 0
    short = H.ln_relu_eval(q['x'], q['gamma'], q['beta'], gy, F32)
    assert {('d_gamma', 'maxabs'), ('d_beta', 'maxabs')} <= _hit(_mutated(q, 0, d_gamma=short['d_gamma'], d_beta=short['d_beta']))


def test_one_pass_variance_on_the_rows_of_mean_100():
    r = H.add_ln_reference(H.EDGE_ROWS, 256, F32, 0.1, 1, True, True)
    one = H.add_ln_eval(r['inp'], r['keep'], 0.1, F32, one_pass=True)
    y, rstd = r['models'][0]['y'].clone(), r['models'][0]['rstd'].clone()
    for row in (2, H.EDGE_ROWS - 1):
        y[row], rstd[row] = one['y'][row], one['rstd'][row]
    bad = {v[:2]: v[2] / v[3] for v in _mutated(r, 0, y=y, rstd=rstd)}
    print('one-pass variance, distance / bound: %s' % {k: round(v, 1) for k, v in bad.items()})
    assert bad[('y', 'maxabs')] >= 10 and bad[('y', 'row')] >= 10 and bad[('rstd', 'relmax')] >= 10


def test_wrong_masks():
    """hashed from the column instead of the flat index, with seed + 1, from the flat index truncated to 16 bits: each moves y
    and d(a) past their bounds, and leaves a non-zero where the host rule drops."""
    r = _big()
    n, c = r['keep'].shape
    flat = np.arange(n * c, dtype=np.uint64).reshape(n, c)
    masks = dict(column=H.keep_mask((n, c), r['seed'], 0.1, flat % np.uint64(c)),
                 seed_plus_1=H.keep_mask((n, c), r['seed'] + 1, 0.1),
                 low_16_bits=H.keep_mask((n, c), r['seed'], 0.1, flat & np.uint64(0xffff)))
    for name, keep in masks.items():
        assert not torch.equal(keep, r['keep']), name
        m = H._finish_add_ln(H.add_ln_eval(r['inp'], keep, 0.1, F32), BF16)
        assert bool((m['d_a'][~r['keep']] != 0).any()), name
        bad = _hit(_mutated(r, 0, **m))
        assert {('y', 'maxabs'), ('y', 'row'), ('d_a', 'row'), ('d_a', 'maxabs')} <= bad, (name, sorted(bad))
    q = H.relu_dropout_reference(1028, F32, 0.1, 1)
    wrong = H.relu_dropout_eval(q['inp'], H.keep_mask((1028,), 2, 0.1), 0.1, F32)
    assert bool((wrong['y'][~q['keep']] != 0).any())
    assert ('y', 'relmax') in _hit(H.violations(H.measure(q, wrong), q['bound']))


def test_missing_factor_swapped_column_truncated_copy_and_rstd():
    r = _big()
    m = r['models'][1]
    # d(a) without 1 / (1 - p)
    plain = H._finish_add_ln(H.add_ln_eval(r['inp'], r['keep'], 0.1, F32, no_scale_in_da=True), BF16)
    assert {('d_a', 'all'), ('d_a', 'col'), ('d_a', 'row'), ('d_a', 'maxabs')} <= _hit(_mutated(r, d_a=plain['d_a']))
    # one column of d(residual) taken from its neighbour
    d_res = m['d_res'].clone()
    d_res[:, 300] = d_res[:, 301]
    assert ('d_res', 'col') in _hit(_mutated(r, d_res=d_res))
    # y_bf16 truncated instead of rounded to nearest even: the check is bit equality with y.bfloat16()
    trunc = (m['y'].view(torch.int32) & -65536).view(F32).bfloat16()
    assert not torch.equal(trunc, m['y'].bfloat16())
    # 1/std off by 1e-3 relative in every row
    for q in (r, H.ln_relu_reference(17, F32)):
        assert {('rstd', 'all'), ('rstd', 'relmax')} <= _hit(_mutated(q, rstd=q['models'][1]['rstd'] * (1.0 + 1e-3)))


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_ln_relu_gate_from_the_normalised_value(dtype):
    q = H.ln_relu_reference(17, dtype)
    wrong = H._finish_ln_relu(H.ln_relu_eval(q['x'], q['gamma'], q['beta'], q['gy'], F32, gate_from_xhat=True), dtype)
    wrong.pop('pre')
    bad = _hit(_mutated(q, 0, **wrong))
    assert {('d_x', 'row'), ('d_x', 'col'), ('d_gamma', 'all'), ('d_beta', 'all')} <= bad, sorted(bad)
