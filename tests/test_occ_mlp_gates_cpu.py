"""The gate-stable rows and the per-feature comparator of occ_mlp_model_helper, without a GPU: the selection delivers what
the bounds rest on, the comparator catches planted faults with the rounded model standing in for a kernel, and on random
rows the same bounds are out of reach (the selection is what makes them available)."""
import pytest
import torch

import occ_mlp_model_helper as M

N = M.PER_FEATURE_ROWS


@pytest.mark.parametrize('mode', M.MODES)
def test_stable_rows_have_no_gate_flips_and_bounds_stay_small(mode):
    """stable_rows succeeds under the candidate cap (asserted in the helper, as is the equality of the gates of every rounded
    model with the exact chain's on every kept row); both gate signs occur; every bound stays below 5e-2."""
    x = M.stable_rows(mode, N)
    assert x.shape == (N, 128) and x.dtype == torch.bfloat16
    E, seen = M.pool_stats(mode)
    assert seen <= M.MAX_CANDIDATES
    print('%s: %d candidates for %d rows, E = (%.4f, %.4f)' % (mode, seen, M.POOL, E[0], E[1]))
    p = M.params()
    assert 16 <= int((p['g1'] < 0).sum()) <= 48 and 16 <= int((p['g2'] < 0).sum()) <= 48
    for kernel in M.KERNELS:
        r = M.reference(mode, N, kernel)
        assert M.same_gates(r['model'], r['exact'])
        for pre in r['exact']['pre']:
            gate = pre > 0
            assert bool(gate.any(0).all()) and bool((~gate).any(0).all())          # every feature is open AND closed somewhere
        assert r['bound'] and max(r['bound'].values()) <= M.MAX_BOUND
        assert not M.violations(r['d_ref'], r['bound'])                            # the unmutated model passes
        print(M.table('%s / %s, %d rows' % (mode, kernel, N), r['d_ref'], None, r['bound']))
    more = M.stable_rows(mode, 3 * N + 1)                                          # more rows than the pool: the pool, indexed
    assert more.shape == (3 * N + 1, 128)
    assert M.same_gates(M.chain(more[-64:], p, mode, 'wave_spec'), M.chain(more[-64:], p, mode))
    assert not torch.equal(M.grad_logits(4)[0], M.grad_logits(4)[1])


def test_exact_chain_is_the_layer_by_layer_fp64_chain():
    """the exact chain against torch.nn.functional in fp64, forward and every gradient (what the existing tests compare with)."""
    F = torch.nn.functional
    p = M.params()
    x, gy = M.stable_rows('unfolded', 65), M.grad_logits(65)
    got = M.chain(x, p, 'unfolded', False, gy)
    pr = {k: (v.bfloat16().double() if k.startswith('w') else v.double()).requires_grad_(True) for k, v in p.items()}
    xr = x.double().requires_grad_(True)
    h = F.relu(F.layer_norm(F.linear(xr, pr['w1'], pr['b1']), (128,), pr['g1'], pr['be1'], 1e-5))
    h = F.relu(F.layer_norm(F.linear(h, pr['w2'], pr['b2']), (128,), pr['g2'], pr['be2'], 1e-5))
    ref = F.linear(h, pr['w3'], pr['b3'])
    ref.backward(gy.double())
    assert float((got['logits'] - ref.detach()).abs().max()) < 1e-12
    assert float((got['x'] - xr.grad).abs().max()) < 1e-12
    for k in M.KEYS:
        assert float((got[k] - pr[k].grad).abs().max()) < 1e-11, k


def _mutated(r, **changes):
    got = dict(r['model'])
    got.update(changes)
    return M.violations(M.distances(got, r['exact']), r['bound'])


def test_comparator_catches_planted_faults():
    """The rounded model stands in for the kernel; each fault must exceed a bound of the quantity it is planted in."""
    r = M.reference('folded', N, 'row_split')
    m = r['model']
    assert not _mutated(r)
    # one d(x) column scaled by 0.97: the weakest column the floor of the denominators (the RMS column norm) leaves whole
    gx = m['x'].clone()
    norms = r['exact']['x'].norm(dim=0)
    col = int(torch.where(norms >= norms.pow(2).mean().sqrt(), norms, norms.max()).argmin())
    gx[:, col] *= 0.97
    assert ('x', 'col') in {v[:2] for v in _mutated(r, x=gx)}
    # features 4 and 16 of h1 swapped in d(W2): the first pair kperm moves
    dw2 = m['w2'].clone()
    dw2[:, [4, 16]] = dw2[:, [16, 4]]
    assert ('w2', 'col') in {v[:2] for v in _mutated(r, w2=dw2)}
    # the last 5 rows left out of every parameter gradient
    gy = r['gy'].clone()
    gy[-5:] = 0
    short = M.chain(r['x'], r['p'], 'folded', 'row_split', gy)
    bad = {v[0] for v in _mutated(r, **{k: short[k] for k in M.FOLDED_KEYS})}
    print('5 of %d rows missing: bounds exceeded for %s' % (N, sorted(bad)))
    assert {'w2', 'w3', 'b3'} <= bad
    # one data row of d(x) replaced by its neighbour's
    gx = m['x'].clone()
    gx[1000] = gx[1001]
    assert ('x', 'data_row') in {v[:2] for v in _mutated(r, x=gx)}
    # the layer-2 rstd off by 1e-3 relative
    f = M.reference('folded', N, 'forward')
    rstd = f['model']['rstd'].clone()
    rstd[:, 1] *= 1.0 + 1e-3
    assert not _mutated(f)
    assert ('rstd', 'bias') in {v[:2] for v in _mutated(f, rstd=rstd)}


@pytest.mark.parametrize('mode', M.MODES)
def test_random_rows_exceed_the_bounds(mode):
    """on random, unfiltered rows gates differ between the two chains and the comparator does exceed the bounds of the
    selected rows: the selection is what makes them available."""
    p = M.params()
    gen = torch.Generator(device='cpu').manual_seed(77)
    x = M.candidates(p, mode, N, gen)
    gy = M.grad_logits(N)
    exact = M.chain(x, p, mode, False, gy)
    model = M.chain(x, p, mode, 'row_split', gy)
    assert not M.same_gates(model, exact)
    bound = M.reference(mode, N, 'row_split')['bound']
    bad = M.violations(M.distances(model, exact), bound)
    print('%s, random rows: %s' % (mode, ', '.join('%s/%s %.3f > %.3f' % v for v in bad)))
    assert {'x', 'w2'} <= {v[0] for v in bad}
