"""The occupancy-MLP kernels (csrc/ver_occ_mlp.hip, through hipops) against the exact fp64 chain on gate-stable rows, with
per-feature bounds formed from the distance between the exact chain and an fp64 model of the kernel's rounding points
(occ_mlp_model_helper: bound = 4 d_ref + 2^-8, never above 5e-2).  One feature column of d(x) wrong by 3 %, a misplaced
kperm pair in d(W2), a tail block of rows missing from a parameter gradient or a 1/std off by 1e-3 exceed these bounds
(test_occ_mlp_gates_cpu.py plants them); the whole-tensor 6-9 % of the random-row tests in test_hip_ops_gpu.py do not see
them.  Every test prints d_ref, the kernel's distance and the bound (docs/HISTORY.md records the 2 048-row ones)."""
import pytest
import torch

import occ_mlp_model_helper as M
from util import pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N = M.PER_FEATURE_ROWS
SCALES = (0.05, 20.0)            # wider data: the rows' 1/std moves across three decades, the selection is redone per scale


def _sizes(ns):
    return [(n, 1.0) for n in ns] + [(N, s) for s in SCALES]


def _leaves(r, mode):
    return {k: r['p'][k].to(DEV).requires_grad_(True) for k in M.keys_of(mode)}


def _hidden(pd, mode):
    """(w1, b1, w2, b2) as the caller of the kernels passes them in this mode."""
    w1, b1 = (pd['w1'], pd['b1']) if mode == 'unfolded' else (None, None)
    w2, b2 = M.center(pd['w2'], pd['b2']) if mode == 'folded_centered' else (pd['w2'], pd['b2'])
    return w1, b1, w2, b2


def _check(title, r, got, mode):
    d = M.distances(M.finish(got, mode), r['exact'])
    print(M.table(title, r['d_ref'], d, r['bound']))
    for k in r['d_ref']:
        assert k in d, k                                   # everything the reference holds was compared
    bad = M.violations(d, r['bound'])
    assert not bad, bad


def _backward(hip, r, mode):
    pd = _leaves(r, mode)
    w1, b1, w2, b2 = _hidden(pd, mode)
    xd = r['x'].to(DEV).requires_grad_(True)
    out = hip.occ_mlp(xd, w1, b1, pd['g1'], pd['be1'], w2, b2, pd['g2'], pd['be2'], pd['w3'], pd['b3'],
                      centered=mode == 'folded_centered')
    out.backward(r['gy'].to(DEV))
    assert xd.grad.dtype == torch.bfloat16 and xd.grad.shape == r['x'].shape
    got = {k: v.grad for k, v in pd.items()}
    for k, v in got.items():
        assert v is not None and v.shape == r['p'][k].shape, k
    got['x'] = xd.grad
    return got


@pytest.mark.parametrize('n,scale', _sizes([1, 63, 65, N, 64 * 4 * 512 + 1]))
@pytest.mark.parametrize('mode', M.MODES)
def test_occ_mlp_forward_on_gate_stable_rows(mode, n, scale):
    """ver_occ_mlp_forward_stats, unfolded / folded / folded + centred, around its 64-row blocks, four waves and 512 persistent
    workgroups: the logits and BOTH columns of rstd against the exact chain."""
    hip = pkg('hipops')
    r = M.reference(mode, n, 'forward', 12, scale)
    pd = {k: v.to(DEV) for k, v in r['p'].items()}
    w1, b1, w2, b2 = _hidden(pd, mode)
    if w1 is None:                                         # folded: W2 in W1's image sections, b1 = 0 (hipops._occ_mlp_forward_packed)
        w1, b1 = w2, torch.zeros(128, device=DEV)
    image = hip.occ_mlp_pack(w1, w2, pd['w3'])
    vec = hip.occ_mlp_vectors(b1, pd['g1'], pd['be1'], b2, pd['g2'], pd['be2'], pd['b3'])
    kw = dict(first_linear=mode == 'unfolded', centered=mode == 'folded_centered')
    x = r['x'].to(DEV)
    logits, rstd = hip.occ_mlp_forward(x, image, vec, 1e-5, want_rstd=True, **kw)
    assert logits.shape == (n, 16) and logits.dtype == torch.bfloat16 and rstd.shape == (n, 2)
    assert torch.equal(hip.occ_mlp_forward(x, image, vec, 1e-5, **kw), logits)          # the statistics change no logit
    _check('forward %s n=%d scale=%g' % (mode, n, scale), r, dict(logits=logits, rstd=rstd), mode)


@pytest.mark.parametrize('n,scale', _sizes([1, 15, 16, 17, N, 16 * 4 * 256 + 1]))
@pytest.mark.parametrize('mode', ['unfolded', 'folded'])
def test_occ_mlp_row_split_backward_on_gate_stable_rows(mode, n, scale, monkeypatch):
    """ver_occ_mlp_backward (16-row iterations, four waves, 256 workgroups) + the host GEMMs of hipops: d(x) and every
    parameter gradient -- d(W1) and d(b1) of the unfolded chain included, which also covers the un-permutation of the fragment
    feature order in OccMLPFunction.backward."""
    hip = pkg('hipops')
    monkeypatch.setattr(hip, '_OCC_MLP_BWD_FUSED', False)
    r = M.reference(mode, n, 'row_split', 12, scale)
    _check('row_split %s n=%d scale=%g' % (mode, n, scale), r, _backward(hip, r, mode), mode)


@pytest.mark.parametrize('n,scale', _sizes([1, 63, 64, 65, 128, 191, N, 64 * 256 + 1, 64 * 513 + 7]))
@pytest.mark.parametrize('save_rstd', [True, False])
@pytest.mark.parametrize('mode', ['folded', 'folded_centered'])
def test_occ_mlp_wave_specialised_backward_on_gate_stable_rows(mode, save_rstd, n, scale, monkeypatch):
    """ver_occ_mlp_backward_fused_slabs, plain and centred, reading the saved 1/std or recomputing it: one block, the A / B pair
    of a round, more blocks than workgroups, a third round."""
    hip = pkg('hipops')
    monkeypatch.setattr(hip, '_OCC_MLP_BWD_FUSED', True)
    monkeypatch.setattr(hip, '_OCC_MLP_SAVE_RSTD', save_rstd)
    r = M.reference(mode, n, 'wave_spec', 12, scale)
    _check('wave_spec %s save_rstd=%d n=%d scale=%g' % (mode, save_rstd, n, scale), r, _backward(hip, r, mode), mode)


def test_occ_mlp_wave_specialised_backward_with_a_device_scale():
    """``grad_scale`` (the upstream factor of the fused loss, a device scalar): the kernel on the unscaled d(logits) against the
    exact chain on d(logits) times the scalar."""
    hip = pkg('hipops')
    gscale = torch.tensor([0.37 / 1234.0], dtype=torch.float32)
    r = M.reference('folded', N, 'wave_spec', 12, 1.0, float(gscale))
    pd = {k: v.to(DEV) for k, v in r['p'].items()}
    vec = hip.occ_mlp_vectors(torch.zeros(128, device=DEV), pd['g1'], pd['be1'], pd['b2'], pd['g2'], pd['be2'], pd['b3'])
    gx, vecs, dw2, dw3, db3 = hip._occ_mlp_backward_fused(r['x'].to(DEV), r['gy'].to(DEV), pd['w2'], pd['w3'], vec, None, 1e-5,
                                                          False, gscale.to(DEV))
    got = dict(x=gx, g1=vecs[0], be1=vecs[1], w2=dw2, b2=vecs[5], g2=vecs[3], be2=vecs[4], w3=dw3, b3=db3)
    _check('wave_spec folded n=%d grad_scale=%.3e' % (N, float(gscale)), r, got, 'folded')
