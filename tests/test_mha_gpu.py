"""ver_mha_forward / _backward (hipops.mha_core) on the GPU against the float64 model of tests/mha_helper.py, and through
``MultiheadAttention(fused=True)`` up to the head.  ``-m gpu``.

Tolerances (the project's precision contract): fp32 operands, max |delta| <= 1e-4 of the model's largest magnitude, per
tensor; bf16 operands, relative L2 <= 1e-2 against the float64 model evaluated on the bf16-rounded inputs.  The model is the
yardstick, never the torch chain and never the kernel itself."""
import copy
import functools
import warnings

import numpy as np
import pytest
import torch

import cases
import dattn3d_helper as dh
import mha_helper as mh
from util import close, golden, pkg

warnings.filterwarnings('ignore')
pytestmark = pytest.mark.gpu
DEV = 'cuda'
OUTS = ('out', 'grad_q', 'grad_k', 'grad_v')
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}

# (B, heads, head_dim, Nq, Nk): the smallest shapes at which each mechanism can go wrong
SHAPES = {
    'vocc': (2, 8, 96, 100, 100),            # vocc.py
    'vocc_layout': (2, 8, 96, 110, 110),     # with the 10 layout queries
    'tiny': (1, 4, 8, 7, 7),                 # everything smaller than one tile, head_dim below the MFMA depth
    'ragged': (3, 2, 40, 17, 33),            # one past a 16-tile and a 32-deep step, Nq != Nk, head_dim no multiple of 32
    'corner': (1, 8, 128, 128, 128),         # the upper corner and the LDS budget
    'grid': (40, 8, 16, 16, 16),             # 320 workgroups, more than the CUs: grid indexing
    'single': (1, 1, 96, 1, 1),              # a single query: P = 1 and dS = 0
}


def _quant(dtype):
    return (lambda t: t.bfloat16().float()) if dtype == torch.bfloat16 else None


@functools.lru_cache(maxsize=None)
def _case(name, dname):
    """(operands, float64 model without dropout) of a named shape, computed once and left unchanged."""
    B, heads, hd, Nq, Nk = SHAPES[name]
    c = mh.make_inputs(sum(map(ord, name)), B, heads, hd, Nq, Nk, quant=_quant(DTYPES[dname]))
    return c, mh.model(c['q'], c['k'], c['v'], heads, grad_out=c['grad_out'])


def check(got, want, dtype, names=OUTS):
    for n in names:
        assert got[n].dtype == dtype and tuple(got[n].shape) == tuple(want[n].shape), n
        (mh.check_f32 if dtype == torch.float32 else mh.check_bf16)(got[n], want[n], n)


def op(c, heads, dtype, p_drop=0.0):
    """hipops.mha_core forward + backward -> dict(out, grad_q, grad_k, grad_v, seed)."""
    hip = pkg('hipops')
    q, k, v = (c[n].to(dtype).to(DEV).requires_grad_(True) for n in ('q', 'k', 'v'))
    out = hip.mha_core(q, k, v, heads, p_drop)
    seed = out.grad_fn.saved_tensors[-1]
    out.backward(c['grad_out'].to(dtype).to(DEV))
    torch.cuda.synchronize()
    return dict(out=out.detach(), grad_q=q.grad, grad_k=k.grad, grad_v=v.grad, seed=int(seed[0]) if seed.numel() else None)


GUARD, GAP, SENTINEL = 64, 16, 777.0


def _guarded(rows, cols, pitch, dtype, fill):
    """A [rows, cols] view with row pitch ``pitch`` inside a flat buffer with GUARD elements on either side; the guard bands
    and the gap columns hold SENTINEL, the view ``fill``."""
    flat = torch.full((2 * GUARD + rows * pitch,), SENTINEL, dtype=dtype, device=DEV)
    view = flat[GUARD:GUARD + rows * pitch].view(rows, pitch)[:, :cols]
    view.fill_(fill)
    return flat, view


def _untouched(flat, rows, cols, pitch):
    body = flat[GUARD:GUARD + rows * pitch].view(rows, pitch)
    return bool((flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all() and (body[:, cols:] == SENTINEL).all())


def abi(c, heads, dtype, p_drop=0.0, seed=None, joint=False):
    """ver_mha_forward + ver_mha_backward through the C ABI with every output pre-filled with NaN inside guard bands.
    ``joint``: q and k are the column halves of one [N, B, 2C + GAP] buffer (Nq == Nk) and grad_q / grad_k those of
    another; otherwise every operand and gradient has its own buffer with pitch C + GAP.  Returns the results and whether
    every guard band and gap column is untouched."""
    hip = pkg('hipops')
    lib, p = hip.lib(), hip._p
    Nq, B, C = c['q'].shape
    Nk = c['k'].shape[0]
    dt = 1 if dtype == torch.bfloat16 else 0
    nan = float('nan')
    bufs = {}

    def buf(name, n, cols, pitch, fill, src=None):
        flat, view = _guarded(n * B, cols, pitch, dtype, fill)
        if src is not None:
            view.copy_(src.to(dtype).to(DEV).reshape(n * B, cols))
        bufs[name] = (flat, n * B, cols, pitch)
        return view

    if joint:
        assert Nq == Nk
        qk = buf('qk', Nq, 2 * C, 2 * C + GAP, 0.0, torch.cat([c['q'], c['k']], -1))
        q, k, ldq, ldk = qk[:, :C], qk[:, C:], 2 * C + GAP, 2 * C + GAP
        gqk = buf('gqk', Nq, 2 * C, 2 * C + GAP, nan)
        gq, gk, ldgq, ldgk = gqk[:, :C], gqk[:, C:], 2 * C + GAP, 2 * C + GAP
    else:
        q, k = buf('q', Nq, C, C + GAP, 0.0, c['q']), buf('k', Nk, C, C + GAP, 0.0, c['k'])
        gq, gk = buf('gq', Nq, C, C + GAP, nan), buf('gk', Nk, C, C + GAP, nan)
        ldq = ldk = ldgq = ldgk = C + GAP
    v = buf('v', Nk, C, C + GAP, 0.0, c['v'])
    gv = buf('gv', Nk, C, C + GAP, nan)
    out = buf('out', Nq, C, C, nan)
    go = c['grad_out'].to(dtype).to(DEV).contiguous()
    lse_flat = torch.full((2 * GUARD + B * heads * Nq,), SENTINEL, dtype=torch.float32, device=DEV)
    lse = lse_flat[GUARD:GUARD + B * heads * Nq]
    lse.fill_(nan)
    seed_t = None if seed is None else torch.tensor([seed], dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    dims = (B, heads, C // heads, Nq, Nk, stream)
    rc = lib.ver_mha_forward(q.data_ptr(), k.data_ptr(), v.data_ptr(), dt, ldq, ldk, C + GAP, p(seed_t), p_drop, out.data_ptr(),
                             lse.data_ptr(), *dims)
    assert rc == 0, lib.ver_last_error()
    rc = lib.ver_mha_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), dt, ldq, ldk, C + GAP, p(go), lse.data_ptr(), p(seed_t),
                              p_drop, gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), ldgq, ldgk, C + GAP, *dims)
    assert rc == 0, lib.ver_last_error()
    torch.cuda.synchronize()
    clean = all(_untouched(*b) for b in bufs.values())
    clean = clean and bool((lse_flat[:GUARD] == SENTINEL).all() and (lse_flat[-GUARD:] == SENTINEL).all())
    res = dict(out=out.reshape(Nq, B, C), grad_q=gq.reshape(Nq, B, C), grad_k=gk.reshape(Nk, B, C), grad_v=gv.reshape(Nk, B, C),
               lse=lse.view(B, heads, Nq))
    return {n: t.clone() for n, t in res.items()}, clean


# ------------------------------------------------------------------------------------------ 1: against the model
@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('name', list(SHAPES))
def test_forward_and_gradients_against_the_float64_model(name, dname):
    c, want = _case(name, dname)
    got = op(c, SHAPES[name][1], DTYPES[dname])
    check(got, want, DTYPES[dname])
    if name == 'single':                                      # softmax of one score is 1 whatever the score is
        assert float(got['grad_q'].abs().max()) == 0.0 and float(got['grad_k'].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ 2: pitched operands
@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('joint', [True, False])
def test_pitched_operands_and_guard_bands(joint, dname):
    """q and k as the halves of one [N, B, 2C + gap] buffer and grad_q / grad_k written into another (joint), or every tensor
    with its own pitch C + gap: the gap columns, the other half and a guard band around every output keep their sentinel,
    and no NaN of the pre-fill survives (every output element is written).  head_dim 24 and 19 rows: nothing is a multiple
    of a tile."""
    dtype = DTYPES[dname]
    B, heads, hd, Nq, Nk = (2, 4, 24, 19, 19) if joint else SHAPES['ragged']
    c = mh.make_inputs(11, B, heads, hd, Nq, Nk, quant=_quant(dtype))
    want = mh.model(c['q'], c['k'], c['v'], heads, grad_out=c['grad_out'])
    got, clean = abi(c, heads, dtype, joint=joint)
    assert clean
    check(got, want, dtype)
    mh.check_f32(got['lse'], want['lse'], 'lse')
    # and the wrapper reads the halves of one Linear output in place and returns one joint gradient
    if joint:
        hip = pkg('hipops')
        qk = torch.cat([c['q'], c['k']], -1).to(dtype).to(DEV).requires_grad_(True)
        v = c['v'].to(dtype).to(DEV).requires_grad_(True)
        C = heads * hd
        for call in (lambda: hip.mha_core(qk[..., :C], qk[..., C:], v, heads), lambda: hip.mha_core_joint(qk, v, heads)):
            qk.grad = v.grad = None
            out = call()
            saved = out.grad_fn.saved_tensors
            assert saved[0].data_ptr() == qk.data_ptr()                               # no copy in front of the kernel
            assert len(saved) == 4 or saved[1].data_ptr() == qk.data_ptr() + C * qk.element_size()
            out.backward(c['grad_out'].to(dtype).to(DEV))
            assert torch.equal(out, got['out']) and torch.equal(v.grad, got['grad_v'])
            assert torch.equal(qk.grad[..., :C], got['grad_q']) and torch.equal(qk.grad[..., C:], got['grad_k'])


# ------------------------------------------------------------------------------------------ 3: extreme scores
@pytest.mark.parametrize('dname', list(DTYPES))
def test_extreme_scores(dname):
    """Row 0 of every (sample, head): logits near +80 (q = a multiple of a direction every key shares); row 1: its negative,
    logits near -80; row 2: q = 0, all scores equal.  Finite and within tolerance."""
    dtype = DTYPES[dname]
    B, heads, hd, Nq, Nk = SHAPES['ragged']
    quant = _quant(dtype) or (lambda t: t)
    c = mh.make_inputs(12, B, heads, hd, Nq, Nk)
    k = c['k'] + 1.0                                          # k_j . 1 = hd +- sqrt(hd)
    q = c['q'].clone()
    q[0] = 80.0 / np.sqrt(hd)                                 # S = 80 (k_j . 1) / hd
    q[1] = -80.0 / np.sqrt(hd)
    q[2] = 0.0
    c = dict(q=quant(q.float()).double(), k=quant(k.float()).double(), v=quant(c['v'].float()).double(),
             grad_out=quant(c['grad_out'].float()).double())
    s = torch.einsum('ibhd,jbhd->bhij', c['q'].view(Nq, B, heads, hd), c['k'].view(Nk, B, heads, hd)) / np.sqrt(hd)
    assert 60 < float(s[:, :, 0].mean()) < 100 and -100 < float(s[:, :, 1].mean()) < -60 and float(s[:, :, 2].abs().max()) == 0
    want = mh.model(c['q'], c['k'], c['v'], heads, grad_out=c['grad_out'])
    check(op(c, heads, dtype), want, dtype)


# ------------------------------------------------------------------------------------------ 4: dropout
@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('p_drop', [0.1, 0.5])
@pytest.mark.parametrize('name', ['vocc', 'ragged'])
def test_dropout_equals_the_model_under_the_host_mask(name, p_drop, dname):
    """Output AND gradients under hipops.dropout_keep_host's mask of the same seed: the backward recomputes the forward's
    decisions.  Another seed gives another output."""
    hip = pkg('hipops')
    dtype = DTYPES[dname]
    B, heads, hd, Nq, Nk = SHAPES[name]
    c, _ = _case(name, dname)
    seed = 12345678901234567
    keep = hip.dropout_keep_host(mh.keep_indices(B, heads, Nq, Nk), seed, p_drop)
    assert abs(float(keep.mean()) - (1 - p_drop)) < 0.05
    want = mh.model(c['q'], c['k'], c['v'], heads, grad_out=c['grad_out'], keep=keep, p_drop=p_drop)
    got, clean = abi(c, heads, dtype, p_drop=p_drop, seed=seed)
    assert clean
    check(got, want, dtype)
    other, _ = abi(c, heads, dtype, p_drop=p_drop, seed=seed + 1)
    assert not torch.equal(other['out'], got['out'])


def test_wrapper_draws_a_fresh_seed_and_its_backward_uses_it():
    hip = pkg('hipops')
    B, heads, hd, Nq, Nk = SHAPES['ragged']
    c, _ = _case('ragged', 'f32')
    a, b = op(c, heads, torch.float32, 0.5), op(c, heads, torch.float32, 0.5)
    assert a['seed'] is not None and a['seed'] != b['seed'] and not torch.equal(a['out'], b['out'])
    keep = hip.dropout_keep_host(mh.keep_indices(B, heads, Nq, Nk), a['seed'], 0.5)
    check(a, mh.model(c['q'], c['k'], c['v'], heads, grad_out=c['grad_out'], keep=keep, p_drop=0.5), torch.float32)


@pytest.mark.parametrize('p_drop', [0.1, 0.5])
def test_dropout_keep_host_agrees_with_the_device(p_drop):
    """ver_relu_dropout_forward on 4096 ones: y > 0 exactly where the host rule keeps."""
    hip = pkg('hipops')
    lib, p = hip.lib(), hip._p
    for seed in (0, 12345678901234567, 2 ** 62 - 1):
        x = torch.ones(4096, device=DEV)
        y = torch.empty_like(x)
        s = torch.tensor([seed], dtype=torch.int64, device=DEV)
        assert lib.ver_relu_dropout_forward(p(x), p(y), p(s), p_drop, 4096, 0, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert np.array_equal((y > 0).cpu().numpy(), hip.dropout_keep_host(np.arange(4096), seed, p_drop))


# ------------------------------------------------------------------------------------------ 5: reproducible
@pytest.mark.parametrize('dname', list(DTYPES))
def test_same_bits_on_every_run_and_for_every_batch_position(dname):
    dtype = DTYPES[dname]
    B, heads, hd, Nq, Nk = SHAPES['ragged']
    c, _ = _case('ragged', dname)
    first, second = op(c, heads, dtype), op(c, heads, dtype)
    alone = op({n: t[:, 1:2] for n, t in c.items()}, heads, dtype)
    for n in OUTS:
        assert torch.equal(first[n], second[n]), n
        assert torch.equal(first[n][:, 1:2], alone[n]), n


def test_empty_query_set_launches_nothing_and_leaves_zero_gradients():
    hip = pkg('hipops')
    q = torch.zeros(0, 2, 32, device=DEV, requires_grad=True)
    k, v = (torch.randn(5, 2, 32, device=DEV).requires_grad_(True) for _ in range(2))
    out = hip.mha_core(q, k, v, 4)
    assert out.shape == (0, 2, 32)
    out.sum().backward()
    assert q.grad.shape == (0, 2, 32) and k.grad.shape == (5, 2, 32)
    assert float(k.grad.abs().max()) == 0.0 and float(v.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ 6: the module
MODULES = {'small': dict(E=32, heads=4, Nq=7, B=2), 'vocc': dict(E=768, heads=8, Nq=100, B=2)}


@functools.lru_cache(maxsize=None)
def _module_case(name, lowp=False):
    """(seeded module on the CPU with dropout 0, inputs, {mode: float64 module's output and gradients}).  ``lowp``: the case
    of the runs under bf16 autocast, whose model is evaluated on the bf16-rounded inputs -- the parameters (autocast rounds
    them in front of every Linear) and the three input tensors hold bf16 values."""
    pkg()
    dec = pkg('modules.voxel_decoder')
    m = MODULES[name]
    mod = dec.MultiheadAttention(embed_dims=m['E'], num_heads=m['heads'], dropout=0.0)
    pkg('synthetic').load_seeded(mod, 91)
    quant = (lambda t: t.bfloat16().float()) if lowp else (lambda t: t)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(quant(p))
    rng = np.random.default_rng(92)
    f = lambda: quant(torch.from_numpy(rng.standard_normal((m['Nq'], m['B'], m['E'])).astype(np.float32)))
    x = dict(query=f(), query_pos=f(), grad=f())
    if lowp:        # what the q / k Linear rounds is query + query_pos: the positions are chosen so that the SUM is a bf16 value
        x['query_pos'] = quant(x['query'] + x['query_pos']) - x['query']
        assert torch.equal(quant(x['query'] + x['query_pos']), x['query'] + x['query_pos'])
    ref = copy.deepcopy(mod).double()
    want = {}
    for training in (False, True):
        ref.train(training)
        want[training] = _module_run(ref, {n: t.double() for n, t in x.items()}, False, 'cpu')
    return mod, x, want


def _module_run(mod, x, autocast, device=DEV):
    q = x['query'].to(device).requires_grad_(True)
    for p in mod.parameters():
        p.grad = None
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        out = mod(q, query_pos=x['query_pos'].to(device))
    if device == DEV:
        out.float().backward(x['grad'].to(device))
    else:                                                     # the float64 module: nothing is narrowed
        out.backward(x['grad'])
    res = dict(out=out.detach().float() if device == DEV else out.detach(), d_query=q.grad)
    res.update({'d_' + n: p.grad.clone() for n, p in mod.named_parameters()})
    return res


def _count_core_calls(monkeypatch):
    hip = pkg('hipops')
    calls = []
    for name in ('mha_core', 'mha_core_joint'):
        real = getattr(hip, name)
        monkeypatch.setattr(hip, name, lambda *a, _real=real, _name=name, **k: calls.append(_name) or _real(*a, **k))
    return calls


@pytest.mark.parametrize('autocast', [False, True])
@pytest.mark.parametrize('training', [False, True])
@pytest.mark.parametrize('name', list(MODULES))
def test_module_fused_and_unfused_against_the_float64_module(name, training, autocast, monkeypatch):
    """One MultiheadAttention (dropout 0), switch off and on, eval and training mode, fp32 and bf16 autocast: the output,
    d(query) and every parameter gradient of BOTH routes against the float64 module -- under autocast the float64 module on
    the bf16-rounded inputs (``_module_case(lowp=True)``).  Measured on an MI355X at the decoder's shape under autocast: out
    1.6e-3 fused / 2.7e-3 unfused, d(in_proj_weight), the worst tensor, 5.3e-3 / 8.2e-3; on unrounded parameters and inputs
    the UNFUSED route is at 1.05e-2 there (input rounding, which is not the arithmetic under test)."""
    mod, x, want = _module_case(name, autocast)
    plain = copy.deepcopy(mod).to(DEV).train(training)
    fused = copy.deepcopy(plain)
    fused.fused = True
    calls = _count_core_calls(monkeypatch)
    got_plain = _module_run(plain, x, autocast)
    assert not calls
    got_fused = _module_run(fused, x, autocast)
    assert calls == ['mha_core_joint']                        # query and key are one tensor: one GEMM for q and k
    assert sorted(got_fused) == sorted(want[training]) and len(got_fused) == 2 + 4
    for route, got in (('unfused', got_plain), ('fused', got_fused)):
        for n in sorted(got):
            w = want[training][n]
            assert float(w.abs().max()) > 0, n
            print(route, end=' ')
            (mh.check_bf16 if autocast else mh.check_f32)(got[n], w, n)


def test_module_deferred_residual_and_batch_first():
    mod, x, _ = _module_case('small')
    plain = copy.deepcopy(mod).to(DEV).train()
    plain.dropout_layer.p = 0.25                              # the deferred dropout is the LayerNorm's: only p travels
    fused = copy.deepcopy(plain)
    fused.fused = True
    q, pos = x['query'].to(DEV), x['query_pos'].to(DEV)
    a, b = plain(q, query_pos=pos, defer_residual=True), fused(q, query_pos=pos, defer_residual=True)
    assert type(a).__name__ == type(b).__name__ == 'PendingResidual' and a.p == b.p == 0.25
    assert b.residual is q and b.branch.is_contiguous()
    mh.check_f32(b.branch, a.branch.double().cpu(), 'branch')
    plain.batch_first = fused.batch_first = True
    plain.eval(), fused.eval()
    mh.check_f32(fused(q.transpose(0, 1), query_pos=pos.transpose(0, 1)),
                 plain(q.transpose(0, 1), query_pos=pos.transpose(0, 1)).double().cpu(), 'batch_first')
    # key given apart from the query: two Linears instead of one GEMM, the same numbers
    key = x['grad'].to(DEV)
    mh.check_f32(fused(q, key=key, value=key), plain(q, key=key, value=key).double().cpu(), 'separate key')


def test_module_refuses_what_it_cannot_fuse():
    mod, x, _ = _module_case('small')
    fused = copy.deepcopy(mod).to(DEV).eval()
    fused.fused = True
    q = x['query'].to(DEV)
    with pytest.raises(RuntimeError, match='key_padding_mask is not supported'):
        fused(q, key_padding_mask=torch.zeros(2, 7, dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError, match='attn_mask is not supported'):
        fused(q, attn_mask=torch.zeros(7, 7, dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError, match='Nq 129.*outside the supported range'):
        fused(torch.zeros(129, 2, 32, device=DEV))
    with pytest.raises(RuntimeError, match='at most 128 queries'):
        pkg('hipops').mha_core(*(torch.zeros(129, 1, 32, device=DEV) for _ in range(3)), 4)


# ------------------------------------------------------------------------------------------ 7: the head
def test_head_with_fused_decoder_self_attention(monkeypatch):
    """The vocc.py multi-task head of test_head_gpu.py with ``MultiheadAttention.fused_attention = True``: all_cls_scores and
    all_bbox_preds against the reference's own vectors (head_vocc.npz, at the tolerance test_head_gpu.py holds the unfused
    head to against them) and against the unfused head (the fp32 bound of test_head_with_fused_decoder_attention)."""
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    pkg()
    syn, dec, hip = pkg('synthetic'), pkg('modules.voxel_decoder'), pkg('hipops')
    g = golden('head_vocc')
    head = pkg('registry').build_head(cases.vocc_head_cfg()).eval()
    code_weights = head.code_weights.detach().clone()
    syn.load_seeded(head, 7)
    head.code_weights.data.copy_(code_weights)
    head = head.to(DEV)
    w2p, org = syn.camera_batch(1, seed=1)
    feats = torch.from_numpy(syn.vit_features(1, seed=0)[0]).to(DEV).unsqueeze(1)
    metas = [{'sample_idx': 'scanA_vp0', 'world2pixel': w2p[0], 'origin': org[0]}]
    assert len([m for m in head.modules() if isinstance(m, dec.MultiheadAttention)]) == 6
    calls = _count_core_calls(monkeypatch)
    with torch.no_grad():
        want = head(feats, metas)
        assert not calls
        monkeypatch.setattr(dec.MultiheadAttention, 'fused_attention', True)
        got = head(feats, metas)
    assert len(calls) == 6
    for k, gk in (('all_cls_scores', 'c3_b0_cls'), ('all_bbox_preds', 'c3_b0_bbox')):
        assert close(got[k].cpu(), g[gk], atol=2e-4, rtol=1e-4), k
        dh.check_f32(got[k], want[k].double().cpu(), k)


# ------------------------------------------------------------------------------------------ 8: capture
def _graph_step(dropout):
    pkg()
    dec = pkg('modules.voxel_decoder')
    mod = dec.MultiheadAttention(embed_dims=32, num_heads=4, dropout=dropout, fused=True)
    pkg('synthetic').load_seeded(mod, 93)
    mod = mod.to(DEV).train()
    rng = np.random.default_rng(94)
    f = lambda: torch.from_numpy(rng.standard_normal((7, 2, 32)).astype(np.float32)).to(DEV)
    query, pos, go = f().requires_grad_(True), f(), f()
    wrt = [query] + list(mod.parameters())

    def step():
        out = mod(query, query_pos=pos)
        return out, torch.autograd.grad(out, wrt, go)

    return step


@pytest.mark.parametrize('dropout', [0.0, 0.1])
def test_module_forward_and_backward_inside_one_graph(dropout):
    """Forward + backward of the fused module in one torch.cuda.graph after an eager warm-up (nothing of the warm-up step is
    kept alive).  dropout 0: both replays give the eager step's bits.  dropout 0.1: the seed is drawn on the device inside
    the graph, so two replays differ, and both are finite."""
    step = _graph_step(dropout)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grads = step()
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append([out.clone()] + [g.clone() for g in grads])
    for r in replays:
        assert all(bool(torch.isfinite(t).all()) for t in r)
    if dropout == 0.0:
        e_out, e_grads = step()
        for a, b, e in zip(replays[0], replays[1], [e_out] + list(e_grads)):
            assert torch.equal(a, b) and torch.equal(a, e)
    else:
        assert not torch.equal(replays[0][0], replays[1][0])
        assert not torch.equal(replays[0][1], replays[1][1])
