"""ver_mha_* without a GPU: the entry points exist and validate their arguments on the host, the float64 model of
tests/mha_helper.py is torch.nn.MultiheadAttention's arithmetic, hipops.dropout_keep_host is a fair coin of the stated rate,
and the module switch changes nothing about parameters."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mha_helper as mh
from util import ROOT, pkg

NAMES = ('ver_mha_supported', 'ver_mha_forward', 'ver_mha_backward')
SEEDS = (0, 1, 12345678901234567, 2 ** 62 - 1)


def _fwd(ptr, B=1, heads=8, hd=96, Nq=100, Nk=100, dtype=0, ld=None, seed=None, p=0.0):
    ld = heads * hd if ld is None else ld
    return (ptr, ptr, ptr, dtype, ld, ld, ld, seed, p, ptr, ptr, B, heads, hd, Nq, Nk, None)


def _bwd(ptr, B=1, heads=8, hd=96, Nq=100, Nk=100, dtype=0, ld=None, seed=None, p=0.0):
    ld = heads * hd if ld is None else ld
    return (ptr, ptr, ptr, dtype, ld, ld, ld, ptr, ptr, seed, p, ptr, ptr, ptr, ld, ld, ld, B, heads, hd, Nq, Nk, None)


def test_header_declares_and_library_exports_the_entry_points():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ver_ops.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(ver_[a-z0-9_]+)\s*\(', text))
    hip = pkg('hipops')
    pkg('csrc.build').build_hip(verbose=False)
    handle = ctypes.CDLL(hip.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in hip.SYMBOLS and name in hip.PROTOTYPES and hasattr(handle, name), name
    assert len(hip.PROTOTYPES['ver_mha_supported'][1]) == 5
    assert len(hip.PROTOTYPES['ver_mha_forward'][1]) == 17 and len(hip.PROTOTYPES['ver_mha_backward'][1]) == 23
    assert hip.ABI_VERSION == 31 and handle.ver_abi_version() == 31          # additive: the version stays


def test_argument_validation_without_gpu():
    lib = pkg('hipops').lib()
    buf = (ctypes.c_float * 16)()
    for call, args in ((lib.ver_mha_forward, _fwd), (lib.ver_mha_backward, _bwd)):
        assert call(*args(None)) == -1 and b'null' in lib.ver_last_error()
        assert call(*args(buf, dtype=2)) == -1 and b'dtype' in lib.ver_last_error()
        assert call(*args(buf, Nq=129)) == -2 and b'at most 128 queries' in lib.ver_last_error()
        assert call(*args(buf, Nk=129)) == -2 and b'128 keys' in lib.ver_last_error()
        assert call(*args(buf, hd=136)) == -2 and b'multiple of 8 up to 128' in lib.ver_last_error()
        assert call(*args(buf, hd=12)) == -2 and b'multiple of 8' in lib.ver_last_error()
        assert call(*args(buf, heads=1, hd=96, ld=100)) == -2 and b'pitch 100' in lib.ver_last_error()
        assert call(*args(buf, heads=2, hd=96, ld=96)) == -2 and b'at least heads * head_dim = 192' in lib.ver_last_error()
        assert call(*args(buf, p=1.0)) == -2 and b'dropout' in lib.ver_last_error()
        assert call(*args(None, B=0)) == 0 and call(*args(None, Nq=0)) == 0     # nothing launched, no pointer looked at
        assert call(*args(None, Nq=0, Nk=0)) == 0
        assert call(*args(buf, Nk=0)) == -1 and call(*args(buf, B=-1)) == -1
        # a NULL seed is fine without dropout (the call gets as far as the range check) and an error with it
        assert call(*args(buf, Nq=129, seed=None, p=0.0)) == -2
        assert call(*args(buf, Nq=129, seed=None, p=0.1)) == -1 and b'null' in lib.ver_last_error()
        assert call(*args(buf, Nq=129, seed=buf, p=0.1)) == -2


def test_supported_range():
    hip = pkg('hipops')
    lib = hip.lib()
    for shape in ((1, 8, 96, 100, 100), (64, 8, 96, 110, 110), (1, 4, 8, 7, 7), (1, 8, 128, 128, 128)):
        assert lib.ver_mha_supported(*shape) == 1, shape
        assert hip.mha_supported(*shape) is True
    for shape in ((1, 8, 96, 129, 100), (1, 8, 96, 100, 129), (1, 8, 136, 100, 100), (1, 8, 12, 100, 100), (1, 8, 96, 0, 100)):
        assert lib.ver_mha_supported(*shape) == 0, shape
        assert hip.mha_supported(*shape) is False


# ------------------------------------------------------------------------------------------ the model
def _torch_mha(with_pos, seed=5, E=32, heads=4, Nq=7, B=2):
    """nn.MultiheadAttention in float64, eval mode, and the decomposition the fused module runs: (module output, autograd
    gradients of the attention's q, k, v inputs) against (out_proj(model out), the in-projections' backward of the model's
    gradients)."""
    torch.manual_seed(seed)
    attn = torch.nn.MultiheadAttention(E, heads, dropout=0.1).double().eval()
    with torch.no_grad():
        attn.in_proj_bias.normal_()
        attn.out_proj.bias.normal_()
    x, pos, grad = (torch.randn(Nq, B, E, dtype=torch.float64) for _ in range(3))
    qin = (x + pos if with_pos else x.clone()).requires_grad_(True)
    kin = (x + pos if with_pos else x.clone()).requires_grad_(True)
    vin = x.clone().requires_grad_(True)
    out = attn(qin, kin, vin)[0]
    out.backward(grad)
    return attn, (qin, kin, vin), grad, out.detach()


@pytest.mark.parametrize('with_pos', [False, True])
def test_model_equals_torch_multihead_attention_in_float64(with_pos):
    attn, (qin, kin, vin), grad, want = _torch_mha(with_pos)
    E = 32
    w, b = attn.in_proj_weight.detach(), attn.in_proj_bias.detach()
    lin = lambda x, lo, hi: x.detach() @ w[lo:hi].T + b[lo:hi]
    q, k, v = lin(qin, 0, E), lin(kin, E, 2 * E), lin(vin, 2 * E, 3 * E)
    d_core = grad @ attn.out_proj.weight.detach()                      # gradient of the attention output
    m = mh.model(q, k, v, 4, grad_out=d_core)
    out = m['out'] @ attn.out_proj.weight.detach().T + attn.out_proj.bias.detach()
    err = dict(out=float((out - want).abs().max()),
               d_q=float((m['grad_q'] @ w[:E] - qin.grad).abs().max()),
               d_k=float((m['grad_k'] @ w[E:2 * E] - kin.grad).abs().max()),
               d_v=float((m['grad_v'] @ w[2 * E:] - vin.grad).abs().max()))
    print(err)
    for key, e in err.items():
        assert e <= 1e-12, (key, e)
    # lse is what it says
    s = torch.einsum('ibhd,jbhd->bhij', q.view(7, 2, 4, 8), k.view(7, 2, 4, 8)) / np.sqrt(8.0)
    assert float((m['lse'] - s.logsumexp(-1)).abs().max()) <= 1e-12


def test_model_with_a_mask_equals_torch_with_the_probabilities_scaled_by_hand():
    heads, hd, Nq, Nk, B, p = 4, 8, 7, 9, 2, 0.25
    c = mh.make_inputs(3, B, heads, hd, Nq, Nk)
    keep = np.random.default_rng(4).random((B, heads, Nq, Nk)) < 0.75
    q, k, v = (c[n].clone().requires_grad_(True) for n in ('q', 'k', 'v'))
    split = lambda t: t.view(t.shape[0], B, heads, hd).permute(1, 2, 0, 3)
    P = (split(q) @ split(k).transpose(-1, -2) / np.sqrt(hd)).softmax(-1)
    out = ((P * torch.from_numpy(keep).double() / (1 - p)) @ split(v)).permute(2, 0, 1, 3).reshape(Nq, B, heads * hd)
    out.backward(c['grad_out'])
    m = mh.model(c['q'], c['k'], c['v'], heads, grad_out=c['grad_out'], keep=keep, p_drop=p)
    for got, want in ((m['out'], out.detach()), (m['grad_q'], q.grad), (m['grad_k'], k.grad), (m['grad_v'], v.grad)):
        assert float((got - want).abs().max()) <= 1e-12
    assert float((m['out'] - mh.model(c['q'], c['k'], c['v'], heads)['out']).abs().max()) > 1e-3      # the mask matters


# ------------------------------------------------------------------------------------------ the keep rule
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('seed', SEEDS)
def test_dropout_keep_host_is_a_fair_coin(seed, p):
    """Over the 2*8*100*100*8 = 1.28 M consecutive indices of eight vocc-shaped calls the kept fraction is within 4 standard
    deviations sqrt(p (1 - p) / n) of 1 - p."""
    hip = pkg('hipops')
    n = 2 * 8 * 100 * 100 * 8
    keep = hip.dropout_keep_host(np.arange(n), seed, p)
    assert keep.dtype == np.bool_ and keep.shape == (n,)
    frac, sd = float(keep.mean()), float(np.sqrt(p * (1 - p) / n))
    print('seed %d p %.1f: kept %.6f, (kept - (1 - p)) / sd = %+.2f' % (seed, p, frac, (frac - (1 - p)) / sd))
    assert abs(frac - (1 - p)) <= 4 * sd


def test_dropout_keep_host_seeds_and_the_zero_rate():
    hip = pkg('hipops')
    idx = np.arange(4096)
    a, b = hip.dropout_keep_host(idx, 1, 0.5), hip.dropout_keep_host(idx, 2, 0.5)
    assert 1024 < int((a != b).sum()) < 3072                      # two seeds: about half of the decisions differ
    assert hip.dropout_keep_host(idx, 12345, 0.0).all()
    assert hip.dropout_keep_host(idx.reshape(2, 4, 16, 32), 1, 0.5).shape == (2, 4, 16, 32)
    assert np.array_equal(hip.dropout_keep_host(idx.reshape(2, 4, 16, 32), 1, 0.5).ravel(), a)


# ------------------------------------------------------------------------------------------ the module switch
def _module(**kw):
    pkg()
    dec = pkg('modules.voxel_decoder')
    torch.manual_seed(0)
    return dec.MultiheadAttention(embed_dims=32, num_heads=4, dropout=0.1, **kw)


def test_module_switch_keeps_parameters_and_defaults_to_off():
    dec = pkg('modules.voxel_decoder')
    plain, fused = _module(), _module(fused=True)
    assert dec.MultiheadAttention.fused_attention is False
    assert plain.fused is None and fused.fused is True
    assert list(plain.state_dict()) == list(fused.state_dict())
    assert 'attn.in_proj_weight' in plain.state_dict() and 'attn.out_proj.bias' in plain.state_dict()
    for k, v in plain.state_dict().items():
        assert torch.equal(v, fused.state_dict()[k]), k
    # ``fused`` does not reach nn.MultiheadAttention (which would refuse the keyword), and other keywords still do
    assert isinstance(fused.attn, torch.nn.MultiheadAttention) and not hasattr(fused.attn, 'fused')
    assert _module(fused=True, add_zero_attn=True).attn.add_zero_attn is True
    cfg = dict(type='MultiheadAttention', embed_dims=32, num_heads=4, dropout=0.1, fused=True)
    assert pkg('registry').ATTENTION.get('MultiheadAttention') is not None
    assert dec.MultiheadAttention(**{k: v for k, v in cfg.items() if k != 'type'}).fused is True


def test_unfused_module_on_cpu_is_unchanged_and_fused_raises():
    plain, fused = _module().eval(), _module(fused=True).eval()
    torch.manual_seed(1)
    x, pos = torch.randn(7, 2, 32), torch.randn(7, 2, 32)
    want = x + plain.attn(x + pos, x + pos, x)[0]
    assert torch.equal(plain(x, query_pos=pos), want)
    with pytest.raises(RuntimeError, match='only on the GPU'):
        fused(x, query_pos=pos)


def test_op_refuses_cpu_tensors():
    hip = pkg('hipops')
    c = mh.make_inputs(1, 1, 2, 8, 3, 3)
    with pytest.raises(RuntimeError, match='GPU'):
        hip.mha_core(c['q'].float(), c['k'].float(), c['v'].float(), 2)
