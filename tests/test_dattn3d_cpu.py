"""ver_dattn3d_* without a GPU: the entry points exist and validate their arguments on the host, the module switch changes
nothing about parameters, and the float64 reference of tests/dattn3d_helper.py reproduces the reference project's own
vectors through the mapping the GPU tests use."""
import ctypes
import os
import re

import pytest
import torch

import cases
import dattn3d_helper as dh
from util import ROOT, golden, pkg

NAMES = ('ver_dattn3d_supported', 'ver_dattn3d_forward', 'ver_dattn3d_backward')


def _fwd(ptr, B=1, Nk=900, heads=8, hd=96, L=1, P=4, Nq=100):
    return (ptr, 0, ptr, ptr, ptr, ptr, ptr, 0, ptr, 0, B, Nk, heads, hd, L, P, Nq, None)


def _bwd(ptr, B=1, Nk=900, heads=8, hd=96, L=1, P=4, Nq=100, gref=None):
    return (ptr, 0, ptr, ptr, ptr, ptr, ptr, 0, ptr, 0, ptr, ptr, ptr, gref, B, Nk, heads, hd, L, P, Nq, None)


def test_header_declares_and_library_exports_the_entry_points():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ver_ops.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(ver_[a-z0-9_]+)\s*\(', text))
    hip = pkg('hipops')
    pkg('csrc.build').build_hip(verbose=False)
    handle = ctypes.CDLL(hip.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in hip.SYMBOLS and hasattr(handle, name), name
    assert len(hip.PROTOTYPES['ver_dattn3d_forward'][1]) == 18 and len(hip.PROTOTYPES['ver_dattn3d_backward'][1]) == 22
    assert hip.ABI_VERSION == 31 and handle.ver_abi_version() == 31          # additive: the version stays


def test_argument_validation_without_gpu():
    lib = pkg('hipops').lib()
    buf = (ctypes.c_float * 16)()
    for call, args in ((lib.ver_dattn3d_forward, _fwd), (lib.ver_dattn3d_backward, _bwd)):
        rc = call(*args(None))
        assert rc == -1 and b'null' in lib.ver_last_error()
        rc = call(*args(buf, L=3, P=11))                                     # levels * points = 33
        assert rc == -2 and b'levels * points' in lib.ver_last_error()
        assert call(*args(buf, hd=129)) == -2 and call(*args(buf, heads=65)) == -2
        assert call(*args(None, B=0)) == 0 and call(*args(None, Nq=0)) == 0   # nothing launched, no pointer looked at
        assert call(*args(buf, Nk=0)) == -1 and call(*args(buf, P=0)) == -1 and call(*args(buf, B=-1)) == -1
    rc = lib.ver_dattn3d_forward(buf, 2, buf, buf, buf, buf, buf, 0, buf, 0, 1, 900, 8, 96, 1, 4, 100, None)
    assert rc == -1 and b'dtype' in lib.ver_last_error()
    # grad_ref alone may be NULL: with every other pointer set the call gets as far as the range check
    assert lib.ver_dattn3d_backward(*_bwd(buf, L=3, P=11, gref=None)) == -2


def test_supported_range():
    hip = pkg('hipops')
    lib = hip.lib()
    assert lib.ver_dattn3d_supported(1, 900, 8, 96, 1, 4, 100) == 1          # vocc.py
    assert lib.ver_dattn3d_supported(64, 900, 8, 96, 1, 4, 128) == 1
    c = cases.MSDA3D_CASES['two_levels']
    assert lib.ver_dattn3d_supported(c['batch'], 34, c['heads'], c['head_dim'], 2, c['points'], c['num_query']) == 1
    assert lib.ver_dattn3d_supported(1, 900, 8, 128, 4, 8, 100) == 1          # levels * points = 32, head_dim = 128
    assert lib.ver_dattn3d_supported(1, 900, 8, 96, 3, 11, 100) == 0
    assert lib.ver_dattn3d_supported(1, 900, 8, 129, 1, 4, 100) == 0
    assert lib.ver_dattn3d_supported(1, 0, 8, 96, 1, 4, 100) == 0
    assert hip.voxel_deform_attn_supported(1, 900, 8, 96, 1, 4, 100) is True
    assert hip.voxel_deform_attn_supported(1, 900, 8, 96, 3, 11, 100) is False


def _module(**kw):
    pkg()
    dec = pkg('modules.voxel_decoder')
    torch.manual_seed(0)
    return dec.VoxelCustomMSDeformableAttention(embed_dims=32, num_heads=4, num_levels=1, num_points=4, **kw)


def test_module_switch_keeps_parameters_and_defaults_to_off():
    dec = pkg('modules.voxel_decoder')
    plain, fused = _module(), _module(fused=True)
    assert dec.VoxelCustomMSDeformableAttention.fused_sampling is False
    assert plain.fused is None and fused.fused is True
    assert list(plain.state_dict()) == list(fused.state_dict())
    assert [k for k, _ in plain.named_parameters()] == [k for k, _ in fused.named_parameters()]
    for k, v in plain.state_dict().items():
        assert torch.equal(v, fused.state_dict()[k]), k
    # built from a config: the registry passes the kwarg through and the config without it builds the unfused module
    cfg = dict(type='VoxelCustomMSDeformableAttention', embed_dims=32, num_heads=4, num_levels=1, num_points=4)
    reg = pkg('registry')
    assert reg.ATTENTION.get('VoxelCustomMSDeformableAttention') is dec.VoxelCustomMSDeformableAttention
    assert dec.VoxelCustomMSDeformableAttention(**{k: v for k, v in cfg.items() if k != 'type'}).fused is None


@pytest.mark.parametrize('fused', [None, True])
def test_module_raises_on_cpu_tensors(fused):
    m = _module(fused=fused)
    q = torch.zeros(5, 2, 32)
    v = torch.zeros(2 * 3 * 3, 2, 32)
    with pytest.raises(RuntimeError, match='only on the GPU'):
        m(q, value=v, reference_points=torch.rand(2, 5, 1, 3), spatial_shapes=torch.tensor([[2, 3, 3]]),
          level_start_index=torch.tensor([0]))


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_op_refuses_cpu_tensors():
    hip = pkg('hipops')
    c = dh.make_inputs(1, 1, [[1, 2, 2]], 1, 4, 2, 1)
    with pytest.raises(RuntimeError, match='GPU'):
        hip.voxel_deform_attn(c['value'], c['shapes'], c['level_start'], c['ref'], c['offsets'], c['logits'])


@pytest.mark.parametrize('name', list(cases.MSDA3D_CASES))
def test_float64_reference_reproduces_the_golden_vectors_through_the_mapping(name):
    """ref = 0, offsets = loc * (W, H, D), logits = log(w) on the operands of ``cases.msda3d_inputs``: the helper's out and
    grad_value are the reference project's own (msda3d_core_*.npz) to 1e-6, and so are grad_loc / grad_w once mapped back --
    which pins the mapping the GPU tests rely on.

    1e-6 is taken in the form of the precision contract, 1e-6 * max(1, max |reference|) per tensor: the stored vectors are
    the reference's FP32 results, and float64 without any mapping (the stored loc and w straight into the grid_sample form)
    is already 1.344e-6 away from the stored ``out`` of vocc_decoder, whose largest entry is 2.307.  Measured here, max
    |delta| through the mapping: vocc_decoder out 1.335e-6 (bound 2.307e-6), grad_value 7.51e-7; two_levels out 1.06e-7,
    grad_value 1.20e-7.  The mapping itself moves the float64 result by 4.7e-8 (the stored fp32 weights of a (query, head)
    do not add up to exactly 1, and softmax(log w) renormalises them)."""
    bound = lambda want: 1e-6 * max(1.0, float(want.abs().max()))
    g = golden('msda3d_core_' + name)
    raw = cases.msda3d_inputs(**cases.MSDA3D_CASES[name])
    c = dh.from_msda3d(raw)
    got = dh.reference(c)
    want_out, want_gv = torch.from_numpy(g['out']).double(), torch.from_numpy(g['grad_value']).double()
    assert float((got['out'] - want_out).abs().max()) <= bound(want_out)
    assert float((got['grad_value'][:, ::3] - want_gv).abs().max()) <= bound(want_gv)
    whd = dh.sizes_whd(raw['shapes'])[None, None, None, :, None, :]
    want_off = torch.from_numpy(g['grad_loc']).double() / whd
    assert float((got['grad_offsets'] - want_off).abs().max()) <= 1e-5 * max(1.0, float(want_off.abs().max()))
    w = torch.from_numpy(raw['w']).double().flatten(3)
    want_log = dh.softmax_backward(w, torch.from_numpy(g['grad_w']).double().flatten(3))
    assert float((got['grad_logits'] - want_log).abs().max()) <= 1e-5 * max(1.0, float(want_log.abs().max()))
    assert float(got['grad_ref'].abs().max()) > 0


def test_generators_keep_every_coordinate_off_the_lattice():
    for quant in (lambda t: t, lambda t: t.bfloat16().float()):
        c = dh.make_inputs(5, 2, [[2, 3, 5], [1, 2, 2]], 2, 5, 23, 3, quant=quant)
        assert dh.lattice_distance(c['shapes'], c['ref'], c['offsets']) >= dh.MIN_DIST
        loc = dh.locations(c['shapes'], c['ref'], c['offsets'])
        assert float(loc.min()) < -0.1 and float(loc.max()) > 1.1          # the samples still span [-0.2, 1.2]
        assert torch.equal(quant(c['offsets']), c['offsets'])
