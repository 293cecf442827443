"""ver_dattn3d_forward / _backward (hipops.voxel_deform_attn) on the GPU against the float64 reference of
tests/dattn3d_helper.py, the reference project's vectors, the present softmax + arithmetic + voxel_msda chain, and through
``VoxelCustomMSDeformableAttention(fused=True)`` up to the head.  ``-m gpu``.

Tolerances (README, "Precision contract"): an f32 output max |delta| <= 1e-4 * max(1, max |reference|) per tensor; an output
stored as bf16 one bf16 rounding more, 2^-8 * |reference| elementwise; module-level runs under bf16 autocast relative L2 <=
1e-2.  Every generated case keeps its sampling coordinates >= 1e-3 away from the lattice (dattn3d_helper)."""
import copy
import functools
import warnings

import numpy as np
import pytest
import torch

import cases
import dattn3d_helper as dh
from util import golden, pkg, rel_l2

warnings.filterwarnings('ignore')
pytestmark = pytest.mark.gpu
DEV = 'cuda'
GRADS = ('grad_value', 'grad_offsets', 'grad_logits', 'grad_ref')

SMALL = dict(seed=61, batch=2, shapes=[[2, 3, 5], [1, 2, 2]], heads=2, head_dim=5, num_query=23, points=3)
WIDE = dict(seed=62, batch=2, shapes=[[4, 15, 15]], heads=8, head_dim=96, num_query=100, points=4)


@functools.lru_cache(maxsize=None)
def _case(name):
    c = dh.make_inputs(**dict(SMALL=SMALL, WIDE=WIDE)[name])
    assert dh.lattice_distance(c['shapes'], c['ref'], c['offsets']) >= dh.MIN_DIST
    return c, dh.reference(c)


def run(c, ref_grad=True, out_dtype=None, dtype=None, backward=True):
    """The op on the operands ``c`` (moved to the GPU; ``dtype``: value / offsets / logits cast to it) -> dict like
    ``dh.reference``."""
    hip = pkg('hipops')
    cast = (lambda t: t.to(dtype)) if dtype is not None else (lambda t: t.float())
    value = cast(c['value']).to(DEV).requires_grad_(True)
    offsets = cast(c['offsets']).to(DEV).requires_grad_(True)
    logits = cast(c['logits']).to(DEV).requires_grad_(True)
    ref = c['ref'].float().to(DEV).requires_grad_(ref_grad)
    out = hip.voxel_deform_attn(value, c['shapes'].to(DEV), c['level_start'].to(DEV), ref, offsets, logits,
                                **({} if out_dtype is None else dict(out_dtype=out_dtype)))
    res = dict(out=out.detach())
    if backward:
        out.backward(c['grad_out'].to(DEV).to(out.dtype))
        res.update(grad_value=value.grad, grad_offsets=offsets.grad, grad_logits=logits.grad, grad_ref=ref.grad)
    torch.cuda.synchronize()
    return res


def check_all_f32(got, want):
    for k in ('out',) + GRADS:
        assert got[k].dtype == torch.float32 and got[k].shape == want[k].shape, k
        dh.check_f32(got[k], want[k], k)


# ------------------------------------------------------------------------------------------ 1, 2: against float64
@pytest.mark.parametrize('name', ['SMALL', 'WIDE'])
def test_fp32_against_the_float64_reference(name):
    """1 (two levels, head_dim 5, 23 queries, 3 points: every index is exercised) and 2 (the decoder's head_dim 96 / 8 heads /
    4 points on the 4 x 15 x 15 volume): out and the four gradients."""
    c, want = _case(name)
    check_all_f32(run(c), want)


# ------------------------------------------------------------------------------------------ 3: the reference's vectors
@pytest.mark.parametrize('name', list(cases.MSDA3D_CASES))
def test_reference_vectors_through_the_mapping(name):
    """msda3d_core_*.npz with ref = 0, offsets = loc * (W, H, D), logits = log(w) (pinned on the CPU by
    test_dattn3d_cpu.py): grad_loc maps to grad_offsets by the division, grad_w to grad_logits by the softmax backward in
    float64.  These operands are fixed, so they cannot be moved off the lattice: their closest coordinate is 2.7e-5 away
    from an integer, and the kernel's fp32 coordinate (three roundings at |pixel| < 32, ulp 1.9e-6, after the rounding of
    the offset itself) is within 4e-6 of the float64 one -- the condition asserted here is 1e-5."""
    g = golden('msda3d_core_' + name)
    raw = cases.msda3d_inputs(**cases.MSDA3D_CASES[name])
    c = dh.from_msda3d(raw)
    c = dict(c, offsets=c['offsets'].float(), logits=c['logits'].float(), ref=c['ref'].float())
    assert dh.lattice_distance(c['shapes'], c['ref'], c['offsets']) >= 1e-5
    got = run(c)
    T = lambda a: torch.from_numpy(a).double()
    dh.check_f32(got['out'], T(g['out']), 'out')
    dh.check_f32(got['grad_value'][:, ::3], T(g['grad_value']), 'grad_value')
    dh.check_f32(got['grad_offsets'], T(g['grad_loc']) / dh.sizes_whd(raw['shapes'])[None, None, None, :, None, :], 'grad_offsets')
    dh.check_f32(got['grad_logits'], dh.softmax_backward(T(raw['w']).flatten(3), T(g['grad_w']).flatten(3)), 'grad_logits')


# ------------------------------------------------------------------------------------------ 4: the present chain
def _chain(c, dtype=torch.float32):
    """softmax + location arithmetic in torch + voxel_msda, as VoxelCustomMSDeformableAttention.forward runs them."""
    hip = pkg('hipops')
    value = c['value'].to(DEV).requires_grad_(True)
    offsets = c['offsets'].float().to(DEV).requires_grad_(True)
    logits = c['logits'].float().to(DEV).requires_grad_(True)
    ref = c['ref'].float().to(DEV).requires_grad_(True)
    b, nq, heads, nlev, npt, _ = offsets.shape
    w = logits.softmax(-1).view(b, nq, heads, nlev, npt)
    normalizer = dh.sizes_whd(c['shapes'], torch.float32).to(DEV)
    loc = ref[:, :, None, :, None, :] + offsets / normalizer[None, None, None, :, None, :]
    out = hip.voxel_msda(value, c['shapes'].to(DEV), c['level_start'].to(DEV), loc, w)
    out.backward(c['grad_out'].to(DEV))
    return dict(out=out.detach(), grad_value=value.grad, grad_offsets=offsets.grad, grad_logits=logits.grad, grad_ref=ref.grad)


@pytest.mark.parametrize('name', ['SMALL', 'WIDE'])
def test_equals_the_present_chain(name):
    c, _ = _case(name)
    got, chain = run(c), _chain(c)
    for k in ('out',) + GRADS:
        dh.check_f32(got[k], chain[k].double().cpu(), k)


# ------------------------------------------------------------------------------------------ 5: bf16 operands
@pytest.mark.parametrize('out_dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('name', ['SMALL', 'WIDE'])
def test_bf16_operands(name, out_dtype):
    """bf16 value / offsets / logits as they are, out in f32 and in bf16, against float64 of the widened operands.  What is
    stored as bf16 (grad_value, grad_offsets, grad_logits; out when asked for) gets the one extra rounding, grad_ref is f32."""
    bf = lambda t: t.bfloat16().float()
    c = dh.make_inputs(**dict(dict(SMALL=SMALL, WIDE=WIDE)[name], quant=bf))
    c['grad_out'] = bf(c['grad_out'])
    assert dh.lattice_distance(c['shapes'], c['ref'], c['offsets']) >= dh.MIN_DIST
    want = dh.reference(c)
    got = run(c, dtype=torch.bfloat16, out_dtype=out_dtype)
    assert got['out'].dtype == out_dtype
    (dh.check_f32 if out_dtype == torch.float32 else dh.check_bf16_stored)(got['out'], want['out'], 'out')
    for k in ('grad_value', 'grad_offsets', 'grad_logits'):
        assert got[k].dtype == torch.bfloat16, k
        dh.check_bf16_stored(got[k], want[k], k)
    assert got['grad_ref'].dtype == torch.float32
    dh.check_f32(got['grad_ref'], want['grad_ref'], 'grad_ref')
    # value in bf16 with out left alone: out comes back in value's dtype
    assert run(c, dtype=torch.bfloat16, backward=False)['out'].dtype == torch.bfloat16


# ------------------------------------------------------------------------------------------ 6: reproducible
def _crowded():
    """The shape of WIDE with every sample inside ONE cell of the 4 x 15 x 15 volume: pixel (x, y) in (7.1, 7.9), z in
    (1.1, 1.9) -- all 2 x 8 x 400 samples of a (batch, head) land on the same 8 keys."""
    c = dh.make_inputs(**WIDE)
    rng = np.random.default_rng(63)
    shape = tuple(c['offsets'].shape[:-1])
    xy = rng.uniform(0.1, 0.9, shape + (2,))
    z = rng.uniform(-0.4, 0.4, shape + (1,))
    c['offsets'] = torch.from_numpy(np.concatenate([xy, z], -1).astype(np.float32))
    c['ref'] = torch.full_like(c['ref'], 0.5)
    return c


def test_gradients_and_output_are_reproducible_under_the_worst_contention():
    c = _crowded()
    assert dh.lattice_distance(c['shapes'], c['ref'], c['offsets']) >= dh.MIN_DIST
    first, second = run(c), run(c)
    for k in ('out',) + GRADS:
        assert torch.equal(first[k], second[k]), k
    touched = (first['grad_value'][0, :, 0].abs().sum(-1) > 0).sum()
    assert int(touched) == 8
    check_all_f32(first, dh.reference(c))


# ------------------------------------------------------------------------------------------ 7: no pre-zeroing
def test_c_abi_writes_every_output_in_full():
    """Through the C ABI with every output buffer full of NaN: finite, and bit for bit what the wrapper returns."""
    hip = pkg('hipops')
    lib = hip.lib()
    c, _ = _case('SMALL')
    want = run(c)
    dev = lambda t, dt=torch.float32: t.to(dt).to(DEV).contiguous()
    value, ref, offsets, logits, go = (dev(c[k]) for k in ('value', 'ref', 'offsets', 'logits', 'grad_out'))
    shapes, lsi = dev(c['shapes'], torch.int64), dev(c['level_start'], torch.int64)
    b, nk, heads, hd = value.shape
    _, nq, _, nlev, npt, _ = offsets.shape
    nan = lambda like: torch.full_like(like, float('nan'))
    out, gv, goff, glog, gref = nan(go), nan(value), nan(offsets), nan(logits), nan(ref)
    p, stream = hip._p, torch.cuda.current_stream().cuda_stream
    dims = (b, nk, heads, hd, nlev, npt, nq, stream)
    assert lib.ver_dattn3d_forward(p(value), 0, p(shapes), p(lsi), p(ref), p(offsets), p(logits), 0, p(out), 0, *dims) == 0
    assert lib.ver_dattn3d_backward(p(value), 0, p(shapes), p(lsi), p(ref), p(offsets), p(logits), 0, p(go), 0, p(gv),
                                    p(goff), p(glog), p(gref), *dims) == 0
    torch.cuda.synchronize()
    for k, t in (('out', out), ('grad_value', gv), ('grad_offsets', goff), ('grad_logits', glog), ('grad_ref', gref)):
        assert bool(torch.isfinite(t).all()), k
        assert torch.equal(t, want[k]), k


# ------------------------------------------------------------------------------------------ 8: edges
def test_every_sample_outside_the_volume():
    c = dict(_case('SMALL')[0])
    c['offsets'] = torch.full_like(c['offsets'], 40.0)            # loc >= 8: far outside on every axis
    got = run(c)
    for k in ('out', 'grad_value', 'grad_offsets', 'grad_ref'):
        assert float(got[k].abs().max()) == 0.0, k
    assert float(got['grad_logits'].abs().max()) == 0.0           # d(weights) is 0, and so is its softmax backward


def test_one_level_one_point_has_no_logit_gradient():
    c = dh.make_inputs(64, 2, [[2, 3, 4]], 2, 8, 9, 1)
    want = dh.reference(c)
    got = run(c)
    assert float(got['grad_logits'].abs().max()) == 0.0           # softmax of one logit is 1 whatever the logit is
    check_all_f32(got, want)


def test_extreme_logits():
    c = dict(_case('SMALL')[0])
    rng = np.random.default_rng(65)
    c['logits'] = torch.from_numpy(rng.choice([-80.0, 80.0], size=tuple(c['logits'].shape)).astype(np.float32))
    got = run(c)
    for k in ('out',) + GRADS:
        assert bool(torch.isfinite(got[k]).all()), k
    check_all_f32(got, dh.reference(c))


def test_single_query():
    c = dh.make_inputs(66, 1, [[2, 3, 5], [1, 2, 2]], 2, 5, 1, 3)
    check_all_f32(run(c), dh.reference(c))


def test_reference_points_without_gradient():
    c, want = _case('SMALL')
    with_ref, without = run(c), run(c, ref_grad=False)
    assert without['grad_ref'] is None
    for k in ('out', 'grad_value', 'grad_offsets', 'grad_logits'):
        assert torch.equal(with_ref[k], without[k]), k


def test_more_keys_than_one_tile_and_more_queries_than_one_chunk():
    """The backward's key tiles (64 keys per workgroup, 16 per wave) and query chunks (30 KiB of samples and grad_out rows):
    909 keys = 14 full tiles + 13 keys, and levels * points = 32 at head_dim 128 allows 12 queries per chunk, so 29 queries
    take three chunks (10 + 10 + 9), the last one short."""
    c = dh.make_inputs(67, 1, [[3, 7, 9], [2, 5, 6], [1, 3, 4], [9, 8, 9]], 3, 128, 29, 8)
    assert c['value'].shape[1] == 909 and c['logits'].shape[-1] == 32
    check_all_f32(run(c), dh.reference(c))


def test_unsupported_shape_raises_with_the_library_message():
    c = dh.make_inputs(68, 1, [[1, 2, 2]] * 3, 1, 4, 2, 11)        # levels * points = 33
    with pytest.raises(RuntimeError, match='levels \\* points > 32'):
        run(c, backward=False)


# ------------------------------------------------------------------------------------------ 9: the module
MODULE_SHAPE = [[2, 5, 6]]


def _modules(seed=81):
    """(the seeded fill, with sampling_offsets scaled so that 3/4 of the samples fall inside the volume; the seed is one
    whose sampling coordinates keep MIN_DIST from the lattice, which the test asserts)"""
    pkg()
    dec = pkg('modules.voxel_decoder')
    plain = dec.VoxelCustomMSDeformableAttention(embed_dims=64, num_heads=4, num_levels=1, num_points=4, dropout=0.1).eval()
    pkg('synthetic').load_seeded(plain, seed)
    with torch.no_grad():
        plain.sampling_offsets.weight.mul_(0.125)
        plain.sampling_offsets.bias.mul_(0.125)
    fused = copy.deepcopy(plain)
    fused.fused = True
    return plain.to(DEV), fused.to(DEV)


def _module_inputs(seed=72, nq=7, bs=2):
    rng = np.random.default_rng(seed)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    return dict(query=f(nq, bs, 64), query_pos=f(nq, bs, 64), value=f(60, bs, 64),
                ref=torch.from_numpy(rng.uniform(0, 1, (bs, nq, 1, 3)).astype(np.float32)), grad=f(nq, bs, 64))


def _module_run(m, x, autocast):
    q, v, r = (x[k].to(DEV).requires_grad_(True) for k in ('query', 'value', 'ref'))
    for p in m.parameters():
        p.grad = None
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        out = m(q, value=v, query_pos=x['query_pos'].to(DEV), reference_points=r,
                spatial_shapes=torch.tensor(MODULE_SHAPE, device=DEV), level_start_index=torch.tensor([0], device=DEV))
    out.float().backward(x['grad'].to(DEV))
    res = dict(out=out.detach().float(), d_query=q.grad, d_value=v.grad, d_ref=r.grad)
    res.update({'d_' + k: p.grad.clone() for k, p in m.named_parameters()})
    return res


@pytest.mark.parametrize('autocast', [False, True])
def test_module_fused_equals_unfused(autocast):
    """One VoxelCustomMSDeformableAttention, fused off and on, eval mode: the output, d(query), d(value),
    d(reference_points) and every parameter gradient.  fp32: the fp32 bound against the unfused module; bf16 autocast:
    relative L2 <= 1e-2.  The sampling coordinates of these operands (from the module's own sampling_offsets Linear, in
    float64) are asserted off the lattice like those of the generated cases."""
    plain, fused = _modules()
    x = _module_inputs()
    with torch.no_grad():
        off = copy.deepcopy(plain.sampling_offsets).cpu().double()((x['query'] + x['query_pos']).permute(1, 0, 2).double())
    assert dh.lattice_distance(MODULE_SHAPE, x['ref'], off.view(2, 7, 4, 1, 4, 3)) >= dh.MIN_DIST
    want, got = _module_run(plain, x, autocast), _module_run(fused, x, autocast)
    assert sorted(got) == sorted(want) and len(want) == 4 + 8
    for k in sorted(want):
        assert float(want[k].abs().max()) > 0, k
        if autocast:
            r = rel_l2(got[k], want[k])
            print('%-28s rel L2 %.3e' % (k, r))
            assert r <= 1e-2, (k, r)
        else:
            dh.check_f32(got[k], want[k].double().cpu(), k)


def test_class_attribute_is_what_none_resolves_to(monkeypatch):
    plain, _ = _modules()
    x = _module_inputs()
    calls = []
    hip = pkg('hipops')
    real = hip.voxel_deform_attn
    monkeypatch.setattr(hip, 'voxel_deform_attn', lambda *a, **k: calls.append(1) or real(*a, **k))
    _module_run(plain, x, False)
    assert not calls
    monkeypatch.setattr(type(plain), 'fused_sampling', True)
    _module_run(plain, x, False)
    assert len(calls) == 1
    plain.fused = False                                            # the instance's word beats the class's
    _module_run(plain, x, False)
    assert len(calls) == 1


# ------------------------------------------------------------------------------------------ 10: the head
def test_head_with_fused_decoder_attention():
    """The vocc.py multi-task head of test_head_gpu.py with the six decoder cross-attentions switched to fused:
    all_cls_scores and all_bbox_preds against the unfused head, fp32 bound."""
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    pkg()
    syn, dec = pkg('synthetic'), pkg('modules.voxel_decoder')
    head = pkg('registry').build_head(cases.vocc_head_cfg()).eval()
    code_weights = head.code_weights.detach().clone()
    syn.load_seeded(head, 7)
    head.code_weights.data.copy_(code_weights)
    head = head.to(DEV)
    w2p, org = syn.camera_batch(1, seed=1)
    feats = torch.from_numpy(syn.vit_features(1, seed=0)[0]).to(DEV).unsqueeze(1)
    metas = [{'sample_idx': 'scanA_vp0', 'world2pixel': w2p[0], 'origin': org[0]}]
    attn = [m for m in head.modules() if isinstance(m, dec.VoxelCustomMSDeformableAttention)]
    assert len(attn) == 6
    with torch.no_grad():
        want = head(feats, metas)
        for m in attn:
            m.fused = True
        got = head(feats, metas)
    for k in ('all_cls_scores', 'all_bbox_preds'):
        dh.check_f32(got[k], want[k].double().cpu(), k)


# ------------------------------------------------------------------------------------------ 11: capture
def test_forward_and_backward_inside_one_graph():
    """Forward + backward of the op from static inputs in one torch.cuda.graph after an eager warm-up; replayed with other
    inputs, the static outputs are what an eager call on those inputs gives, bit for bit (nothing in the op depends on what
    its buffers held)."""
    hip = pkg('hipops')
    a, b = dh.make_inputs(81, 2, [[2, 3, 5], [1, 2, 2]], 2, 5, 23, 3), dh.make_inputs(82, 2, [[2, 3, 5], [1, 2, 2]], 2, 5, 23, 3)
    shapes, lsi = a['shapes'].to(DEV), a['level_start'].to(DEV)
    names = ('value', 'ref', 'offsets', 'logits')
    static = {k: a[k].to(DEV).requires_grad_(True) for k in names}
    go = a['grad_out'].to(DEV)

    def step():
        out = hip.voxel_deform_attn(static['value'], shapes, lsi, static['ref'], static['offsets'], static['logits'])
        return out, torch.autograd.grad(out, [static[k] for k in names], go)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grads = step()
    with torch.no_grad():
        for k in names:
            static[k].copy_(b[k].to(DEV))
        go.copy_(b['grad_out'].to(DEV))
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    want = run(b)
    assert torch.equal(out, want['out'])
    for g, k in zip(grads, ('grad_value', 'grad_ref', 'grad_offsets', 'grad_logits')):
        assert torch.equal(g, want[k]), k
    check_all_f32(want, dh.reference(b))
