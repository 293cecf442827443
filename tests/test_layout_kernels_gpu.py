"""The data-movement kernels of the coarse-to-fine head (csrc/ver_lattice.hip, csrc/ver_layout.hip) through their hipops
wrappers, every launch form at the smallest shape that reaches it, against the element-by-element models of
layout_kernels_helper.py (test_layout_kernels_cpu.py proves that each case reaches the form it prints, and that the models
are the operations).  Copies are compared bit for bit (NaN payloads included), sums on integer data exactly; every output
starts as a sentinel, and what an operation does not own still holds it afterwards -- the models keep it there too.  The
only tolerances are the two N(0,1) scatter cases, at the bounds test_hip_ops_gpu.py already uses."""
import functools

import pytest
import torch

import layout_kernels_helper as K
from util import close, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, BF16 = torch.float32, torch.bfloat16


def _hip():
    return pkg('hipops')


def _ids(cases):
    return [c['name'] for c in cases]


def _sentinel(shape, dtype):
    return torch.full(tuple(shape), K.SENTINEL, dtype=dtype, device=DEV)


def _rows(c):
    return c['B'] * c['Zr'] * c['H'] * c['W']


@functools.lru_cache(maxsize=None)
def _lattice(name, kind):
    """(plain, the same in the case's layout) of a gather / scatter case, built once"""
    c = next(c for c in K.GATHER_CASES + K.CONST_CASES + K.STRIDE_GATHER + K.STRIDE_SCATTER if c['name'] == name)
    make = K.raw_data if kind == 'raw' else K.int_data
    plain = make((c['B'], c['Zs'], c['H'], c['W'], c['C']), c['dtype'], 17)
    return plain, K.to_layout(plain, c['layout'])


# --------------------------------------------------------------------------------------------------- gather / scatter
@pytest.mark.parametrize('case', K.GATHER_CASES + K.CONST_CASES + K.STRIDE_GATHER,
                         ids=_ids(K.GATHER_CASES + K.CONST_CASES + K.STRIDE_GATHER))
def test_lattice_gather(case):
    taps, offs, coffs, stride = K.case_geometry(case)
    plain, src = _lattice(case['name'], 'raw')
    const = K.raw_data((case['Zr'] * case['H'] * case['W'], case['nconst'], case['cw']), case['dtype'], 19) if case['nconst'] else None
    want = K.gather_ref(plain, taps, offs, stride, case['Zr'], const=const, const_offs=coffs)
    print('k_lattice_gather<%d>:' % case['layout'], K.gather_form(_rows(case), case['C'], case['dtype'], len(taps)),
          'const blocks %d x %d' % (case['nconst'], case['cw']))
    col = _sentinel(want.shape, case['dtype'])
    _hip().lattice_gather(src.to(DEV), col, taps, offs, (case['H'], case['W']), case['layout'], row_z=case['Zr'],
                          const_rows=None if const is None else const.to(DEV), const_offset=coffs or None)
    assert int((want == K.SENTINEL).sum()) >= _rows(case) * 8 * (len(taps) + 1)             # the gaps are there, and kept
    assert K.same_bits(col.cpu(), want)


SCATTER_CASES = [c for c in K.GATHER_CASES if not K.scatter_form(1, c['C'], c['dtype'])['refuse']] + K.STRIDE_SCATTER


@pytest.mark.parametrize('case', SCATTER_CASES, ids=_ids(SCATTER_CASES))
def test_lattice_scatter_on_integers(case):
    taps, offs, _, stride = K.case_geometry(case)
    B, Zr, Zs, H, W, C, layout, dtype = (case[k] for k in ('B', 'Zr', 'Zs', 'H', 'W', 'C', 'layout', 'dtype'))
    K.exact_ok(K.max_terms(taps, 1, Zr, Zs, H, W))
    gcol = K.int_data((_rows(case), stride), dtype, 23)
    want = K.to_layout(K.scatter_ref(gcol, taps, offs, B, Zr, Zs, H, W, C).to(dtype), layout)
    print('k_lattice_scatter<%s, %d>:' % (dtype, layout), K.scatter_form(B * Zs * H * W, C, dtype), '%d taps' % len(taps))
    gsrc = _sentinel(want.shape, dtype)
    _hip().lattice_scatter(gcol.to(DEV), gsrc, taps, offs, (H, W), layout, row_z=Zr)
    assert torch.equal(gsrc.cpu(), want)


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_lattice_scatter_on_normal_data(dtype):
    """N(0,1) against the fp64 adjoint at the tolerances of test_lattice_gather_scatter_with_offsets (1e-5 fp32, 4e-2 bf16)"""
    B, Zr, Zs, H, W, C, layout = 2, 2, 4, 4, 6, 24 if dtype == BF16 else 12, 3
    taps = K.TAP_LISTS['lat18']
    offs, _, stride = K.col_plan(len(taps), C, 5)
    gcol = torch.randn(B * Zr * H * W, stride, generator=torch.Generator().manual_seed(29)).to(dtype)
    want = K.to_layout(K.scatter_ref(gcol, taps, offs, B, Zr, Zs, H, W, C), layout)
    gsrc = _sentinel(want.shape, dtype)
    _hip().lattice_scatter(gcol.to(DEV), gsrc, taps, offs, (H, W), layout, row_z=Zr)
    print('k_lattice_scatter<%s, %d>:' % (dtype, layout), K.scatter_form(B * Zs * H * W, C, dtype), 'max |got - want| = %.3e'
          % float((gsrc.double().cpu() - want).abs().max()))
    assert close(gsrc.float().cpu(), want, atol=K.SCATTER_TOL[dtype], rtol=K.SCATTER_TOL[dtype])


def test_lattice_scatter_refuses_more_than_256_vectors_per_position():
    case = next(c for c in K.GATHER_CASES if c['name'] == 'cv320_f32_l2')
    taps, offs, _, stride = K.case_geometry(case)
    assert K.scatter_form(1, case['C'], case['dtype'])['refuse']
    gsrc = _sentinel(K.layout_shape(case['B'], case['Zs'], case['H'], case['W'], case['C'], case['layout']), F32)
    with pytest.raises(RuntimeError, match='256'):
        _hip().lattice_scatter(K.int_data((_rows(case), stride), F32, 1).to(DEV), gsrc, taps, offs, (case['H'], case['W']),
                               case['layout'], row_z=case['Zr'])
    assert bool((gsrc == K.SENTINEL).all())


# ---------------------------------------------------------------------------------------------------- im2col / col2im
@pytest.mark.parametrize('name', list(K.IM2COL_CASES))
def test_lattice_im2col_and_col2im(name):
    B, Z, H, W, C, dtype, taps = K.IM2COL_CASES[name]
    K.exact_ok(K.max_terms(taps, 1, Z, Z, H, W))
    plain = K.raw_data((B, Z, H, W, C), dtype, 31)
    offs = [t * C for t in range(len(taps))]
    print('k_lattice_im2col:', K.im2col_form(B * Z * H * W, len(taps), C, dtype), '%d taps' % len(taps))
    src = plain.to(DEV).requires_grad_(True)
    col = _hip().lattice_im2col(src, taps)
    assert K.same_bits(col.detach().cpu(), K.gather_ref(plain, taps, offs, len(taps) * C, Z))
    g = K.int_data(tuple(col.shape), dtype, 37)
    col.backward(g.to(DEV))
    assert src.grad.dtype == dtype
    assert torch.equal(src.grad.cpu(), K.scatter_ref(g, taps, offs, B, Z, Z, H, W, C).to(dtype))


# ---------------------------------------------------------------------------------------------------------- transpose
def _cf_buffer(B, stride, offset, dtype, fill=None):
    """a channel-first buffer [B, stride] that starts ``offset`` elements past an aligned address, inside a sentinel frame"""
    base = _sentinel((B * stride + 16,), dtype)
    cf = base[offset:offset + B * stride].view(B, stride)
    if fill is not None:
        cf.copy_(fill)
    assert cf.is_contiguous() and cf.data_ptr() % 16 == offset * K.esize(dtype)
    return base, cf


@pytest.mark.parametrize('case', K.TRANSPOSE_CASES, ids=_ids(K.TRANSPOSE_CASES))
def test_lattice_transpose(case):
    B, Z, H, W, C, dtype, off = (case[k] for k in ('B', 'Z', 'H', 'W', 'C', 'dtype', 'cf_offset'))
    stride = C * Z * H * W + case['tail']
    plain = K.raw_data((B, Z, H, W, C), dtype, 41)
    want_cf = K.channel_first_ref(plain, stride)
    for to_cf in (True, False):
        form = K.transpose_form(B, Z, H, W, C, dtype, to_cf, stride, off)
        assert form['form'] == case['want'] and (not case['R'] or not to_cf or (form['R'] == case['R'] and form['hr'] > 1))
        print('k_lattice_transpose%s, to_cf = %s:' % ('_v' if form['form'] == 'vector' else '', to_cf), form)
    for layout in K.transpose_layouts(case):
        src = K.to_layout(plain, layout)
        base, cf = _cf_buffer(B, stride, off, dtype)
        _hip().lattice_transpose(src.to(DEV), cf, (H, W), layout, True)
        assert K.same_bits(cf.cpu(), want_cf), layout                                         # (the tail's sentinel included)
        assert bool((base[:off] == K.SENTINEL).all()) and bool((base[off + B * stride:] == K.SENTINEL).all())
        base, cf = _cf_buffer(B, stride, off, dtype, want_cf.to(DEV))
        back = _sentinel(src.shape, dtype)
        _hip().lattice_transpose(back, cf, (H, W), layout, False)
        assert K.same_bits(back.cpu(), src), layout
        assert K.same_bits(cf.cpu(), want_cf)


def test_lattice_transpose_width_limit_and_empty_batch():
    hip = _hip()
    assert K.transpose_form(2, 1, 2, 128, 4, F32, True, 1024)['form'] == 'refuse'
    cl, cf = _sentinel((2, 1, 2, 128, 4), F32), _sentinel((2, 1024), F32)
    for to_cf in (True, False):
        with pytest.raises(RuntimeError, match='too wide'):
            hip.lattice_transpose(cl, cf, (2, 128), 0, to_cf)
    assert bool((cl == K.SENTINEL).all()) and bool((cf == K.SENTINEL).all())
    for to_cf in (True, False):                                                               # B = 0: no launch, no error
        hip.lattice_transpose(_sentinel((0, 1, 2, 128, 4), F32), _sentinel((0, 1024), F32), (2, 128), 0, to_cf)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------- lattice_rows
@pytest.mark.parametrize('case', K.ROWS_CASES, ids=_ids(K.ROWS_CASES))
def test_lattice_rows(case):
    hip = _hip()
    B, Z, H, W, C, rm = (case[k] for k in ('B', 'Z', 'H', 'W', 'C', 'rm'))
    plain = K.raw_data((B, Z, H, W, C), BF16, 43)
    want_rows = K.lattice_rows_ref(plain, rm)
    rows_in = K.raw_data((rm['total'],), BF16, 47)
    want_plain = K.lattice_from_rows_ref(rows_in, rm, B, Z, H, W, C)
    for to_rows in (True, False):
        print('k_lattice_rows, to_rows = %s:' % to_rows, K.rows_form(Z, H, W, C, rm, to_rows), 'quarter %d period %d'
              % (rm['quarter'], rm['period']))
    assert int((want_rows == K.SENTINEL).sum()) >= 12 * (len(rm['seg_off']) + 1)              # gaps and slack, kept
    for layout in range(4):
        src = K.to_layout(plain, layout)
        buf = _sentinel((rm['total'],), BF16)
        hip.lattice_rows(src.to(DEV), buf, rm, (H, W), layout, True)
        assert K.same_bits(buf.cpu(), want_rows), layout
        got = _sentinel(src.shape, BF16)
        hip.lattice_rows(got, rows_in.to(DEV), rm, (H, W), layout, False)
        assert K.same_bits(got.cpu(), K.to_layout(want_plain, layout)), layout


def test_lattice_rows_refusals():
    hip = _hip()

    def call(Z, H, W, C, rm, B=1, short=0):
        cl = _sentinel((B, Z, H, W, C), BF16)
        buf = _sentinel((rm['total'] - short,), BF16)
        try:
            hip.lattice_rows(cl, buf, rm, (H, W), 0, True)
        finally:
            assert bool((buf == K.SENTINEL).all())
    rm = K.make_row_map(8 * 4 * 4100, 4100, 4100, (4100,), 1)
    with pytest.raises(RuntimeError, match='4096'):
        call(4, 205, 20, 8, rm)
    rm = K.make_row_map(4096, 1024, 64, (4, 56), 2)
    assert K.row_map_refusal(rm, 4, 8, 8, 16) == 'cover'
    with pytest.raises(RuntimeError, match='cover'):
        call(4, 8, 8, 16, rm, B=2)
    rm = K.make_row_map(16 * 4 * 8 * 6, 48, 16, (16,), 2)
    with pytest.raises(RuntimeError, match='W %'):
        call(4, 8, 6, 16, rm, B=2)
    rm = K.make_row_map(4096, 1024, 64, (4, 60), 2)
    assert K.row_map_refusal(rm, 4, 8, 8, 16) is None
    with pytest.raises(ValueError, match='needed'):
        call(4, 8, 8, 16, rm, B=2, short=rm['total'] - max(rm['seg_base']) - 2 * rm['seg_rows'][0] * rm['seg_pitch'][0] + 4)


# --------------------------------------------------------------------------------------------------------- run copies
@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('name', K.RUN_CASES)
def test_run_gather_and_scatter(name, dtype):
    hip = _hip()
    c = K.run_case(name, dtype)
    total = c['B'] * c['n_rows']
    start, aug = c['run_start'].to(DEV), c['aug_idx'].to(DEV)
    image = K.raw_data((c['B'], c['image_stride']), dtype, 53)
    print('k_run_copy<gather>:', K.run_copy_form(total, c['runs'], c['run_len'], c['n_aug'], dtype, True))
    rows = _sentinel((total, c['row_elems']), dtype)
    hip.run_gather(image.to(DEV), start, aug, rows, c['n_rows'], c['run_len'])
    assert K.same_bits(rows.cpu(), K.run_gather_ref(image, c))                                 # (row padding: the sentinel)
    if not c['tiling']:
        return
    print('k_run_copy<scatter>:', K.run_copy_form(total, c['runs'], c['run_len'], 0, dtype, False))
    src = K.raw_data((total, c['row_elems']), dtype, 59)
    img = _sentinel((c['B'], c['image_stride']), dtype)
    hip.run_scatter(src.to(DEV), img, start, c['n_rows'], c['run_len'])
    assert K.same_bits(img.cpu(), K.run_scatter_ref(src, c))                                   # (image padding: the sentinel)


# -------------------------------------------------------------------------------------------- ConvTranspose3d weights
def _same_or_nan(got, want):
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(K.bits(got)[~nan], K.bits(want)[~nan])


@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('ci,co', K.PAIR_CASES)
def test_convt_weight_taps_and_adjoint(ci, co, dtype):
    hip = _hip()
    w = torch.randn(ci, co, 3, 5, 5, generator=torch.Generator().manual_seed(61))
    sp = K.weight_specials()
    w.view(-1)[5:5 + len(sp)] = sp
    w.view(-1)[-len(sp):] = sp                                                                 # (in the ragged last pair group too)
    w.view(-1)[3] = float('nan')
    print('k_convt_weight_fwd / _bwd: %d pairs = %d groups of 64, the last of %d' % (ci * co, -(-ci * co // 64), (ci * co - 1) % 64 + 1))
    wd = w.to(DEV).requires_grad_(True)
    got = hip.convt_weight_taps(wd, dtype)
    assert got.dtype == dtype and _same_or_nan(got.detach().cpu(), K.taps_ref(w, dtype))
    g = K.raw_data((75, ci, co), dtype, 67)
    got.backward(g.to(DEV))
    assert _same_or_nan(wd.grad.cpu(), K.taps_adjoint_ref(g))


@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('ci,co', K.BLOCK_CASES)
def test_convt_weight_blocks_both_ways(ci, co, dtype):
    hip = _hip()
    ld = 2 * co + 4
    off, rows = K.block_offsets_case(ci, co, ld)
    w = K.int_data((ci, co, 3, 5, 5), F32, 71)
    print('k_convt_weight_fwd_blocks / _bwd_blocks: %d pairs, groups of 128 (bf16 backward, forward) or 64' % (ci * co))
    blocks = _sentinel((rows, ld), dtype)
    hip.convt_weight_forward_blocks(w.to(DEV), off.to(DEV), blocks, ci, co)
    want = K.forward_blocks_ref(w, off, ld, torch.full((rows, ld), K.SENTINEL, dtype=dtype))
    assert int((want == K.SENTINEL).sum()) >= rows * ld - 85 * ci * co and torch.equal(blocks.cpu(), want)
    s = K.int_data((rows, ld), dtype, 73)
    pb, dv = K.int_data((ci,), dtype, 79), K.int_data((75, co), dtype, 83)
    for bias in (False, True):                                   # at most 4 + 4 + 16: exact
        got = hip.convt_weight_backward_blocks(s.to(DEV), off.to(DEV), pb.to(DEV) if bias else None, dv.to(DEV) if bias else None, ci, co)
        want = K.backward_blocks_ref(s, off, ld, ci, co, pb if bias else None, dv if bias else None)
        assert got.dtype == F32 and torch.equal(got.double().cpu(), want)


@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('ci,ncols', K.VEC_CASES)
def test_blocks_vec_both_ways(ci, ncols, dtype):
    hip = _hip()
    s, block_rows, x, gv = K.vec_case(ci, ncols, dtype)
    print('k_blocks_vec_fwd / _bwd:', K.blocks_vec_form(ci, ncols), 'block rows', block_rows.tolist())
    got = hip.blocks_vec_forward(s.to(DEV), block_rows.to(DEV), ci, x.to(DEV))
    assert got.dtype == F32 and torch.equal(got.double().cpu(), K.blocks_vec_ref(s, block_rows, ci, x))
    got = hip.blocks_vec_backward(s.to(DEV), block_rows.to(DEV), ci, gv.to(DEV))
    assert got.dtype == F32 and torch.equal(got.double().cpu(), K.blocks_vec_adjoint_ref(s, block_rows, ci, gv))
