"""The fragment and accumulator maps of the two GEMM bodies (csrc/ver_gemm.hip, csrc/ver_wgrad.hip) on the one MFMA shape
they run, v_mfma_f32_16x16x32_bf16 (csrc/ver_gemm_tile.h).  Needs an MI355X: run with ``-m gpu``.

* Exact arithmetic.  Operands are integers in [-4, 4] held in bf16: every product (|.| <= 16) and every fp32 partial sum
  (|.| <= 16 K < 2^24, asserted on the CPU before a launch) is exact in any summation order, so the result must EQUAL the
  fp64 product -- after the one bf16 rounding of C, and with no rounding at all for an fp32 d(weight).  A lane that reads
  another row, k-group or column, or stores an accumulator register to another element, changes integers: no tolerance.
  Shapes are the smallest that reach every path: a full 256-row tile plus 16 rows, a full column tile plus 64 ragged columns,
  K = 96 (three phases: fewer than the ring of four) and 288 (nine: the ring wraps), K slices; 309 gradient rows = 19 slabs
  of 16 (odd) + 5 rows (zero fill past M), one and two row chunks, A as a column range of a wider matrix.
* Implicit operands (B = 2, H = W = 4, C = 64, layouts 0 / 2 / 3, the 18 taps of a lattice layer -- on a 4 x 4 grid they leave
  it across every border -- and two pattern segments): bit for bit the explicit kernels on the tap matrix ver_lattice_gather
  writes, and exactly the fp64 tap matrix of test_lattice_gemm_gpu.tap_matrix_ref on integer data.
* One N(0,1) case per entry point against fp64, with the bounds of tests/test_lattice_gemm_gpu.py for the same comparison
  (REL_L2, MAX_REL for a bf16 result; _fp32_sum_bound for an fp32 weight gradient): imported, no new numbers."""
import functools

import pytest
import torch

from test_lattice_gemm_gpu import LAT_TAPS, PW2, _close_bf16, _fp32_sum_bound, tap_matrix_ref
from util import pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LAYOUTS = (0, 2, 3)
B, H, W, C = 2, 4, 4, 64
# the K axis of the implicit cases: nine taps, pattern block 1, nine taps, pattern block 0
SEGS = LAT_TAPS[:9] + [('c', 1)] + LAT_TAPS[9:] + [('c', 0)]
PLANES = [(3 * t + 1) % 2 for t in range(len(LAT_TAPS))]       # ver_gemm_nn_planes: the source lattice of every tap


def _hip():
    return pkg('hipops')


def _ints(gen, *shape):
    return torch.randint(-4, 5, shape, generator=gen).to(torch.bfloat16)


def _exact_ok(k):
    assert k * 16 < 2 ** 24, 'partial sums of %d products of magnitude <= 16 must stay exact in fp32' % k


def _round_bf16(x64):
    """fp64 integers below 2^24 -> fp32 (exact) -> bf16: the kernel's one rounding."""
    return x64.float().bfloat16()


# --------------------------------------------------------------------------------------------- shared inputs
@functools.lru_cache(maxsize=None)
def _gemm_case(kind):
    """(a [272, 288], w [288, 320], bias [320]) on the CPU; 'int': integers in [-4, 4], 'randn': N(0,1) rounded to bf16."""
    gen = torch.Generator(device='cpu').manual_seed(11)
    if kind == 'int':
        return _ints(gen, 272, 288), _ints(gen, 288, 320), torch.randint(-4, 5, (320,), generator=gen).float()
    return torch.randn(272, 288, generator=gen).bfloat16(), torch.randn(288, 320, generator=gen).bfloat16(), torch.randn(320, generator=gen)


@functools.lru_cache(maxsize=None)
def _wgrad_case(kind):
    """(wide [309, 384] whose columns 32..351 are A, g [309, 272]) on the CPU."""
    gen = torch.Generator(device='cpu').manual_seed(12)
    if kind == 'int':
        return _ints(gen, 309, 384), _ints(gen, 309, 272)
    return torch.randn(309, 384, generator=gen).bfloat16(), torch.randn(309, 272, generator=gen).bfloat16()


@functools.lru_cache(maxsize=None)
def _lattice_case(kind):
    """Two plain lattices [B, 4, H, W, C] (the second: the other plane of the planes form) and a pattern table [2 H W, 2, PW2]."""
    gen = torch.Generator(device='cpu').manual_seed(13)
    make = (lambda *s: _ints(gen, *s)) if kind == 'int' else (lambda *s: torch.randn(*s, generator=gen).bfloat16())
    return make(B, 4, H, W, C), make(B, 4, H, W, C), make(2 * H * W, 2, PW2)


def _seg_offsets(segs):
    offs, k = [], 0
    for t in segs:
        offs.append(k)
        k += PW2 if t[0] == 'c' else C
    return offs, k


def _gathered(hip, e, layout, segs, table):
    """The explicit tap matrix of ``segs`` as ver_lattice_gather writes it (pattern blocks included, in the same pass)."""
    offs, k = _seg_offsets(segs)
    a = torch.full((B * 2 * H * W, k), 7.0, dtype=torch.bfloat16, device=DEV)
    taps = [t for t in segs if t[0] != 'c']
    toffs = [o for t, o in zip(segs, offs) if t[0] != 'c']
    blocks = {t[1]: o for t, o in zip(segs, offs) if t[0] == 'c'}
    kw = dict(const_rows=table, const_offset=[blocks[i] for i in range(table.shape[1])]) if blocks else {}
    hip.lattice_gather(e, a, taps, toffs, (H, W), layout, row_z=2, **kw)
    return a


# --------------------------------------------------------------------------------------------- ver_gemm_nn, exact
@pytest.mark.parametrize('with_bias', [False, True], ids=['no bias', 'bias'])
@pytest.mark.parametrize('K', [96, 288], ids=['K 96: fewer phases than the ring', 'K 288: the ring wraps'])
def test_gemm_nn_is_exact_on_small_integers(K, with_bias):
    hip = _hip()
    a, w, bias = _gemm_case('int')
    _exact_ok(K + 1)
    ref = a[:, :K].double() @ w[:K].double() + (bias.double() if with_bias else 0.0)
    # (a: a column range of the wider matrix)
    got = hip.gemm_nn(a.to(DEV)[:, :K], w.to(DEV)[:K], bias=bias.to(DEV) if with_bias else None, splits=1)
    assert torch.equal(got.cpu(), _round_bf16(ref))


def test_gemm_nn_splitk_is_exact_on_small_integers():
    """Two K slices (160 + 128 columns) through fp32 partial tiles and k_gemm_reduce, with the bias."""
    hip = _hip()
    a, w, bias = _gemm_case('int')
    _exact_ok(a.shape[1] + 1)
    ref = a.double() @ w.double() + bias.double()
    got = hip.gemm_nn(a.to(DEV), w.to(DEV), bias=bias.to(DEV), splits=2)
    assert torch.equal(got.cpu(), _round_bf16(ref))


# --------------------------------------------------------------------------------------------- ver_wgrad_tn, exact
@pytest.mark.parametrize('splits,dtype', [(1, torch.float32), (1, torch.bfloat16), (2, torch.float32)],
                         ids=['direct store fp32', 'direct store bf16', 'two row chunks + reduce'])
def test_wgrad_tn_is_exact_on_small_integers(splits, dtype):
    hip = _hip()
    wide, g = _wgrad_case('int')
    _exact_ok(wide.shape[0])
    a = wide.to(DEV)[:, 32:352]
    ref = wide[:, 32:352].double().t() @ g.double()
    got = hip.wgrad_tn(a, g.to(DEV), out_dtype=dtype, splits=splits).cpu()
    assert tuple(got.shape) == (320, 272)
    if dtype == torch.float32:
        assert torch.equal(got.double(), ref)
    else:
        assert torch.equal(got, _round_bf16(ref))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('splits', [1, 8])
def test_wgrad_tn_without_rows_writes_zeros(splits, dtype):
    """M = 0, Ka = N = 64: no product kernel -- the launcher's tail zero-fills the ``splits`` partial tiles and the reduce
    writes the 64 x 64 result over what was there, for one chunk too (nothing is stored directly without rows)."""
    hip = _hip()
    out = torch.full((64, 64), 7.0, dtype=dtype, device=DEV)
    got = hip.wgrad_tn(torch.zeros(0, 64, dtype=torch.bfloat16, device=DEV), torch.zeros(0, 64, dtype=torch.bfloat16, device=DEV),
                       out=out, out_dtype=dtype, splits=splits)
    assert got is out and torch.equal(out, torch.zeros(64, 64, dtype=dtype, device=DEV))


# --------------------------------------------------------------------------------------------- implicit forms
@pytest.mark.parametrize('layout', LAYOUTS)
def test_implicit_forward_equals_explicit_and_fp64(layout):
    """ver_gemm_nn_segments: bit for bit ver_gemm_nn on the gathered matrix; on integers exactly the fp64 tap matrix, also with
    the position table and the bias."""
    hip, from_plain = _hip(), pkg('dense_heads._cpu_algebra').from_plain
    gen = torch.Generator(device='cpu').manual_seed(20 + layout)
    offs, k = _seg_offsets(SEGS)
    _exact_ok(k + 2)
    n = 320
    for kind in ('int', 'randn'):
        plain, _, table = _lattice_case(kind)
        e, tab = from_plain(plain, layout).to(DEV), table.to(DEV)
        w = (_ints(gen, k, n) if kind == 'int' else (torch.randn(k, n, generator=gen) * 0.05).bfloat16())
        a = _gathered(hip, e, layout, SEGS, tab)
        a_ref = tap_matrix_ref(plain, SEGS, H, W, table)
        assert torch.equal(a.cpu().double(), a_ref)
        got = hip.gemm_nn_taps(e, layout, (H, W), SEGS, w.to(DEV), const_rows=tab)
        assert torch.equal(got, hip.gemm_nn(a, w.to(DEV), splits=1)), kind
        if kind == 'int':
            assert torch.equal(got.cpu(), _round_bf16(a_ref @ w.double()))
            rowpos = torch.randint(-4, 5, (2 * H * W, n), generator=gen).float()
            bias = torch.randint(-4, 5, (n,), generator=gen).float()
            got = hip.gemm_nn_taps(e, layout, (H, W), SEGS, w.to(DEV), const_rows=tab, rowpos=rowpos.to(DEV), bias=bias.to(DEV))
            assert torch.equal(got.cpu(), _round_bf16(a_ref @ w.double() + rowpos.double().repeat(B, 1) + bias.double()))
        else:
            _close_bf16(got, a_ref @ w.double(), 'segments')


@pytest.mark.parametrize('layout', LAYOUTS)
def test_implicit_planes_equal_explicit_and_fp64(layout):
    """ver_gemm_nn_planes: tap t reads lattice PLANES[t] of two -- the explicit matrix takes block t from that lattice's
    gathered matrix."""
    hip, from_plain = _hip(), pkg('dense_heads._cpu_algebra').from_plain
    gen = torch.Generator(device='cpu').manual_seed(30 + layout)
    k, n = len(LAT_TAPS) * C, 200
    _exact_ok(k)
    for kind in ('int', 'randn'):
        p0, p1, _ = _lattice_case(kind)
        lat = torch.stack([from_plain(p0, layout), from_plain(p1, layout)]).to(DEV).contiguous()
        mats = [_gathered(hip, lat[i], layout, LAT_TAPS, None) for i in range(2)]
        refs = [tap_matrix_ref(p, LAT_TAPS, H, W) for p in (p0, p1)]
        a = torch.cat([mats[pl][:, t * C:(t + 1) * C] for t, pl in enumerate(PLANES)], 1).contiguous()
        a_ref = torch.cat([refs[pl][:, t * C:(t + 1) * C] for t, pl in enumerate(PLANES)], 1)
        w = (_ints(gen, k, n) if kind == 'int' else (torch.randn(k, n, generator=gen) * 0.05).bfloat16())
        got = hip.gemm_nn_taps(lat, layout, (H, W), LAT_TAPS, w.to(DEV), planes=PLANES)
        assert torch.equal(got, hip.gemm_nn(a, w.to(DEV), splits=1)), kind
        if kind == 'int':
            assert torch.equal(got.cpu(), _round_bf16(a_ref @ w.double()))
        else:
            _close_bf16(got, a_ref @ w.double(), 'planes')


@pytest.mark.parametrize('layout', LAYOUTS)
def test_implicit_wgrad_equals_explicit_and_fp64(layout):
    """ver_wgrad_tn_segments: bit for bit ver_wgrad_tn on the gathered matrix with one and two row chunks; on integers exactly
    the fp64 tap matrix."""
    hip, from_plain = _hip(), pkg('dense_heads._cpu_algebra').from_plain
    gen = torch.Generator(device='cpu').manual_seed(40 + layout)
    m, n = B * 2 * H * W, 272
    _exact_ok(m)
    for kind in ('int', 'randn'):
        plain, _, table = _lattice_case(kind)
        e, tab = from_plain(plain, layout).to(DEV), table.to(DEV)
        g = _ints(gen, m, n) if kind == 'int' else torch.randn(m, n, generator=gen).bfloat16()
        a = _gathered(hip, e, layout, SEGS, tab)
        a_ref = tap_matrix_ref(plain, SEGS, H, W, table)
        ref = a_ref.t() @ g.double()
        for splits in (1, 2):
            got = hip.wgrad_tn_segments(e, layout, (H, W), SEGS, g.to(DEV), out_dtype=torch.float32, const_rows=tab, splits=splits)
            assert torch.equal(got, hip.wgrad_tn(a, g.to(DEV), out_dtype=torch.float32, splits=splits)), (kind, splits)
            if kind == 'int':
                assert torch.equal(got.cpu().double(), ref), splits
            else:
                assert bool(((got.cpu().double() - ref).abs() <= _fp32_sum_bound(a_ref, g.double(), splits)).all()), splits
        got16 = hip.wgrad_tn_segments(e, layout, (H, W), SEGS, g.to(DEV), out_dtype=torch.bfloat16, const_rows=tab, splits=1)
        if kind == 'int':
            assert torch.equal(got16.cpu(), _round_bf16(ref))
        else:
            _close_bf16(got16, ref, 'segments, bf16')


# --------------------------------------------------------------------------------------------- N(0,1) against fp64
def test_gemm_nn_randn_against_fp64():
    """ver_gemm_nn and ver_gemm_nn_splitk on N(0,1) operands: REL_L2 / MAX_REL of test_lattice_gemm_gpu (one bf16 rounding of
    an fp32 sum of exact products)."""
    hip = _hip()
    a, w, bias = _gemm_case('randn')
    ref = a.double() @ w.double() + bias.double()
    for splits in (1, 2):
        _close_bf16(hip.gemm_nn(a.to(DEV), w.to(DEV), bias=bias.to(DEV), splits=splits), ref, splits)


def test_wgrad_tn_randn_against_fp64():
    """ver_wgrad_tn on N(0,1) operands: fp32 within _fp32_sum_bound element by element, bf16 within REL_L2 / MAX_REL."""
    hip = _hip()
    wide, g = _wgrad_case('randn')
    a_ref = wide[:, 32:352].double()
    ref = a_ref.t() @ g.double()
    a = wide.to(DEV)[:, 32:352]
    for splits in (1, 2):
        got = hip.wgrad_tn(a, g.to(DEV), out_dtype=torch.float32, splits=splits).cpu().double()
        assert bool(((got - ref).abs() <= _fp32_sum_bound(a_ref, g.double(), splits)).all()), splits
    _close_bf16(hip.wgrad_tn(a, g.to(DEV), out_dtype=torch.bfloat16, splits=1), ref, 'bf16')
