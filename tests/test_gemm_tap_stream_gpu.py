"""The tap stream of the implicit-operand GEMMs (csrc/ver_gemm.hip: ver_gemm_nn_segments, ver_gemm_nn_planes) where a segment
descriptor is fetched one segment ahead.  Needs an MI355X: run with ``-m gpu``.

The kernel walks the K axis segment by segment; the descriptor of segment t + 1 is requested when segment t begins, the two
requests of the prologue follow each other directly, and the look-ahead stops at the last table entry.  The cases put a
segment switch at each of those places:

* one-phase segments -- pattern width 32 = one phase: K starts with two pattern segments (both prologue requests switch), has
  two more back to back in the middle and ends on one;
* 64 segments, the table's limit (the 18 lattice taps repeated, pattern blocks in between): the last descriptor is entry 63;
* the planes form with three source planes, another plane at every tap -- the first tap of K and the tap right behind a
  pattern segment included;
* one N(0,1) run per entry point.

Shape: B = 3, H = 6, W = 8 (P = 96 rows per viewpoint, M = 288: one full 256-row tile that crosses two viewpoint borders and a
32-row tile with 224 rows past M), C = 64, N = 320 (a full column tile + 64), layouts 0 / 2 / 3.  Data are integers in [-4, 4]
as in test_gemm_mfma_shape_gpu.py: every product and every fp32 partial sum (|.| <= 16 K < 2^24, asserted before a launch) is
exact, so the result EQUALS the fp64 product after its one bf16 rounding -- with the position table and the bias too -- and is
bit for bit ver_gemm_nn on the explicit operand, which is built from test_lattice_gemm_gpu.tap_matrix_ref (the gather kernel
does not take every pattern width)."""
import functools

import pytest
import torch

from test_lattice_gemm_gpu import LAT_TAPS, tap_matrix_ref
from util import pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LAYOUTS = (0, 2, 3)
B, H, W, C, N = 3, 6, 8, 64, 320
PW = 32                                 # pattern width: one phase of the kernel
NBLK = 4

ONE_PHASE = [('c', 0), ('c', 1)] + LAT_TAPS[:9] + [('c', 2), ('c', 3)] + LAT_TAPS[9:] + [('c', 1)]
FULL_TABLE = LAT_TAPS + [('c', 3)] + LAT_TAPS + [('c', 0)] + LAT_TAPS + [('c', 2)] + LAT_TAPS[:7]
PLANE_SEGS = LAT_TAPS[:9] + [('c', 1)] + LAT_TAPS[9:]
NPLANES = 3
PLANE_OF = [(t + 1) % NPLANES for t in range(len(PLANE_SEGS))]     # first tap: plane 1; the tap behind the pattern: plane 2
CASES = {'one-phase segments': ONE_PHASE, '64 segments': FULL_TABLE}


def _hip():
    return pkg('hipops')


def _kdim(segs):
    return sum(PW if t[0] == 'c' else C for t in segs)


def _exact_ok(k):
    assert k * 16 < 2 ** 24, 'partial sums of %d products of magnitude <= 16 must stay exact in fp32' % k


def _round_bf16(x64):
    return x64.float().bfloat16()


@functools.lru_cache(maxsize=None)
def _data(kind):
    """NPLANES plain lattices [B, 4, H, W, C], a pattern table [2 H W, NBLK, PW], rowpos [2 H W, N], bias [N] on the CPU."""
    gen = torch.Generator(device='cpu').manual_seed(51)
    if kind == 'int':
        make = lambda *s: torch.randint(-4, 5, s, generator=gen).to(torch.bfloat16)
    else:
        make = lambda *s: torch.randn(*s, generator=gen).bfloat16()
    planes = [make(B, 4, H, W, C) for _ in range(NPLANES)]
    return planes, make(2 * H * W, NBLK, PW), make(2 * H * W, N).float(), make(N).float()


@functools.lru_cache(maxsize=None)
def _weights(kind, k):
    gen = torch.Generator(device='cpu').manual_seed(52 + k)
    if kind == 'int':
        return torch.randint(-4, 5, (k, N), generator=gen).to(torch.bfloat16)
    return (torch.randn(k, N, generator=gen) * 0.05).bfloat16()


@functools.lru_cache(maxsize=None)
def _segments_ref(name, kind):
    """fp64 tap matrix of a segments case (plane 0 is the lattice)."""
    planes, table, _, _ = _data(kind)
    return tap_matrix_ref(planes[0], CASES[name], H, W, table)


@functools.lru_cache(maxsize=None)
def _planes_ref(kind):
    """fp64 tap matrix of the planes case: segment t from the tap matrix of plane PLANE_OF[t]."""
    planes, table, _, _ = _data(kind)
    refs = [tap_matrix_ref(p, PLANE_SEGS, H, W, table) for p in planes]
    cols, k = [], 0
    for t, pl in zip(PLANE_SEGS, PLANE_OF):
        wdt = PW if t[0] == 'c' else C
        cols.append(refs[pl][:, k:k + wdt])
        k += wdt
    return torch.cat(cols, 1)


def _check(hip, run, a_ref, kind):
    """``run(rowpos, bias)`` = the implicit product: bit for bit the explicit kernel on a_ref; on integers the fp64 product."""
    _, _, rowpos, bias = _data(kind)
    k = a_ref.shape[1]
    _exact_ok(k + 2)
    assert a_ref.shape[0] == B * 2 * H * W and k % 32 == 0
    w = _weights(kind, k)
    a = a_ref.to(torch.bfloat16)
    assert torch.equal(a.double(), a_ref)
    wd, bd, rd = w.to(DEV), bias.to(DEV), rowpos.to(DEV)
    got = run(wd, None, bd)
    assert tuple(got.shape) == (a_ref.shape[0], N)
    assert torch.equal(got, hip.gemm_nn(a.to(DEV), wd, bias=bd, splits=1)), kind
    if kind == 'int':
        prod = a_ref @ w.double()
        assert torch.equal(got.cpu(), _round_bf16(prod + bias.double()))
        full = run(wd, rd, bd)
        assert torch.equal(full.cpu(), _round_bf16(prod + rowpos.double().repeat(B, 1) + bias.double()))


def _run_segments(hip, name, layout, kind):
    from_plain = pkg('dense_heads._cpu_algebra').from_plain
    planes, table, _, _ = _data(kind)
    e, tab = from_plain(planes[0], layout).to(DEV), table.to(DEV)
    return lambda w, rowpos, bias: hip.gemm_nn_taps(e, layout, (H, W), CASES[name], w, const_rows=tab, rowpos=rowpos, bias=bias)


def _run_planes(hip, layout, kind):
    from_plain = pkg('dense_heads._cpu_algebra').from_plain
    planes, table, _, _ = _data(kind)
    lat = torch.stack([from_plain(p, layout) for p in planes]).to(DEV).contiguous()
    tab = table.to(DEV)
    return lambda w, rowpos, bias: hip.gemm_nn_taps(lat, layout, (H, W), PLANE_SEGS, w, const_rows=tab, rowpos=rowpos, bias=bias,
                                                    planes=PLANE_OF)


def test_the_cases_are_what_they_claim():
    assert _kdim(ONE_PHASE[:2]) == 64 and ONE_PHASE[-1][0] == 'c' and ONE_PHASE[11][0] == ONE_PHASE[12][0] == 'c'
    assert len(FULL_TABLE) == 64 and sum(t[0] == 'c' for t in FULL_TABLE) == 3
    assert all(a != b for a, b in zip(PLANE_OF, PLANE_OF[1:])) and PLANE_OF[0] != 0 and set(PLANE_OF) == set(range(NPLANES))
    assert PLANE_SEGS[9][0] == 'c' and PLANE_OF[10] != PLANE_OF[8]
    for segs in (ONE_PHASE, FULL_TABLE, PLANE_SEGS):
        _exact_ok(_kdim(segs) + 2)


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('name', list(CASES))
def test_segments_equal_explicit_and_fp64(name, layout):
    hip = _hip()
    _check(hip, _run_segments(hip, name, layout, 'int'), _segments_ref(name, 'int'), 'int')


@pytest.mark.parametrize('layout', LAYOUTS)
def test_planes_equal_explicit_and_fp64(layout):
    hip = _hip()
    _check(hip, _run_planes(hip, layout, 'int'), _planes_ref('int'), 'int')


@pytest.mark.parametrize('layout', LAYOUTS)
def test_segments_randn_bit_for_bit_explicit(layout):
    hip = _hip()
    _check(hip, _run_segments(hip, 'one-phase segments', layout, 'randn'), _segments_ref('one-phase segments', 'randn'), 'randn')


@pytest.mark.parametrize('layout', LAYOUTS)
def test_planes_randn_bit_for_bit_explicit(layout):
    hip = _hip()
    _check(hip, _run_planes(hip, layout, 'randn'), _planes_ref('randn'), 'randn')
