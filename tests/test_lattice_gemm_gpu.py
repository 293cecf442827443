"""The implicit-operand GEMMs of the three lattice (ConvTranspose3d) layers against a plain fp64 definition, at the geometries
where their addressing can go wrong: non-square and odd lattices, one slab per viewpoint, rows that fill no tile, row chunks
that start inside a viewpoint, 2 H W at and past the 2 048 rows per viewpoint of ver_wgrad_tn_segments' LDS tables, and an
empty batch.  Needs an MI355X: run with ``-m gpu``.

* kernels (hipops.gemm_nn_taps, hipops.wgrad_tn_segments, upsample._dgrad_implicit) against ``tap_matrix_ref``, the tap matrix
  written out from the plain [B, 4, H, W, C] lattice with ``F.pad`` and slicing -- nothing of the package's own gather /
  im2col / scatter; only ``_cpu_algebra.from_plain`` to lay the input out as the kernels read it;
* layers (upsample._Layer0Z4, _LatticeLayerZ4 plain and planar, bf16 with the fp32 ConvTranspose3d weight) against fp64
  autograd of ``conv_transpose3d`` on the full volume, read at the even lattice.

Every kernel test also builds the reference with one deliberate addressing mistake (``wrong_tap_matrix_ref``) and requires
the kernel to be at least ``NEG`` times its bound away from it: the shape really tells a right addressing rule from a wrong one.

Bounds:
* ``REL_L2`` = 3e-3, ``MAX_REL`` = 2^-7 (x max |ref|): a bf16 result is one rounding of an fp32 sum of exact bf16 products --
  at most 2^-9 of each element (rel_l2 ~1e-3 in practice), so rel_l2 keeps 1.5x and the element-wise bound 4x headroom;
* fp32 weight gradients: see ``_fp32_sum_bound``;
* ``GRAD_REL`` = 1e-2 for the gradients of a whole layer: a few bf16 roundings in sequence (class partial sums, the two
  output halves of a tap, d(K^T b_prev)) that need not cancel; each also no further from fp64 than the explicit path x 1.05."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from util import pkg, rel_l2

pytestmark = pytest.mark.gpu
DEV = 'cuda'

REL_L2 = 3e-3           # one bf16 rounding (<= 2^-9 relative) of an fp32 sum of exact products
MAX_REL = 2.0 ** -7     # element-wise: 2^-9 |ref| <= 2^-9 max |ref|, 4x headroom for the fp32 sums
GRAD_REL = 1e-2         # a layer's gradients: several bf16 roundings of fp32 sums in sequence
NEG = 10                # the kernel must sit at least 10 bounds away from the wrong reference
PW2 = 192               # width of a pattern block of the class layout (upsample._PW2: lo | hi halves of 96)
L1_TAPS = [(2 * j, bb - 2, cc - 2) for bb in range(5) for cc in range(5) for j in range(2)]      # layer 1: 5 x 5 x 2 blocks
LAT_TAPS = [(2 * j, dy, dx) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for j in range(2)]          # layers 2-3: 3 x 3 x 2 blocks
GEOM = dict(stride=(1, 2, 2), padding=(2, 4, 4), dilation=(2, 2, 2), output_padding=(0, 1, 1))   # head:251-258


def _mods():
    return pkg('hipops'), pkg('dense_heads.upsample'), pkg('dense_heads._cpu_algebra').from_plain


# --------------------------------------------------------------------------------------------- the fp64 definition
def tap_matrix_ref(plain, taps, H, W, const=None):
    """The tap matrix of a Z = 4 lattice layer by its definition, in fp64 (differentiable: autograd gives its adjoint).
    plain [B, 4, H, W, C].  Row ((b 2 + zl) H + y) W + x; a tap (dz, dy, dx) is the block plain[b, zl + dz, y + dy, x + dx, :],
    zeros outside the H x W grid; a pattern segment ('c', k) is block k of ``const`` [2 H W, blocks, width] at the row's
    position r % (2 H W)."""
    plain = plain.double()
    B, Z, h, w, C = plain.shape
    assert Z == 4 and (h, w) == (H, W)
    r = max([max(abs(t[1]), abs(t[2])) for t in taps if t[0] != 'c'] + [0])
    pad = F.pad(plain, (0, 0, r, r, r, r))
    cols = []
    for t in taps:
        if t[0] == 'c':
            cols.append(const[:, t[1]].double().reshape(1, 2, H, W, -1).expand(B, -1, -1, -1, -1))
        else:
            dz, dy, dx = t
            cols.append(pad[:, dz:dz + 2, r + dy:r + dy + H, r + dx:r + dx + W])
    return torch.cat(cols, -1).reshape(B * 2 * H * W, -1)


def wrong_tap_matrix_ref(plain, taps, H, W, const=None):
    """``tap_matrix_ref`` with one deliberate addressing mistake: H and W swapped in the row numbering (the lattice read as a
    W x H grid) -- or, on a square lattice, where that swap changes nothing, one tap's (dy, dx) transposed."""
    if H != W:
        B, C = plain.shape[0], plain.shape[-1]
        return tap_matrix_ref(plain.reshape(B, 4, W, H, C), taps, W, H, const)
    i = next(i for i, t in enumerate(taps) if t[0] != 'c' and t[1] != t[2])
    taps = list(taps)
    taps[i] = (taps[i][0], taps[i][2], taps[i][1])
    return tap_matrix_ref(plain, taps, H, W, const)


def _close_bf16(got, ref, what):
    got = got.double().cpu()
    assert rel_l2(got, ref) < REL_L2, (what, rel_l2(got, ref))
    assert float((got - ref).abs().max()) <= MAX_REL * float(ref.abs().max()), (what, float((got - ref).abs().max()))


def _far(got, wrong, what):
    d = rel_l2(got.double().cpu(), wrong)
    assert d >= NEG * REL_L2, ('the wrong reference is within %g: this shape does not discriminate' % d, what)


def _fp32_sum_bound(a_ref, g, splits):
    """Element-wise bound on an fp32 A^T G over M rows, A and G in bf16: a product of two bf16 values has at most 16 significant
    bits and is exact in fp32; the M products of an element are added up in fp32 (MFMA accumulators over each row chunk, then
    the ``splits`` chunk partials), so every path through the sum has at most M + splits additions, each rounding by at most
    2^-23 relative (2^-24 with round-to-nearest; 2^-23 also covers truncating adders), and the classic recursive-summation bound
    gives |fl(s) - s| <= (M + splits) 2^-23 sum_m |a_mi g_mj| (to first order; here (M + S) 2^-23 < 1e-3)."""
    m = a_ref.shape[0]
    return (m + splits) * 2.0 ** -23 * (a_ref.abs().t() @ g.abs())


def _inputs(B, H, W, C, seed):
    gen = torch.Generator(device='cpu').manual_seed(seed)
    return gen, torch.randn(B, 4, H, W, C, generator=gen).bfloat16()


def _const_table(H, W, gen):
    """A pattern table of random bf16 values (the layer's own 0/1 patterns would hide a wrong row position)."""
    return torch.randn(2 * H * W, 4, PW2, generator=gen).bfloat16()


# --------------------------------------------------------------------------------------------- forward: ver_gemm_nn_taps
# (edge, layout, B, H, W, C, N); layout 0 = layer 1's plain lattice and 50 taps, 2 = z-split, 3 = planar z-split (even H, W)
GEMM_CASES = [
    ('layout 0, non-square 6x10', 0, 2, 6, 10, 64, 200),
    ('layout 0, non-square 10x6, tile-multiple N', 0, 2, 10, 6, 64, 256),
    ('layout 0, non-square 4x14, C 128', 0, 1, 4, 14, 128, 200),
    ('layout 0, odd 5x9', 0, 2, 5, 9, 64, 200),
    ('layout 0, smallest P = 16 (2x4): taps off the grid in every direction', 0, 3, 2, 4, 64, 200),
    ('layout 0, ragged rows: P = 30, M = 90', 0, 3, 5, 3, 64, 200),
    ('layout 0, C 768 at B 1', 0, 1, 2, 6, 768, 256),
    ('layout 2, non-square 6x10, N 1536', 2, 2, 6, 10, 64, 1536),
    ('layout 2, non-square 10x6, C 128', 2, 2, 10, 6, 128, 200),
    ('layout 2, non-square 4x14', 2, 2, 4, 14, 64, 200),
    ('layout 2, odd 5x9', 2, 2, 5, 9, 64, 200),
    ('layout 2, smallest P = 16 (2x4)', 2, 3, 2, 4, 64, 256),
    ('layout 2, ragged rows: P = 30, M = 90', 2, 3, 5, 3, 128, 200),
    ('layout 2, C 768, N 1536 at B 1', 2, 1, 6, 10, 768, 1536),
    ('layout 3, non-square 6x10', 3, 2, 6, 10, 64, 200),
    ('layout 3, non-square 10x6, N 1536', 3, 1, 10, 6, 64, 1536),
    ('layout 3, non-square 4x14', 3, 2, 4, 14, 64, 200),
    ('layout 3, smallest P = 16 (2x4), C 128', 3, 3, 2, 4, 128, 200),
    ('layout 3, C 768 at B 1', 3, 1, 4, 14, 768, 200),
    ('LDS limit of the weight gradient: P = 2048 (32x32)', 3, 1, 32, 32, 64, 256),
    ('LDS limit of the weight gradient: P = 2048 (16x64)', 2, 1, 16, 64, 64, 200),
    ('past the weight-gradient limit: P = 3200 (40x40)', 3, 1, 40, 40, 64, 200),
    ('the largest P of the forward\'s old admission rule: 64 800 (180x180)', 2, 1, 180, 180, 64, 200),
]


@pytest.mark.parametrize('edge,layout,B,H,W,C,N', GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_nn_taps_against_fp64(edge, layout, B, H, W, C, N):
    """ver_gemm_nn_taps / _segments against tap_matrix_ref @ W in fp64: the plain taps (layer 1's 50 for layout 0, the 18 of
    layers 2-3 otherwise), the same with the position table, the bias and a strided ``out=`` view (guard columns untouched),
    and the class segments of a lattice layer with pattern blocks read from a random table."""
    hip, ups, from_plain = _mods()
    gen, plain = _inputs(B, H, W, C, 1000 * layout + 10 * H + W)
    e = from_plain(plain, layout).to(DEV)
    taps = L1_TAPS if layout == 0 else LAT_TAPS
    w = (torch.randn(len(taps) * C, N, generator=gen) * 0.05).bfloat16()
    a_ref = tap_matrix_ref(plain, taps, H, W)
    ref = a_ref @ w.double()
    got = hip.gemm_nn_taps(e, layout, (H, W), taps, w.to(DEV))
    _close_bf16(got, ref, 'taps')
    _far(got, wrong_tap_matrix_ref(plain, taps, H, W) @ w.double(), 'taps')
    del a_ref
    m = B * 2 * H * W
    if m > 20000:                           # (the 180 x 180 lattice: the plain product only -- its fp64 reference is 0.6 GB)
        return
    rowpos = torch.randn(2 * H * W, N, generator=gen)
    bias = torch.randn(N, generator=gen)
    wide = torch.full((m, N + 16), 7.0, device=DEV, dtype=torch.bfloat16)
    got = hip.gemm_nn_taps(e, layout, (H, W), taps, w.to(DEV), rowpos=rowpos.to(DEV), bias=bias.to(DEV), out=wide[:, 8:8 + N])
    _close_bf16(got, ref + rowpos.double().repeat(B, 1) + bias.double(), 'rowpos + bias')
    assert float(wide[:, :8].min()) == 7.0 == float(wide[:, :8].max()), 'left guard columns written'
    assert float(wide[:, 8 + N:].min()) == 7.0 == float(wide[:, 8 + N:].max()), 'right guard columns written'
    if layout == 0:
        return
    table = _const_table(H, W, gen)
    for cls in ((0, 0), (0, 1)):            # (0, 0): three pattern blocks between the taps; (0, 1): one at the end
        segs = ups._class_segments_z4(cls, C)
        a_ref = tap_matrix_ref(plain, segs, H, W, table)
        ws = (torch.randn(a_ref.shape[1], N, generator=gen) * 0.05).bfloat16()
        got = hip.gemm_nn_taps(e, layout, (H, W), segs, ws.to(DEV), const_rows=table.to(DEV))
        _close_bf16(got, a_ref @ ws.double(), cls)
        _far(got, wrong_tap_matrix_ref(plain, segs, H, W, table) @ ws.double(), cls)


# --------------------------------------------------------------------------------------------- weight gradient
# (edge, layout, B, H, W, C, N, row-chunk counts; 0 = the library's choice)
WGRAD_CASES = [
    ('layout 0, non-square 6x10', 0, 2, 6, 10, 64, 200, (0, 3)),
    ('layout 0, non-square 10x6, C 128', 0, 1, 10, 6, 128, 256, (0,)),
    ('layout 0, non-square 4x14', 0, 1, 4, 14, 64, 200, (0, 2)),
    ('layout 0, odd 5x9', 0, 2, 5, 9, 64, 200, (0, 2)),
    ('layout 0, smallest P = 16 (2x4)', 0, 3, 2, 4, 64, 256, (1, 2)),
    ('layout 0, ragged rows: P = 30, M = 90, chunks inside viewpoints', 0, 3, 5, 3, 64, 200, (1, 2, 3, 7)),
    ('layout 2, non-square 6x10', 2, 2, 6, 10, 64, 200, (0, 2)),
    ('layout 2, non-square 10x6', 2, 2, 10, 6, 64, 200, (0, 3)),
    ('layout 2, non-square 4x14, N 1536', 2, 2, 4, 14, 64, 1536, (0,)),
    ('layout 2, odd 5x9', 2, 2, 5, 9, 128, 200, (0, 2)),
    ('layout 2, smallest P = 16 (2x4)', 2, 3, 2, 4, 64, 200, (1, 5)),
    ('layout 2, ragged rows: P = 30, M = 90, chunks inside viewpoints', 2, 3, 5, 3, 64, 200, (1, 2, 3, 7)),
    ('layout 2, C 768 at B 1', 2, 1, 4, 6, 768, 256, (0,)),
    ('layout 3, non-square 6x10', 3, 2, 6, 10, 64, 200, (0, 2)),
    ('layout 3, non-square 10x6, C 128', 3, 2, 10, 6, 128, 200, (0,)),
    ('layout 3, non-square 4x14', 3, 2, 4, 14, 64, 200, (0, 3)),
    ('layout 3, smallest P = 16 (2x4)', 3, 3, 2, 4, 64, 256, (1, 3)),
    ('LDS limit: P = 2048 (32x32), layout 3', 3, 1, 32, 32, 64, 200, (0, 3)),
    ('LDS limit: P = 2048 (16x64), layout 2', 2, 1, 16, 64, 64, 256, (0, 5)),
    ('LDS limit: P = 2048 (32x32), layout 0', 0, 1, 32, 32, 64, 200, (0,)),
]


@pytest.mark.parametrize('edge,layout,B,H,W,C,N,splits', WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_wgrad_tn_segments_against_fp64(edge, layout, B, H, W, C, N, splits):
    """ver_wgrad_tn_segments against tap_matrix_ref^T @ G in fp64, in fp32 (``_fp32_sum_bound``) and bf16 output, for every
    row-chunk count given (a chunk boundary of a count that does not divide the rows lands inside a viewpoint, where the
    offset-table wrap takes the next viewpoint's rows; 7 chunks of 90 rows leave four chunks empty): layer 1's 50 taps for
    layout 0, the class segments (0, 0) and (0, 1) of a lattice layer, pattern blocks from a random table, otherwise."""
    hip, ups, from_plain = _mods()
    gen, plain = _inputs(B, H, W, C, 2000 * layout + 10 * H + W)
    e = from_plain(plain, layout).to(DEV)
    m = B * 2 * H * W
    g = torch.randn(m, N, generator=gen).bfloat16()
    table = _const_table(H, W, gen)
    forms = [(L1_TAPS, None)] if layout == 0 else [(ups._class_segments_z4(cls, C), table) for cls in ((0, 0), (0, 1))]
    for segs, cst in forms:
        a_ref = tap_matrix_ref(plain, segs, H, W, cst)
        ref = a_ref.t() @ g.double()
        wrong = wrong_tap_matrix_ref(plain, segs, H, W, cst).t() @ g.double()
        kw = dict(const_rows=cst.to(DEV)) if cst is not None else {}
        for s in splits:
            s_eff = s or hip.lib().ver_wgrad_tn_segments_splits(B, H, W, ctypes.c_long(a_ref.shape[1]), N, ctypes.c_long(N))
            got = hip.wgrad_tn_segments(e, layout, (H, W), segs, g.to(DEV), out_dtype=torch.float32, splits=s, **kw).double().cpu()
            bound = _fp32_sum_bound(a_ref, g.double(), s_eff)
            err = (got - ref).abs()
            assert bool((err <= bound).all()), (s, float((err / bound.clamp(min=1e-30)).max()))
            assert float((got - wrong).norm()) >= NEG * float(bound.norm()), ('wrong reference within 10 bounds', s)
            got16 = hip.wgrad_tn_segments(e, layout, (H, W), segs, g.to(DEV), out_dtype=torch.bfloat16, splits=s, **kw)
            _close_bf16(got16, ref, ('bf16', s))
            _far(got16, wrong, ('bf16', s))


# --------------------------------------------------------------------------------------------- d(input)
# (edge, kind, B, H, W, Ci, Co); 'l0': layer 1 (plain source, one output-gradient plane), 'lat': a class-stacked layer
DGRAD_CASES = [
    ('layer 1, non-square 6x10', 'l0', 2, 6, 10, 64, 64),
    ('layer 1, non-square 10x6, Co 128', 'l0', 1, 10, 6, 64, 128),
    ('layer 1, odd 5x9', 'l0', 2, 5, 9, 64, 64),
    ('layer 1, smallest P = 16 (2x4)', 'l0', 3, 2, 4, 64, 64),
    ('lattice layer, non-square 4x14', 'lat', 2, 4, 14, 64, 64),
    ('lattice layer, non-square 10x6, C 128', 'lat', 2, 10, 6, 128, 128),
    ('lattice layer, odd 5x9', 'lat', 2, 5, 9, 64, 64),
    ('lattice layer, ragged rows: P = 30, M = 90', 'lat', 3, 5, 3, 64, 64),
    ('lattice layer, smallest P = 16 (2x4)', 'lat', 3, 2, 4, 64, 64),
    ('lattice layer, P = 2048 (16x64)', 'lat', 1, 16, 64, 64, 64),
    ('lattice layer, P = 3200 (40x40)', 'lat', 1, 40, 40, 64, 64),
]


def _dgrad_ref(ups, kind, g, weights, B, H, W, ci, build):
    """d(input) by the definition: the adjoint (torch autograd) of ``build`` -- the tap matrices of every class -- applied to
    g_p W_p^T, summed over the classes p; plain [B, 4, H, W, Ci] fp64."""
    x = torch.zeros(B, 4, H, W, ci, dtype=torch.float64, requires_grad=True)
    g, weights = g.double(), weights.double()
    if kind == 'l0':
        loss = (build(x, L1_TAPS, H, W) * (g[0] @ weights.t())).sum()
    else:
        table = torch.zeros(2 * H * W, 4, PW2, dtype=torch.float64)
        loss = 0
        for p, cls in enumerate(ups._CLASSES):
            segs, r0 = ups._class_segments_z4(cls, ci), ups._class_rows_z4(ci)[cls][0]
            a = build(x, segs, H, W, table)
            loss = loss + (a * (g[p] @ weights[r0:r0 + a.shape[1]].t())).sum()
    loss.backward()
    return x.grad


@pytest.mark.parametrize('edge,kind,B,H,W,ci,co', DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_implicit_input_gradient_against_fp64(edge, kind, B, H, W, ci, co):
    """upsample._dgrad_implicit (ver_gemm_nn_planes over the class planes of the output gradient) against the fp64 adjoint of
    tap_matrix_ref applied to sum_p g_p W_p^T."""
    hip, ups, from_plain = _mods()
    gen = torch.Generator(device='cpu').manual_seed(3000 + 10 * H + W + ci)
    m = B * 2 * H * W
    if kind == 'l0':
        assert ups._layer0_z4_plan(ci, 'cpu')[0] == L1_TAPS                # (the block order of layer 1's weight rows)
        rows = 50 * ci
    else:                                                                    # the class-stacked matrix: every class's segments
        rows = sum(PW2 if t[0] == 'c' else ci for cls in ups._CLASSES for t in ups._class_segments_z4(cls, ci))
    weights = (torch.randn(rows, 2 * co, generator=gen) * 0.1).bfloat16()
    g = torch.randn(1 if kind == 'l0' else 4, m, 2 * co, generator=gen).bfloat16()
    got = ups._dgrad_implicit(kind, g.to(DEV), weights.to(DEV), B, H, W, ci, co)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (B, 2, H, W, 2, ci)
    ref = from_plain(_dgrad_ref(ups, kind, g, weights, B, H, W, ci, tap_matrix_ref), 2)
    _close_bf16(got, ref, kind)
    _far(got, from_plain(_dgrad_ref(ups, kind, g, weights, B, H, W, ci, wrong_tap_matrix_ref), 2), kind)


# --------------------------------------------------------------------------------------------- empty batch
def test_empty_batch_gives_zeros():
    """B = 0: ver_gemm_nn_taps returns without a launch (an empty result), ver_wgrad_tn_segments and ver_wgrad_tn write zeros
    (their M == 0 branches: a kernel zero fill of the workspace, then the reduce) in fp32 and bf16, with one chunk and with
    several; return code 0 throughout (hipops raises otherwise)."""
    hip, ups, from_plain = _mods()
    C, N, H, W = 64, 200, 6, 10
    table = _const_table(H, W, torch.Generator(device='cpu').manual_seed(7)).to(DEV)
    segs = ups._class_segments_z4((0, 0), C)
    for layout in (0, 2, 3):
        e = from_plain(torch.zeros(0, 4, H, W, C, dtype=torch.bfloat16), layout).to(DEV)
        taps = L1_TAPS if layout == 0 else LAT_TAPS
        out = hip.gemm_nn_taps(e, layout, (H, W), taps, torch.ones(len(taps) * C, N, dtype=torch.bfloat16, device=DEV))
        assert tuple(out.shape) == (0, N)
        g = torch.zeros(0, N, dtype=torch.bfloat16, device=DEV)
        s_, kw = (taps, {}) if layout == 0 else (segs, dict(const_rows=table))
        ka = len(taps) * C if layout == 0 else 18 * C + 3 * PW2
        for dt in (torch.float32, torch.bfloat16):
            for splits in (0, 1, 3):
                out = torch.full((ka, N), 7.0, dtype=dt, device=DEV)
                hip.wgrad_tn_segments(e, layout, (H, W), s_, g, out=out, splits=splits, **kw)
                assert float(out.abs().max()) == 0.0, (layout, dt, splits)
    for splits in (0, 1, 4):
        out = torch.full((128, N), 7.0, device=DEV)
        hip.wgrad_tn(torch.zeros(0, 128, dtype=torch.bfloat16, device=DEV), torch.zeros(0, N, dtype=torch.bfloat16, device=DEV),
                     out=out, out_dtype=torch.float32, splits=splits)
        assert float(out.abs().max()) == 0.0, splits


# --------------------------------------------------------------------------------------------- whole layers
def _full_volume(plain, bias):
    """data lattice [B, 4, h, w, C] + the bias of the layer before -> the dense input [B, C, 4, 2h, 2w] of the next
    ConvTranspose3d (odd rows / columns hold the bias: SURVEY A.4)."""
    B, Z, h, w, C = plain.shape
    vol = bias.view(1, C, 1, 1, 1).expand(B, C, Z, 2 * h, 2 * w).clone()
    vol[:, :, :, ::2, ::2] = plain.permute(0, 4, 1, 2, 3)
    return vol


def _layer_ref(layer, plain, raw, bias, prev_bias, g_plain):
    """fp64 autograd of conv_transpose3d(full input, W, b) read at the even lattice -> (out, d_in, d_W, d_b, d_prev) plain."""
    x = plain.double().requires_grad_(True)
    w = raw.double().requires_grad_(True)
    b = bias.double().requires_grad_(True)
    pb = prev_bias.double().requires_grad_(True)
    vol = x.permute(0, 4, 1, 2, 3) if layer == 1 else _full_volume(x, pb)
    out = F.conv_transpose3d(vol, w, b, **GEOM)[:, :, :, ::2, ::2].permute(0, 2, 3, 4, 1)
    (out * g_plain.double()).sum().backward()
    return out.detach(), x.grad, w.grad, b.grad, (pb.grad if layer > 1 else None)


def _layer_gpu(ups, layer, x_in, raw, bias, prev_bias, g):
    """One layer on the GPU from the kernel layout of its input; -> (out, d_in, d_W, d_b, d_prev) in the kernel layouts."""
    x = x_in.clone().requires_grad_(True)
    w = raw.clone().requires_grad_(True)
    b = bias.clone().requires_grad_(True)
    pb = prev_bias.clone().requires_grad_(True)
    if layer == 1:
        out = ups._Layer0Z4.apply(x, None, b.bfloat16(), w)
    else:
        out = ups._LatticeLayerZ4.apply(x, None, b.bfloat16(), pb.bfloat16(), layer == 3, w)
    out.backward(g)
    torch.cuda.synchronize()
    return out.detach(), x.grad, w.grad, b.grad, (pb.grad if layer > 1 else None)


def _spy(monkeypatch, hip):
    calls = {'gemm_nn_taps': 0, 'wgrad_tn_segments': 0}
    for name in calls:
        real = getattr(hip, name)

        def wrapped(*a, _real=real, _name=name, **k):
            calls[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(hip, name, wrapped)
    return calls


def _layer_case(layer, bev, B, seed):
    """bf16-representable inputs of one layer of a (bev_h, bev_w) grid: its input lattice (h, w) = the BEV grid for layers 1-2,
    twice it for layer 3."""
    H, W = bev
    h, w = (H, W) if layer < 3 else (2 * H, 2 * W)
    C = 64
    gen = torch.Generator(device='cpu').manual_seed(seed)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).bfloat16().float()
    plain = r(B, 4, h, w, C)
    raw, bias, prev_bias = r(C, C, 3, 5, 5, sc=0.05), r(C, sc=0.5), r(C, sc=0.5)
    oh, ow = (h, w) if layer == 1 else (2 * h, 2 * w)
    g_plain = r(B, 4, oh, ow, C)
    return h, w, plain, raw, bias, prev_bias, g_plain


LAYOUT_IN = {1: 0, 2: 2, 3: 3}          # the kernel layout of each layer's input and output
LAYOUT_OUT = {1: 2, 2: 3, 3: 3}
BEV_GRIDS = [((15, 15), 'the vocc anchor'), ((12, 20), 'non-square'), ((20, 12), 'non-square, transposed'), ((9, 15), 'odd'),
             ((16, 16), 'layer 3 at P = 2048'), ((20, 20), 'layer 3 at P = 3200, past the weight-gradient kernel')]
LAYER_CASES = [(bev, layer) for bev, _ in BEV_GRIDS for layer in (1, 2, 3)]


@pytest.mark.parametrize('bev,layer', LAYER_CASES, ids=['bev%dx%d-layer%d' % (bev + (layer,)) for bev, layer in LAYER_CASES])
def test_lattice_layer_against_fp64_conv_transpose(monkeypatch, bev, layer):
    """One lattice layer in bf16 (C = 64, the fp32 ConvTranspose3d weight) with the implicit path forced at any row count
    (upsample._OWN_GEMM_MIN_ROWS = 0) against fp64 conv_transpose3d: output and every gradient; the gradients also against the
    explicit path (upsample._IMPLICIT_TAPS = False).  Where ver_wgrad_tn_segments cannot take the lattice (2 H W > 2 048:
    layer 3 of a 20 x 20 grid) the layer must take the explicit path in both passes instead of failing in backward()."""
    hip, ups, from_plain = _mods()
    B = 1
    h, w, plain, raw, bias, prev_bias, g_plain = _layer_case(layer, bev, B, 4000 + 100 * bev[0] + bev[1] + layer)
    lin, lout = LAYOUT_IN[layer], LAYOUT_OUT[layer]
    x_in = from_plain(plain.bfloat16(), lin).to(DEV)
    g = from_plain(g_plain.bfloat16(), lout).to(DEV)
    args = (raw.to(DEV), bias.to(DEV), prev_bias.to(DEV), g)
    monkeypatch.setattr(ups, '_OWN_GEMM_MIN_ROWS', 0)
    calls = _spy(monkeypatch, hip)
    implicit = _layer_gpu(ups, layer, x_in, *args)
    if 2 * h * w <= 2048:
        assert calls['gemm_nn_taps'] > 0 and calls['wgrad_tn_segments'] > 0, calls
    else:
        assert calls == {'gemm_nn_taps': 0, 'wgrad_tn_segments': 0}, calls
    monkeypatch.setattr(ups, '_IMPLICIT_TAPS', False)
    before = dict(calls)
    explicit = _layer_gpu(ups, layer, x_in, *args)
    assert calls == before, 'the explicit path ran an implicit-operand kernel'
    ref = _layer_ref(layer, plain, raw, bias, prev_bias, g_plain)
    _close_bf16(implicit[0], from_plain(ref[0], lout), 'output')
    refs = [from_plain(ref[1], lin)] + list(ref[2:])
    for name, got, exp, want in zip(('d(input)', 'd(W)', 'd(b)', 'd(prev bias)'), implicit[1:], explicit[1:], refs):
        if want is None:
            continue
        e_i, e_e = rel_l2(got.double().cpu(), want), rel_l2(exp.double().cpu(), want)
        assert e_i < GRAD_REL, (name, e_i)
        assert e_i <= e_e * 1.05, (name, e_i, e_e)           # (5 %: the same fp32 sums in another order, rounded alike)


def test_layer3_of_a_20x20_grid_at_the_default_threshold(monkeypatch):
    """The shape a user reaches with bev_h = bev_w = 20 and five viewpoints: layer 3 has 16 000 rows, past the implicit path's
    row threshold, on a 40 x 40 lattice (2 H W = 3 200) that ver_wgrad_tn_segments cannot take.  No patched threshold: the
    layer runs forward and backward; output and d(input) of viewpoints 0 and 4 against fp64 (the fp64 reference of all five is
    too slow on the CPU), the weight and bias gradients against the explicit path."""
    hip, ups, from_plain = _mods()
    B, layer = 5, 3
    assert B * 2 * 40 * 40 >= ups._OWN_GEMM_MIN_ROWS
    h, w, plain, raw, bias, prev_bias, g_plain = _layer_case(layer, (20, 20), B, 4999)
    x_in = from_plain(plain.bfloat16(), 3).to(DEV)
    g = from_plain(g_plain.bfloat16(), 3).to(DEV)
    args = (raw.to(DEV), bias.to(DEV), prev_bias.to(DEV), g)
    got = _layer_gpu(ups, layer, x_in, *args)
    monkeypatch.setattr(ups, '_IMPLICIT_TAPS', False)
    explicit = _layer_gpu(ups, layer, x_in, *args)
    vp = [0, 4]
    ref = _layer_ref(layer, plain[vp], raw, bias, prev_bias, g_plain[vp])
    _close_bf16(got[0][:, vp], from_plain(ref[0], 3), 'output, viewpoints 0 and 4')
    assert rel_l2(got[1][:, vp].double().cpu(), from_plain(ref[1], 3)) < GRAD_REL
    for name, a, b in zip(('d(W)', 'd(b)', 'd(prev bias)'), got[2:], explicit[2:]):
        assert rel_l2(a.double(), b.double()) < GRAD_REL, name
