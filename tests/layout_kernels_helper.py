"""Reference models and case tables for the data-movement kernels of the coarse-to-fine head (csrc/ver_lattice.hip,
csrc/ver_layout.hip).  CPU only.  Every model is written from the definition in include/ver_ops.h with explicit index
arithmetic; none calls a kernel or the plan-specific CPU forms of dense_heads/upsample.py.  The ``*_form`` functions restate
the launchers' own rules (which kernel, which tile, how many workgroups), so that test_layout_kernels_cpu.py can prove that
a case reaches the branch it is named after and test_layout_kernels_gpu.py can print it.

Data: copies move random BIT PATTERNS (NaN payloads, infinities, -0 and subnormals included, the named specials planted at
the start), compared as integers; sums use integers in [-4, 4], at most 64 terms: every partial sum is exact in fp32 and the
result (|sum| <= 256) exact in bf16."""
import functools

import numpy as np
import torch

F32, BF16 = torch.float32, torch.bfloat16
SENTINEL = 7.0
LAT_TAPS = [(2 * j, dy, dx) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for j in range(2)]
SCATTER_TOL = {F32: 1e-5, BF16: 4e-2}        # test_hip_ops_gpu.py::test_lattice_gather_scatter_with_offsets


def esize(dtype):
    return 2 if dtype == BF16 else 4


def bits(t):
    """the raw bits of an fp32 / bf16 tensor as integers (NaN-safe equality)"""
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


_SPECIAL16 = [0x7FC0, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x807F, 0x7FC1, 0xFFFF, 0x0000]      # NaN, +-inf, -0, subnormals, payloads


def raw_data(shape, dtype, seed):
    """random bit patterns of ``dtype`` with the special values at the start"""
    gen = torch.Generator(device='cpu').manual_seed(seed)
    n = int(np.prod(shape))
    if dtype == BF16:
        v = torch.randint(-2 ** 15, 2 ** 15, (n,), generator=gen, dtype=torch.int32).to(torch.int16)
        sp = torch.tensor([s - 65536 if s >= 32768 else s for s in _SPECIAL16], dtype=torch.int16)
    else:
        v = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=gen, dtype=torch.int64).to(torch.int32)
        sp = torch.tensor([(s << 16) - 2 ** 32 if s >= 32768 else s << 16 for s in _SPECIAL16], dtype=torch.int32)
        sp[4] = 1                                                                          # the smallest fp32 subnormal
    v[:min(n, len(sp))] = sp[:n]
    return v.view(dtype).reshape(shape)


def int_data(shape, dtype, seed):
    gen = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randint(-4, 5, tuple(shape), generator=gen).to(dtype)


def exact_ok(terms):
    """sums of ``terms`` integers of magnitude <= 4: every partial sum exact in fp32, the result exact in bf16"""
    assert terms * 4 <= 256, '%d terms of magnitude <= 4 leave the integers bf16 holds exactly' % terms


# ------------------------------------------------------------------------------------------------------------ layouts
def layout_shape(B, Z, H, W, C, layout):
    return {0: (B, Z, H, W, C), 1: (4, B, Z, H // 2, W // 2, C), 2: (B, 2, H, W, 2, C),
            3: (4, B, 2, H // 2, W // 2, 2, C)}[layout]


def layout_legal(layout, Z, H, W):
    return (not (layout & 1) or (H % 2 == 0 and W % 2 == 0)) and (layout < 2 or Z == 4)


def layout_index(b, z, y, x, B, Z, H, W, layout, swap_parity=False):
    """index of the C-vector of lattice position (b, z, y, x) in the storage of ``layout`` (include/ver_ops.h)"""
    plane = 2 * (y % 2) + (x % 2) if not swap_parity else 2 * (x % 2) + (y % 2)
    if layout == 0:
        return ((b * Z + z) * H + y) * W + x
    if layout == 1:                     # four planes [B, Z, H/2, W/2, C]; plane 2 pm + pn = positions (2y'+pm, 2x'+pn)
        return (((plane * B + b) * Z + z) * (H // 2) + y // 2) * (W // 2) + x // 2
    if layout == 2:                     # [B, 2, H, W, 2, C]: row (b, z & 1, y, x), channel block z >> 1
        return (((b * 2 + z % 2) * H + y) * W + x) * 2 + z // 2
    return ((((plane * B + b) * 2 + z % 2) * (H // 2) + y // 2) * (W // 2) + x // 2) * 2 + z // 2


def _bzyx(B, Z, H, W):
    r = torch.arange(B * Z * H * W)
    return r // (Z * H * W), r // (H * W) % Z, r // W % H, r % W


def to_layout(plain, layout, swap_parity=False):
    B, Z, H, W, C = plain.shape
    assert layout_legal(layout, Z, H, W)
    idx = layout_index(*_bzyx(B, Z, H, W), B, Z, H, W, layout, swap_parity)
    out = torch.empty(layout_shape(B, Z, H, W, C, layout), dtype=plain.dtype)
    out.view(-1, C)[idx] = plain.reshape(-1, C)
    return out


def from_layout(e, layout, B, Z, H, W):
    C = e.shape[-1]
    idx = layout_index(*_bzyx(B, Z, H, W), B, Z, H, W, layout)
    return e.reshape(-1, C)[idx].view(B, Z, H, W, C)


# ------------------------------------------------------------------------------------------- tap matrix and its adjoint
def gather_ref(plain, taps, offs, stride, Zr, fill=SENTINEL, const=None, const_offs=None, swap_xy=False):
    """col[r, offs[t] .. + C) = plain[b, zr + dz_t, y + dy_t, x + dx_t, :] (0 outside), r = ((b Zr + zr) H + y) W + x; columns no
    tap or constant block names keep ``fill``; constant block k of row position r % (Zr H W) goes to const_offs[k]."""
    B, Zs, H, W, C = plain.shape
    b, zr, y, x = _bzyx(B, Zr, H, W)
    col = torch.full((B * Zr * H * W, stride), fill, dtype=plain.dtype)
    zero = torch.zeros((), dtype=plain.dtype)
    for (dz, dy, dx), o in zip(taps, offs):
        if swap_xy:
            dy, dx = dx, dy
        sz, sy, sx = zr + dz, y + dy, x + dx
        ok = (sz >= 0) & (sz < Zs) & (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
        v = plain[b, sz.clamp(0, Zs - 1), sy.clamp(0, H - 1), sx.clamp(0, W - 1)]
        col[:, o:o + C] = torch.where(ok[:, None], v, zero)
    if const is not None:
        pos = torch.arange(col.shape[0]) % (Zr * H * W)
        for k, o in enumerate(const_offs):
            col[:, o:o + const.shape[2]] = const[pos, k]
    return col


def selection(taps, B, Zr, Zs, H, W):
    """the 0/1 selection of the tap matrix as a sparse list: per tap (rows of col, plain positions they read)"""
    b, zr, y, x = _bzyx(B, Zr, H, W)
    out = []
    for dz, dy, dx in taps:
        sz, sy, sx = zr + dz, y + dy, x + dx
        ok = (sz >= 0) & (sz < Zs) & (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
        rows = ok.nonzero().squeeze(1)
        out.append((rows, (((b * Zs + sz) * H + sy) * W + sx)[rows]))
    return out


def scatter_ref(gcol, taps, offs, B, Zr, Zs, H, W, C):
    """the adjoint of ``gather_ref`` in the tap blocks: fp64 plain [B, Zs, H, W, C], the transpose of the selection"""
    out = torch.zeros(B * Zs * H * W, C, dtype=torch.float64)
    for (rows, pos), o in zip(selection(taps, B, Zr, Zs, H, W), offs):
        out.index_add_(0, pos, gcol[rows, o:o + C].double())
    return out.view(B, Zs, H, W, C)


def max_terms(taps, B, Zr, Zs, H, W):
    n = torch.zeros(B * Zs * H * W, dtype=torch.int64)
    for rows, pos in selection(taps, B, Zr, Zs, H, W):
        n.index_add_(0, pos, torch.ones_like(pos))
    return int(n.max())


def gather_walk(CV, ntaps, wrap=True):
    """k_lattice_gather's copy loop: the (tap, vector) pair lane ``i % 256`` holds at flat vector i of a row"""
    per_row, dt, dv = ntaps * CV, 256 // CV, 256 % CV
    out = [None] * per_row
    for tid in range(min(256, per_row)):
        t, v = tid // CV, tid % CV
        for i in range(tid, per_row, 256):
            out[i] = (t, v)
            t, v = t + dt, v + dv
            if wrap and v >= CV:
                t, v = t + 1, v - CV
    return out


def gather_by_walk(col, taps, offs, C, dtype, wrap, fill=SENTINEL):
    """``col`` (a gather_ref result) with the vectors the walk never names left at ``fill``"""
    ve = 16 // esize(dtype)
    CV = C // ve
    seen = set(p for p in gather_walk(CV, len(taps), wrap) if p[0] < len(taps) and p[1] < CV)
    out = col.clone()
    for t in range(len(taps)):
        for v in range(CV):
            if (t, v) not in seen:
                out[:, offs[t] + v * ve:offs[t] + (v + 1) * ve] = fill
    return out


def gather_form(rows, C, dtype, ntaps):
    CV = C * esize(dtype) // 16
    return dict(CV=CV, dt=256 // CV, dv=256 % CV, trips=-(-ntaps * CV // 256), grid=min(rows, 8192), strided=rows > 8192,
                rows_per_group=-(-rows // 8192))


def scatter_form(npos, C, dtype):
    CV = C * esize(dtype) // 16
    if CV > 256:
        return dict(CV=CV, refuse=True)
    G = min(256 // CV, 4)
    groups = -(-npos // G)
    return dict(CV=CV, refuse=False, G=G, idle=256 - G * CV, grid=min(groups, 8192), strided=groups > 8192)


def im2col_form(rows, ntaps, C, dtype):
    total = rows * ntaps * (C * esize(dtype) // 16)
    return dict(total=total, grid=min(-(-total // 256), 8192), strided=total > 8192 * 256)


def col_plan(ntaps, C, seed, nconst=0, cw=0):
    """column offsets of the tap blocks in permuted order with 8-element gaps, the constant blocks behind them"""
    perm = np.random.RandomState(seed).permutation(ntaps)
    offs = [8 + int(perm[t]) * (C + 8) for t in range(ntaps)]
    end = 8 + ntaps * (C + 8)
    const_offs = [end + (nconst - 1 - k) * (cw + 8) for k in range(nconst)]
    return offs, const_offs, end + nconst * (cw + 8)


def _taps64():
    taps = [(2 * (i % 2) - 2 * (i // 32), (i // 2) % 8 - 3, (i // 16) * 3 - 4) for i in range(60)]
    return taps + [(0, 5, 0), (2, 0, 7), (4, 0, 0), (0, -4, -6)]              # whole blocks outside the 4 x 6 lattice


TAP_LISTS = {'lat18': LAT_TAPS, 'one': [(0, 1, -1)], 'seven': LAT_TAPS[3:10], 'max64': _taps64()}
# im2col: the 80-tap maximum, 60 taps near (at most 60 terms per element of the adjoint) and 20 beyond any lattice used here
TAPS80 = ([(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-2, -1, 0, 1, 2) for dx in (-2, -1, 0, 1)] +
          [(0, 100 + i, 0) for i in range(10)] + [(0, 0, -100 - i) for i in range(10)])
# (B, Z, H, W, C, dtype, taps): 80 taps and 1 tap, Z = 1, the 1 024 000-vector geometry, and 2 150 400 vectors: past the grid cap
IM2COL_CASES = {'taps80_bf16': (2, 4, 5, 7, 8, BF16, TAPS80), 'taps80_f32': (2, 3, 5, 7, 4, F32, TAPS80),
                'one_tap': (2, 4, 5, 7, 16, BF16, [(1, -1, 2)]), 'z1': (2, 1, 5, 7, 8, BF16, TAPS80),
                'rows12800': (2, 4, 40, 40, 8, BF16, TAPS80), 'grid_cap': (2, 4, 60, 56, 8, BF16, TAPS80)}


def z_sizes(layout):
    """(Zs, Zr) of the gather / scatter cases"""
    return (4, 2) if layout >= 2 else (3, 3)


def _gcase(name, layout, dtype, C, taps='lat18', B=2, H=4, W=6, nconst=0, cw=0, Zr=None, Zs=None):
    zs, zr = z_sizes(layout)
    return dict(name=name, layout=layout, dtype=dtype, C=C, taps=taps, B=B, H=H, W=W, nconst=nconst, cw=cw,
                Zs=Zs or zs, Zr=Zr or zr)


CV_SWEEP = [(BF16, 8, 1), (F32, 4, 1), (BF16, 24, 3), (BF16, 96, 12), (BF16, 768, 96), (F32, 768, 192)]


def _gather_cases():
    out = []
    for dtype, C, cv in CV_SWEEP:
        for layout in range(4):
            out.append(_gcase('cv%d_%s_l%d' % (cv, 'bf16' if dtype == BF16 else 'f32', layout), layout, dtype, C))
    out.append(_gcase('cv320_f32_l2', 2, F32, 1280))
    for taps in ('one', 'seven', 'max64'):
        for layout in (0, 3):
            out.append(_gcase('%s_cv3_l%d' % (taps, layout), layout, BF16, 24, taps))
    out.append(_gcase('max64_cv96_l2', 2, BF16, 768, 'max64'))
    for layout in (1, 2):              # CV = 12 with more than 256 vectors per row: the (tap, vector) walk advances and wraps
        out.append(_gcase('max64_cv12_l%d' % layout, layout, BF16, 96, 'max64'))
    out.append(_gcase('max64_cv1_l1', 1, BF16, 8, 'max64'))
    out.append(_gcase('max64_cv1_f32_l0', 0, F32, 4, 'max64'))
    return out


GATHER_CASES = _gather_cases()
CONST_CASES = [_gcase('const1', 2, BF16, 24, nconst=1, cw=8), _gcase('const8', 1, BF16, 24, nconst=8, cw=16),
               _gcase('const8_wide', 2, BF16, 24, nconst=8, cw=264), _gcase('const8_f32', 0, F32, 12, nconst=8, cw=4)]
# grid stride: more than 8 192 rows (gather), an odd row count that takes some workgroups through three rows (both parity
# tables, unevenly), more than 32 768 positions (scatter: G = 4, more than 8 192 groups)
STRIDE_GATHER = [_gcase('rows8640', 2, BF16, 8, taps='two', B=3, H=40, W=36),
                 _gcase('rows16815', 0, BF16, 8, taps='two', B=5, H=59, W=57, Zr=1, Zs=3)]
STRIDE_SCATTER = [_gcase('pos33600', 3, BF16, 8, taps='two', B=3, H=56, W=50)]
TAP_LISTS['two'] = [(0, 0, 1), (2, -1, 0)]


def case_geometry(case):
    taps = TAP_LISTS[case['taps']]
    offs, const_offs, stride = col_plan(len(taps), case['C'], 7 + len(taps), case['nconst'], case['cw'])
    return taps, offs, const_offs, stride


# ------------------------------------------------------------------------------------------------- channel-first rows
def _cf_index(Z, H, W, C, swap_xy=False):
    z, y, x, c = torch.meshgrid(torch.arange(Z), torch.arange(H), torch.arange(W), torch.arange(C), indexing='ij')
    idx = ((c * Z + z) * W + x) * H + y if swap_xy else ((c * Z + z) * H + y) * W + x
    return idx.reshape(-1)


def channel_first_ref(plain, cf_stride, fill=SENTINEL, swap_xy=False, y0_zero_R=None):
    """cf[b, ((c Z + z) H + y) W + x] = plain[b, z, y, x, c]; the tail of a row keeps ``fill``.  y0_zero_R: the tile rows of
    a kernel whose spatial tiles all start at y = 0 (tiles of R rows)."""
    B, Z, H, W, C = plain.shape
    cf = torch.full((B, cf_stride), fill, dtype=plain.dtype)
    src = plain if y0_zero_R is None else plain[:, :, torch.arange(H) % y0_zero_R]
    cf[:, _cf_index(Z, H, W, C, swap_xy)] = src.reshape(B, -1)
    return cf


def from_channel_first(cf, Z, H, W, C):
    return cf[:, _cf_index(Z, H, W, C)].view(cf.shape[0], Z, H, W, C)


def tile_rows(H, W, es, to_wide):
    """R of the vector transposes / ver_lattice_rows: towards channel-first (rows) the largest divisor of H whose 32-channel
    tile stays under 48 KB and 1 200 positions; the other way one row"""
    R = 1
    if to_wide:
        for cand in range(1, H + 1):
            if H % cand == 0 and 32 * (cand * W + 4) * es <= 48 * 1024 and cand * W <= 1200:
                R = cand
    return R


def transpose_form(B, Z, H, W, C, dtype, to_cf, cf_stride, cf_offset=0):
    """the launcher's choice; cf_offset: elements between an aligned address and the channel-first buffer"""
    es = esize(dtype)
    vc, vx = 16 // es, 8 // es
    if B == 0:
        return dict(form='none')
    pre = dict(w=W % vx == 0, c=C % vc == 0, stride=cf_stride % vx == 0, align=(cf_offset * es) % 8 == 0, zhw=(Z * H * W) % vx == 0)
    if all(pre.values()) and 128 * (W + 4) * es <= 64 * 1024:
        R = tile_rows(H, W, es, to_cf)
        ch = 32 if to_cf else 128
        return dict(form='vector', R=R, hr=H // R, ch=ch, blocks=-(-C // ch), lds=ch * (R * W + 4) * es, pre=pre,
                    grid=B * Z * (H // R) * -(-C // ch))
    lds = 128 * (W + 1) * es
    if lds > 64 * 1024:
        return dict(form='refuse', pre=pre)
    return dict(form='scalar', R=1, hr=H, ch=128, blocks=-(-C // 128), lds=lds, pre=pre, grid=B * Z * H * -(-C // 128))


def _tcase(name, dtype, Z, H, W, C, B=2, tail=8, cf_offset=0, want='vector', fails=None, R=None):
    return dict(name=name, dtype=dtype, Z=Z, H=H, W=W, C=C, B=B, tail=tail, cf_offset=cf_offset, want=want, fails=fails, R=R)


TRANSPOSE_CASES = [
    _tcase('tiles_bf16', BF16, 4, 16, 64, 40, R=8), _tcase('tiles_f32', F32, 4, 16, 32, 36, R=8),
    _tcase('min_bf16', BF16, 4, 2, 4, 8), _tcase('min_f32', F32, 4, 2, 2, 4),
    _tcase('z1_bf16', BF16, 1, 4, 8, 16), _tcase('z3_f32', F32, 3, 4, 6, 8),
    _tcase('w_bf16', BF16, 4, 4, 6, 8, want='scalar', fails='w'), _tcase('w_f32', F32, 4, 4, 3, 4, want='scalar', fails='w'),
    _tcase('c_bf16', BF16, 4, 4, 8, 12, want='scalar', fails='c'), _tcase('c_f32', F32, 4, 4, 6, 6, want='scalar', fails='c'),
    _tcase('stride_bf16', BF16, 4, 4, 8, 8, tail=1, want='scalar', fails='stride'),
    _tcase('stride_f32', F32, 4, 4, 6, 4, tail=1, want='scalar', fails='stride'),
    _tcase('align_bf16', BF16, 4, 4, 8, 8, cf_offset=1, want='scalar', fails='align'),
    _tcase('align_f32', F32, 4, 4, 6, 4, cf_offset=1, want='scalar', fails='align'),
    _tcase('c130_bf16', BF16, 4, 4, 6, 130, want='scalar', fails=None), _tcase('c130_f32', F32, 3, 2, 5, 130, want='scalar', fails=None),
    _tcase('w126_f32', F32, 1, 2, 126, 4, want='scalar', fails=None),
]


def transpose_layouts(case):
    return [l for l in range(4) if layout_legal(l, case['Z'], case['H'], case['W'])]


# ---------------------------------------------------------------------------------------------------------- row map
def make_row_map(L, quarter, period, seg_lens, B, slack=8, gap=12):
    """a hand-made map: segment pitches with ``slack`` beyond (L / quarter) seg_len, bases with gaps in DEScending order"""
    n, nk, n_rows = len(seg_lens), L // quarter, quarter // period
    seg_off = [sum(seg_lens[:j]) for j in range(n)]
    pitch = [nk * s + slack for s in seg_lens]
    base, pos = [0] * n, gap
    for j in reversed(range(n)):
        base[j] = pos
        pos += B * n_rows * pitch[j] + gap
    return dict(quarter=quarter, period=period, seg_off=seg_off, seg_len=list(seg_lens), seg_base=base, seg_pitch=pitch,
                seg_rows=[n_rows] * n, total=pos)


def row_map_refusal(rm, Z, H, W, C):
    """the launcher's rules (ver_lattice_rows), None when the map is legal"""
    L, q, p, n = C * Z * H * W, rm['quarter'], rm['period'], len(rm['seg_off'])
    if not 1 <= n <= 8:
        return 'nseg'
    if not (L < 2 ** 31 and q > 0 and p > 0 and L % q == 0 and q % p == 0):
        return 'quarter / period'
    if not (W % 4 == 0 and C % 8 == 0 and (Z * H * W) % 4 == 0):
        return 'W % 4, C % 8'
    if not (p <= 4096 and q % (H * W) == 0):
        return 'period > 4096 or a plane straddles two quarters'
    covered = 0
    for j in range(n):
        so, sl, sp, sb, sr = (rm[k][j] for k in ('seg_off', 'seg_len', 'seg_pitch', 'seg_base', 'seg_rows'))
        if not (so == covered and sl > 0 and sl % 4 == 0 and sp % 4 == 0 and sb % 4 == 0 and sb >= 0 and sr * p == q and
                (L // q) * sl <= sp):
            return 'segment %d' % j
        covered += sl
    if covered != p:
        return 'cover'
    if 128 * (W + 4) * 2 > 64 * 1024:
        return 'too wide'
    return None


def _segment_dest(rm, b, k, row, off, seg_of):
    dest = torch.full_like(off, -1)
    for j in range(len(rm['seg_off'])):
        so, sl = rm['seg_off'][j], rm['seg_len'][j]
        m = (seg_of >= so) & (seg_of < so + sl)
        dest[m] = rm['seg_base'][j] + (b * rm['seg_rows'][j] + row[m]) * rm['seg_pitch'][j] + k[m] * sl + (off[m] - so)
    assert bool((dest >= 0).all())
    return dest


def row_map_dest(flat, b, rm):
    """element of ``rows`` that holds channel-first flat index ``flat`` of sample b: flat = k quarter + row period + off"""
    k, rem = flat // rm['quarter'], flat % rm['quarter']
    row, off = rem // rm['period'], rem % rm['period']
    return _segment_dest(rm, b, k, row, off, off)


def row_map_dest_tiled(flat, b, rm, P, wrap=True):
    """the kernel's route to the same element: (k, row, off) of the first piece of a channel's tile run (P positions), the
    piece's position added, wrapped over as many periods as it takes.  Returns (dest, most wraps of one piece)."""
    flat0 = flat // P * P
    k, rem = flat0 // rm['quarter'], flat0 % rm['quarter']
    row, off = rem // rm['period'], rem % rm['period'] + (flat - flat0)
    wraps = off // rm['period']
    seg_of = off % rm['period']
    if wrap:
        row, off = row + wraps, seg_of
    return _segment_dest(rm, b, k, row, off, seg_of), int(wraps.max())


def lattice_rows_ref(plain, rm, fill=SENTINEL, dest=row_map_dest):
    B, Z, H, W, C = plain.shape
    L = C * Z * H * W
    cf = channel_first_ref(plain, L)
    buf = torch.full((rm['total'],), fill, dtype=plain.dtype)
    flat = torch.arange(L)
    for b in range(B):
        buf[dest(flat, b, rm)] = cf[b]
    return buf


def lattice_from_rows_ref(rows, rm, B, Z, H, W, C):
    flat = torch.arange(C * Z * H * W)
    cf = torch.stack([rows[row_map_dest(flat, b, rm)] for b in range(B)])
    return from_channel_first(cf, Z, H, W, C)


def rows_form(Z, H, W, C, rm, to_rows):
    R = tile_rows(H, W, 2, to_rows)
    ch = 32 if to_rows else 128
    P = R * W
    flat = torch.arange(C * Z * H * W)
    _, wraps = row_map_dest_tiled(flat, 0, rm, P)
    return dict(R=R, hr=H // R, run=P, ch=ch, blocks=-(-C // ch), wraps=wraps, nseg=len(rm['seg_off']),
                slots=rm['period'] // 4, k_max=C * Z * H * W // rm['quarter'] - 1)


SEGS = {'p16_1': (16, (16,)), 'p16_2': (16, (4, 12)), 'p64_8': (64, (4, 4, 8, 8, 8, 8, 12, 12)), 'p64_2': (64, (4, 60)),
        'p256_1': (256, (256,)), 'p256_2': (256, (4, 252)),
        'p80_3': (80, (16, 4, 60))}      # (C = 40 only: a tile run starts inside a period and wraps in its middle)


def _rcase(name, Z, H, W, C, quarter, period, segs, B=2):
    return dict(name=name, Z=Z, H=H, W=W, C=C, B=B, rm=make_row_map(C * Z * H * W, quarter, period, segs, B))


def _rows_cases():
    out = []
    for C in (16, 40):                                       # geometry A
        L = C * 4 * 64
        for sname, (period, segs) in SEGS.items():
            for qname, quarter in (('plane', 64), ('quarter', L // 4), ('all', L)):
                if L % quarter or quarter % period or quarter % 64:
                    continue
                case = _rcase('A_c%d_%s_%s' % (C, sname, qname), 4, 8, 8, C, quarter, period, segs)
                if row_map_refusal(case['rm'], 4, 8, 8, C) is None:
                    out.append(case)
    out.append(_rcase('B_tiles', 4, 16, 64, 8, 1024, 256, (4, 252)))          # geometry B: two spatial tiles per plane
    out.append(_rcase('B_tiles_p64', 4, 16, 64, 8, 8192, 64, SEGS['p64_8'][1]))
    out.append(_rcase('C_last_slot', 4, 16, 16, 16, 4096, 4096, (4, 4092)))     # geometry C: slot 1023 of the table
    return out


ROWS_CASES = _rows_cases()


# -------------------------------------------------------------------------------------------------------- run copies
def run_copy_form(rows_total, runs, run_len, n_aug, dtype, gather):
    ve = 8 // esize(dtype)
    per_row = runs * (run_len // ve) + (n_aug if gather else 0)
    want = -(-rows_total // 4) if per_row <= 256 else -(-rows_total * per_row // 1024)
    return dict(per_row=per_row, form='rows' if per_row <= 256 else 'flat', tail=rows_total % 4 if per_row <= 256 else 0,
                grid=min(max(want, 1), 16384), strided=want > 16384)


def run_case(name, dtype):
    """tables of a run-copy case: dict(B, n_rows, runs, run_len, n_aug, row_elems, image_len, image_stride, run_start, aug_idx,
    tiling) -- 'tiling': the runs tile the image exactly once (what the scatter needs), else they overlap"""
    ve = 8 // esize(dtype)
    spec = {  # B, n_rows, runs, run_len, n_aug, row padding, image padding, tiling
        'tail1': (3, 3, 2, 8, 0, 0, 0, True), 'tail2': (2, 5, 3, 4, 3, 8, 4, True), 'tail3': (3, 5, 2, 12, 3, 4, 8, True),
        'overlap': (2, 5, 3, 8, 3, 4, 4, False), 'flat': (1, 7, 3, 100 * ve, 5, 4, 8, True),
        'flat_overlap': (1, 7, 3, 100 * ve, 5, 4, 8, False), 'stride': (1, 65541, 1, ve, 0, 0, 0, True)}[name]
    B, n_rows, runs, run_len, n_aug, rpad, ipad, tiling = spec
    rs = np.random.RandomState(len(name) + run_len)
    n = n_rows * runs
    image_len = n * run_len
    if tiling:
        start = rs.permutation(n) * run_len
    else:
        start = rs.randint(0, (image_len - run_len) // 4 + 1, n) * 4
    return dict(name=name, B=B, n_rows=n_rows, runs=runs, run_len=run_len, n_aug=n_aug, row_elems=runs * run_len + n_aug + rpad +
                (-(runs * run_len + n_aug + rpad)) % 4, image_len=image_len, image_stride=image_len + ipad, tiling=tiling,
                run_start=torch.from_numpy(start.reshape(n_rows, runs).astype(np.int32)),
                aug_idx=torch.from_numpy(rs.randint(0, image_len, (n_rows, n_aug)).astype(np.int32)))


RUN_CASES = ['tail1', 'tail2', 'tail3', 'overlap', 'flat', 'flat_overlap', 'stride']


def _run_rows(c, dup_tail):
    total = c['B'] * c['n_rows']
    r = torch.arange(total)
    src = r.clone()
    if dup_tail:                      # the rows of the last, partial four-row trip all take the trip's first row
        src[total // 4 * 4:] = total // 4 * 4
    return r, src // c['n_rows'], src % c['n_rows']


def run_gather_ref(image, c, fill=SENTINEL, dup_tail=False):
    """rows[(b n_rows + i), k run_len + o] = image[b, run_start[i, k] + o]; rows[.., runs run_len + j] = image[b, aug_idx[i, j]]"""
    r, b, i = _run_rows(c, dup_tail)
    rows = torch.full((len(r), c['row_elems']), fill, dtype=image.dtype)
    o, rl = torch.arange(c['run_len']), c['run_len']
    for k in range(c['runs']):
        rows[:, k * rl:(k + 1) * rl] = image[b[:, None], c['run_start'][i, k].long()[:, None] + o]
    for j in range(c['n_aug']):
        rows[:, c['runs'] * rl + j] = image[b, c['aug_idx'][i, j].long()]
    return rows


def run_scatter_ref(rows, c, fill=SENTINEL, dup_tail=False):
    """image[b, run_start[i, k] + o] = rows[(b n_rows + i), k run_len + o]; what no run names keeps ``fill``"""
    r, b, i = _run_rows(c, dup_tail)
    image = torch.full((c['B'], c['image_stride']), fill, dtype=rows.dtype)
    o, rl = torch.arange(c['run_len']), c['run_len']
    for k in range(c['runs']):
        image[b[:, None], c['run_start'][i, k].long()[:, None] + o] = rows[:, k * rl:(k + 1) * rl]
    return image


# ------------------------------------------------------------------------------------------- ConvTranspose3d weights
PAIR_CASES = [(5, 7), (3, 43), (8, 8)]
BLOCK_CASES = [(5, 6), (3, 44)]                   # forward_blocks / backward_blocks: even Co; 132 pairs = two groups of 128


def taps_ref(w, dtype, flip=(2, 3, 4), skip_ragged=False):
    """correlation taps [75, Ci, Co] of a ConvTranspose3d weight [Ci, Co, 3, 5, 5]: tap (a, b, c) = w[.., 2-a, 4-b, 4-c]"""
    ci, co = w.shape[:2]
    out = w.flip(*flip).permute(2, 3, 4, 0, 1).reshape(75, ci, co).to(dtype)
    if skip_ragged:
        out.view(75, -1)[:, ci * co // 64 * 64:] = 0
    return out


def taps_adjoint_ref(g):
    _, ci, co = g.shape
    return g.float().view(3, 5, 5, ci, co).permute(3, 4, 0, 1, 2).flip(2, 3, 4).contiguous()


def weight_specials():
    """fp32 values whose bf16 rounding is the interesting part: exact ties both ways, +-inf, subnormals, -0, overflow to inf"""
    b = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x80000000,
         0x7F7FFFFF, 0x00008000, 0x00018000]
    return torch.tensor([v - 2 ** 32 if v >= 2 ** 31 else v for v in b], dtype=torch.int32).view(F32)


def block_offsets_case(ci, co, ld):
    """a hand-made offset table [75][2]: tap t's block at row slot (7 t) % 75 (lower half), every third tap also in the upper
    half of slot (11 t + 3) % 75, every fifth tap nowhere; returns (int64 [75, 2], rows of the stacked matrix)"""
    off = torch.full((75, 2), -1, dtype=torch.int64)
    for t in range(75):
        if t % 5 == 4:
            continue
        off[t, 0] = ((7 * t) % 75) * ci * ld
        if t % 3 == 0:
            off[t, 1] = ((11 * t + 3) % 75) * ci * ld + co
    return off, 75 * ci


def forward_blocks_ref(w, off, ld, blocks):
    """tap t's [Ci x Co] block written at element offsets off[t][0..1] of ``blocks`` (row pitch ld); the rest untouched"""
    ci, co = w.shape[:2]
    k = taps_ref(w, blocks.dtype)
    flat = blocks.clone().view(-1)
    for t in range(75):
        for h in range(2):
            o = int(off[t, h])
            if o < 0:
                continue
            for i in range(ci):
                flat[o + i * ld:o + i * ld + co] = k[t, i]
    return flat.view(blocks.shape)


def backward_blocks_ref(blocks, off, ld, ci, co, prev_bias=None, grad_v=None):
    flat = blocks.double().reshape(-1)
    k = torch.zeros(75, ci, co, dtype=torch.float64)
    for t in range(75):
        for h in range(2):
            o = int(off[t, h])
            if o < 0:
                continue
            for i in range(ci):
                k[t, i] += flat[o + i * ld:o + i * ld + co]
        if prev_bias is not None:
            k[t] += prev_bias.double()[:, None] * grad_v[t].double()[None, :]
    return k.view(3, 5, 5, ci, co).permute(3, 4, 0, 1, 2).flip(2, 3, 4).contiguous()


def blocks_vec_ref(blocks, block_rows, ci, x):
    """vec[b][col] = sum_ci x[ci] blocks[block_rows[b] + ci][col], fp64"""
    s = blocks.double()
    return torch.stack([sum(float(x[i]) * s[int(r) + i] for i in range(ci)) for r in block_rows])


def blocks_vec_adjoint_ref(blocks, block_rows, ci, grad_vec):
    """grad_x[ci] = sum_b sum_col blocks[block_rows[b] + ci][col] grad_vec[b][col], fp64"""
    s, g = blocks.double(), grad_vec.double()
    return torch.stack([sum((s[int(r) + i] * g[n]).sum() for n, r in enumerate(block_rows)) for i in range(ci)])


def blocks_vec_form(ci, ncols):
    per = -(-ci // 8)
    return dict(xblocks=-(-(ncols // 2) // 256), live_last=ncols // 2 - (-(-(ncols // 2) // 256) - 1) * 256,
                slices=[max(0, min(ci, (z + 1) * per) - z * per) for z in range(8)])


VEC_CASES = [(9, 520), (1, 520), (9, 6)]           # (Ci, ncols): a second x-block with four live lanes; slices 2,2,2,2,1,0,0,0


@functools.lru_cache(maxsize=None)
def vec_case(ci, ncols, dtype):
    """(stacked matrix [rows, ncols] of integers, block rows in arbitrary order with a repeat, x, grad_vec)"""
    rows = 4 * ci + 3
    s = int_data((rows, ncols), dtype, 3 * ci + ncols)
    block_rows = torch.tensor([2 * ci + 3, 0, ci + 1, 0, 3 * ci + 3], dtype=torch.int64)
    x = int_data((ci,), F32, ci)
    gv = int_data((len(block_rows), ncols), F32, ncols)
    return s, block_rows, x, gv
