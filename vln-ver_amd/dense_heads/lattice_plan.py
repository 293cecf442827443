"""Index geometry of the even-lattice ``ConvTranspose3d`` layers (``upsample.py``): the column order of a layer's tap matrix,
the row order of its stacked weight matrix, and the index tables the Functions and the HIP kernels address both with.  numpy
and index tensors only: no autograd, no kernel calls, no environment reads.  Every table is built -- and uploaded -- once per
argument tuple (``_memo``), so the warm-up step of a captured graph (graphs.py) leaves no host-to-device copy for the capture.

Parity-class layers (layers 1 and 2 of the stack).  All four output classes (pm, pn) read taps of the same 3x3x3
neighbourhood (dz in {-2,0,2}, dy, dx in {-1,0,1}) of the input lattice: class pn=1 only dx in {0,1}, pm=1 only dy in {0,1}.
So ONE 27-tap matrix A [B*Z*H*W, Kt] serves the four classes (27 instead of 75 tap blocks are written / read back).  The
(dy, dx) pairs are ordered in four groups
    G1 = (dy-, dx-) | G2 = (dy+, dx-) | G3 = (dy+, dx+) | G4 = (dy-, dx+)      (- : -1, + : {0, 1})
so that EVERY class is one contiguous column range: (0,0) = G1..G4, (1,0) = G2 G3, (1,1) = G3, (0,1) = G3 G4.  Four constant
blocks P_class = [75 0/1 pattern columns | 1 | 0 ...] sit between the groups, with weight rows (K[tap]^T prev_bias | bias):
the bias-valued odd positions of the input and the layer bias ride in the same GEMM.  Layout of a row (C = channels):
    [P00 | G1 | P10 | G2 | P11 | G3 | G4 | P01]
  (0,0): P00..G4 (P10, P11 meet zero weight rows)      (1,0): P10 G2 P11 G3 (P11 -> zero rows)
  (1,1): P11 G3                                          (0,1): G3 G4 P01

Z = 4 (vocc.py: bev_z = 4).  The z taps of the stack are dz in {-2, 0, +2}: with four z-layers every output layer has exactly
TWO in-range taps -- z = 0,1 read the input layers (z, z+2), z = 2,3 read (z-2, z) -- and both halves read the SAME pair
(zl, zl+2), zl = z & 1.  So the tap matrix needs only the rows (b, zl, y, x) and 2 instead of 3 z blocks per (dy, dx); the two
output halves come out of ONE GEMM side by side, A [B*2*H*W, K] x [W_lo | W_hi] [K, 2*Co]: block j (dz = 2 j) meets
K[a = 1 + j] in W_lo and K[a = j] in W_hi (``_half_taps``), and a constant block is the pair [P_lo | P_hi].
"""
import functools

import numpy as np
import torch

from ._cpu_algebra import CLASSES as _CLASSES

# width of a constant block: 75 pattern columns + the ones column, padded to 96 so that the lo | hi pair of a Z = 4 layer is 192
# = 3 x 64 columns and every segment of the K axis starts on a multiple of 64 -- what the implicit operand loaders want
# (ver_gemm_nn_segments: whole 32-column phases; ver_wgrad_tn_segments: a wave's 64-column piece inside ONE segment)
_PW = 96
_PW2 = 2 * _PW                                                         # lo | hi constant blocks


def _memo(fn):
    """``fn(*args)`` once per argument tuple, a ``torch.device`` keyed by its string."""
    cache = {}

    @functools.wraps(fn)
    def memoised(*args):
        key = tuple(str(a) if isinstance(a, torch.device) else a for a in args)
        if key not in cache:
            cache[key] = fn(*args)
        return cache[key]
    return memoised


def _index(a, device):
    return torch.from_numpy(np.asarray(a, dtype=np.int64)).to(device)


def _group_of(dyi, dxi):
    yp, xp = dyi > 0, dxi > 0
    return 0 if (not yp and not xp) else 1 if (yp and not xp) else 2 if (yp and xp) else 3


class _Columns:
    """Column geometry of a class-layout tap matrix with ``nz`` z blocks per (dy, dx) and constant blocks ``pw`` wide:
    ``order``: the blocks (dxi, dyi, zi) in column order -- groups G1..G4, inside a group (dx, dy, z); ``taps``: their
    (dz, dy, dx); ``start``: first block of every group (+ the block count); ``layout``: per class its K axis as segments
    ('b', block position) / ('c', class whose constant block sits there), in column order."""

    def __init__(self, nz, pw):
        self.pw = pw
        blocks = [(dxi, dyi, zi) for dxi in range(3) for dyi in range(3) for zi in range(nz)]
        self.order = sorted(blocks, key=lambda b: (_group_of(b[1], b[0]), b))
        # nz = 3: dz in {-2, 0, 2} around the row's z; nz = 2: rows are the lower layers zl, dz in {0, 2}
        self.taps = [(2 * (zi + 2 - nz), dyi - 1, dxi - 1) for dxi, dyi, zi in self.order]
        groups = [_group_of(dyi, dxi) for dxi, dyi, _ in self.order]
        g = self.start = [groups.index(q) for q in range(4)] + [len(blocks)]
        b = lambda lo, hi: [('b', t) for t in range(lo, hi)]
        self.layout = {
            (0, 0): [('c', (0, 0))] + b(g[0], g[1]) + [('c', (1, 0))] + b(g[1], g[2]) + [('c', (1, 1))] + b(g[2], g[4]),
            (1, 0): [('c', (1, 0))] + b(g[1], g[2]) + [('c', (1, 1))] + b(g[2], g[3]),
            (1, 1): [('c', (1, 1))] + b(g[2], g[3]),
            (0, 1): b(g[2], g[4]) + [('c', (0, 1))],
        }

    def width(self, c):
        return len(self.order) * c + 4 * self.pw

    def block_offset(self, t, c):
        """column of the t-th block: P00 sits before G1, P10 before G2, P11 before G3."""
        return self.pw * (1 + (t >= self.start[1]) + (t >= self.start[2])) + t * c

    def block_offsets(self, c):
        return [self.block_offset(t, c) for t in range(len(self.order))]

    def const_offset(self, cls, c):
        g, pw = self.start, self.pw
        return {(0, 0): 0, (1, 0): pw + g[1] * c, (1, 1): 2 * pw + g[2] * c, (0, 1): 3 * pw + g[4] * c}[cls]

    def first_column(self, cls, c):
        kind, val = self.layout[cls][0]
        return self.block_offset(val, c) if kind == 'b' else self.const_offset(val, c)


_COLS3 = _Columns(3, _PW)             # any Z: 27 blocks
_COLS4 = _Columns(2, _PW2)            # Z = 4: 18 blocks, both output halves side by side


def _tap_id(a, bb, cc):
    """index of tap (a, bb, cc) in the 75-tap correlation kernel."""
    return (a * 5 + bb) * 5 + cc


def _half_taps(bb, cc, j):
    """Z = 4: ids of the taps through which block (bb, cc, j) feeds the lower (a = 1 + j) / upper (a = j) output half."""
    return _tap_id(1 + j, bb, cc), _tap_id(j, bb, cc)


def _class_half_taps(cls, t):
    """``_half_taps`` of the t-th block of ``_COLS4`` as class ``cls`` sees it."""
    dxi, dyi, j = _COLS4.order[t]
    bb, cc = 2 * dyi - cls[0], 2 * dxi - cls[1]
    assert 0 <= bb < 5 and 0 <= cc < 5
    return _half_taps(bb, cc, j)


def _class_tap_id(pm, pn, t):
    """id in the 75-tap correlation kernel of the t-th block for class (pm, pn), or None."""
    dxi, dyi, dzi = _COLS3.order[t]
    bb, cc = 2 * dyi - pm, 2 * dxi - pn
    return _tap_id(dzi, bb, cc) if 0 <= bb < 5 and 0 <= cc < 5 else None


# blocks (bb, cc, j) of the 5x5x2 neighbourhood of the first Z = 4 layer (every tap hits data), in column order
_L0_BLOCKS = [(bb, cc, j) for bb in range(5) for cc in range(5) for j in range(2)]


@_memo
def _constant_pattern(z, h_in, w_in, device, dtype):
    """[Z*h_in*w_in, 75] 0/1: tap (a,b,c) of output position (z,m,n) lands in-bounds on a
    NON-data position of a full-resolution input of size (Z, h_in, w_in) whose data lattice is the
    even rows/cols."""
    zz, mm, nn = np.meshgrid(np.arange(z), np.arange(h_in), np.arange(w_in), indexing='ij')
    pat = np.zeros((z, h_in, w_in, 3, 5, 5), dtype=np.float32)
    for a in range(3):
        iz = zz - 2 + 2 * a
        for b in range(5):
            iy = mm - 2 + b
            for c in range(5):
                ix = nn - 2 + c
                inb = (iz >= 0) & (iz < z) & (iy >= 0) & (iy < h_in) & (ix >= 0) & (ix < w_in)
                data = (iy % 2 == 0) & (ix % 2 == 0)
                pat[:, :, :, a, b, c] = inb & ~data
    return torch.from_numpy(pat.reshape(z * h_in * w_in, 75)).to(device=device, dtype=dtype)


@_memo
def _class_patterns(z, h, w, device, dtype):
    """[4][Z*H*W, _PW]: constant-block columns of class p for an input lattice (Z,H,W)."""
    full = _constant_pattern(z, 2 * h, 2 * w, device, dtype).view(z, 2 * h, 2 * w, 75)
    pats = []
    for pm, pn in _CLASSES:
        p = full.new_zeros(z, h, w, _PW)
        p[..., :75] = full[:, pm::2, pn::2]
        p[..., 75] = 1
        pats.append(p.view(z * h * w, _PW))
    return pats


@_memo
def _const_rows_z4(ci, hc, wc, device, dtype):
    """The constant-pattern blocks of one viewpoint's rows of a Z = 4 lattice layer, as the gather kernel copies them:
    [2*hc*wc, 4 classes, 2*_PW] = per class [P_lo | P_hi], and their column offsets."""
    blocks = []
    for pat in _class_patterns(4, hc, wc, device, dtype):
        halves = pat.view(2, 2 * hc * wc, _PW)                  # output z = zl (lower), zl + 2 (upper)
        blocks.append(torch.cat([halves[0], halves[1]], 1))
    table = torch.stack(blocks, 1).contiguous()                 # [2hw, 4, 2*_PW]
    return table, [_COLS4.const_offset(cls, ci) for cls in _CLASSES]


@_memo
def _layer_plan(ci, device):
    """-> ({class: (col_start, col_end, row index into the stacked weight rows [75*ci data | 4*_PW own-constant | 3*_PW
    dummy zero])}, columns of the tap matrix, stacked rows)."""
    n_data = 75 * ci
    dummy = n_data + 4 * _PW                         # next free dummy row
    plan = {}
    for cls, segs in _COLS3.layout.items():
        rows = []
        for kind, val in segs:
            if kind == 'b':
                tid = _class_tap_id(*cls, val)
                assert tid is not None
                rows.append(np.arange(tid * ci, (tid + 1) * ci))
            elif val == cls:                         # own constant block
                p = _CLASSES.index(val)
                rows.append(np.arange(n_data + p * _PW, n_data + (p + 1) * _PW))
            else:                                    # foreign constant block: zero rows
                rows.append(np.arange(dummy, dummy + _PW))
                dummy += _PW
        rows = np.concatenate(rows)
        c0 = _COLS3.first_column(cls, ci)
        plan[cls] = (c0, c0 + len(rows), _index(rows, device))
    assert dummy == n_data + 7 * _PW
    return plan, _COLS3.width(ci), dummy


@_memo
def _layer0_z4_plan(ci, device):
    """blocks (bb, cc, j) of the 5x5x2 neighbourhood: their taps and column offsets; row indices into k.reshape(75*ci, co)
    of the taps feeding the lower (a = 1 + j) and the upper (a = j) output half."""
    taps = [(2 * j, bb - 2, cc - 2) for bb, cc, j in _L0_BLOCKS]
    lo, hi = zip(*[[np.arange(ci) + t * ci for t in _half_taps(*blk)] for blk in _L0_BLOCKS])
    return taps, [i * ci for i in range(50)], _index(np.concatenate(lo), device), _index(np.concatenate(hi), device)


def _class_rows_z4(ci):
    """{class: (first row of the class in the class-stacked [sum K_c, 2 Co] buffer (classes in _CLASSES order),
    [(kind, val, first row inside the class)])}."""
    out, roff = {}, 0
    for cls in _CLASSES:
        segs, r = [], 0
        for kind, val in _COLS4.layout[cls]:
            segs.append((kind, val, r))
            r += ci if kind == 'b' else _PW2
        out[cls] = (roff, segs)
        roff += r
    return out


def _class_blocks_z4(ci):
    """Every tap block of the class-stacked buffer, in row order: (class index, class, first row, block position t)."""
    for p, (cls, (roff, segs)) in enumerate(_class_rows_z4(ci).items()):
        for kind, val, r0 in segs:
            if kind == 'b':
                yield p, cls, roff + r0, val


def _class_segments_z4(cls, ci):
    """The K axis of class ``cls`` as the segments ``hipops.gemm_nn_taps`` takes, in column order of the tap matrix: a tap
    (dz, dy, dx) per block, ('c', p) for the constant-pattern block of class index p."""
    return [_COLS4.taps[val] if kind == 'b' else ('c', _CLASSES.index(val)) for kind, val in _COLS4.layout[cls]]


@_memo
def _block_offsets(kind, ci, co, device):
    """int64 [75, 2] for ``ver_convt_weight_backward_blocks``: element offsets, inside the [rows, 2 Co] weight-gradient
    buffer of a z-split layer, of the [Ci x Co] block that holds tap t's "lower half" / "upper half" gradient (-1: none).
    kind 'l0': layer 0 (50 blocks (bb, cc, j) in a row); 'lat': the class-stacked buffer of the parity-class layers."""
    if kind == 'l0':
        blocks = [(_half_taps(*blk), i * ci) for i, blk in enumerate(_L0_BLOCKS)]
    else:
        blocks = [(_class_half_taps(cls, t), row) for _, cls, row, t in _class_blocks_z4(ci)]
    off = np.full((75, 2), -1, dtype=np.int64)
    for taps, row in blocks:
        for half, t in enumerate(taps):
            assert off[t, half] == -1
            off[t, half] = row * 2 * co + half * co
    a = np.arange(75) // 25
    assert ((off[:, 0] >= 0) == (a >= 1)).all() and ((off[:, 1] >= 0) == (a <= 1)).all()
    return _index(off, device)


@_memo
def _dgrad_plan(kind, ci, device):
    """d(input) of a Z = 4 layer as gather-form products: per input half j the blocks that read it -- (first row of the
    block in the layer's stacked weight matrix) as an index tensor, and the (dz, dy, dx) taps / source planes of
    ``hipops.gemm_nn_taps`` on the output gradient: block (class p, dy, dx, j) of the forward contributes
    g_p[cell - (dy, dx)][half h] W_block[:, h]^T for both output halves h (K order: block, h, co).
    kind 'l0': layer 1 (one plane, 25 (bb, cc) blocks per j); 'lat': the class-stacked layers (4 planes)."""
    per_j = ([], [])
    if kind == 'l0':
        for i, (bb, cc, j) in enumerate(_L0_BLOCKS):
            per_j[j].append((0, i * ci, bb - 2, cc - 2))
    else:
        for p, _, row, t in _class_blocks_z4(ci):
            dxi, dyi, j = _COLS4.order[t]
            per_j[j].append((p, row, dyi - 1, dxi - 1))
    # both input halves read the SAME (class, dy, dx, h) sequence of the output gradient: one operand, weights side by side
    assert [q[2:] for q in per_j[0]] == [q[2:] for q in per_j[1]] and [q[0] for q in per_j[0]] == [q[0] for q in per_j[1]]
    rows = np.stack([np.stack([np.arange(r0, r0 + ci) for _, r0, _, _ in per_j[j]]) for j in range(2)], 1)    # (block, j, ci)
    taps = [(2 * h, -dy, -dx) for _, _, dy, dx in per_j[0] for h in range(2)]
    planes = [p for p, _, _, _ in per_j[0] for _ in range(2)]
    return _index(rows.reshape(-1), device), taps, planes, len(per_j[0])


@_memo
def _aug_rows_z4(ci, device):
    """Rows of the class-stacked buffer viewed as [2 sum K_c, Co] (row 2r + half) that hold the gradient of a class's own
    constant block: [4 classes x (lower, upper)] x _PW."""
    idx = []
    for cls, (roff, segs) in _class_rows_z4(ci).items():
        r0 = next(r for kind, val, r in segs if kind == 'c' and val == cls)
        idx.append(2 * (roff + r0 + np.arange(_PW)))                    # [P_lo] rows, lower-half columns
        idx.append(2 * (roff + r0 + _PW + np.arange(_PW)) + 1)          # [P_hi] rows, upper-half columns
    return _index(np.concatenate(idx), device)


@_memo
def _stack_tables_z4(ci, device):
    """Index tables of the class-stacked weight matrix S [sum K_c, 2 Co] of a Z = 4 lattice layer (rows: ``_class_rows_z4``),
    viewed as S2 [2 sum K_c, Co] (row 2 r + half) where rows are addressed:
    ``block_rows`` int64 [50]: first row of every tap block; ``tap_slot`` int64 [75]: 2 * block + half of ONE slot that
    holds tap t (a tap with a = 1 sits in two: the lower half of j = 0 and the upper half of j = 1; the first is taken);
    ``const_rows`` / ``const_src``: the S2 rows of all constant blocks and, for each, the row of [vaug (_PW) | zero row] it
    holds (own block, matching half: K^T b_prev | bias | 0; everything else zero)."""
    block_rows, tap_slot = [], np.full(75, -1, dtype=np.int64)
    for i, (_, cls, row, t) in enumerate(_class_blocks_z4(ci)):
        block_rows.append(row)
        for half, tap in enumerate(_class_half_taps(cls, t)):
            if tap_slot[tap] < 0:
                tap_slot[tap] = 2 * i + half
    const_rows, const_src = [], []
    for cls, (roff, segs) in _class_rows_z4(ci).items():
        for kind, val, r0 in segs:
            if kind == 'c':
                for r in range(_PW2):                           # rows [P_lo (_PW) | P_hi (_PW)] of the block
                    for half in range(2):
                        const_rows.append(2 * (roff + r0 + r) + half)
                        live = val == cls and ((r < _PW and half == 0) or (r >= _PW and half == 1))
                        const_src.append(r % _PW if live else _PW)
    assert (tap_slot >= 0).all() and len(block_rows) == 50
    return tuple(_index(a, device) for a in (block_rows, tap_slot, const_rows, const_src))


@_memo
def _layer_plan_z4(ci, device):
    """-> ({class: (c0, c1, lo, hi, lohi)}, columns of the tap matrix, stacked rows, taps, column offsets of the 18 blocks):
    per class one column range and the rows of the stacked weight matrix [75*ci taps | 4 x _PW (K^T b_prev | bias | 0) |
    zero rows] feeding the lower / upper output half; lohi = (lo0, hi0, lo1, hi1, ...): ONE gather of the stacked rows
    gives [K, 2, Co] = [W_lo | W_hi] row by row."""
    n_data = 75 * ci
    dummy = [n_data + 4 * _PW] * 2                   # next free zero row of the lower / upper half

    def zeros(half, n):
        dummy[half] += n
        return np.arange(dummy[half] - n, dummy[half])

    plan = {}
    for cls, segs in _COLS4.layout.items():
        halves = ([], [])
        for kind, val in segs:
            if kind == 'b':
                for half, tap in enumerate(_class_half_taps(cls, val)):
                    halves[half].append(np.arange(ci) + tap * ci)
            elif val == cls:                         # own constant block: [P_lo | P_hi]
                p = _CLASSES.index(val)
                own = np.arange(n_data + p * _PW, n_data + (p + 1) * _PW)
                halves[0].extend([own, zeros(0, _PW)])
                halves[1].extend([zeros(1, _PW), own])
            else:                                    # foreign constant block
                halves[0].append(zeros(0, _PW2))
                halves[1].append(zeros(1, _PW2))
        lo, hi = np.concatenate(halves[0]), np.concatenate(halves[1])
        c0 = _COLS4.first_column(cls, ci)
        plan[cls] = (c0, c0 + len(lo), _index(lo, device), _index(hi, device), _index(np.stack([lo, hi], 1).reshape(-1), device))
    return plan, _COLS4.width(ci), max(dummy), _COLS4.taps, _COLS4.block_offsets(ci)
