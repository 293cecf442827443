"""Coarse-to-fine upsampling of the voxel volume: the three ``ConvTranspose3d(768,768,(3,5,5),
stride=(1,2,2), padding=(2,4,4), dilation=(2,2,2), output_padding=(0,1,1))`` layers of the
reference head (dense_heads/voxelformer_occupancy_head.py:251-258, applied at :560), computed
on the *even lattice*.

With stride 2 AND dilation 2 in H/W the output index is ``o = 2*(i + k - 2)``: only even output
rows/cols ever receive data, every odd one equals the bias exactly (verified
bit-exactly against the reference).  So layer l+1 sees an input that is its predecessor's bias
vector on 3/4 of the positions.  Writing E_l for the data lattice of layer l's input:

    E_{l+1}[z,m,n] = b_l + sum_{a,b,c} K_l[a,b,c]^T X_l[z-2+2a, m-2+b, n-2+c]
    X_l[y,x]       = E_l[y/2,x/2] if y,x both even else b_{l-1}          (l >= 1)

* data taps: per output parity class (m%2, n%2) only the taps with (m%2+b), (n%2+c) even hit the
  data lattice -> four small correlations over E_l (3x3, 3x2, 2x3, 2x2 taps x 3 in z) = im2col +
  one GEMM each.  Useful MACs: 79.6 + 79.6 + 318.5 GFLOP instead of 79.6 + 318.5 + 1274 (3.5x);
* constant taps: sum of (K_l[tap]^T b_{l-1}) over the in-bounds non-data taps -- a [positions,75]
  0/1 pattern matrix (fixed by the geometry) times a [75,768] matrix.

This module holds the device switch (``_algebra``), the layers as autograd Functions with hand-written backward passes, the
GEMM dispatch (``mm_fwd``, ``rows_tn``) and the entry points; the index geometry of the tap matrices and of the stacked
weight matrices is ``lattice_plan.py``.  Every layer is one Function per formulation:

* ``_LatticeLayer`` (any Z), ``_Layer0Z4Taps`` / ``_LatticeLayerZ4Taps`` (Z = 4, a third fewer FLOPs: lattice_plan.py) take the
  correlation taps ``k`` [75,Ci,Co] and run on torch ops of any dtype and device (data movement through ``_algebra``): what
  the CPU suite checks in fp64 against ``conv_transpose3d``;
* ``_Layer0Z4Raw`` / ``_LatticeLayerZ4Raw`` (GPU, fp32 / bf16 lattices) take the fp32 ``ConvTranspose3d`` weight itself, keep
  ONE stacked weight buffer per layer, and run on explicit tap matrices or, where ``_implicit_taps`` admits the shape, on
  operands the kernels read straight from the lattice.

``_Layer0Z4.apply(x, k, bias, raw=None)`` / ``_LatticeLayerZ4.apply(e, k, bias, prev_bias, planar, raw=None)`` are how a Z = 4
layer is called (``upsample_lattice``, the GPU suite): the fp32-weight Function when ``raw`` is given, else the torch-taps one.

``full_volume`` scatters the last lattice into the dense ``[B,C,Z,8H,8W]`` tensor the reference's raw ``.view`` expects.
"""
import os

import torch

from . import _cpu_algebra
from ._cpu_algebra import ZS_PLAIN, ZS_PLANAR_SPLIT, ZS_SPLIT, planar_to_plain, planar_zs_to_plain, zs_to_plain
from ._cpu_algebra import plain_to_planar  # noqa: F401  (tests/test_hip_ops_gpu.py fetches it through this module)
from .lattice_plan import (_CLASSES, _COLS3, _COLS4, _PW, _PW2, _aug_rows_z4, _block_offsets, _class_patterns, _class_rows_z4,
                           _class_segments_z4, _const_rows_z4, _dgrad_plan, _layer0_z4_plan, _layer_plan, _layer_plan_z4,
                           _stack_tables_z4)

KERNEL = (3, 5, 5)
GEOM = dict(stride=(1, 2, 2), padding=(2, 4, 4), dilation=(2, 2, 2), output_padding=(0, 1, 1))
_HIP_DTYPES = (torch.float32, torch.bfloat16)


class _HipAlgebra:
    """The data-movement operations of the lattice algebra on the HIP kernels (GPU tensors; fp32 / bf16 -- other dtypes of a
    GPU tensor, e.g. an fp64 check on the device, go through the torch formulation).  Same signatures as ``_cpu_algebra``."""

    @staticmethod
    def corr_weight(weight, dtype):
        if weight.dtype == torch.float32 and dtype in _HIP_DTYPES:
            from ..hipops import convt_weight_taps
            return convt_weight_taps(weight, dtype)                       # one LDS-tiled transpose each way
        return _cpu_algebra.corr_weight(weight, dtype)

    @staticmethod
    def im2col(e, taps):
        from ..hipops import lattice_im2col
        return lattice_im2col(e.contiguous(), taps)

    @staticmethod
    def gather27(e, planar, a_mat, ci, hc, wc, taps, offs):
        from ..hipops import lattice_gather
        lattice_gather(e.contiguous(), a_mat, taps, offs, (hc, wc), 1 if planar else 0)

    @staticmethod
    def scatter27(d_a, planar, shape, ci, hc, wc, taps, offs):
        from ..hipops import lattice_scatter
        return lattice_scatter(d_a, d_a.new_empty(shape), taps, offs, (hc, wc), 1 if planar else 0)

    @staticmethod
    def gather_z4(e, layout, a_mat, taps, offs, ci, hc, wc, const=None):
        """``const`` = (table, column offsets): the kernel also writes the constant-pattern blocks of the four parity
        classes.  -> True when it did."""
        from ..hipops import lattice_gather
        if const is not None and e.dtype in _HIP_DTYPES:
            lattice_gather(e.contiguous(), a_mat, taps, offs, (hc, wc), layout, row_z=2, const_rows=const[0], const_offset=const[1])
            return True
        lattice_gather(e.contiguous(), a_mat, taps, offs, (hc, wc), layout, row_z=2)
        return False

    @staticmethod
    def scatter_z4(d_a, layout, shape, taps, offs, ci, hc, wc):
        from ..hipops import lattice_scatter
        return lattice_scatter(d_a, d_a.new_empty(shape), taps, offs, (hc, wc), layout, row_z=2)

    @staticmethod
    def channels_last(x0, dt):
        b, c, z, h, w = x0.shape
        pos = z * h * w
        if dt in _HIP_DTYPES:
            vx = 4 if dt == torch.bfloat16 else 2
            for wd in range(min(pos, 120), 0, -1):        # rows of the flattened positions: 8-byte multiples, tile <= 64 KB
                if pos % wd == 0 and wd % vx == 0:
                    return _ChannelsLast.apply(x0, dt, (pos // wd, wd))
        return _cpu_algebra.channels_last(x0, dt)


def _algebra(t):
    """THE device switch of this module: the HIP kernels for a GPU tensor, the torch formulation (``_cpu_algebra``, what the
    CPU suite checks in fp64) for a CPU tensor.  Nothing here is chosen by "extension missing": hipops raises."""
    return _HipAlgebra if t.is_cuda else _cpu_algebra


def _on_hip(t):
    return _algebra(t) is _HipAlgebra


def is_reference_geometry(conv):
    return (tuple(conv.kernel_size) == KERNEL and tuple(conv.stride) == GEOM['stride'] and
            tuple(conv.padding) == GEOM['padding'] and tuple(conv.dilation) == GEOM['dilation'] and
            tuple(conv.output_padding) == GEOM['output_padding'] and conv.groups == 1)


_to_plain, _from_plain = _cpu_algebra.to_plain, _cpu_algebra.from_plain


def _corr_weight(weight, dtype):
    """ConvTranspose weight [Ci,Co,3,5,5] -> correlation taps as ONE contiguous [75, Ci, Co]
    tensor in the compute dtype, tap index = (a*5+b)*5+c, K[a,b,c] = Wt[:, :, 2-a, 4-b, 4-c]."""
    return _algebra(weight).corr_weight(weight, dtype)


def _im2col(e, taps):
    """e [B,Z,H,W,C] channels-last; taps: list of (dz,dy,dx) offsets (zero outside the lattice)
    -> [B*Z*H*W, len(taps)*C] (ver_lattice_im2col / ver_lattice_col2im on the GPU)."""
    return _algebra(e).im2col(e, taps)


def _bias_through_taps(prev_bias, k):
    """prev_bias [Ci] @ k [75,Ci,Co] -> [75,Co] (the bias-valued odd positions of the input seen through every tap).  As a
    batched [1 x Ci] x [Ci x Co] product: ``torch.matmul`` of a vector with a 3-D tensor first makes a TRANSPOSED contiguous
    copy of all 75 tap blocks (88 MB at 768 channels, 190 us -- a fifth of the weight-side time of a one-viewpoint step)."""
    t, ci, _ = k.shape
    return torch.bmm(prev_bias.view(1, 1, ci).expand(t, 1, ci).contiguous(), k).squeeze(1)


def _stacked_rows(k, bias, prev_bias, total_rows):
    """Weight rows of a parity-class layer in the torch-taps formulation (``_layer_plan`` / ``_layer_plan_z4`` index them):
    75 tap blocks | per class (K^T prev_bias | bias | 0) | zero rows."""
    _, ci, co = k.shape
    v = _bias_through_taps(prev_bias.to(k.dtype), k)                          # [75, Co]
    vaug = torch.cat([v, bias.to(k.dtype)[None], v.new_zeros(_PW - 76, co)])
    return torch.cat([k.reshape(75 * ci, co), vaug, vaug, vaug, vaug, v.new_zeros(total_rows - 75 * ci - 4 * _PW, co)])


def _stacked_rows_backward(d_rows, k, prev_bias):
    """adjoint of ``_stacked_rows``: -> (d_k, d_bias, d_prev_bias)."""
    _, ci, co = k.shape
    dt = k.dtype
    n_data = 75 * ci
    acc = torch.float64 if dt == torch.float64 else torch.float32
    d_vaug = d_rows[n_data:n_data + 4 * _PW].view(4, _PW, co).sum(0, dtype=acc)
    d_v = d_vaug[:75].to(dt)
    # v = prev_bias @ k
    d_k = torch.addcmul(d_rows[:n_data].view(75, ci, co), prev_bias.to(dt)[None, :, None], d_v[:, None, :])
    d_prev = torch.bmm(k, d_v.unsqueeze(2)).sum(0).squeeze(1)
    return d_k, d_vaug[75].to(prev_bias.dtype), d_prev.to(prev_bias.dtype)


def _layer0(e, k, bias):
    """All 75 taps hit data.  e [B,Z,H,W,C] channels-last -> E_1 [B,Z,H,W,Co]."""
    b, z, h, w, c = e.shape
    taps = [(2 * a - 2, bb - 2, cc - 2) for a in range(3) for bb in range(5) for cc in range(5)]
    a_mat = _im2col(e, taps)
    out = torch.addmm(bias, a_mat, k.reshape(75 * c, -1))
    return out.view(b, z, h, w, -1)


def _gather27(e, planar, a_mat, ci, hc, wc):
    _algebra(e).gather27(e, planar, a_mat, ci, hc, wc, _COLS3.taps, _COLS3.block_offsets(ci))


def _scatter27(d_a, planar, shape, ci, hc, wc):
    """adjoint of _gather27: gradient of the source lattice (plain or planar like the source)."""
    return _algebra(d_a).scatter27(d_a, planar, shape, ci, hc, wc, _COLS3.taps, _COLS3.block_offsets(ci))


class _LatticeLayer(torch.autograd.Function):
    """Parity-class layer (layers 1 and 2 of the stack) for any Z: one 27-block tap matrix, one GEMM per class
    (lattice_plan.py).  Every class GEMM writes its own contiguous output plane: the result is PLANAR [4,B,Z,H,W,Co]
    (plane 2pm+pn = positions (2y+pm, 2x+pn) of the (2H, 2W) lattice) and is consumed as such by the next layer's gather and
    by occ_proj -- the lattice is never interleaved."""

    @staticmethod
    def forward(ctx, e, k, bias, prev_bias, planar):
        """e: data lattice, plain [B,Z,H,W,C] or planar [4,B,Z,H/2,W/2,C], of a full input that equals ``prev_bias`` off the
        lattice; k [75,Ci,Co] correlation taps; -> planar output [4,B,Z,H,W,Co] (H, W = combined size of the input)."""
        if planar:
            _, b, z, hh, wh, ci = e.shape
            hc, wc = 2 * hh, 2 * wh
        else:
            b, z, hc, wc, ci = e.shape
        co = k.shape[-1]
        plan, kt, total_rows = _layer_plan(ci, e.device)
        m = b * z * hc * wc
        a_mat = e.new_empty(m, kt)
        _gather27(e, planar, a_mat, ci, hc, wc)
        a3 = a_mat.view(b, z * hc * wc, kt)
        for cls, pat in zip(_CLASSES, _class_patterns(z, hc, wc, e.device, e.dtype)):
            o = _COLS3.const_offset(cls, ci)
            a3[:, :, o:o + _PW] = pat
        rows = _stacked_rows(k, bias, prev_bias, total_rows)
        out = e.new_empty(4, m, co)
        for p, cls in enumerate(_CLASSES):
            c0, c1, ridx = plan[cls]
            torch.mm(a_mat[:, c0:c1], rows.index_select(0, ridx), out=out[p])
        ctx.save_for_backward(a_mat, rows, k, prev_bias)
        ctx.geom = (planar, tuple(e.shape), hc, wc)
        return out.view(4, b, z, hc, wc, co)

    @staticmethod
    def backward(ctx, grad_out):
        a_mat, rows, k, prev_bias = ctx.saved_tensors
        planar, e_shape, hc, wc = ctx.geom
        _, ci, co = k.shape
        plan, kt, total_rows = _layer_plan(ci, a_mat.device)
        m = a_mat.shape[0]
        g = grad_out.contiguous().view(4, m, co)
        d_a = a_mat.new_empty(m, kt)
        d_a[:, kt - _PW:] = 0                                   # P01 is outside class (0,0)'s range
        d_rows = rows.new_empty(total_rows, co)
        for p, cls in enumerate(_CLASSES):
            c0, c1, ridx = plan[cls]
            w = rows.index_select(0, ridx)
            if p == 0:                                          # class (0,0): initialises every tap block
                torch.mm(g[p], w.t(), out=d_a[:, c0:c1])
            else:
                torch.addmm(d_a[:, c0:c1], g[p], w.t(), out=d_a[:, c0:c1])
            d_rows.index_copy_(0, ridx, rows_tn(a_mat[:, c0:c1], g[p]))
        d_e = _scatter27(d_a, planar, e_shape, ci, hc, wc)
        return (d_e, *_stacked_rows_backward(d_rows, k, prev_bias), None)


# ------------------------------------------------------------------------------------------------
# Z = 4: rows (b, zl, y, x) only, both output halves side by side out of ONE GEMM (lattice_plan.py).  Lattices are kept Z-SPLIT,
# [B, 2 (zl), H, W, 2 (zh), C] (z = 2*zh + zl): exactly the GEMM output [rows, 2*Co].
def _gather_z4(e, layout, a_mat, taps, offs, ci, hc, wc, with_const=False):
    """rows (b, zl, y, x); tap (dz in {0,2}, dy, dx) reads input layer zl + dz.  ``with_const``: ask for the constant-pattern
    blocks of the four parity classes in the same pass.  -> True when they were written (else the caller fills them)."""
    const = _const_rows_z4(ci, hc, wc, e.device, e.dtype) if with_const else None
    return _algebra(e).gather_z4(e, layout, a_mat, taps, offs, ci, hc, wc, const)


def _scatter_z4(d_a, layout, shape, taps, offs, ci, hc, wc):
    return _algebra(d_a).scatter_z4(d_a, layout, shape, taps, offs, ci, hc, wc)


# Implicit tap matrix (round 6): from `_OWN_GEMM_MIN_ROWS` rows on, the GEMMs of a bf16 lattice layer read their A operand
# straight from the lattice (a tap block of a row is the contiguous channel vector of a neighbouring cell, fetched by the kernels'
# LDS-DMA): the forward product (ver_gemm_nn_segments), the weight gradient (ver_wgrad_tn_segments) and d(input) as ONE
# gather-form product per input half over the four class planes of the output gradient (ver_gemm_nn_planes: d_e[cell] = sum
# over (class, tap, output half) of g_class[cell - tap] W^T, fp32 sums over all classes and taps rounded once).  Neither the
# tap matrix (10 GB for layer 3 at 192 viewpoints) nor its gradient is written, no ver_lattice_scatter.  Below, the skinny /
# library paths on the explicit matrix are faster.  VER_IMPLICIT_TAPS=0: explicit everywhere.
_IMPLICIT_TAPS = os.environ.get('VER_IMPLICIT_TAPS', '1') != '0'


def _implicit_taps(e, layout, rows, combined_hw, ci, raw, const_width):
    """True when a layer with source lattice ``e`` (layout 0 / 2 / 3), ``rows`` = B * 2 * H * W over the combined (H, W) lattice
    and pattern blocks of ``const_width`` columns (0: none) takes the implicit-operand kernels.  THE place that decides: the
    forward product (ver_gemm_nn_segments) and the weight gradient (ver_wgrad_tn_segments) must both take the shape, or the
    layer runs on explicit tap matrices in both passes -- ver_wgrad_tn_segments stops at 2 H W = 2 048 (its offset tables in
    LDS), so e.g. layer 3 of a 20 x 20 BEV grid (2 H W = 3 200) goes the explicit way, as it did before the implicit kernels."""
    if not (_IMPLICIT_TAPS and _OWN_GEMM and raw is not None and _on_hip(e) and e.dtype == torch.bfloat16 and rows >= _OWN_GEMM_MIN_ROWS):
        return False
    from ..hipops import gemm_nn_taps_supported, wgrad_tn_segments_supported
    return gemm_nn_taps_supported(e, layout, None, ci) and wgrad_tn_segments_supported(e, layout, combined_hw, ci, const_width, None)


def _dgrad_implicit(kind, g_planes, weights, b, hc, wc, ci, co):
    """d(input) lattice, z-split [B,2,hc,wc,2,Ci], from the output gradient ``g_planes`` bf16 [planes, B*2*hc*wc, 2 Co] and the
    layer's stacked weight matrix ``weights`` [rows, 2 Co] (``_dgrad_plan``): ONE product [M, blocks * 2 Co] x [., 2 Ci]."""
    from ..hipops import gemm_nn_taps
    lat = g_planes.view(g_planes.shape[0], b, 2, hc, wc, 2, co)
    rows, taps, planes, nb = _dgrad_plan(kind, ci, g_planes.device)
    # W [(block, h, co), (j, ci)] = S[row of block (.., j) + ci, h Co + co]: the two input halves' blocks transposed, side by side
    wcat = weights.index_select(0, rows).view(nb, 2 * ci, 2 * co).transpose(1, 2).reshape(nb * 2 * co, 2 * ci)
    d_e = gemm_nn_taps(lat if kind != 'l0' else lat[0], ZS_SPLIT, (hc, wc), taps, wcat, planes=planes if kind != 'l0' else None,
                       timer_class='head_gemm_dgrad')
    return d_e.view(b, 2, hc, wc, 2, ci)


def _dgrad_explicit_l0(g, wmat, shape, taps, offs, ci, h, w):
    """d(input) of the first Z = 4 layer through the explicit d(tap matrix): library GEMM + scatter."""
    with gemm_timed('head_gemm_dgrad', g.shape[0], g.shape[1], wmat.shape[0]):
        d_a = torch.mm(g, wmat.t())
    return _scatter_z4(d_a, ZS_PLAIN, shape, taps, offs, ci, h, w)


class _Layer0Z4Taps(torch.autograd.Function):
    """First layer for Z = 4, torch-taps formulation: every tap hits data.  x plain [B,4,H,W,Ci], k [75,Ci,Co] -> z-split
    [B,2,H,W,2,Co]."""

    @staticmethod
    def forward(ctx, x, k, bias):
        b, _, h, w, ci = x.shape
        co = k.shape[-1]
        taps, offs, lo, hi = _layer0_z4_plan(ci, x.device)
        a_mat = x.new_empty(b * 2 * h * w, 50 * ci)
        _gather_z4(x, ZS_PLAIN, a_mat, taps, offs, ci, h, w)
        rows = k.reshape(75 * ci, co)
        wmat = torch.cat([rows.index_select(0, lo), rows.index_select(0, hi)], 1)    # [50 ci, 2 co] = [W_lo | W_hi]
        out = mm_fwd(a_mat, wmat, bias=torch.cat([bias, bias]))
        ctx.save_for_backward(a_mat, wmat)
        ctx.geom = (tuple(x.shape), ci, co, h, w)
        return out.view(b, 2, h, w, 2, co)

    @staticmethod
    def backward(ctx, grad_out):
        a_mat, wmat = ctx.saved_tensors
        shape, ci, co, h, w = ctx.geom
        taps, offs, lo, hi = _layer0_z4_plan(ci, a_mat.device)
        g = grad_out.contiguous().view(-1, 2 * co)
        d_x = _dgrad_explicit_l0(g, wmat, shape, taps, offs, ci, h, w)
        d_w = rows_tn(a_mat, g)                                                        # [50 ci, 2 co]
        d_b = g.sum(0, dtype=torch.float64 if g.dtype == torch.float64 else torch.float32)
        d_lo = d_w.new_zeros(75 * ci, co)
        d_hi = d_w.new_zeros(75 * ci, co)
        d_lo.index_copy_(0, lo, d_w[:, :co])
        d_hi.index_copy_(0, hi, d_w[:, co:])
        return d_x, (d_lo + d_hi).view(75, ci, co), (d_b[:co] + d_b[co:]).to(g.dtype)


class _Layer0Z4Raw(torch.autograd.Function):
    """First layer for Z = 4, fp32-weight formulation (GPU training steps): ``raw`` is the fp32 ConvTranspose3d weight
    [Ci,Co,3,5,5]; [W_lo | W_hi] is written by ONE kernel from it (no tap tensor, no row gathers) and the backward returns its
    gradient straight from the GEMM's (``ver_convt_weight_backward_blocks``).  x plain [B,4,H,W,Ci] -> z-split [B,2,H,W,2,Co]."""

    @staticmethod
    def forward(ctx, x, raw, bias):
        from ..hipops import convt_weight_forward_blocks
        b, _, h, w, ci = x.shape
        co = raw.shape[1]
        taps, offs, _, _ = _layer0_z4_plan(ci, x.device)
        ctx.implicit = _implicit_taps(x, ZS_PLAIN, b * 2 * h * w, (h, w), ci, raw, 0)
        if ctx.implicit:
            operand = x.contiguous()                                                   # the lattice itself
        else:
            operand = x.new_empty(b * 2 * h * w, 50 * ci)                              # its tap matrix
            _gather_z4(x, ZS_PLAIN, operand, taps, offs, ci, h, w)
        wmat = convt_weight_forward_blocks(raw, _block_offsets('l0', ci, co, x.device), x.new_empty(50 * ci, 2 * co), ci, co)
        bias2 = torch.cat([bias, bias])
        if ctx.implicit:
            from ..hipops import gemm_nn_taps
            out = gemm_nn_taps(operand, ZS_PLAIN, (h, w), taps, wmat, bias=bias2.to(x.dtype).float())
        else:
            out = mm_fwd(operand, wmat, bias=bias2)
        ctx.save_for_backward(operand, wmat)
        ctx.geom = (tuple(x.shape), ci, co, h, w)
        return out.view(b, 2, h, w, 2, co)

    @staticmethod
    def backward(ctx, grad_out):
        from ..hipops import convt_weight_backward_blocks
        operand, wmat = ctx.saved_tensors
        shape, ci, co, h, w = ctx.geom
        taps, offs, _, _ = _layer0_z4_plan(ci, operand.device)
        g = grad_out.contiguous().view(-1, 2 * co)
        if ctx.implicit:
            from ..hipops import wgrad_tn_segments
            d_x = zs_to_plain(_dgrad_implicit('l0', g[None], wmat, shape[0], h, w, ci, co))
            d_w = wgrad_tn_segments(operand, ZS_PLAIN, (h, w), taps, g)
        else:
            d_x = _dgrad_explicit_l0(g, wmat, shape, taps, offs, ci, h, w)
            d_w = rows_tn(operand, g)                                                  # [50 ci, 2 co]
        d_b = g.sum(0, dtype=torch.float32)
        d_raw = convt_weight_backward_blocks(d_w, _block_offsets('l0', ci, co, d_w.device), None, None, ci, co)
        return d_x, d_raw, (d_b[:co] + d_b[co:]).to(g.dtype)


def _geom_z4(e, planar):
    """-> (kernel layout, B, combined H, W, Ci) of a z-split [B,2,H,W,2,C] or planar z-split [4,B,2,H/2,W/2,2,C] lattice."""
    if planar:
        _, b, _, hh, wh, _, ci = e.shape
        return ZS_PLANAR_SPLIT, b, 2 * hh, 2 * wh, ci
    b, _, hc, wc, _, ci = e.shape
    return ZS_SPLIT, b, hc, wc, ci


def _tap_matrix_z4(e, layout, b, hc, wc, ci):
    """The explicit 18-block tap matrix [B*2*hc*wc, kt] of a Z = 4 parity-class layer, constant blocks included."""
    _, kt, _, taps, offs = _layer_plan_z4(ci, e.device)
    a_mat = e.new_empty(b * 2 * hc * wc, kt)
    if not _gather_z4(e, layout, a_mat, taps, offs, ci, hc, wc, with_const=True):
        a3 = a_mat.view(b, 2 * hc * wc, kt)
        for cls, pat in zip(_CLASSES, _class_patterns(4, hc, wc, e.device, e.dtype)):
            o = _COLS4.const_offset(cls, ci)
            halves = pat.view(2, 2 * hc * wc, _PW)              # output z = zl (lower), zl + 2 (upper)
            a3[:, :, o:o + _PW] = halves[0]
            a3[:, :, o + _PW:o + _PW2] = halves[1]
    return a_mat


def _class_ranges_z4(ci, device):
    """Per class (c0, c1, r0, r1): its column range in the tap matrix and its row range in the class-stacked weight buffer
    [sum K_c, 2 Co] (classes in _CLASSES order), and the rows of that buffer."""
    plan, rows = _layer_plan_z4(ci, device)[0], _class_rows_z4(ci)
    ranges = [(plan[cls][0], plan[cls][1], rows[cls][0], rows[cls][0] + plan[cls][1] - plan[cls][0]) for cls in _CLASSES]
    return ranges, ranges[-1][3]


def _dgrad_class(d_a, p, g_p, w, c0, c1):
    """d(tap matrix) of one class, ``g_p w^T``, into the class's column range (the ranges overlap: class (0,0) comes first and
    initialises every tap block).  (library GEMMs: a one-pass kernel of our own over all four classes was built and measured
    7 % slower, scratch/experiments/k_dgrad_nt.hip.inc)"""
    with gemm_timed('head_gemm_dgrad', g_p.shape[0], g_p.shape[1], c1 - c0):
        if p == 0:
            torch.mm(g_p, w.t(), out=d_a[:, c0:c1])
        else:
            torch.addmm(d_a[:, c0:c1], g_p, w.t(), out=d_a[:, c0:c1])


class _LatticeLayerZ4Taps(torch.autograd.Function):
    """Parity-class layer for Z = 4, torch-taps formulation.  e: z-split [B,2,H,W,2,C] or planar z-split
    [4,B,2,H/2,W/2,2,C]; k [75,Ci,Co] -> planar z-split output [4,B,2,H,W,2,Co] (H, W = combined size of the input)."""

    @staticmethod
    def forward(ctx, e, k, bias, prev_bias, planar):
        layout, b, hc, wc, ci = _geom_z4(e, planar)
        co = k.shape[-1]
        plan, _, total_rows, _, _ = _layer_plan_z4(ci, e.device)
        a_mat = _tap_matrix_z4(e, layout, b, hc, wc, ci)
        out = e.new_empty(4, a_mat.shape[0], 2 * co)
        rows = _stacked_rows(k, bias, prev_bias, total_rows)
        ws = []
        for p, cls in enumerate(_CLASSES):
            c0, c1, _, _, lohi = plan[cls]
            ws.append(rows.index_select(0, lohi).view(c1 - c0, 2 * co))           # [W_lo | W_hi], one gather
            mm_fwd(a_mat[:, c0:c1], ws[p], out=out[p])
        ctx.save_for_backward(a_mat, k, prev_bias, *ws)
        ctx.geom = (layout, tuple(e.shape), hc, wc)
        return out.view(4, b, 2, hc, wc, 2, co)

    @staticmethod
    def backward(ctx, grad_out):
        a_mat, k, prev_bias, *ws = ctx.saved_tensors
        layout, e_shape, hc, wc = ctx.geom
        _, ci, co = k.shape
        plan, kt, total_rows, taps, offs = _layer_plan_z4(ci, a_mat.device)
        m = a_mat.shape[0]
        g = grad_out.contiguous().view(4, m, 2 * co)
        d_a = a_mat.new_empty(m, kt)
        d_a[:, kt - _PW2:] = 0                                  # P01 is outside class (0,0)'s range
        d_lo = a_mat.new_zeros(total_rows, co)
        d_hi = a_mat.new_zeros(total_rows, co)
        for p, cls in enumerate(_CLASSES):
            c0, c1, lo, hi, _ = plan[cls]
            _dgrad_class(d_a, p, g[p], ws[p], c0, c1)
            d_w = rows_tn(a_mat[:, c0:c1], g[p])
            d_lo.index_copy_(0, lo, d_w[:, :co])
            d_hi.index_copy_(0, hi, d_w[:, co:])
        d_e = _scatter_z4(d_a, layout, e_shape, taps, offs, ci, hc, wc)
        del d_a
        return (d_e, *_stacked_rows_backward(d_lo + d_hi, k, prev_bias), None)


class _LatticeLayerZ4Raw(torch.autograd.Function):
    """Parity-class layer for Z = 4, fp32-weight formulation (GPU training steps): ``raw`` is the fp32 ConvTranspose3d weight
    [Ci,Co,3,5,5].  The weight side of the step does not shrink with the batch (config.latency): the four class matrices
    [W_lo | W_hi] are ONE stacked buffer S [sum K_c, 2 Co] written straight from the parameter
    (ver_convt_weight_forward_blocks); v = b_prev^T K[t] for all taps is one pass over S (ver_blocks_vec_forward); the constant
    rows (K^T b_prev | bias | 0) go in by one indexed copy -- no tap tensor, no 88-MB concatenation, no row gather per class.
    The four class weight gradients are written into one buffer of the same shape and turned into the parameter's gradient by
    ONE kernel.  Lattices as in ``_LatticeLayerZ4Taps``."""

    @staticmethod
    def forward(ctx, e, raw, bias, prev_bias, planar):
        from ..hipops import blocks_vec_forward, convt_weight_forward_blocks
        layout, b, hc, wc, ci = _geom_z4(e, planar)
        co = raw.shape[1]
        dt = e.dtype
        m = b * 2 * hc * wc
        ctx.implicit = _implicit_taps(e, layout, m, (hc, wc), ci, raw, _PW2)
        operand = e.contiguous() if ctx.implicit else _tap_matrix_z4(e, layout, b, hc, wc, ci)      # the lattice | its tap matrix
        out = e.new_empty(4, m, 2 * co)
        ranges, n_rows = _class_ranges_z4(ci, e.device)
        block_rows, tap_slot, const_rows, const_src = _stack_tables_z4(ci, e.device)
        stack = e.new_empty(n_rows, 2 * co)
        convt_weight_forward_blocks(raw, _block_offsets('lat', ci, co, e.device), stack, ci, co)
        v = blocks_vec_forward(stack, block_rows, ci, prev_bias).view(-1, co).index_select(0, tap_slot)     # [75, Co] fp32
        vaug = torch.cat([v.to(dt), bias.to(dt)[None], v.new_zeros(_PW - 75, co, dtype=dt)])                # + one zero row
        stack.view(-1, co).index_copy_(0, const_rows, vaug.index_select(0, const_src))
        for p, (cls, (c0, c1, r0, r1)) in enumerate(zip(_CLASSES, ranges)):
            if ctx.implicit:
                from ..hipops import gemm_nn_taps
                gemm_nn_taps(operand, layout, (hc, wc), _class_segments_z4(cls, ci), stack[r0:r1],
                             const_rows=_const_rows_z4(ci, hc, wc, e.device, dt)[0], out=out[p])
            else:
                mm_fwd(operand[:, c0:c1], stack[r0:r1], out=out[p])
        ctx.save_for_backward(operand, stack, prev_bias)
        ctx.geom = (layout, tuple(e.shape), b, hc, wc, ci, co)
        return out.view(4, b, 2, hc, wc, 2, co)

    @staticmethod
    def backward(ctx, grad_out):
        from ..hipops import blocks_vec_backward, convt_weight_backward_blocks
        operand, stack, prev_bias = ctx.saved_tensors
        layout, e_shape, b, hc, wc, ci, co = ctx.geom
        _, kt, _, taps, offs = _layer_plan_z4(ci, operand.device)
        ranges, n_rows = _class_ranges_z4(ci, operand.device)
        dt = operand.dtype
        m = b * 2 * hc * wc
        g = grad_out.contiguous().view(4, m, 2 * co)
        if not ctx.implicit:
            d_a = operand.new_empty(m, kt)
            d_a[:, kt - _PW2:] = 0                              # P01 is outside class (0,0)'s range
        d_stack = operand.new_empty(n_rows, 2 * co)
        for p, (cls, (c0, c1, r0, r1)) in enumerate(zip(_CLASSES, ranges)):
            if ctx.implicit:
                from ..hipops import wgrad_tn_segments
                wgrad_tn_segments(operand, layout, (hc, wc), _class_segments_z4(cls, ci), g[p], out=d_stack[r0:r1],
                                  const_rows=_const_rows_z4(ci, hc, wc, operand.device, dt)[0])
            else:
                _dgrad_class(d_a, p, g[p], stack[r0:r1], c0, c1)
                rows_tn(operand[:, c0:c1], g[p], out=d_stack[r0:r1])
        if ctx.implicit:
            d_e = _dgrad_implicit('lat', g, stack, b, hc, wc, ci, co)              # z-split [B,2,hc,wc,2,Ci]
            if layout == ZS_PLANAR_SPLIT:                                           # -> the planar form of the source lattice
                d_e = d_e.view(b, 2, hc // 2, 2, wc // 2, 2, 2, ci).permute(3, 5, 0, 1, 2, 4, 6, 7).reshape(e_shape)
        else:
            d_e = _scatter_z4(d_a, layout, e_shape, taps, offs, ci, hc, wc)
            del d_a
        # own constant blocks of the four classes -> d(v | bias); every tap's two half gradients + prev_bias (x) d(v)
        # -> the gradient of the ConvTranspose3d weight, in one pass over the stacked buffer
        own = d_stack.view(-1, co).index_select(0, _aug_rows_z4(ci, d_stack.device)).view(8, _PW, co)
        d_vaug = own.sum(0, dtype=torch.float32)
        d_v = d_vaug[:75].to(dt)
        pb = prev_bias.to(dt)
        d_raw = convt_weight_backward_blocks(d_stack, _block_offsets('lat', ci, co, d_stack.device), pb, d_v, ci, co)
        # d(b_prev) = sum_t K[t] d_v[t]: d_v scattered to ONE slot per tap of the stacked weights, one pass over them
        block_rows, tap_slot, _, _ = _stack_tables_z4(ci, d_stack.device)
        dv2 = d_vaug.new_zeros(2 * block_rows.numel(), co).index_copy_(0, tap_slot, d_vaug[:75])
        d_prev = blocks_vec_backward(stack, block_rows, ci, dv2.view(block_rows.numel(), 2 * co))
        return d_e, d_raw, d_vaug[75].to(prev_bias.dtype), d_prev.to(prev_bias.dtype), None


class _Layer0Z4:
    """First layer for Z = 4: taps ``k`` [75,Ci,Co], or ``raw`` = the fp32 ConvTranspose3d weight (then ``k`` is not read)."""

    @staticmethod
    def apply(x, k, bias, raw=None):
        return _Layer0Z4Taps.apply(x, k, bias) if raw is None else _Layer0Z4Raw.apply(x, raw, bias)


class _LatticeLayerZ4:
    """Parity-class layer for Z = 4: ``k`` or ``raw`` as in ``_Layer0Z4``."""

    @staticmethod
    def apply(e, k, bias, prev_bias, planar, raw=None):
        if raw is None:
            return _LatticeLayerZ4Taps.apply(e, k, bias, prev_bias, planar)
        return _LatticeLayerZ4Raw.apply(e, raw, bias, prev_bias, planar)


def gemm_timed(name, m, k, n):
    """HIP-event bracket around one library GEMM of the head ([m, k] x [k, n]) for bench.py's dense-part roofline entry
    (hipops.timed: free unless a KernelTimer is set)."""
    from ..hipops import timed
    return timed(name, 2.0 * m * k * n)


# Forward GEMMs of the lattice layers on ver_gemm_nn (csrc/ver_gemm.hip) from this many rows on (and K >= 2048); below, and
# for every other dtype / device, the library.  Measured on the 192-viewpoint shapes (scratch/r05/gemm_bench.py): layer 3
# 1 266-1 292 -> 1 312-1 338 TFLOP/s, layers 1 / 2 1 121-1 210 -> 1 310; occ_proj (K = 832) and the 8-viewpoint shapes are
# faster in the library and stay there.  VER_OWN_GEMM=0: library everywhere.
_OWN_GEMM = os.environ.get('VER_OWN_GEMM', '1') == '1'
# (round 6: 14 000 instead of 49 152 -- with the implicit operands layer 3 of an eight-viewpoint step (14 400 rows) and layers 1-2 of a
#  64-viewpoint one gain 0.5-1.6 %; 3 000 loses 9 % at eight viewpoints: too few tiles)
_OWN_GEMM_MIN_ROWS = int(os.environ.get('VER_OWN_GEMM_MIN_ROWS', '14000'))
# ... and the skinny products of the small-batch steps (config.latency: 450 / 1 800 rows at one viewpoint per step) cut into K
# slices: the library's best recorded solution runs (450 x 38 400) x (38 400 x 1 536) in 144 us on 12 workgroups, the weight
# matrix alone streams in 15
_OWN_GEMM_SKINNY_ROWS = 2048


def mm_fwd(a, w, out=None, bias=None):
    """``a @ w (+ bias)`` for the forward GEMM of a layer: a [M, K] (may be a column range of the tap matrix), w [K, N]
    row-major, optional bias [N]; ``out`` [M, N] is written when given."""
    m, k = a.shape
    n = w.shape[1]
    if _OWN_GEMM and _on_hip(a) and a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and k >= 2048 and \
            (m >= _OWN_GEMM_MIN_ROWS or m <= _OWN_GEMM_SKINNY_ROWS):
        from ..hipops import gemm_nn, gemm_nn_splits, gemm_nn_supported
        if gemm_nn_supported(a, w) and (out is None or (out.stride(-1) == 1 and out.dtype == torch.bfloat16)) and \
                (m >= _OWN_GEMM_MIN_ROWS or gemm_nn_splits(m, k, n) > 1):
            # (the library adds the bias as a bf16 vector: the same rounded values here)
            return gemm_nn(a, w, None if bias is None else bias.to(a.dtype).float(), out)
    with gemm_timed('head_gemm_fwd', m, k, n):
        if bias is None:
            return torch.mm(a, w, out=out) if out is not None else torch.mm(a, w)
        b = bias.to(a.dtype)
        return torch.addmm(b, a, w, out=out) if out is not None else torch.addmm(b, a, w)


def rows_tn(a, g, out_dtype=None, out=None):
    """a^T g for tall operands (a [M,K] may be a column range of a wider matrix, g [M,N]): the weight gradient of a GEMM
    layer, rows on the contraction axis.  bf16 GPU operands run on ``ver_wgrad_tn`` (csrc/ver_wgrad.hip: both
    operands streamed row-major into LDS, fragments through transposing LDS reads, fp32 partial sums over row chunks
    added up in fp32: 1.3 PFLOP/s where the library's T x N class reaches 1.05); everything else
    (fp32 / fp64, CPU tensors of the algebra tests) is a plain matmul."""
    if _on_hip(a) and a.dtype == torch.bfloat16 and g.dtype == torch.bfloat16:
        from ..hipops import wgrad_tn, wgrad_tn_supported
        if g.stride(-1) != 1 or g.stride(0) % 8:
            g = g.contiguous()
        if wgrad_tn_supported(a, g):
            return wgrad_tn(a, g, out_dtype=out_dtype if out is None else out.dtype, out=out)
    if out is not None:                                  # (a row range of a stacked gradient buffer)
        return torch.mm(a.t(), g, out=out) if out.dtype == a.dtype else out.copy_(torch.mm(a.t(), g))
    res = torch.mm(a.t(), g)
    return res if out_dtype is None else res.to(out_dtype)


def _compute_dtype(x):
    """bf16 under ``torch.autocast`` (im2col, GEMM operands and lattices all in bf16, fp32
    accumulation inside the GEMM), else the input's dtype."""
    if _on_hip(x) and torch.is_autocast_enabled('cuda'):
        return torch.get_autocast_dtype('cuda')
    return x.dtype


class _ChannelsLast(torch.autograd.Function):
    """x0 [B,C,Z,H,W] (the head's raw view of the encoder output, head:558) -> the compute dtype, channels-last
    [B,Z,H,W,C]; one cast + one LDS-tiled transpose each way (``ver_lattice_transpose`` over the flattened Z*H*W
    positions) instead of a cast of the permuted view and an element-wise strided copy."""

    @staticmethod
    def forward(ctx, x0, dt, split):
        from ..hipops import lattice_transpose
        b, c, z, h, w = x0.shape
        cf = x0.to(dt).contiguous().view(b, c * z * h * w)
        e = torch.empty(b, z, h, w, c, dtype=dt, device=x0.device)
        lattice_transpose(e.view(b, 1, split[0], split[1], c), cf, split, 0, False)
        ctx.split, ctx.in_dtype = split, x0.dtype
        return e

    @staticmethod
    def backward(ctx, g):
        from ..hipops import lattice_transpose
        b, z, h, w, c = g.shape
        g = g.contiguous()
        cf = torch.empty(b, c * z * h * w, dtype=g.dtype, device=g.device)
        lattice_transpose(g.view(b, 1, ctx.split[0], ctx.split[1], c), cf, ctx.split, 0, True)
        return cf.view(b, c, z, h, w).to(ctx.in_dtype), None, None


def _channels_last(x0, dt):
    return _algebra(x0).channels_last(x0, dt)


def upsample_lattice(x0, weights, biases):
    """x0 [B,C,Z,H,W] -> (E_3, last bias).  E_3 holds the even positions of the reference's dense
    output ``up_sample(x0)`` [B,C,Z,8H,8W], as a PLANAR lattice [4,B,Z,2H,2W,C] or, for Z = 4, planar
    z-split [4,B,2,2H,2W,2,C] (``_cpu_algebra.planar_to_plain`` / ``planar_zs_to_plain`` give the channels-last
    [B,Z,4H,4W,C] lattice)."""
    dt = _compute_dtype(x0)
    e = _channels_last(x0, dt)
    bs = [b.to(dt) for b in biases]
    if e.shape[1] == 4 and _on_hip(e) and dt in _HIP_DTYPES and all(_on_hip(w) and w.dtype == torch.float32 for w in weights):
        # GPU: the layers take the ConvTranspose3d weights themselves (taps made inside, weight gradient made from the class
        # GEMMs' gradients by one kernel: the weight-side work of a step does not shrink with the batch)
        e = _Layer0Z4.apply(e, None, bs[0], weights[0])
        e = _LatticeLayerZ4.apply(e, None, bs[1], bs[0], False, weights[1])
        e = _LatticeLayerZ4.apply(e, None, bs[2], bs[1], True, weights[2])
        return e, bs[2]
    ks = [_corr_weight(w, dt) for w in weights]
    if e.shape[1] == 4:                                   # bev_z = 4: z-split path (a third fewer FLOPs)
        e = _Layer0Z4.apply(e, ks[0], bs[0])
        e = _LatticeLayerZ4.apply(e, ks[1], bs[1], bs[0], False)
        e = _LatticeLayerZ4.apply(e, ks[2], bs[2], bs[1], True)
        return e, bs[2]
    e = _layer0(e, ks[0], bs[0])
    e = _LatticeLayer.apply(e, ks[1], bs[1], bs[0], False)
    e = _LatticeLayer.apply(e, ks[2], bs[2], bs[1], True)
    return e, bs[2]


def full_volume(e, bias):
    """Even lattice (plain [B,Z,H,W,C], planar [4,B,Z,H/2,W/2,C] or planar z-split
    [4,B,2,H/2,W/2,2,C]) + bias -> dense [B,C,Z,2H,2W] (odd rows/cols = bias)."""
    if e.dim() == 7:
        e = planar_zs_to_plain(e)
    elif e.dim() == 6:
        e = planar_to_plain(e)
    b, z, h, w, c = e.shape
    y = bias.view(1, c, 1, 1, 1).expand(b, c, z, 2 * h, 2 * w).contiguous()
    y[:, :, :, ::2, ::2] = e.permute(0, 4, 1, 2, 3)
    return y


def upsample_dense(x0, weights, biases):
    """Drop-in value of ``nn.Sequential(ConvTranspose3d x3)(x0)`` for the reference geometry."""
    e, b = upsample_lattice(x0, weights, biases)
    return full_volume(e, b)
