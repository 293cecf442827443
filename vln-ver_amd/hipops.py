"""ctypes binding of libver_hip.so (C ABI: include/ver_ops.h) + the autograd wrappers.

There is NO fallback: if the library is missing or a tensor is not on the GPU these
functions raise.  PyTorch is used only for device memory, the current HIP stream and
autograd bookkeeping.
"""
import ctypes
import os
import re

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

_PKG = os.path.dirname(os.path.abspath(__file__))
# (VER_HIP_LIB: another build of the same ABI, e.g. the host-ASan build libver_hip_asan.so of tests/test_abi_cpu.py)
LIB_PATH = os.environ.get('VER_HIP_LIB') or os.path.join(_PKG, 'libver_hip.so')
ABI_VERSION = 31
HEADER = os.path.join(os.path.dirname(_PKG), 'include', 'ver_ops.h')
_PARAMS = {'int': ctypes.c_int, 'long': ctypes.c_long, 'float': ctypes.c_float}
_RETURNS = {'int': ctypes.c_int, 'long': ctypes.c_long, 'const char*': ctypes.c_char_p}


class HipLibraryError(RuntimeError):
    pass


def prototypes(path=HEADER):
    """{name: (return type, parameter types)}, as ctypes, of every ``RET ver_name(ARGS);`` the C header declares.  Exactly
    the header's grammar: RET is int, long or const char*; a parameter with a ``*`` is a pointer, any other is
    ``int|long|float name``; ``(void)`` is no parameter.  Anything else raises, as does a ``ver_name(`` that did not
    parse as a declaration."""
    if not os.path.exists(path):
        raise HipLibraryError('%s not found: the C ABI is bound from its prototypes' % path)
    text = re.sub(r'/\*.*?\*/|//[^\n]*|^\s*#[^\n]*', ' ', open(path).read(), flags=re.S | re.M)
    out = {}
    for ret, name, params in re.findall(r'([^;{}()]*?)\b(ver_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text):
        ret = _RETURNS.get(' '.join(ret.split()))
        params = [] if params.strip() == 'void' else [' '.join(q.split()) for q in params.split(',')]
        args = [ctypes.c_void_p if '*' in q else _PARAMS.get(q.rpartition(' ')[0]) for q in params]
        if ret is None or None in args:
            raise HipLibraryError('%s: %s(%s): a type outside int / long / float / pointer' % (path, name, ', '.join(params)))
        out[name] = (ret, args)
    unread = set(re.findall(r'\b(ver_[a-z0-9_]+)\s*\(', text)) - set(out)
    if unread:
        raise HipLibraryError('%s: no prototype read for %s' % (path, ', '.join(sorted(unread))))
    return out


PROTOTYPES = prototypes()
SYMBOLS = tuple(PROTOTYPES)

_lib = None


def lib():
    """Load libver_hip.so once; raise loudly when it is absent or stale."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                '%s not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                '(hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback.' % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (ret, params) in PROTOTYPES.items():
            if not hasattr(handle, name):
                raise HipLibraryError('%s does not export %s' % (LIB_PATH, name))
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = ret, params
        if handle.ver_abi_version() != ABI_VERSION:
            raise HipLibraryError('libver_hip.so ABI %d != expected %d: rebuild'
                                  % (handle.ver_abi_version(), ABI_VERSION))
        _lib = handle
    return _lib


def _check(rc, what):
    if rc != 0:
        msg = lib().ver_last_error()
        raise RuntimeError('%s failed (%d): %s' % (what, rc, msg.decode() if msg else ''))


class KernelTimer:
    """Optional HIP-event timing of every C-ABI launch (bench.py's roofline leg).  Events are
    recorded on the stream the kernel is launched on (torch's current stream)."""

    def __init__(self):
        self.records = []          # (name, start_event, end_event, meta)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1, meta in self.records:
            d = out.setdefault(name, dict(count=0, ms=0.0, flops=0.0, meta=meta))
            d['count'] += 1
            d['ms'] += e0.elapsed_time(e1)
            if meta and 'flops' in meta:
                d['flops'] += meta['flops']
        return out


KERNEL_TIMER = None


def _launch(name, fn, meta=None):
    """Run ``fn`` (one C-ABI call) and check its return code; time it when a timer is set."""
    timer = KERNEL_TIMER
    if timer is None:
        return _check(fn(), name)
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = fn()
    e1.record()
    timer.records.append((name, e0, e1, meta))
    return _check(rc, name)


class timed:
    """``with timed('head_gemm_fwd', flops): torch.mm(...)`` -- the same HIP-event bracket as ``_launch`` for work that is
    not a C-ABI call (the library GEMMs of the head), so that bench.py can put the dense part's achieved TFLOP/s next to
    the gather's GB/s.  Free when no timer is set."""

    def __init__(self, name, flops=0.0):
        self.name, self.flops = name, flops

    def __enter__(self):
        self.timer = KERNEL_TIMER
        if self.timer is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.timer is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.timer.records.append((self.name, self.e0, e1, dict(flops=self.flops)))
        return False


def _p(t):
    """Address of a tensor's data for a pointer parameter: None (NULL) for None, 0 (NULL) for an empty tensor, where the
    C side returns early."""
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gpu(t, name, dtype=None):
    if not t.is_cuda:
        raise RuntimeError('%s must be a GPU tensor: the VER ops only exist as HIP kernels' % name)
    if dtype is not None and t.dtype != dtype:
        raise TypeError('%s must be %s, got %s' % (name, dtype, t.dtype))
    return t.contiguous()


# ------------------------------------------------------------------------------------------
class MultiScaleDeformableAttnFunction_fp32(Function):
    """Same call signature and gradient contract as the reference's wrapper of the mmcv op
    (bevformer/modules/multi_scale_deformable_attn_function.py:90-163)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type='cuda', cast_inputs=torch.float32)
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations,
                attention_weights, im2col_step):
        value = _gpu(value, 'value', torch.float32)
        loc = _gpu(sampling_locations, 'sampling_locations', torch.float32)
        aw = _gpu(attention_weights, 'attention_weights', torch.float32)
        shapes = _gpu(value_spatial_shapes, 'value_spatial_shapes').to(torch.int64)
        lsi = _gpu(value_level_start_index, 'value_level_start_index').to(torch.int64)
        bs, nk, heads, hd = value.shape
        _, nq, _, nl, npt, _ = loc.shape
        ctx.im2col_step = im2col_step
        out = value.new_empty(bs, nq, heads * hd)
        _check(lib().ver_msda_forward(_p(value), _p(shapes), _p(lsi), _p(loc), _p(aw), _p(out),
                                      bs, nk, heads, hd, nl, npt, nq, im2col_step, _stream()),
               'ver_msda_forward')
        ctx.save_for_backward(value, shapes, lsi, loc, aw)
        return out

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type='cuda')
    def backward(ctx, grad_output):
        value, shapes, lsi, loc, aw = ctx.saved_tensors
        bs, nk, heads, hd = value.shape
        _, nq, _, nl, npt, _ = loc.shape
        grad_value = torch.zeros_like(value)
        grad_loc = torch.zeros_like(loc)
        grad_aw = torch.zeros_like(aw)
        go = _gpu(grad_output, 'grad_output').float().contiguous()
        _check(lib().ver_msda_backward(_p(value), _p(shapes), _p(lsi), _p(loc), _p(aw), _p(go),
                                       _p(grad_value), _p(grad_loc), _p(grad_aw), bs, nk, heads, hd,
                                       nl, npt, nq, ctx.im2col_step, _stream()),
               'ver_msda_backward')
        return grad_value, None, None, grad_loc, grad_aw, None


# the reference selects the fp32 variant for every dtype (spatial_cross_attention.py:388-391)
MultiScaleDeformableAttnFunction_fp16 = MultiScaleDeformableAttnFunction_fp32


# ------------------------------------------------------------------------------------------
class HitTable:
    """Per-batch visibility structure (layout: include/ver_ops.h, "Hit table")."""

    __slots__ = ('uv', 'vis', 'vis_list', 'vis_cnt', 'zero_list', 'zero_cnt', 'fwd_list', 'fwd_cnt',
                 'B', 'Ncam', 'Nq', 'D')

    def __init__(self, B, Ncam, Nq, D, device):
        self.B, self.Ncam, self.Nq, self.D = B, Ncam, Nq, D
        self.uv = torch.empty(B, Ncam, Nq, D, 2, dtype=torch.float32, device=device)
        self.vis = torch.empty(B, Nq, dtype=torch.uint8, device=device)
        self.vis_list = torch.empty(B, Ncam, Nq, dtype=torch.int32, device=device)
        self.vis_cnt = torch.empty(B, Ncam, dtype=torch.int32, device=device)
        self.zero_list = torch.empty(B, Nq, dtype=torch.int32, device=device)
        self.zero_cnt = torch.empty(B, dtype=torch.int32, device=device)
        self.fwd_list = torch.empty(B, Ncam, Nq, dtype=torch.int32, device=device)
        self.fwd_cnt = torch.empty(B, Ncam, 2, dtype=torch.int32, device=device)

    def mask(self):
        """bool [Ncam, B, Nq, 1] in the reference's bev_mask layout (for inspection/tests)."""
        bits = torch.arange(self.Ncam, device=self.vis.device, dtype=torch.uint8)
        m = (self.vis[None] >> bits[:, None, None]) & 1
        return m.bool().unsqueeze(-1)


def project_points(world2pixel, origin, pc_range, bev_z, bev_h, bev_w, img_w=1280.0, img_h=1024.0):
    """get_reference_points('3d') + point_sampling + list building for B viewpoints
    (voxel_encoder.py:54-83,119-195).  world2pixel f32[B,Ncam,4,4], origin f32[B,3]."""
    w2p = _gpu(world2pixel, 'world2pixel', torch.float32)
    org = _gpu(origin, 'origin', torch.float32)
    B, ncam = w2p.shape[0], w2p.shape[1]
    nq = bev_z * bev_h * bev_w
    hit = HitTable(B, ncam, nq, 1, w2p.device)
    rng = (ctypes.c_float * 6)(*[float(v) for v in pc_range])
    _launch('ver_project_points', lambda: lib().ver_project_points(
        _p(w2p), _p(org), rng, B, ncam, bev_z, bev_h, bev_w, img_w, img_h,
        _p(hit.uv), _p(hit.vis), _p(hit.vis_list), _p(hit.vis_cnt), _p(hit.zero_list), _p(hit.zero_cnt),
        _p(hit.fwd_list), _p(hit.fwd_cnt), _stream()))
    return hit


def hits_from_mask(reference_points_cam, bev_mask):
    """Hit table from tensors in the reference's layout: reference_points_cam
    [Ncam,B,Nq,D,2], bev_mask [Ncam,B,Nq,D] (spatial_cross_attention.py:86-87)."""
    ncam, B, nq, D = bev_mask.shape
    mask = _gpu(bev_mask, 'bev_mask').to(torch.uint8).contiguous()
    hit = HitTable(B, ncam, nq, D, mask.device)
    hit.uv.copy_(reference_points_cam.to(torch.float32).permute(1, 0, 2, 3, 4))
    _check(lib().ver_hits_from_mask(_p(mask), B, ncam, nq, D, _p(hit.vis), _p(hit.vis_list),
                                    _p(hit.vis_cnt), _p(hit.zero_list), _p(hit.zero_cnt), _p(hit.fwd_list),
                                    _p(hit.fwd_cnt), _stream()),
           'ver_hits_from_mask')
    return hit


_SIDE_STREAMS = {}
SCA_PREZERO = True       # False (assign from a script): the gather zero-fills in line instead of on a side stream


def _side_stream(device):
    st = _SIDE_STREAMS.get(device)
    if st is None:
        st = _SIDE_STREAMS[device] = torch.cuda.Stream(device=device)
    return st


class PreparedSlots:
    """Output buffer of one ``ver_sca_forward`` call whose zero fill is already under way on a side stream."""
    __slots__ = ('slots', 'done')

    def __init__(self, slots, done):
        self.slots, self.done = slots, done


def sca_prepare_slots(hit, row_floats):
    """Allocate the gather's output and zero-fill the rows ``hit.zero_list`` names on a SIDE stream
    (``ver_sca_zero_rows``).  The fill depends on the hit table only, so a caller that does this before the
    projections feeding the gather (value_proj, sampling_offsets / attention_weights) hides it under them instead
    of paying it in front of the gather.  Returns None when it cannot be overlapped safely (stream capture,
    ``SCA_PREZERO`` False): ``sca_gather`` then fills in line, as before."""
    if not SCA_PREZERO or torch.cuda.is_current_stream_capturing():
        return None
    dev = hit.vis.device
    slots = torch.empty(hit.B, hit.Nq, row_floats, dtype=torch.float32, device=dev)
    main, side = torch.cuda.current_stream(dev), _side_stream(dev)
    # the block may still be in use by kernels queued on the main stream: the fill starts where the main stream is now
    side.wait_stream(main)
    slots.record_stream(side)       # (a buffer dropped before the gather consumed it must outlive the fill)
    with torch.cuda.stream(side):
        _launch('ver_sca_zero_rows', lambda: lib().ver_sca_zero_rows(
            _p(hit.zero_list), _p(hit.zero_cnt), _p(slots), hit.B, hit.Nq, row_floats, _stream()))
        done = torch.cuda.Event()
        done.record(side)
    return PreparedSlots(slots, done)


class SCAGatherFunction(Function):
    """slots = fused multi-view gather (ver_sca_forward / ver_sca_backward).

    ``value`` may be fp32 or bf16 (what ``value_proj`` emits under bf16 autocast).  fp32 tiles: fp32 arithmetic
    throughout, like the reference's fp32-forced op.  bf16 tiles at the vocc.py shape: the points of a (voxel, head,
    corner) are accumulated in packed fp16, everything after the corner fold in fp32 (contract: include/ver_ops.h)."""

    @staticmethod
    def forward(ctx, value, offsets, logits, hit, map_h, map_w, prepared=None, head_major=False, lowp_out=False):
        if value.dtype not in (torch.float32, torch.bfloat16):
            value = value.float()
        value = _gpu(value, 'value')
        offsets = _gpu(offsets, 'offsets').float().contiguous()
        logits = _gpu(logits, 'logits').float().contiguous()
        vdt = 1 if value.dtype == torch.bfloat16 else 0
        if head_major:                      # value [heads, B, Ncam, Nk, hd] (VER_SCA_VALUE_HEAD_MAJOR)
            heads, B, ncam, nk, hd = value.shape
        else:
            B, ncam, nk, heads, hd = value.shape
        points = logits.shape[-1]
        nq = hit.Nq
        assert nk == map_h * map_w and B == hit.B and ncam == hit.Ncam
        assert offsets.shape == (B, nq, heads, points, 2) and logits.shape == (B, nq, heads, points)
        flags = 2 if head_major else 0
        if prepared is not None:
            slots = prepared.slots
            assert slots.shape == (B, nq, heads * hd) and slots.dtype == torch.float32 and slots.is_contiguous()
            # (long done: it ran under the GEMMs.  With a KernelTimer the join is bracketed by events on the launch stream:
            #  what bench.py reports as the part of the zero fill that was NOT hidden)
            with timed('ver_sca_zero_wait'):
                torch.cuda.current_stream(slots.device).wait_event(prepared.done)
            with timed('ver_event_floor'):          # (an empty bracket: what two event records cost by themselves)
                pass
            flags |= 1                                                               # VER_SCA_ROWS_PREZEROED
        else:
            slots = torch.empty(B, nq, heads * hd, dtype=torch.float32, device=value.device)
        _launch('ver_sca_forward', lambda: lib().ver_sca_forward(
            _p(value), vdt, _p(offsets), _p(logits), _p(hit.uv), _p(hit.vis), _p(hit.vis_list),
            _p(hit.vis_cnt), _p(hit.zero_list), _p(hit.zero_cnt), _p(hit.fwd_list), _p(hit.fwd_cnt), _p(slots),
            B, ncam, nq, hit.D, heads, hd,
            points, map_h, map_w, flags, _stream()), meta=dict(prezeroed=bool(flags & 1), head_major=head_major))
        ctx.save_for_backward(value, offsets, logits)
        ctx.hit, ctx.map_hw, ctx.vdt, ctx.head_major = hit, (map_h, map_w), vdt, head_major
        if lowp_out and vdt == 1:
            # the consumer is a bf16 GEMM (output_proj under autocast): hand it the bf16 copy it would make anyway -- the
            # gradient then comes back in bf16 and ver_sca_backward reads it as it is (VER_SCA_GRAD_SLOTS_BF16) instead of
            # a cast kernel writing an fp32 copy for it first
            return slots.to(torch.bfloat16)
        return slots

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_slots):
        value, offsets, logits = ctx.saved_tensors
        hit = ctx.hit
        map_h, map_w = ctx.map_hw
        if ctx.head_major:
            heads, B, ncam, nk, hd = value.shape
        else:
            B, ncam, nk, heads, hd = value.shape
        points = logits.shape[-1]
        # the matrix-core backward rounds d(value) to bf16 itself (no separate cast pass over the tensor)
        gdt = lib().ver_sca_backward_grad_dtype(ctx.vdt, hd, points, map_h, map_w)
        gs = _gpu(grad_slots, 'grad_slots')
        gs_bf16 = gs.dtype == torch.bfloat16 and gdt == 1
        gs = gs.contiguous() if gs_bf16 else gs.float().contiguous()
        # d(value) is always written in the REFERENCE layout [B, Ncam, Nk, heads, hd]; for a head-major value it is handed
        # back as the permuted view of that buffer (same shape as value, no copy)
        g_value = torch.empty((B, ncam, nk, heads, hd), dtype=torch.bfloat16 if gdt == 1 else torch.float32, device=value.device)
        g_off = torch.empty_like(offsets)
        g_log = torch.empty_like(logits)
        _launch('ver_sca_backward', lambda: lib().ver_sca_backward(
            _p(value), ctx.vdt, _p(offsets), _p(logits), _p(hit.uv), _p(hit.vis), _p(hit.vis_list),
            _p(hit.vis_cnt), _p(hit.fwd_list), _p(hit.fwd_cnt), _p(gs), _p(g_value), gdt, _p(g_off), _p(g_log), B, ncam,
            hit.Nq, hit.D, heads,
            hd, points, map_h, map_w, (2 if ctx.head_major else 0) | (4 if gs_bf16 else 0), _stream()),
            meta=dict(grad_slots_bf16=gs_bf16))
        g_value = g_value.to(value.dtype)
        if ctx.head_major:
            g_value = g_value.permute(3, 0, 1, 2, 4)
        return g_value, g_off, g_log, None, None, None, None, None, None


def sca_gather(value, offsets, logits, hit, map_h, map_w, prepared=None, head_major=False, lowp_out=False):
    return SCAGatherFunction.apply(value, offsets, logits, hit, map_h, map_w, prepared, head_major, lowp_out)


def sca_head_major_supported(dtype, head_dim, points, map_h, map_w):
    """True where ``ver_sca_forward`` / ``ver_sca_backward`` read a head-major value tensor (contiguous tiles)."""
    return dtype == torch.bfloat16 and bool(lib().ver_sca_head_major_supported(1, head_dim, points, map_h, map_w))


class HeadMajorLinearFunction(Function):
    """``value_proj`` writing the head-major layout: x bf16 [M, C_in], weight [heads*hd, C_in], bias [heads*hd] ->
    [heads, M, hd]: one plain GEMM per head into its slab of the output (no stride-0 batch operand: those fault inside
    some hipBLASLt solutions when TunableOp tries them, dense_heads/row_linear.py).  The gradient comes
    back as the permuted view of a reference-layout [M, heads*hd] buffer (SCAGatherFunction.backward), so d(weight) is a
    plain split-row GEMM over [M, heads*hd]; d(x) likewise when it is needed."""

    @staticmethod
    def forward(ctx, x, weight, bias, heads):
        m, c_in = x.shape
        w = weight.to(x.dtype)
        hd = w.shape[0] // heads
        out = x.new_empty(heads, m, hd)
        b = bias.to(x.dtype).view(heads, hd)
        w3 = w.view(heads, hd, c_in)
        for h in range(heads):
            torch.addmm(b[h], x, w3[h].t(), out=out[h])
        ctx.save_for_backward(x, w)
        ctx.heads = heads
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        heads = ctx.heads
        m = x.shape[0]
        g2 = g.permute(1, 0, 2).reshape(m, -1)              # [M, heads*hd]: a view when g is the gather's permuted buffer
        from .dense_heads.upsample import rows_tn
        dw = rows_tn(g2, x) if ctx.needs_input_grad[1] else None        # [heads*hd, C_in]
        db = g2.sum(0, dtype=torch.float32) if ctx.needs_input_grad[2] else None
        dx = g2 @ w if ctx.needs_input_grad[0] else None
        return dx, dw, db, None


def head_major_linear(x, weight, bias, heads):
    return HeadMajorLinearFunction.apply(x, weight, bias, heads)


# ------------------------------------------------------------------------------------------
class LatticeIm2colFunction(Function):
    """col = im2col(lattice) for the even-lattice upsample (ver_lattice_im2col / _col2im).
    lattice [B,Z,H,W,C] channels-last, fp32 or bf16 -> [B*Z*H*W, ntaps*C]."""

    @staticmethod
    def forward(ctx, lattice, taps):
        lattice = _gpu(lattice, 'lattice')
        if lattice.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError('lattice must be fp32 or bf16')
        B, Z, H, W, C = lattice.shape
        flat = [int(v) for t in taps for v in t]
        arr = (ctypes.c_int * len(flat))(*flat)
        dt = 1 if lattice.dtype == torch.bfloat16 else 0
        col = torch.empty(B * Z * H * W, len(taps) * C, dtype=lattice.dtype, device=lattice.device)
        _launch('ver_lattice_im2col', lambda: lib().ver_lattice_im2col(
            _p(lattice), _p(col), arr, len(taps), B, Z, H, W, C, dt, _stream()))
        ctx.geom = (B, Z, H, W, C, dt, arr, len(taps))
        return col

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_col):
        B, Z, H, W, C, dt, arr, ntaps = ctx.geom
        want = torch.bfloat16 if dt else torch.float32
        g = _gpu(grad_col, 'grad_col').to(want).contiguous()
        grad = torch.empty(B, Z, H, W, C, dtype=want, device=g.device)
        _launch('ver_lattice_col2im', lambda: lib().ver_lattice_col2im(
            _p(g), _p(grad), arr, ntaps, B, Z, H, W, C, dt, _stream()))
        return grad, None


def lattice_im2col(lattice, taps):
    return LatticeIm2colFunction.apply(lattice, taps)


class ConvTWeightFunction(Function):
    """ConvTranspose3d weight fp32 [Ci,Co,3,5,5] -> correlation taps [75,Ci,Co] (fp32 or bf16),
    ver_convt_weight_forward / _backward."""

    @staticmethod
    def forward(ctx, weight, dtype):
        weight = _gpu(weight, 'weight')
        if weight.dtype != torch.float32 or tuple(weight.shape[2:]) != (3, 5, 5):
            raise TypeError('weight must be fp32 [Ci,Co,3,5,5]')
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError('taps dtype must be fp32 or bf16')
        weight = weight.contiguous()
        ci, co = weight.shape[:2]
        taps = torch.empty(75, ci, co, dtype=dtype, device=weight.device)
        dt = 1 if dtype == torch.bfloat16 else 0
        _launch('ver_convt_weight_forward', lambda: lib().ver_convt_weight_forward(
            _p(weight), _p(taps), ci * co, dt, _stream()))
        ctx.shape, ctx.dt, ctx.dtype = tuple(weight.shape), dt, dtype
        return taps

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_taps):
        g = _gpu(grad_taps, 'grad_taps').to(ctx.dtype).contiguous()
        ci, co = ctx.shape[:2]
        gw = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        _launch('ver_convt_weight_backward', lambda: lib().ver_convt_weight_backward(
            _p(g), _p(gw), ci * co, ctx.dt, _stream()))
        return gw, None


def convt_weight_taps(weight, dtype):
    return ConvTWeightFunction.apply(weight, dtype)


def convt_weight_backward_blocks(blocks, block_offsets, prev_bias, grad_v, ci, co):
    """ver_convt_weight_backward_blocks (no autograd): the fp32 gradient [Ci,Co,3,5,5] of a ConvTranspose3d weight from the
    class-stacked weight gradients of a lattice layer: ``blocks`` [rows, ld] (fp32 or bf16, unit column stride); tap t is
    the sum of the [Ci x Co] blocks at element offsets ``block_offsets[t]`` (int64 [75,2] on the device, -1 = none) plus
    ``prev_bias[ci] * grad_v[t, co]`` (both in blocks' dtype, or both None)."""
    src = _gpu(blocks, 'blocks')
    if src.dim() != 2 or src.stride(1) != 1 or src.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError('convt_weight_backward_blocks: blocks must be an fp32 / bf16 matrix with unit column stride')
    off = _gpu(block_offsets, 'block_offsets')
    if off.dtype != torch.int64 or tuple(off.shape) != (75, 2) or not off.is_contiguous():
        raise TypeError('convt_weight_backward_blocks: block_offsets must be a contiguous int64 [75, 2]')
    if (prev_bias is None) != (grad_v is None):
        raise ValueError('convt_weight_backward_blocks: prev_bias and grad_v come together')
    if prev_bias is not None:
        prev_bias = _gpu(prev_bias, 'prev_bias').to(src.dtype).contiguous()
        grad_v = _gpu(grad_v, 'grad_v').to(src.dtype).contiguous()
        if prev_bias.numel() != ci or tuple(grad_v.shape) != (75, co):
            raise ValueError('convt_weight_backward_blocks: prev_bias [Ci] and grad_v [75, Co] expected')
    gw = torch.empty(ci, co, 3, 5, 5, dtype=torch.float32, device=src.device)
    dt = 1 if src.dtype == torch.bfloat16 else 0
    _launch('ver_convt_weight_backward_blocks', lambda: lib().ver_convt_weight_backward_blocks(
        _p(src), _p(off), src.stride(0), _p(prev_bias), _p(grad_v), _p(gw), ci, co, dt, _stream()))
    return gw


def convt_weight_forward_blocks(weight, block_offsets, blocks, ci, co):
    """ver_convt_weight_forward_blocks (no autograd): the fp32 ConvTranspose3d weight [Ci,Co,3,5,5] written into the
    class-stacked weight matrix ``blocks`` [rows, ld] (fp32 or bf16, unit column stride): tap t at element offsets
    ``block_offsets[t]`` (int64 [75,2] on the device, -1 = none).  Rows that hold no tap block are not touched."""
    w = _gpu(weight, 'weight')
    dst = _gpu(blocks, 'blocks')
    if w.dtype != torch.float32 or not w.is_contiguous() or tuple(w.shape) != (ci, co, 3, 5, 5):
        raise TypeError('convt_weight_forward_blocks: weight must be a contiguous fp32 [Ci, Co, 3, 5, 5]')
    if dst.dim() != 2 or dst.stride(1) != 1 or dst.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError('convt_weight_forward_blocks: blocks must be an fp32 / bf16 matrix with unit column stride')
    off = _gpu(block_offsets, 'block_offsets')
    if off.dtype != torch.int64 or tuple(off.shape) != (75, 2) or not off.is_contiguous():
        raise TypeError('convt_weight_forward_blocks: block_offsets must be a contiguous int64 [75, 2]')
    _launch('ver_convt_weight_forward_blocks', lambda: lib().ver_convt_weight_forward_blocks(
        _p(w), _p(off), dst.stride(0), _p(dst), ci, co, 1 if dst.dtype == torch.bfloat16 else 0, _stream()))
    return blocks


def _blocks_vec_args(blocks, block_rows, name):
    src = _gpu(blocks, 'blocks')
    if src.dim() != 2 or src.stride(1) != 1 or src.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError('%s: blocks must be an fp32 / bf16 matrix with unit column stride' % name)
    rows = _gpu(block_rows, 'block_rows')
    if rows.dtype != torch.int64 or rows.dim() != 1 or not rows.is_contiguous():
        raise TypeError('%s: block_rows must be a contiguous int64 vector' % name)
    return src, rows


def blocks_vec_forward(blocks, block_rows, ci, x):
    """ver_blocks_vec_forward (no autograd): x fp32 [Ci] through every [Ci x ncols] block of ``blocks`` (first rows
    ``block_rows``, int64 on the device) -> fp32 [nblocks, ncols]."""
    src, rows = _blocks_vec_args(blocks, block_rows, 'blocks_vec_forward')
    x = _gpu(x, 'x').float().contiguous()
    if x.numel() != ci:
        raise ValueError('blocks_vec_forward: x must have Ci elements')
    part = torch.empty(8, rows.numel(), src.shape[1], dtype=torch.float32, device=src.device)      # 8 slices of ci
    _launch('ver_blocks_vec_forward', lambda: lib().ver_blocks_vec_forward(
        _p(src), _p(rows), rows.numel(), src.stride(0), ci, src.shape[1], _p(x), _p(part),
        1 if src.dtype == torch.bfloat16 else 0, _stream()))
    return part.sum(0)


def blocks_vec_backward(blocks, block_rows, ci, grad_vec):
    """ver_blocks_vec_backward (no autograd): the adjoint of ``blocks_vec_forward`` in x: fp32 [Ci]."""
    src, rows = _blocks_vec_args(blocks, block_rows, 'blocks_vec_backward')
    gv = _gpu(grad_vec, 'grad_vec').float().contiguous()
    if tuple(gv.shape) != (rows.numel(), src.shape[1]):
        raise ValueError('blocks_vec_backward: grad_vec must be [nblocks, ncols]')
    part = torch.empty(rows.numel(), ci, dtype=torch.float32, device=src.device)                     # one row per block
    _launch('ver_blocks_vec_backward', lambda: lib().ver_blocks_vec_backward(
        _p(src), _p(rows), rows.numel(), src.stride(0), ci, src.shape[1], _p(gv), _p(part),
        1 if src.dtype == torch.bfloat16 else 0, _stream()))
    return part.sum(0)


PLAIN, PLANAR, ZSPLIT, PLANAR_ZSPLIT = 0, 1, 2, 3      # lattice layouts of ver_lattice_gather / _transpose


def _lattice_dims(t, layout):
    """(B, Zs, C) of a lattice tensor in the given layout."""
    s = t.shape
    if layout == PLAIN:          # [B,Z,H,W,C]
        return s[0], s[1], s[4]
    if layout == PLANAR:         # [4,B,Z,H/2,W/2,C]
        return s[1], s[2], s[5]
    if layout == ZSPLIT:         # [B,2,H,W,2,C]
        return s[0], 4, s[5]
    return s[1], 4, s[6]         # [4,B,2,H/2,W/2,2,C]


def lattice_transpose(channels_last, channel_first, combined_hw, layout, to_channel_first):
    """ver_lattice_transpose (no autograd): channels_last lattice in one of the four layouts
    <-> channel_first [B, stride] rows holding [C,Z,H,W] at their start."""
    cl, cf = _gpu(channels_last, 'channels_last'), _gpu(channel_first, 'channel_first')
    if not (cl.is_contiguous() and cf.is_contiguous() and cl.dtype == cf.dtype):
        raise ValueError('lattice_transpose: contiguous buffers of one dtype required')
    if cl.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError('lattice_transpose: fp32 or bf16')
    H, W = combined_hw
    B, Z, C = _lattice_dims(cl, int(layout))
    dt = 1 if cl.dtype == torch.bfloat16 else 0
    _launch('ver_lattice_transpose', lambda: lib().ver_lattice_transpose(
        _p(cl), _p(cf), cf.shape[1], B, Z, H, W, C, layout, to_channel_first, dt, _stream()))


def lattice_rows(channels_last, rows, row_map, combined_hw, layout, to_rows):
    """ver_lattice_rows (no autograd): bf16 lattice (channels-last, layout 0-3) <-> ``rows``, ONE flat bf16 buffer that
    holds the operand matrices of all pattern groups; ``row_map``: dict(quarter, period, seg_off, seg_len, seg_base,
    seg_pitch, seg_rows) of dense_heads/occ_proj_lattice.py (element offsets into ``rows``)."""
    cl, buf = _gpu(channels_last, 'channels_last'), _gpu(rows, 'rows')
    if not (cl.is_contiguous() and buf.is_contiguous() and cl.dtype == torch.bfloat16 and buf.dtype == torch.bfloat16):
        raise TypeError('lattice_rows: contiguous bf16 buffers required')
    H, W = combined_hw
    B, Z, C = _lattice_dims(cl, int(layout))
    n = len(row_map['seg_off'])
    need = max(b + B * r * p for b, r, p in zip(row_map['seg_base'], row_map['seg_rows'], row_map['seg_pitch']))
    if buf.numel() < need:
        raise ValueError('lattice_rows: rows buffer of %d elements, %d needed' % (buf.numel(), need))
    ints = lambda k: (ctypes.c_int * n)(*[int(v) for v in row_map[k]])
    base = (ctypes.c_long * n)(*[int(v) for v in row_map['seg_base']])
    _launch('ver_lattice_rows', lambda: lib().ver_lattice_rows(
        _p(cl), _p(buf), row_map['quarter'], row_map['period'], n, ints('seg_off'), ints('seg_len'),
        base, ints('seg_pitch'), ints('seg_rows'), B, Z, H, W, C, layout, to_rows, 1, _stream()))


def run_gather(image, run_start, aug_idx, rows, n_rows, run_len):
    """ver_run_gather (no autograd): image [B, stride] -> rows [B*n_rows, row_elems]; run_start int32 [n_rows, runs],
    aug_idx int32 [n_rows, n_aug] (indices into a sample's image row)."""
    img, out = _gpu(image, 'image'), _gpu(rows, 'rows')
    if not (img.is_contiguous() and out.is_contiguous() and img.dtype == out.dtype):
        raise ValueError('run_gather: contiguous buffers of one dtype required')
    if img.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError('run_gather: fp32 or bf16')
    B = img.shape[0]
    runs, n_aug = run_start.shape[1], aug_idx.shape[1]
    _launch('ver_run_gather', lambda: lib().ver_run_gather(
        _p(img), img.shape[1], _p(run_start), _p(aug_idx), _p(out), B, n_rows, runs, run_len, n_aug, out.shape[1],
        1 if img.dtype == torch.bfloat16 else 0, _stream()))


def run_scatter(rows, image, run_start, n_rows, run_len):
    """ver_run_scatter (no autograd): rows [B*n_rows, row_elems] -> the runs of image [B, stride]."""
    src, img = _gpu(rows, 'rows'), _gpu(image, 'image')
    if not (img.is_contiguous() and src.is_contiguous() and img.dtype == src.dtype):
        raise ValueError('run_scatter: contiguous buffers of one dtype required')
    if img.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError('run_scatter: fp32 or bf16')
    B = img.shape[0]
    _launch('ver_run_scatter', lambda: lib().ver_run_scatter(
        _p(src), _p(img), img.shape[1], _p(run_start), B, n_rows, run_start.shape[1], run_len,
        src.shape[1], 1 if img.dtype == torch.bfloat16 else 0, _stream()))


def _tap_args(taps, col_offset):
    flat = [int(v) for t in taps for v in t]
    return (ctypes.c_int * len(flat))(*flat), (ctypes.c_long * len(col_offset))(*[int(o) for o in col_offset])


def lattice_gather(src, col, taps, col_offset, combined_hw, layout, row_z=None, const_rows=None, const_offset=None):
    """ver_lattice_gather (no autograd): src lattice in `layout` -> tap blocks of
    col [B*row_z*H*W, stride] at the given column offsets (row_z defaults to the source's z count).
    ``const_rows`` [row_z*H*W, n_blocks, width] + ``const_offset`` (n_blocks column offsets): constant-pattern blocks of
    one viewpoint's rows, written into every viewpoint's rows by the same kernel."""
    src, col = _gpu(src, 'src'), _gpu(col, 'col')
    if not (src.is_contiguous() and col.is_contiguous() and src.dtype == col.dtype):
        raise ValueError('lattice_gather: contiguous src / col of one dtype required')
    H, W = combined_hw
    B, Zs, C = _lattice_dims(src, int(layout))
    Zr = Zs if row_z is None else int(row_z)
    arr, offs = _tap_args(taps, col_offset)
    dt = 1 if src.dtype == torch.bfloat16 else 0
    cptr, coffs, nblk, cw = None, None, 0, 0
    if const_rows is not None:
        const_rows = _gpu(const_rows, 'const_rows')
        if not (const_rows.is_contiguous() and const_rows.dtype == col.dtype and const_rows.shape[0] == Zr * H * W):
            raise ValueError('lattice_gather: const_rows must be a contiguous [row_z*H*W, blocks, width] table of col.dtype')
        nblk, cw = int(const_rows.shape[1]), int(const_rows.shape[2])
        cptr, coffs = _p(const_rows), (ctypes.c_long * nblk)(*[int(o) for o in const_offset])
    _launch('ver_lattice_gather', lambda: lib().ver_lattice_gather(
        _p(src), _p(col), arr, offs, col.shape[1], len(taps), B, Zr, Zs, H, W, C, layout, dt, cptr, coffs, nblk, cw, _stream()))
    return col


def lattice_scatter(grad_col, grad_src, taps, col_offset, combined_hw, layout, row_z=None):
    """ver_lattice_scatter (no autograd): the adjoint of ``lattice_gather`` into grad_src (overwritten)."""
    grad_col, grad_src = _gpu(grad_col, 'grad_col'), _gpu(grad_src, 'grad_src')
    if not (grad_src.is_contiguous() and grad_col.is_contiguous() and grad_src.dtype == grad_col.dtype):
        raise ValueError('lattice_scatter: contiguous buffers of one dtype required')
    H, W = combined_hw
    B, Zs, C = _lattice_dims(grad_src, int(layout))
    Zr = Zs if row_z is None else int(row_z)
    arr, offs = _tap_args(taps, col_offset)
    dt = 1 if grad_src.dtype == torch.bfloat16 else 0
    _launch('ver_lattice_scatter', lambda: lib().ver_lattice_scatter(
        _p(grad_col), _p(grad_src), arr, offs, grad_col.shape[1], len(taps), B, Zr, Zs, H, W, C, layout, dt, _stream()))
    return grad_src


# ------------------------------------------------------------------------------------------
class LayerNormReluFunction(Function):
    """relu(layer_norm(x)) over rows of 128 channels (ver_ln_relu_forward / _backward);
    x fp32 or bf16 [..., 128], output in x's dtype."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x = _gpu(x, 'x')
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError('x must be fp32 or bf16')
        w = x.shape[-1]
        n = x.numel() // w
        gamma = _gpu(gamma, 'gamma').float().contiguous()
        beta = _gpu(beta, 'beta').float().contiguous()
        dt = 1 if x.dtype == torch.bfloat16 else 0
        y = torch.empty_like(x)
        mean = torch.empty(n, dtype=torch.float32, device=x.device)
        rstd = torch.empty(n, dtype=torch.float32, device=x.device)
        _launch('ver_ln_relu_forward', lambda: lib().ver_ln_relu_forward(
            _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), n, w, eps, dt, _stream()))
        ctx.save_for_backward(x, gamma, beta, mean, rstd)
        ctx.dt = dt
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        w = x.shape[-1]
        n = x.numel() // w
        gy = _gpu(grad_y, 'grad_y').to(x.dtype).contiguous()
        gx = torch.empty_like(x)
        gg = torch.empty(w, dtype=torch.float32, device=x.device)
        gb = torch.empty(w, dtype=torch.float32, device=x.device)
        _launch('ver_ln_relu_backward', lambda: lib().ver_ln_relu_backward(
            _p(x), _p(gy), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(gx), _p(gg), _p(gb), n, w, ctx.dt, _stream()))
        return gx, gg, gb, None


def layer_norm_relu(x, gamma, beta, eps=1e-5):
    return LayerNormReluFunction.apply(x, gamma, beta, eps)


# ------------------------------------------------------------------------------------------
class LabelRangeFlag:
    """Sticky device-side "a label was outside [0, C]" flag of the fused focal loss, with an ASYNCHRONOUS host mirror:
    every fused call ORs into the device int (ver_focal_loss_forward) and queues a copy of it into pinned host memory;
    ``poll()`` reads the newest copy that has already arrived -- no device synchronisation -- and raises once it is
    set, so a bad label is reported one or two calls later, every call after that, whatever the caller does with the
    NaN loss in between (the head cleans NaNs out of its losses, as the reference does).  ``poll(sync=True)`` waits."""

    _per_device = {}

    def __init__(self, device):
        self.dev = torch.zeros(1, dtype=torch.int32, device=device)
        self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.event = None
        self.classes = None

    @classmethod
    def of(cls, device):
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        f = cls._per_device.get(key)
        if f is None:
            f = cls._per_device[key] = cls(device)
        return f

    def mirror(self, classes):
        if torch.cuda.is_current_stream_capturing():
            return
        self.classes = classes
        if self.event is not None and not self.event.query():
            return                                          # the previous copy is still in flight: do not overwrite it
        self.host.copy_(self.dev, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()

    def poll(self, sync=False):
        if torch.cuda.is_current_stream_capturing():
            return                                          # (no event queries / host reads inside a capture)
        if sync:
            # always the blocking read: fused calls under stream capture never queued a mirror copy (mirror() is a
            # no-op there), and a queued mirror may predate the offending call
            self.host.copy_(self.dev)
        elif self.event is None or not self.event.query():
            return
        if int(self.host[0]) != 0:
            raise RuntimeError(self._message())

    def _message(self):
        return ('FocalLoss: a target label outside [0, %s] reached the fused focal loss on %s (the loss of that call was '
                'NaN; F.one_hot raises on it in the reference)' % (self.classes, self.dev.device))

    def reset(self):
        self.dev.zero_()
        self.host.zero_()
        self.event = None


class AssignmentFlag(LabelRangeFlag):
    """The same sticky flag for ``lsa_solve``: a cost matrix with a NaN / -inf among its valid entries or without a finite
    assignment (scipy raises on both in the reference's assigner) left its rows unmatched."""

    _per_device = {}

    def _message(self):
        return ('HungarianAssigner3D: a cost matrix with a NaN / -inf entry or without a finite assignment reached lsa_solve '
                'on %s (its queries were all left unmatched; scipy.optimize.linear_sum_assignment raises on it in the '
                'reference)' % (self.dev.device,))


def _class_weight_table(class_weight, classes, device):
    """The ``class_weight`` argument of the weighted focal-loss entries as they read it: fp32 [C + 1], contiguous, on the
    logits' device (one factor per label value; index C = the empty label).  Checked, never converted: a conversion here
    would be a copy per step, and a table the caller overwrites in place must stay the one a captured step reads."""
    if not torch.is_tensor(class_weight):
        raise TypeError('class_weight must be a tensor')
    if class_weight.dtype != torch.float32 or not class_weight.is_contiguous() or class_weight.device != device:
        raise ValueError('class_weight must be a contiguous fp32 tensor on %s' % (device,))
    if tuple(class_weight.shape) != (classes + 1,):
        raise ValueError('class_weight must be [%d] (one factor per label in [0, %d]), got %s'
                         % (classes + 1, classes, tuple(class_weight.shape)))
    return class_weight.detach()


class SigmoidFocalLossSumFunction(Function):
    """sum over all elements of mmdet's sigmoid focal loss (ver_focal_loss_forward / _backward):
    logits fp32|bf16 [N, C] with C % 8 == 0, target int64 [N] in [0, C]; returns an fp32 scalar.
    ``class_weight`` (fp32 [C + 1] or None): row n is multiplied by class_weight[target[n]] (the ``_cw`` entries); no
    gradient flows to it.  uint8 targets (C <= 254; the labels of an ``OccupancyTargets``) are read as they are by the
    ``_u8`` entries -- the same partials and gradients, bit for bit, without an int64 [N] copy; every other integer dtype
    is widened to int64."""

    @staticmethod
    def forward(ctx, logits, target, gamma, alpha, class_weight=None):
        logits = _gpu(logits, 'logits')
        if logits.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError('logits must be fp32 or bf16')
        logits = logits.contiguous()
        target = _gpu(target, 'target')
        if target.dtype != torch.uint8:
            target = target.to(torch.int64).contiguous()
        n, c = logits.shape
        if target.shape != (n,):
            raise ValueError('target must be [N]')
        u8 = '_u8' if target.dtype == torch.uint8 else ''
        if u8 and c > 254:
            raise ValueError('uint8 targets hold at most 254 classes and the empty label, got %d classes' % c)
        dt = 1 if logits.dtype == torch.bfloat16 else 0
        blocks = lib().ver_focal_loss_blocks(n, c)
        partial = torch.zeros(blocks, dtype=torch.float32, device=logits.device)
        flag = LabelRangeFlag.of(logits.device)
        flag.poll()                                          # a bad label of an EARLIER call is reported here
        if class_weight is None:
            entry = getattr(lib(), 'ver_focal_loss_forward' + u8)
            _launch('ver_focal_loss_forward' + u8, lambda: entry(
                _p(logits), _p(target), _p(partial), n, c, gamma, alpha, dt, _p(flag.dev), _stream()))
            ctx.save_for_backward(logits, target)
        else:
            table = _class_weight_table(class_weight, c, logits.device)
            entry = getattr(lib(), 'ver_focal_loss_forward%s_cw' % u8)
            _launch('ver_focal_loss_forward%s_cw' % u8, lambda: entry(
                _p(logits), _p(target), _p(table), _p(partial), n, c, gamma, alpha, dt, _p(flag.dev), _stream()))
            ctx.save_for_backward(logits, target, table)
        flag.mirror(c)
        ctx.cfg = (gamma, alpha, dt)
        return partial.sum()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        logits, target = ctx.saved_tensors[:2]
        gamma, alpha, dt = ctx.cfg
        n, c = logits.shape
        scale = _gpu(grad_out, 'grad_out').float().reshape(1).contiguous()
        grad = torch.empty_like(logits)
        u8 = '_u8' if target.dtype == torch.uint8 else ''
        if len(ctx.saved_tensors) == 2:
            entry = getattr(lib(), 'ver_focal_loss_backward' + u8)
            _launch('ver_focal_loss_backward' + u8, lambda: entry(
                _p(logits), _p(target), _p(scale), _p(grad), n, c, gamma, alpha, dt, _stream()))
        else:
            table = ctx.saved_tensors[2]
            entry = getattr(lib(), 'ver_focal_loss_backward%s_cw' % u8)
            _launch('ver_focal_loss_backward%s_cw' % u8, lambda: entry(
                _p(logits), _p(target), _p(table), _p(scale), _p(grad), n, c, gamma, alpha, dt, _stream()))
        return grad, None, None, None, None


def sigmoid_focal_loss_sum(logits, target, gamma=2.0, alpha=0.25, class_weight=None):
    return SigmoidFocalLossSumFunction.apply(logits, target, float(gamma), float(alpha), class_weight)


# ------------------------------------------------------------------------------------------
def occ_mlp_pack(w1, w2, w3):
    """fp32 nn.Linear weights of ``occ_branches`` -> MFMA fragment image (ver_occ_mlp_pack)."""
    w1, w2, w3 = (_gpu(w, 'weight').detach().float().contiguous() for w in (w1, w2, w3))
    if w1.shape != (128, 128) or w2.shape != (128, 128) or w3.shape != (16, 128):
        raise ValueError('occ_mlp is built for Linear(128,128) x2 + Linear(128,16)')
    image = torch.empty(lib().ver_occ_mlp_image_bytes() // 2, dtype=torch.bfloat16, device=w1.device)
    _launch('ver_occ_mlp_pack', lambda: lib().ver_occ_mlp_pack(_p(w1), _p(w2), _p(w3), _p(image), _stream()))
    return image


def occ_mlp_vectors(b1, g1, be1, b2, g2, be2, b3):
    vec = torch.cat([_gpu(v, 'vector').detach().float().reshape(-1) for v in (b1, g1, be1, b2, g2, be2, b3)])
    if vec.numel() != lib().ver_occ_mlp_vector_floats():
        raise ValueError('occ_mlp vectors: expected 6x128 + 16 floats')
    return vec.contiguous()


# True: on centred rows the forward kernel saves 1/std of both LayerNorms per row (8 B on 288 B of traffic) and the fused
# backward kernel reads them back instead of recomputing the statistics.  False selects the recomputing form of that kernel
# on centred rows too (test_occ_mlp_backward_with_saved_statistics_equals_the_recomputing_kernel compares the two).
_OCC_MLP_SAVE_RSTD = True
# True: the folded MLP's backward is ver_occ_mlp_backward_fused.  False selects the row-split kernel + host GEMM for d(W2),
# the only backward of the unfolded MLP (test_occ_mlp_fused_with_folded_first_linear and
# test_occ_mlp_backward_kernels_on_ragged_sizes run both as each other's second opinion).
_OCC_MLP_BWD_FUSED = True


def occ_mlp_forward(x, image, vectors, eps=1e-5, first_linear=True, centered=False, want_rstd=False):
    """x bf16 [..., 128] -> logits bf16 [..., 16] (ver_occ_mlp_forward).  ``first_linear=False``: x is already the
    output of the first Linear (folded into its producer).  ``centered``: the hidden Linears' weights / biases were
    centred over their output axis (VER_OCC_MLP_CENTERED): the LayerNorms skip the mean pass.  ``want_rstd``: returns
    ``(logits, rstd f32 [N, 2])`` -- 1/std of the two LayerNorms per row, for ver_occ_mlp_backward_fused_stats."""
    x = _gpu(x, 'x')
    if x.dtype != torch.bfloat16 or x.shape[-1] != 128:
        raise TypeError('x must be bf16 [..., 128]')
    x = x.contiguous()
    n = x.numel() // 128
    logits = torch.empty(x.shape[:-1] + (16,), dtype=torch.bfloat16, device=x.device)
    rstd = torch.empty(n, 2, dtype=torch.float32, device=x.device) if want_rstd else None
    _launch('ver_occ_mlp_forward', lambda: lib().ver_occ_mlp_forward_stats(
        _p(x), _p(image), _p(vectors), _p(logits), _p(rstd), n, 128, 16, eps,
        (1 if first_linear else 0) | (2 if centered else 0), _stream()))
    return (logits, rstd) if want_rstd else logits


def _occ_mlp_wants_rstd(folded, centered, n):
    return bool(_OCC_MLP_SAVE_RSTD and _OCC_MLP_BWD_FUSED and folded and centered and n < (1 << 28))


def _occ_mlp_forward_packed(x, w1, b1, g1, be1, w2, b2, g2, be2, w3, b3, eps, centered, save_rstd):
    """Pack the fragment image and the vectors, run the forward (w1 None: folded first Linear) and, where ``save_rstd`` and the
    backward will read them, keep the LayerNorm statistics: ``(image, vec, logits, rstd or None)``."""
    folded = w1 is None
    if folded:
        # (the folded kernels read W2 from W1's image sections: natural k order forward, natural-order output rows
        #  in the dgrad -- the layouts a chain that starts with a LayerNorm on the loaded rows needs)
        w1, b1 = w2, torch.zeros(128, device=x.device)
    image = occ_mlp_pack(w1, w2, w3)
    vec = occ_mlp_vectors(b1, g1, be1, b2, g2, be2, b3)
    has_rstd = save_rstd and _occ_mlp_wants_rstd(folded, centered, x.numel() // 128)
    out = occ_mlp_forward(x, image, vec, eps, first_linear=not folded, centered=centered, want_rstd=has_rstd)
    logits, rstd = out if has_rstd else (out, None)
    return image, vec, logits, rstd


def _occ_mlp_backward_fused(x2, gl, w2, w3, vec, rstd, eps, centered, gscale):
    """ver_occ_mlp_backward_fused_stats on rows x2 [N,128], d(logits) gl [N,16] (times the device scalar ``gscale`` if given):
    d(W2) and every other parameter gradient accumulated in the kernel, no side tensors.  Returns
    ``(gx, vecs [6,128] = d gamma1, d beta1, -, d gamma2, d beta2, d b2, dw2, dw3, db3)``."""
    n = x2.shape[0]
    gx = torch.empty_like(x2)
    pg = torch.empty(6 * 128 + 16 * 128 + 16 + 128 * 128, dtype=torch.float32, device=x2.device)
    # every workgroup's share of the parameter gradients goes to a slab of its own and the slabs are summed in a fixed order
    # (ver_occ_mlp_backward_fused_slabs): two runs on the same inputs give the same bits, which the entries that add with
    # float atomics do not
    slab_bytes = lib().ver_occ_mlp_backward_fused_slab_bytes(n)
    slabs = torch.empty(max(slab_bytes // 4, 1), dtype=torch.float32, device=x2.device)
    _launch('ver_occ_mlp_backward_fused', lambda: lib().ver_occ_mlp_backward_fused_slabs(
        _p(x2), _p(gl), _p(w2.float().contiguous()), _p(w3.float().contiguous()), _p(vec),
        _p(rstd), _p(gx), _p(pg), _p(slabs), slab_bytes, n, 128, 16, eps, _p(gscale), 2 if centered else 0, _stream()))
    vecs = pg[:768].view(6, 128)
    dw3 = pg[768:768 + 2048].view(16, 128)
    db3 = pg[768 + 2048:768 + 2048 + 16]
    dw2 = pg[768 + 2048 + 16:].view(128, 128)
    return gx, vecs, dw2, dw3, db3


def _rows_tn(a, b, chunk=8000):
    """a^T b in fp32 for tall a [N,P], b [N,Q] (N ~ 1e7, P,Q <= 128): the row dimension is split into chunks run as ONE
    batched GEMM (a plain GEMM would own a single output tile and run on one CU)."""
    n = a.shape[0]
    s = n // chunk
    main = s * chunk
    prod = a.new_zeros((a.shape[1], b.shape[1]), dtype=torch.float32)
    if s:
        prod += torch.bmm(a[:main].view(s, chunk, -1).transpose(1, 2), b[:main].view(s, chunk, -1)).sum(0, dtype=torch.float32)
    if main < n:
        prod += (a[main:].t() @ b[main:]).float()
    return prod


_FRAG_ORDER = {}


def _frag_order(device):
    """inverse of the kernels' fragment feature order: inv[feature] = column."""
    key = str(device)
    if key not in _FRAG_ORDER:
        pos = torch.arange(128)
        t, g, j = pos // 32, (pos % 32) // 8, pos % 8
        feat = 32 * t + torch.where(j < 4, 4 * g + j, 16 + 4 * g + j - 4)
        inv = torch.empty(128, dtype=torch.long)
        inv[feat] = pos
        _FRAG_ORDER[key] = inv.to(device)
    return _FRAG_ORDER[key]


class OccMLPFunction(Function):
    """``occ_branches`` (head:241-248) as one fused kernel each way (ver_occ_mlp_*): x bf16 [N,128]
    -> logits bf16 [N,16].  Nothing but x is kept for the backward pass (the chain is re-computed)."""

    @staticmethod
    def forward(ctx, x, w1, b1, g1, be1, w2, b2, g2, be2, w3, b3, eps, centered=False):
        x = _gpu(x, 'x').contiguous()
        # w1 is None: the first Linear was folded into the producer of x (two Linears in a row compose, see
        # VoxelFormerOccupancyHead.occupancy_from_volume); the kernels then run it as the identity and its weight
        # gradient -- a [128, N] x [N, 128] product over all rows -- is not formed here at all
        ctx.folded = w1 is None
        ctx.eps, ctx.centered = eps, bool(centered)
        image, vec, logits, rstd = _occ_mlp_forward_packed(x, w1, b1, g1, be1, w2, b2, g2, be2, w3, b3, eps, centered,
                                                           save_rstd=any(ctx.needs_input_grad))
        ctx.has_rstd = rstd is not None
        ctx.save_for_backward(x, image, vec, w2.detach(), w3.detach(), *((rstd,) if ctx.has_rstd else ()))
        return logits

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_logits):
        x, image, vec, w2, w3 = ctx.saved_tensors[:5]
        rstd = ctx.saved_tensors[5] if ctx.has_rstd else None
        shape = x.shape
        x2 = x.view(-1, 128)
        n = x2.shape[0]
        gl = _gpu(grad_logits, 'grad_logits').to(torch.bfloat16).contiguous().view(n, 16)
        if ctx.folded and _OCC_MLP_BWD_FUSED:
            gx, vecs, dw2, dw3, db3 = _occ_mlp_backward_fused(x2, gl, w2, w3, vec, rstd, ctx.eps, ctx.centered, None)
            return (gx.view(shape), None, None, vecs[0], vecs[1], dw2, vecs[5], vecs[3], vecs[4], dw3, db3, None, None)
        gx, ga2, h1 = (torch.empty_like(x2) for _ in range(3))
        ga1 = None if ctx.folded else torch.empty_like(x2)
        pg = torch.empty(6 * 128 + 16 * 128 + 16, dtype=torch.float32, device=x.device)
        _launch('ver_occ_mlp_backward', lambda: lib().ver_occ_mlp_backward(
            _p(x2), _p(gl), _p(image), _p(vec), _p(gx), _p(ga1), _p(ga2), _p(h1), _p(pg),
            n, 128, 16, ctx.eps, 0 if ctx.folded else 1, _stream()))
        inv = _frag_order(x.device)
        vecs = pg[:768].view(6, 128)
        dw3 = pg[768:768 + 2048].view(16, 128)
        db3 = pg[768 + 2048:]
        dw2 = _rows_tn(ga2, h1)
        if ctx.folded:                               # h1 comes back in natural feature order
            dw2 = dw2.index_select(0, inv)
            return (gx.view(shape), None, None, vecs[0], vecs[1], dw2, vecs[5], vecs[3], vecs[4], dw3, db3, None, None)
        dw2 = dw2.index_select(0, inv).index_select(1, inv)
        dw1 = _rows_tn(ga1, x2)
        dw1 = dw1.index_select(0, inv)
        return (gx.view(shape), dw1, vecs[2], vecs[0], vecs[1], dw2, vecs[5], vecs[3], vecs[4], dw3, db3, None, None)


class OccMLPFocalLossFunction(Function):
    """sum over all elements of the sigmoid focal loss of ``occ_branches(x)`` against integer targets -- the occupancy term
    of a TRAINING step that needs the loss and its gradient, not the logits (folded first Linear, fused bf16 kernels):
    forward = ``ver_occ_mlp_forward`` + ``ver_focal_loss_forward_grad``, which leaves the UNSCALED gradient of the loss sum
    in the logits buffer; backward = ``ver_occ_mlp_backward_fused`` reading that buffer with the incoming scalar as
    ``grad_scale``.  No backward pass of the focal loss over the [N, 16] tensor, no scaled copy of it."""

    @staticmethod
    def forward(ctx, x, g1, be1, w2, b2, g2, be2, w3, b3, target, eps, gamma, alpha, centered, class_weight=None):
        x = _gpu(x, 'x').contiguous()
        _, vec, logits, rstd = _occ_mlp_forward_packed(x, None, None, g1, be1, w2, b2, g2, be2, w3, b3, eps, centered,
                                                       save_rstd=True)
        ctx.has_rstd = rstd is not None
        l2 = logits.view(-1, 16)
        n = l2.shape[0]
        target = _gpu(target, 'target')
        as_bytes = target.dtype == torch.uint8                # (labels the caller has permuted / counted as bytes)
        target = (target if as_bytes else target.to(torch.int64)).contiguous()
        if target.shape != (n,):
            raise ValueError('target must be [N]')
        blocks = lib().ver_focal_loss_blocks(n, 16)
        partial = torch.zeros(blocks, dtype=torch.float32, device=x.device)
        flag = LabelRangeFlag.of(x.device)
        flag.poll()
        if class_weight is None:
            entry = lib().ver_focal_loss_forward_grad_u8 if as_bytes else lib().ver_focal_loss_forward_grad
            _launch('ver_focal_loss_forward_grad', lambda: entry(
                _p(l2), _p(target), _p(partial), _p(l2), n, 16, gamma, alpha, 1, _p(flag.dev), _stream()))                  # (in place: the logits buffer now holds d loss / d logits)
        else:                                                 # ... times the row's class weight: the MLP backward is the same
            table = _class_weight_table(class_weight, 16, x.device)
            entry = lib().ver_focal_loss_forward_grad_u8_cw if as_bytes else lib().ver_focal_loss_forward_grad_cw
            _launch('ver_focal_loss_forward_grad_cw', lambda: entry(
                _p(l2), _p(target), _p(table), _p(partial), _p(l2), n, 16, gamma, alpha, 1, _p(flag.dev), _stream()))
        flag.mirror(16)
        ctx.save_for_backward(x, vec, w2.detach(), w3.detach(), l2, *((rstd,) if ctx.has_rstd else ()))
        ctx.eps, ctx.centered = eps, bool(centered)
        return partial.sum()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, vec, w2, w3, gl = ctx.saved_tensors[:5]
        rstd = ctx.saved_tensors[5] if ctx.has_rstd else None
        gscale = _gpu(grad_out, 'grad_out').float().reshape(1).contiguous()
        gx, vecs, dw2, dw3, db3 = _occ_mlp_backward_fused(x.view(-1, 128), gl, w2, w3, vec, rstd, ctx.eps, ctx.centered, gscale)
        return (gx.view(x.shape), vecs[0], vecs[1], dw2, vecs[5], vecs[3], vecs[4], dw3, db3, None, None, None, None, None, None)


def occ_mlp_focal_loss_sum(x, g1, be1, w2, b2, g2, be2, w3, b3, target, eps=1e-5, gamma=2.0, alpha=0.25, centered=False,
                           class_weight=None):
    return OccMLPFocalLossFunction.apply(x, g1, be1, w2, b2, g2, be2, w3, b3, target, eps, float(gamma), float(alpha), centered,
                                         class_weight)


def occ_mlp(x, w1, b1, g1, be1, w2, b2, g2, be2, w3, b3, eps=1e-5, centered=False):
    """``centered``: the caller passes hidden Linears whose weights / biases are centred over the output axis (and, with
    w1 None, has centred the folded first Linear in the producer of x): the forward LayerNorms skip the mean pass."""
    return OccMLPFunction.apply(x, w1, b1, g1, be1, w2, b2, g2, be2, w3, b3, eps, centered)


# ------------------------------------------------------------------------------------------
class AddDropoutLayerNormFunction(Function):
    """y = LayerNorm(residual + dropout(a)) as one pass each way (ver_add_ln_*): the tail of both branches of an
    encoder layer.  Returns (y fp32, y_bf16 or None): the bf16 copy is what the next Linear reads under autocast."""

    @staticmethod
    def forward(ctx, a, residual, gamma, beta, p_drop, eps, want_bf16):
        a = _gpu(a, 'a')
        if a.dtype not in (torch.float32, torch.bfloat16):
            a = a.float()
        a = a.contiguous()
        res = _gpu(residual, 'residual').float().contiguous()
        C = a.shape[-1]
        n = a.numel() // C
        y = torch.empty_like(res)
        y16 = torch.empty(res.shape, dtype=torch.bfloat16, device=res.device) if want_bf16 else None
        mean = torch.empty(n, dtype=torch.float32, device=res.device)
        rstd = torch.empty_like(mean)
        seed = torch.randint(0, 2 ** 62, (1,), device=res.device, dtype=torch.int64) if p_drop > 0 else None
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        _launch('ver_add_ln_forward', lambda: lib().ver_add_ln_forward(
            _p(a), 1 if a.dtype == torch.bfloat16 else 0, _p(res), _p(g), _p(b), _p(seed), p_drop, eps, _p(y), _p(y16),
            _p(mean), _p(rstd), n, C, _stream()))
        ctx.save_for_backward(a, res, g, mean, rstd, seed if seed is not None else torch.empty(0, device=res.device))
        ctx.p_drop, ctx.has_y16 = p_drop, want_bf16
        if want_bf16:
            return y, y16
        return y, None

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y, grad_y16):
        a, res, g, mean, rstd, seed = ctx.saved_tensors
        C = a.shape[-1]
        n = a.numel() // C
        gy = (torch.zeros_like(res) if grad_y is None else _gpu(grad_y, 'grad_y').float().contiguous())
        gy16 = None
        if ctx.has_y16 and grad_y16 is not None:
            gy16 = _gpu(grad_y16, 'grad_y_bf16').to(torch.bfloat16).contiguous()
        d_a = torch.empty_like(a)
        d_res = torch.empty_like(res)
        dg = torch.empty(C, dtype=torch.float32, device=res.device)
        db = torch.empty_like(dg)
        _launch('ver_add_ln_backward', lambda: lib().ver_add_ln_backward(
            _p(gy), _p(gy16), _p(a), 1 if a.dtype == torch.bfloat16 else 0, _p(res), _p(g), _p(mean), _p(rstd),
            _p(seed) if ctx.p_drop > 0 else None, ctx.p_drop, _p(d_a), _p(d_res), _p(dg), _p(db), n, C, _stream()))
        return d_a, d_res, dg, db, None, None, None


class ReluDropoutFunction(Function):
    """y = dropout(relu(x)) in one pass (ver_relu_dropout_*); the backward pass needs y only."""

    @staticmethod
    def forward(ctx, x, p_drop):
        x = _gpu(x, 'x')
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        x = x.contiguous()
        y = torch.empty_like(x)
        seed = torch.randint(0, 2 ** 62, (1,), device=x.device, dtype=torch.int64) if p_drop > 0 else None
        _launch('ver_relu_dropout_forward', lambda: lib().ver_relu_dropout_forward(
            _p(x), _p(y), _p(seed), p_drop, x.numel(), 1 if x.dtype == torch.bfloat16 else 0, _stream()))
        ctx.save_for_backward(y)
        ctx.p_drop = p_drop
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        y, = ctx.saved_tensors
        gy = _gpu(grad_y, 'grad_y').to(y.dtype).contiguous()
        gx = torch.empty_like(y)
        _launch('ver_relu_dropout_backward', lambda: lib().ver_relu_dropout_backward(
            _p(y), _p(gy), _p(gx), ctx.p_drop, y.numel(), 1 if y.dtype == torch.bfloat16 else 0, _stream()))
        return gx, None


def relu_dropout(x, p_drop=0.0):
    """dropout(relu(x)), x fp32 or bf16 with a multiple of 4 elements."""
    return ReluDropoutFunction.apply(x, float(p_drop))


def add_dropout_layer_norm(a, residual, gamma, beta, p_drop=0.0, eps=1e-5, want_bf16=False):
    """(y fp32, y_bf16 | None) = LayerNorm(residual + dropout(a)); C = a.shape[-1] in {256, 512, 768, 1024}."""
    return AddDropoutLayerNormFunction.apply(a, residual, gamma, beta, float(p_drop), float(eps), bool(want_bf16))


# ------------------------------------------------------------------------------------------
class VoxelMSDeformAttnFunction(Function):
    """3-D (trilinear) deformable sampling of the detection decoder
    (voxel_temporal_self_attention.py:275-335) on ver_msda3d_forward / _backward."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, level_start_index, sampling_locations, attention_weights):
        value = _gpu(value, 'value').float().contiguous()
        loc = _gpu(sampling_locations, 'sampling_locations').float().contiguous()
        aw = _gpu(attention_weights, 'attention_weights').float().contiguous()
        shapes = _gpu(spatial_shapes, 'spatial_shapes').to(torch.int64).contiguous()
        lsi = _gpu(level_start_index, 'level_start_index').to(torch.int64).contiguous()
        bs, nk, heads, hd = value.shape
        _, nq, _, nl, npt, _ = loc.shape
        out = value.new_empty(bs, nq, heads * hd)
        _launch('ver_msda3d_forward', lambda: lib().ver_msda3d_forward(
            _p(value), _p(shapes), _p(lsi), _p(loc), _p(aw), _p(out), bs, nk, heads, hd, nl, npt, nq, _stream()))
        ctx.save_for_backward(value, shapes, lsi, loc, aw)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        value, shapes, lsi, loc, aw = ctx.saved_tensors
        bs, nk, heads, hd = value.shape
        _, nq, _, nl, npt, _ = loc.shape
        gv, gl, ga = torch.zeros_like(value), torch.zeros_like(loc), torch.zeros_like(aw)
        go = _gpu(grad_output, 'grad_output').float().contiguous()
        _launch('ver_msda3d_backward', lambda: lib().ver_msda3d_backward(
            _p(value), _p(shapes), _p(lsi), _p(loc), _p(aw), _p(go), _p(gv), _p(gl), _p(ga), bs, nk, heads,
            hd, nl, npt, nq, _stream()))
        return gv, None, None, gl, ga


def voxel_msda(value, spatial_shapes, level_start_index, sampling_locations, attention_weights):
    return VoxelMSDeformAttnFunction.apply(value, spatial_shapes, level_start_index, sampling_locations,
                                           attention_weights)


def _lowp(t, name):
    """fp32 and bf16 operands go to the kernels as they are; anything else is widened to fp32."""
    t = _gpu(t, name)
    return t if t.dtype in (torch.float32, torch.bfloat16) else t.float()


def voxel_deform_attn_supported(bs, num_keys, heads, head_dim, levels, points, num_query):
    """Whether ver_dattn3d_* take the shape (the range is stated in include/ver_ops.h); no device call."""
    return bool(lib().ver_dattn3d_supported(bs, num_keys, heads, head_dim, levels, points, num_query))


class VoxelDeformAttnFunction(Function):
    """The detection decoder's 3-D deformable attention from the raw Linear outputs (ver_dattn3d_forward / _backward):
    softmax over the points, loc = ref + offsets / (W, H, D) and the trilinear sampling in one launch, the backward in two,
    with every gradient written in full (no zero fills) and a reproducible grad_value."""

    @staticmethod
    def forward(ctx, value, spatial_shapes, level_start_index, reference_points, offsets, logits, out_dtype=None):
        value = _lowp(value, 'value')
        offsets = _lowp(offsets, 'offsets')
        logits = _lowp(logits, 'logits')
        if logits.dtype != offsets.dtype:
            logits = logits.to(offsets.dtype)
        ref = _gpu(reference_points, 'reference_points').float().contiguous()
        shapes = _gpu(spatial_shapes, 'spatial_shapes').to(torch.int64).contiguous()
        lsi = _gpu(level_start_index, 'level_start_index').to(torch.int64).contiguous()
        bs, nk, heads, hd = value.shape
        _, nq, _, nl, npt, _ = offsets.shape
        assert logits.shape == (bs, nq, heads, nl * npt) and ref.shape == (bs, nq, nl, 3)
        vdt = 1 if value.dtype == torch.bfloat16 else 0
        qdt = 1 if offsets.dtype == torch.bfloat16 else 0
        out_dtype = out_dtype or value.dtype
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise TypeError('out_dtype must be torch.float32 or torch.bfloat16, got %s' % out_dtype)
        odt = 1 if out_dtype == torch.bfloat16 else 0
        out = torch.empty(bs, nq, heads * hd, dtype=out_dtype, device=value.device)
        _launch('ver_dattn3d_forward', lambda: lib().ver_dattn3d_forward(
            _p(value), vdt, _p(shapes), _p(lsi), _p(ref), _p(offsets), _p(logits), qdt, _p(out), odt, bs, nk, heads, hd, nl,
            npt, nq, _stream()))
        ctx.save_for_backward(value, shapes, lsi, ref, offsets, logits)
        ctx.ref_like = (reference_points.shape, reference_points.dtype)
        ctx.out_dtype = out_dtype
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        value, shapes, lsi, ref, offsets, logits = ctx.saved_tensors
        bs, nk, heads, hd = value.shape
        _, nq, _, nl, npt, _ = offsets.shape
        vdt = 1 if value.dtype == torch.bfloat16 else 0
        qdt = 1 if offsets.dtype == torch.bfloat16 else 0
        odt = 1 if ctx.out_dtype == torch.bfloat16 else 0
        go = _gpu(grad_output, 'grad_output').to(ctx.out_dtype).contiguous()
        # (an empty query set launches nothing: only then is there something to clear)
        gv = torch.empty_like(value) if bs * nq else torch.zeros_like(value)
        goff, glog = torch.empty_like(offsets), torch.empty_like(logits)
        gref = torch.empty_like(ref) if ctx.needs_input_grad[3] else None
        _launch('ver_dattn3d_backward', lambda: lib().ver_dattn3d_backward(
            _p(value), vdt, _p(shapes), _p(lsi), _p(ref), _p(offsets), _p(logits), qdt, _p(go), odt, _p(gv), _p(goff),
            _p(glog), _p(gref), bs, nk, heads, hd, nl, npt, nq, _stream()))
        shape, dtype = ctx.ref_like
        return gv, None, None, None if gref is None else gref.view(shape).to(dtype), goff, glog, None


def voxel_deform_attn(value, spatial_shapes, level_start_index, reference_points, offsets, logits, out_dtype=None):
    """value f32|bf16 [bs,Nk,heads,hd] (value_proj's output), reference_points [bs,Nq,L,3] in [0,1], offsets f32|bf16
    [bs,Nq,heads,L,P,3] and logits [bs,Nq,heads,L*P] (the raw outputs of sampling_offsets / attention_weights) ->
    [bs,Nq,heads*hd] in ``out_dtype`` (fp32 | bf16; None: value's).  bf16 operands are passed through; a shape outside the
    library's range raises with its message."""
    return VoxelDeformAttnFunction.apply(value, spatial_shapes, level_start_index, reference_points, offsets, logits,
                                         out_dtype)


# ------------------------------------------------------------------------------------------
def mha_supported(B, heads, head_dim, Nq, Nk):
    """Whether ver_mha_* take the shape (the range is stated in include/ver_ops.h); no device call."""
    return bool(lib().ver_mha_supported(B, heads, head_dim, Nq, Nk))


def dropout_keep_host(indices, seed, p_drop):
    """The kernels' dropout keep rule (csrc/ver_common.h keep_elem) in numpy: bool array, True where the element with flat
    index ``indices`` is kept under ``seed``.  uint64 wrap-around arithmetic; the threshold is computed in float32, as the
    kernels compute it."""
    import numpy as np
    idx = np.asarray(indices).astype(np.uint64)
    with np.errstate(over='ignore'):
        h = idx * np.uint64(0x9E3779B97F4A7C15) + np.uint64(int(seed) & (2 ** 64 - 1))
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xc4ceb9fe1a85ec53)
        h ^= h >> np.uint64(33)
    thresh = np.uint64(int((np.float32(1.0) - np.float32(p_drop)) * np.float32(16777216.0)))
    return (h & np.uint64(0xffffff)) < thresh


def pack_host(grad, scale, wire_dtype=torch.float32):
    """``ver_grad_pack``'s arithmetic on one gradient in numpy (csrc/ver_optim.hip bf16_round): the fp32 product
    ``grad * scale``; for a bf16 wire rounded once to nearest-even on the bit pattern -- a NaN becomes the quiet NaN
    0x7fc0, +-inf stay, a finite product past the largest bf16 rounds to +-inf.  -> float32 array (fp32 wire) or the
    uint16 bit patterns (bf16 wire), flat."""
    import numpy as np
    g = np.ascontiguousarray(np.asarray(grad, dtype=np.float32)).reshape(-1)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        prod = (g * np.float32(scale)).astype(np.float32)
    if wire_dtype == torch.float32:
        return prod
    if wire_dtype != torch.bfloat16:
        raise TypeError('pack_host: wire dtype float32 or bfloat16, got %s' % (wire_dtype,))
    u = prod.view(np.uint32).astype(np.uint64)
    rounded = ((u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    return np.where((u & np.uint64(0x7fffffff)) > np.uint64(0x7f800000), np.uint16(0x7fc0), rounded)


def _row_pitch(t):
    """(t or a contiguous copy of it, elements between consecutive rows of its flattened leading dimensions): a [N, B, C]
    view with last-dimension stride 1 and a uniform row pitch (a column slice of a wider GEMM output) goes as it is."""
    _, b, c = t.shape
    ld = t.stride(0) if b == 1 else t.stride(1)
    if (t.stride(2) == 1 and (b == 1 or t.stride(0) == b * ld) and ld >= c and ld % 8 == 0
            and t.data_ptr() % 16 == 0):
        return t, ld
    return t.contiguous(), c


def _mha_operand(t, name):
    """A GPU tensor in fp32 or bf16 (anything else is widened to fp32); unlike ``_gpu`` it leaves a strided view alone."""
    if not t.is_cuda:
        raise RuntimeError('%s must be a GPU tensor: the VER ops only exist as HIP kernels' % name)
    return t if t.dtype in (torch.float32, torch.bfloat16) else t.float()


class MultiheadAttentionCoreFunction(Function):
    """Softmax attention between the input projections and out_proj (ver_mha_forward / _backward): q [Nq, B, C], k, v
    [Nk, B, C] in the layout the Linears leave them in -> [Nq, B, C].  One launch each way; the backward recomputes the
    probabilities and the dropout decisions from q, k, the saved row log-sum-exp and the seed.  ``k`` None: ``q`` is the
    [N, B, 2C] output of ONE Linear whose column halves are q and k; the kernels read them in place and write grad_q and
    grad_k as the halves of one gradient for it."""

    @staticmethod
    def forward(ctx, q, k, v, heads, p_drop):
        joint = k is None
        q, v = _mha_operand(q, 'q'), _mha_operand(v, 'v')
        if joint:
            qk = q.contiguous()
            c = qk.shape[-1] // 2
            q, k = qk[..., :c], qk[..., c:]
        else:
            k = _mha_operand(k, 'k').to(q.dtype)
        v = v.to(q.dtype)
        nq, bs, c = q.shape
        nk = k.shape[0]
        assert k.shape == (nk, bs, c) and v.shape == (nk, bs, c) and c % heads == 0
        (q, ldq), (k, ldk), (v, ldv) = _row_pitch(q), _row_pitch(k), _row_pitch(v)
        out = torch.empty(nq, bs, c, dtype=q.dtype, device=q.device)
        lse = torch.empty(bs, heads, nq, dtype=torch.float32, device=q.device)
        seed = torch.randint(0, 2 ** 62, (1,), device=q.device, dtype=torch.int64) if p_drop > 0 else None
        dt = 1 if q.dtype == torch.bfloat16 else 0
        _launch('ver_mha_forward', lambda: lib().ver_mha_forward(
            _p(q), _p(k), _p(v), dt, ldq, ldk, ldv, _p(seed), p_drop, _p(out), _p(lse), bs, heads, c // heads, nq, nk,
            _stream()))
        saved = (qk, v) if joint else (q, k, v)
        ctx.save_for_backward(*saved, lse, seed if seed is not None else torch.empty(0, device=q.device))
        ctx.heads, ctx.p_drop, ctx.joint = heads, p_drop, joint
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        # (an empty query set launches nothing: only then is there something to clear)
        if ctx.joint:
            qk, v, lse, seed = ctx.saved_tensors
            c = qk.shape[-1] // 2
            q, k = qk[..., :c], qk[..., c:]
            gqk = torch.empty_like(qk)
            gq, gk = gqk[..., :c], gqk[..., c:]
        else:
            q, k, v, lse, seed = ctx.saved_tensors
            new = torch.empty if q.numel() else torch.zeros
            gq, gk = new(q.shape, dtype=q.dtype, device=q.device), new(k.shape, dtype=q.dtype, device=q.device)
        nq, bs, c = q.shape
        nk = k.shape[0]
        (q, ldq), (k, ldk), (v, ldv) = _row_pitch(q), _row_pitch(k), _row_pitch(v)      # (copies were made in forward)
        go = _gpu(grad_out, 'grad_out').to(q.dtype).contiguous()
        gv = (torch.empty if q.numel() else torch.zeros)(nk, bs, c, dtype=q.dtype, device=q.device)
        ldg = 2 * c if ctx.joint else c
        _launch('ver_mha_backward', lambda: lib().ver_mha_backward(
            _p(q), _p(k), _p(v), 1 if q.dtype == torch.bfloat16 else 0, ldq, ldk, ldv, _p(go), _p(lse),
            _p(seed) if ctx.p_drop > 0 else None, ctx.p_drop, _p(gq), _p(gk), _p(gv), ldg, ldg, c, bs, ctx.heads,
            c // ctx.heads, nq, nk, _stream()))
        if ctx.joint:
            return gqk, None, gv, None, None
        return gq, gk, gv, None, None


def mha_core(q, k, v, heads, p_drop=0.0):
    """softmax(q k^T / sqrt(head_dim)) (with dropout ``p_drop`` on the probabilities) times v, per head: q [Nq, B, C], k and v
    [Nk, B, C], fp32 or bf16 -> [Nq, B, C] in q's dtype.  Views with a last-dimension stride of 1 and a uniform row pitch
    (the column halves of one [N, B, 2C] Linear output) are read in place, anything else is made contiguous.  A shape
    outside the library's range raises with its message."""
    return MultiheadAttentionCoreFunction.apply(q, k, v, int(heads), float(p_drop))


def mha_core_joint(qk, v, heads, p_drop=0.0):
    """``mha_core(qk[..., :C], qk[..., C:], v, heads, p_drop)`` for the [N, B, 2C] output of one Linear, with grad_q and grad_k
    written as the halves of ONE gradient for ``qk`` (autograd would otherwise pad each half's gradient to the full width
    and add the two)."""
    return MultiheadAttentionCoreFunction.apply(qk, None, v, int(heads), float(p_drop))


# ------------------------------------------------------------------------------------------
def occ_predict(logits, threshold=0.25):
    """Sparse occupancy prediction (ver_occ_predict; head:1505-1540): logits fp32|bf16 [N, C] ->
    int64 [K, 2] pairs (row index, class) of the rows whose best class probability reaches ``threshold``,
    in ascending row order.  One device->host read of K, as the reference's ``torch.where``."""
    logits = _gpu(logits, 'logits')
    if logits.dtype not in (torch.float32, torch.bfloat16):
        logits = logits.float()
    logits = logits.contiguous()
    n, c = logits.shape
    dt = 1 if logits.dtype == torch.bfloat16 else 0
    nb = lib().ver_occ_predict_blocks(n)
    work = torch.empty(max(nb, 1), dtype=torch.int32, device=logits.device)
    pairs = torch.empty(max(n, 1), 2, dtype=torch.int64, device=logits.device)
    count = torch.empty(1, dtype=torch.int64, device=logits.device)
    _launch('ver_occ_predict', lambda: lib().ver_occ_predict(
        _p(logits), dt, n, c, threshold, _p(work), _p(pairs), _p(count), _stream()))
    return pairs[:int(count.item())]


def occ_predict_classes(logits, threshold=0.25):
    """The class byte of every row under ``occ_predict``'s rule -- the same kernels, so the same decisions bit for bit --
    WITHOUT the host read of the pair count: logits fp32|bf16 [..., C] -> uint8 [...], ``C`` = empty.  The compaction's
    (row, class) pairs are scattered back into a dense map; the slots at and past the device-side count are steered to a
    spare element by integer masking.  Launches only: capturable."""
    logits = _gpu(logits, 'logits')
    if logits.dtype not in (torch.float32, torch.bfloat16):
        logits = logits.float()
    lead, c = logits.shape[:-1], logits.shape[-1]
    logits = logits.reshape(-1, c).contiguous()
    n = logits.shape[0]
    cls = torch.full((n + 1,), c, dtype=torch.uint8, device=logits.device)
    if n == 0:
        return cls[:0].view(lead)
    dt = 1 if logits.dtype == torch.bfloat16 else 0
    work = torch.empty(lib().ver_occ_predict_blocks(n), dtype=torch.int32, device=logits.device)
    pairs = torch.empty(n, 2, dtype=torch.int64, device=logits.device)
    count = torch.empty(1, dtype=torch.int64, device=logits.device)
    _launch('ver_occ_predict', lambda: lib().ver_occ_predict(
        _p(logits), dt, n, c, threshold, _p(work), _p(pairs), _p(count), _stream()))
    live = (torch.arange(n, device=logits.device) < count).to(torch.int64)      # 1 for the pairs the kernel wrote
    row = pairs[:, 0] * live + (1 - live) * n                                   # (an unwritten slot holds anything: times 0)
    cls.scatter_(0, row, (pairs[:, 1] * live).to(torch.uint8))
    return cls[:n].view(lead)


def occ_confusion(logits, labels, thresholds=(0.25,), samples=1, hist=None):
    """Occupancy confusion matrix (ver_occ_confusion; the histogram of the reference's ``SSCMetrics.add_batch``):
    logits fp32|bf16 [samples * rows, C] (any leading shape), labels u8 with one entry per logit row in the same order
    (``>= C + 1``: ignored) -> int64 hist [samples, T, C + 1, C + 1] (row = label, column = prediction, column C =
    empty) for the T ``thresholds``.  ``hist``: an int64 buffer of that shape to ACCUMULATE into (a fresh zeroed one
    otherwise).  No host synchronisation."""
    logits = _gpu(logits, 'logits')
    if logits.dtype not in (torch.float32, torch.bfloat16):
        logits = logits.float()
    c = logits.shape[-1]
    logits = logits.reshape(-1, c).contiguous()
    labels = _gpu(labels, 'labels', torch.uint8).reshape(-1)
    n = logits.shape[0]
    if labels.numel() != n:
        raise ValueError('occ_confusion: %d labels for %d logit rows' % (labels.numel(), n))
    if samples < 1 or n % samples:
        raise ValueError('occ_confusion: %d rows do not split into %d samples' % (n, samples))
    thr = [float(t) for t in thresholds]
    k = c + 1
    shape = (samples, len(thr), k, k)
    if hist is None:
        hist = torch.zeros(shape, dtype=torch.int64, device=logits.device)
    elif (tuple(hist.shape) != shape or hist.dtype != torch.int64 or not hist.is_contiguous()
          or hist.device != logits.device):
        raise ValueError('occ_confusion: hist must be a contiguous int64 %s tensor on %s' % (shape, logits.device))
    dt = 1 if logits.dtype == torch.bfloat16 else 0
    host_thr = (ctypes.c_float * max(len(thr), 1))(*thr)
    _launch('ver_occ_confusion', lambda: lib().ver_occ_confusion(
        _p(logits), dt, n // samples, samples, c, _p(labels), host_thr, len(thr), _p(hist), _stream()))
    return hist


def _occ_mlp_eval_args(who, x, image, vectors):
    """Checked inputs of the classifying forward launches: x bf16 [N, 128] contiguous; inference only."""
    x = _gpu(x, 'x')
    if x.dtype != torch.bfloat16 or x.shape[-1] != 128:
        raise TypeError('x must be bf16 [..., 128]')
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, image, vectors)):
        raise RuntimeError('%s has no backward pass: call it under torch.no_grad()' % who)
    return x.contiguous().view(-1, 128)


def occ_mlp_confusion(x, image, vectors, labels, thresholds=(0.25,), samples=1, hist=None, eps=1e-5, first_linear=True,
                      centered=False):
    """``occ_confusion(occ_mlp_forward(x, image, vectors, ...), labels, thresholds, samples, hist)`` in ONE launch that
    writes no logits (ver_occ_mlp_confusion): x bf16 [samples * rows, 128], labels u8 one per row -> int64 hist
    [samples, T, 17, 17], accumulated into ``hist`` when given.  Exactly the counts of the two-kernel pair.  ``no_grad`` only."""
    x = _occ_mlp_eval_args('occ_mlp_confusion', x, image, vectors)
    n = x.shape[0]
    labels = _gpu(labels, 'labels', torch.uint8).reshape(-1).contiguous()
    if labels.numel() != n:
        raise ValueError('occ_mlp_confusion: %d labels for %d rows' % (labels.numel(), n))
    if samples < 1 or n % samples:
        raise ValueError('occ_mlp_confusion: %d rows do not split into %d samples' % (n, samples))
    thr = [float(t) for t in thresholds]
    shape = (samples, len(thr), 17, 17)
    if hist is None:
        hist = torch.zeros(shape, dtype=torch.int64, device=x.device)
    elif (tuple(hist.shape) != shape or hist.dtype != torch.int64 or not hist.is_contiguous() or hist.device != x.device):
        raise ValueError('occ_mlp_confusion: hist must be a contiguous int64 %s tensor on %s' % (shape, x.device))
    host_thr = (ctypes.c_float * max(len(thr), 1))(*thr)
    _launch('ver_occ_mlp_confusion', lambda: lib().ver_occ_mlp_confusion(
        _p(x), _p(image), _p(vectors), _p(labels), n // samples, samples, host_thr, len(thr), _p(hist), 128, 16, eps,
        (1 if first_linear else 0) | (2 if centered else 0), _stream()))
    return hist


def occ_mlp_classes(x, image, vectors, threshold=0.25, want_prob=False, eps=1e-5, first_linear=True, centered=False):
    """The class of every row without its logits (ver_occ_mlp_classes): x bf16 [..., 128] -> uint8 [...]: the class
    ``occ_predict(occ_mlp_forward(x, ...), threshold)`` pairs with the row, 16 for an empty one.  ``want_prob``: returns
    ``(classes, prob f32 [...])``, the fp32 sigmoid of the best class.  ``no_grad`` only."""
    lead = x.shape[:-1]
    x = _occ_mlp_eval_args('occ_mlp_classes', x, image, vectors)
    n = x.shape[0]
    cls = torch.empty(n, dtype=torch.uint8, device=x.device)
    prob = torch.empty(n, dtype=torch.float32, device=x.device) if want_prob else None
    _launch('ver_occ_mlp_classes', lambda: lib().ver_occ_mlp_classes(
        _p(x), _p(image), _p(vectors), _p(cls), _p(prob), n, float(threshold), 128, 16, eps,
        (1 if first_linear else 0) | (2 if centered else 0), _stream()))
    cls = cls.view(lead)
    return (cls, prob.view(lead)) if want_prob else cls


# ------------------------------------------------------------------------------------------
LSA_MAX = 1024            # ver_lsa_solve: rows and column capacity of a problem


def lsa_solve(cost, ncols, match=None, bad=None):
    """Batched rectangular linear sum assignment (ver_lsa_solve; ``scipy.optimize.linear_sum_assignment`` on
    ``cost[p, :, :ncols[p]]`` for every problem p): cost fp32 [..., R, Ccap], ncols int32 with one entry per problem ->
    int32 match [..., R], the column assigned to each row or -1.  ``match``: a contiguous int32 buffer of that shape to
    write into; ``bad``: an int32 device scalar that gets 1 ORed in when a problem could not be solved (NaN / -inf, no
    finite assignment; never cleared here).  One launch, no allocation besides ``match``, no host synchronisation."""
    cost = _gpu(cost, 'cost', torch.float32)
    if cost.dim() < 2:
        raise ValueError('lsa_solve: cost must be [..., R, Ccap]')
    r, ccap = cost.shape[-2:]
    lead = tuple(cost.shape[:-2])
    n = 1
    for d in lead:
        n *= d
    ncols = _gpu(ncols, 'ncols', torch.int32).reshape(-1)
    if ncols.numel() != n:
        raise ValueError('lsa_solve: %d column counts for %d problems' % (ncols.numel(), n))
    if match is None:
        match = torch.empty(lead + (r,), dtype=torch.int32, device=cost.device)
    elif (tuple(match.shape) != lead + (r,) or match.dtype != torch.int32 or not match.is_contiguous()
          or match.device != cost.device):
        raise ValueError('lsa_solve: match must be a contiguous int32 %s tensor on %s' % (lead + (r,), cost.device))
    if bad is not None and (bad.numel() != 1 or bad.dtype != torch.int32 or bad.device != cost.device):
        raise ValueError('lsa_solve: bad must be one int32 on %s' % (cost.device,))
    if r == 0:
        return match
    _launch('ver_lsa_solve', lambda: lib().ver_lsa_solve(_p(cost), _p(ncols), _p(match), _p(bad), n, r, ccap, _stream()))
    return match


# ------------------------------------------------------------------------------------------
SET_LOSS_MAX_CLASSES = 64     # ver_det_costs / ver_det_set_loss_*: C (Q and Gcap: LSA_MAX)


def _set_loss_operands(what, all_cls, all_box, gts, min_ld):
    """The operands the three set-loss entry points share, checked: (cls | None, dtype code, box, boxes, labels, counts,
    (L, B, Q, C, Gcap, box_ld))."""
    gt_boxes, gt_labels, counts = gts
    box = _gpu(all_box, 'all_box', torch.float32)
    if box.dim() != 4 or box.shape[-1] < min_ld:
        raise ValueError('%s: all_box must be [L, B, Q, >= %d], got %s' % (what, min_ld, tuple(box.shape)))
    nl, bs, nq, ld = box.shape
    dev = box.device
    gt_boxes = _gpu(gt_boxes, 'gts.boxes', torch.float32)
    if gt_boxes.dim() != 3 or gt_boxes.shape[0] != bs or gt_boxes.shape[2] != 9 or gt_boxes.device != dev:
        raise ValueError('%s: gts.boxes must be [%d, Gcap, 9] on %s, got %s' % (what, bs, dev, tuple(gt_boxes.shape)))
    cap = gt_boxes.shape[1]
    counts = _counts(counts, 'gts.counts', what, bs, dev)
    if counts is None:
        raise ValueError('%s: gts.counts is required' % what)
    ncls, code = 0, 0
    if all_cls is not None:
        all_cls = _gpu(all_cls, 'all_cls')
        if all_cls.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError('%s: all_cls must be float32 or bfloat16, got %s' % (what, all_cls.dtype))
        if all_cls.dim() != 4 or tuple(all_cls.shape[:3]) != (nl, bs, nq) or all_cls.device != dev:
            raise ValueError('%s: all_cls must be [%d, %d, %d, C] on %s, got %s' % (what, nl, bs, nq, dev, tuple(all_cls.shape)))
        ncls, code = all_cls.shape[3], 1 if all_cls.dtype == torch.bfloat16 else 0
        gt_labels = _gpu(gt_labels, 'gts.labels', torch.int64)
        if tuple(gt_labels.shape) != (bs, cap) or gt_labels.device != dev:
            raise ValueError('%s: gts.labels must be int64 [%d, %d] on %s' % (what, bs, cap, dev))
    else:
        gt_labels = None
    if nq > LSA_MAX or cap > LSA_MAX or ncls > SET_LOSS_MAX_CLASSES:
        raise ValueError('%s: Q=%d Gcap=%d C=%d (at most %d, %d, %d)' % (what, nq, cap, ncls, LSA_MAX, LSA_MAX, SET_LOSS_MAX_CLASSES))
    return all_cls, code, box, gt_boxes, gt_labels, counts, (nl, bs, nq, ncls, cap, ld)


def det_costs(all_cls, all_box, gts, w_cls=1.0, alpha=0.25, gamma=2.0, eps=1e-12, w_reg=1.0):
    """Matching costs of every (decoder layer, sample) in one launch (ver_det_costs): all_cls fp32 | bf16 [L, B, Q, C] logits
    or None (the room-layout form: regression cost alone), all_box fp32 [L, B, Q, >= 8] box codes, gts = (boxes fp32
    [B, Gcap, 9], labels int64 [B, Gcap], counts int32 [B]) as ``PaddedGts`` holds them -> cost fp32 [L, B, Q, Gcap]:
    ``FocalLossCost`` (w_cls, alpha, gamma, eps) + ``BBox3DL1Cost`` (w_reg) on the normalised box, 0 in the columns past a
    sample's count, NaN where a valid label lies outside [0, C).  No allocation besides ``cost``, no host synchronisation."""
    if all_cls is not None and all_cls.dtype not in (torch.float32, torch.bfloat16):
        all_cls = all_cls.float()
    cls, code, box, gt_boxes, gt_labels, counts, (nl, bs, nq, ncls, cap, ld) = _set_loss_operands('det_costs', all_cls, all_box.float(), gts, 8)
    cost = torch.empty(nl, bs, nq, cap, dtype=torch.float32, device=box.device)
    if cost.numel():
        _launch('ver_det_costs', lambda: lib().ver_det_costs(
            _p(cls), code, _p(box), ld, _p(gt_boxes), _p(gt_labels), _p(counts), _p(cost), nl, bs, nq, ncls, cap,
            float(w_cls), float(alpha), float(gamma), float(eps), float(w_reg), _stream()))
    return cost


def _set_loss_forward(all_cls, all_box, match, gts, code_weights, alpha, gamma, bad):
    """Launch ver_det_set_loss_forward -> (sums fp32 [2, L], npos int32 [L], the checked operands for the backward)."""
    what = 'det_set_loss'
    cls, code, box, gt_boxes, gt_labels, counts, dims = _set_loss_operands(what, all_cls, all_box, gts, 10)
    nl, bs, nq, ncls, cap, ld = dims
    dev = box.device
    match = _gpu(match, 'match', torch.int32)
    if tuple(match.shape) != (nl, bs, nq) or match.device != dev:
        raise ValueError('%s: match must be int32 [%d, %d, %d] on %s' % (what, nl, bs, nq, dev))
    code_weights = _gpu(code_weights.detach(), 'code_weights', torch.float32)
    if code_weights.numel() < 10 or code_weights.device != dev:
        raise ValueError('%s: code_weights must hold ten fp32 weights on %s' % (what, dev))
    if bad is not None and (bad.numel() != 1 or bad.dtype != torch.int32 or bad.device != dev):
        raise ValueError('%s: bad must be one int32 on %s' % (what, dev))
    sums = torch.empty(2, nl, dtype=torch.float32, device=dev)
    npos = torch.empty(nl, dtype=torch.int32, device=dev)
    if nl:
        _launch('ver_det_set_loss_forward', lambda: lib().ver_det_set_loss_forward(
            _p(cls), code, _p(box), ld, _p(match), _p(gt_boxes), _p(gt_labels), _p(counts), _p(code_weights), _p(sums),
            _p(npos), _p(bad), nl, bs, nq, ncls, cap, float(alpha), float(gamma), _stream()))
    return sums, npos, (cls, box, match, gt_boxes, gt_labels, counts, code_weights), dims, code


def det_set_loss_sums(all_cls, all_box, match, gts, code_weights, alpha=0.25, gamma=2.0, bad=None):
    """The raw per-layer sums of ``det_set_loss`` without autograd: (sums fp32 [2, L] = focal, code-weighted L1; npos int32
    [L]), before the weights, the normalisers and ``nan_to_num``.  No caller in the package: it is how the tests read the
    kernel's own output (bit-reproducibility, the NaN of a flagged layer, which ``det_set_loss`` cleans away)."""
    return _set_loss_forward(all_cls, all_box, match, gts, code_weights, alpha, gamma, bad)[:2]


class DetSetLossFunction(Function):
    """Focal and L1 terms of all decoder layers from the match (ver_det_set_loss_forward / _backward):
    -> (loss_cls [L], loss_bbox [L], npos int32 [L]), loss = nan_to_num(loss_weight * sums / norm).  Gradients flow to
    ``all_cls`` and ``all_box`` only; a layer whose loss nan_to_num cleaned passes none, as torch's nan_to_num does."""

    @staticmethod
    def forward(ctx, all_cls, all_box, match, gt_boxes, gt_labels, counts, code_weights, norm, loss_weights, alpha, gamma, bad):
        from .modules.bricks import const_tensor
        sums, npos, operands, dims, code = _set_loss_forward(all_cls, all_box, match, (gt_boxes, gt_labels, counts), code_weights,
                                                             alpha, gamma, bad)
        dev = sums.device
        norm = _gpu(norm.detach(), 'norm', torch.float32)
        if tuple(norm.shape) != (2, dims[0]) or norm.device != dev:
            raise ValueError('det_set_loss: norm must be fp32 [2, %d] on %s' % (dims[0], dev))
        weights = const_tensor([[float(loss_weights[0])], [float(loss_weights[1])]], dev, torch.float32)
        raw = weights * sums / norm
        ctx.save_for_backward(*operands, weights / norm * torch.isfinite(raw))
        ctx.dims, ctx.code, ctx.alpha, ctx.gamma = dims, code, float(alpha), float(gamma)
        loss = torch.nan_to_num(raw)
        ctx.mark_non_differentiable(npos)
        return loss[0], loss[1], npos

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_cls_loss, grad_box_loss, _grad_npos):
        cls, box, match, gt_boxes, gt_labels, counts, code_weights, factor = ctx.saved_tensors
        nl, bs, nq, ncls, cap, ld = ctx.dims
        grads = [torch.zeros_like(factor[0]) if g is None else g.float() for g in (grad_cls_loss, grad_box_loss)]
        scale = (torch.stack(grads) * factor).contiguous()
        grad_cls = None if cls is None else torch.empty_like(cls)
        grad_box = torch.empty_like(box)
        if box.numel():
            _launch('ver_det_set_loss_backward', lambda: lib().ver_det_set_loss_backward(
                _p(cls), ctx.code, _p(box), ld, _p(match), _p(gt_boxes), _p(gt_labels), _p(counts), _p(code_weights), _p(scale),
                _p(grad_cls), _p(grad_box), nl, bs, nq, ncls, cap, ctx.alpha, ctx.gamma, _stream()))
        return (grad_cls, grad_box) + (None,) * 10


def det_set_loss(all_cls, all_box, match, gts, code_weights, norm, loss_weights=(1.0, 1.0), alpha=0.25, gamma=2.0, bad=None):
    """The detection set loss of every decoder layer in one launch each way: all_cls fp32 | bf16 [L, B, Q, C] (None: the
    layout form, loss_cls is 0), all_box fp32 [L, B, Q, >= 10], match int32 [L, B, Q] (``lsa_solve``), gts = (boxes, labels,
    counts) as in ``det_costs``, code_weights fp32 [10], norm fp32 [2, L] (the classification and box normalisers per layer),
    loss_weights = (focal, L1) -> (loss_cls [L], loss_bbox [L], npos int32 [L] = matched rows per layer).
    ``bad``: an int32 device scalar that gets 1 ORed in when a match or a matched label is out of range (that layer's losses
    are NaN before nan_to_num, 0 after).  No gradient flows to the ground truth, ``code_weights`` or ``norm``."""
    gt_boxes, gt_labels, counts = gts
    if all_cls is not None and all_cls.dtype not in (torch.float32, torch.bfloat16):
        all_cls = all_cls.float()
    return DetSetLossFunction.apply(all_cls, all_box.float(), match, gt_boxes, gt_labels, counts, code_weights, norm,
                                    tuple(loss_weights), alpha, gamma, bad)


# ------------------------------------------------------------------------------------------
DET_MATCH_MAX_BOXES = 1024      # ver_det_match: Pcap, Gcap
DET_MATCH_MAX_PAIRS = 16384     # ver_det_match: Pcap * Gcap
DET_MATCH_MAX_THRESHOLDS = 8


def _boxes7(t, name, what):
    t = _gpu(t, name, torch.float32)
    if t.dim() != 3 or t.shape[-1] != 7:
        raise ValueError('%s: %s must be [S, N, 7] = (x, y, z_bottom, dx, dy, dz, yaw), got %s' % (what, name, tuple(t.shape)))
    return t


def _counts(t, name, what, s, device):
    if t is None:
        return None
    t = _gpu(t, name, torch.int32).reshape(-1)
    if t.numel() != s or t.device != device:
        raise ValueError('%s: %s must hold one int32 per sample (%d) on %s' % (what, name, s, device))
    return t


def box3d_overlaps(a, b, na=None, nb=None):
    """Rotated 3-D box IoU (ver_box3d_overlaps; mmdet3d ``overlaps(mode='iou')`` as the reference's indoor_eval.py:102 calls
    it, batched): a fp32 [S, A, 7], b fp32 [S, B, 7] bottom-centre boxes (x, y, z, dx, dy, dz, yaw); na / nb: int32 [S]
    valid boxes per sample (None: all) -> fp32 [S, A, B], 0 for slots beyond the counts and for boxes with a non-finite
    entry or a dimension <= 0.  One launch, no host synchronisation."""
    a, b = _boxes7(a, 'a', 'box3d_overlaps'), _boxes7(b, 'b', 'box3d_overlaps')
    if a.shape[0] != b.shape[0] or a.device != b.device:
        raise ValueError('box3d_overlaps: a %s and b %s must share the sample axis and the device' % (tuple(a.shape), tuple(b.shape)))
    s, ca, cb = a.shape[0], a.shape[1], b.shape[1]
    na, nb = _counts(na, 'na', 'box3d_overlaps', s, a.device), _counts(nb, 'nb', 'box3d_overlaps', s, a.device)
    iou = torch.empty(s, ca, cb, dtype=torch.float32, device=a.device)
    if iou.numel():
        _launch('ver_box3d_overlaps', lambda: lib().ver_box3d_overlaps(_p(a), _p(na), _p(b), _p(nb), _p(iou), s, ca, cb, _stream()))
    return iou


def det_match(pred_boxes, pred_labels, pred_scores, pred_valid, gt_boxes, gt_labels, ngt, thresholds, npos):
    """Per-image matching of the indoor detection protocol (ver_det_match; the reference's eval_det_cls,
    indoor_eval.py:54-143): pred_boxes fp32 [S, P, 7], pred_labels int32 [S, P], pred_scores fp32 [S, P], pred_valid uint8
    [S, P]; gt_boxes fp32 [S, G, 7], gt_labels int32 [S, G], ngt int32 [S]; ``thresholds``: 1..8 IoU thresholds;
    ``npos``: a contiguous int64 [num_classes] tensor that the valid ground truths per class are ADDED to.
    -> (iou_max fp32, gt_index int32, tp_bits uint8), each [S, P]: the best same-class ground truth of every valid
    prediction and, per threshold bit, whether it is the first in (score descending, slot ascending) order to claim it.
    One launch, no host synchronisation."""
    what = 'det_match'
    pred_boxes, gt_boxes = _boxes7(pred_boxes, 'pred_boxes', what), _boxes7(gt_boxes, 'gt_boxes', what)
    s, p = pred_boxes.shape[:2]
    g = gt_boxes.shape[1]
    dev = pred_boxes.device
    pred_labels = _gpu(pred_labels, 'pred_labels', torch.int32)
    pred_scores = _gpu(pred_scores, 'pred_scores', torch.float32)
    pred_valid = _gpu(pred_valid, 'pred_valid', torch.uint8)
    gt_labels = _gpu(gt_labels, 'gt_labels', torch.int32)
    for name, t, shape in (('pred_labels', pred_labels, (s, p)), ('pred_scores', pred_scores, (s, p)),
                           ('pred_valid', pred_valid, (s, p)), ('gt_boxes', gt_boxes, (s, g, 7)), ('gt_labels', gt_labels, (s, g))):
        if tuple(t.shape) != shape or t.device != dev:
            raise ValueError('%s: %s must be %s on %s, got %s on %s' % (what, name, shape, dev, tuple(t.shape), t.device))
    ngt = _counts(ngt, 'ngt', what, s, dev)
    if ngt is None:
        raise ValueError('det_match: ngt is required')
    thr = [float(t) for t in thresholds]
    if not 1 <= len(thr) <= DET_MATCH_MAX_THRESHOLDS:
        raise ValueError('det_match: %d thresholds (1..%d)' % (len(thr), DET_MATCH_MAX_THRESHOLDS))
    if npos.dim() != 1 or npos.dtype != torch.int64 or not npos.is_contiguous() or npos.device != dev or npos.numel() < 1:
        raise ValueError('det_match: npos must be a contiguous int64 [num_classes] tensor on %s' % (dev,))
    if p < 1 or p > DET_MATCH_MAX_BOXES or g > DET_MATCH_MAX_BOXES or p * g > DET_MATCH_MAX_PAIRS:
        raise ValueError('det_match: P=%d G=%d (1 <= P <= %d, G <= %d, P * G <= %d)'
                         % (p, g, DET_MATCH_MAX_BOXES, DET_MATCH_MAX_BOXES, DET_MATCH_MAX_PAIRS))
    iou_max = torch.empty(s, p, dtype=torch.float32, device=dev)
    gt_index = torch.empty(s, p, dtype=torch.int32, device=dev)
    tp_bits = torch.empty(s, p, dtype=torch.uint8, device=dev)
    if s:
        host_thr = (ctypes.c_float * len(thr))(*thr)
        _launch('ver_det_match', lambda: lib().ver_det_match(
            _p(pred_boxes), _p(pred_labels), _p(pred_scores), _p(pred_valid), _p(gt_boxes), _p(gt_labels), _p(ngt), host_thr,
            len(thr), _p(iou_max), _p(gt_index), _p(tp_bits), _p(npos), npos.numel(), s, p, g, _stream()))
    return iou_max, gt_index, tp_bits


# ------------------------------------------------------------------------------------------
DET_DECODE_MAX_SLOTS = 1024     # ver_det_decode: K
DET_DECODE_MAX_KEYS = 16384     # ver_det_decode: Q * C


def det_decode(cls, box, center_range, score_threshold=None, bottom_center=True, k=None):
    """NMS-free decoding of one decoder layer in one launch (ver_det_decode): cls fp32 | bf16 [B, Q, C] logits, or None (the
    room-layout form: every query, in order, no scores); box fp32 [B, Q, 8 | 10] normalised codes (a slice of wider rows is
    read in place); ``center_range``: six numbers; ``score_threshold``: None or a number; ``bottom_center``: z = cz - h / 2;
    ``k``: slots per sample (None: min(Q * C, 1024); the layout form always has Q).
    -> (boxes fp32 [B, K, 7 | 9], scores fp32 [B, K], labels int32 [B, K], valid uint8 [B, K], query int32 [B, K]).  Slot j is
    the j-th entry in (logit descending, flat index ascending) order, a NaN after every number; ``valid``: centre inside the
    range, score above the threshold, logit not a NaN.  No host synchronisation."""
    what = 'det_decode'
    if not box.is_cuda:
        raise RuntimeError('box must be a GPU tensor: the VER ops only exist as HIP kernels')
    if box.dtype != torch.float32:
        raise TypeError('box must be %s, got %s' % (torch.float32, box.dtype))
    if box.dim() != 3 or box.shape[-1] not in (8, 10) or box.shape[1] < 1:
        raise ValueError('%s: box must be [B, Q >= 1, 8 | 10] normalised codes, got %s' % (what, tuple(box.shape)))
    bs, nq, codes = box.shape
    if not (box.stride(2) == 1 and box.stride(1) >= codes and (bs <= 1 or box.stride(0) == nq * box.stride(1))):
        box = box.contiguous()
    ld, dev = box.stride(1), box.device
    ncls, code = 0, 0
    if cls is not None:
        cls = _gpu(cls, 'cls')
        if cls.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError('%s: cls must be float32 or bfloat16, got %s' % (what, cls.dtype))
        if cls.dim() != 3 or tuple(cls.shape[:2]) != (bs, nq) or cls.shape[2] < 1 or cls.device != dev:
            raise ValueError('%s: cls must be [%d, %d, C >= 1] on %s, got %s on %s' % (what, bs, nq, dev, tuple(cls.shape), cls.device))
        ncls, code = cls.shape[2], 1 if cls.dtype == torch.bfloat16 else 0
        keys = nq * ncls
        k = min(keys, DET_DECODE_MAX_SLOTS) if k is None else int(k)
    else:
        keys = nq
        k = nq if k is None else int(k)
        if k != nq:
            raise ValueError('%s: the layout form decodes every query: k=%d, Q=%d' % (what, k, nq))
    if not 1 <= k <= min(keys, DET_DECODE_MAX_SLOTS) or keys > DET_DECODE_MAX_KEYS:
        raise ValueError('%s: k=%d Q*C=%d (1 <= k <= min(Q*C, %d), Q*C <= %d)' % (what, k, keys, DET_DECODE_MAX_SLOTS, DET_DECODE_MAX_KEYS))
    rng = [float(v) for v in center_range]
    if len(rng) != 6:
        raise ValueError('%s: center_range holds %d numbers (6)' % (what, len(rng)))
    flags = (1 if bottom_center else 0) | (2 if score_threshold is not None else 0)
    boxes = torch.empty(bs, k, codes - 1, dtype=torch.float32, device=dev)
    scores = torch.empty(bs, k, dtype=torch.float32, device=dev)
    labels = torch.empty(bs, k, dtype=torch.int32, device=dev)
    valid = torch.empty(bs, k, dtype=torch.uint8, device=dev)
    query = torch.empty(bs, k, dtype=torch.int32, device=dev)
    if bs:
        host_rng = (ctypes.c_float * 6)(*rng)
        _launch('ver_det_decode', lambda: lib().ver_det_decode(
            _p(cls), code, _p(box), ld, _p(boxes), _p(scores), _p(labels), _p(valid), _p(query), host_rng,
            float(score_threshold or 0.0), flags, bs, nq, ncls, k, codes, _stream()))
    return boxes, scores, labels, valid, query


# ------------------------------------------------------------------------------------------
# Occupancy targets (ver_occ_targets): the sparse (voxel, class) annotation of a batch -> byte labels + occupied counts.
def _occ_offsets(offsets, n, name):
    """int32 [bs + 1] offsets as numpy, checked: ascending from 0 to ``n``."""
    import numpy as np
    off = np.asarray(offsets)
    if off.ndim != 1 or off.size < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError('%s must be an integer [bs + 1] array' % name)
    if off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
        raise ValueError('%s must ascend from 0 to %d' % (name, n))
    return off.astype(np.int64)


def occ_targets_host(pairs, offsets, voxel_num, zdim, classes, row_table=None, invalid=None, invalid_offsets=None):
    """The contract of ``ver_occ_targets`` (include/ver_ops.h) in numpy, written from its semantics: the model the tests hold
    the kernel to, and the CPU route of the head.  pairs int [n_total, 2] (flat voxel index, class), offsets int [bs + 1];
    invalid int [n_invalid] with invalid_offsets [bs + 1] or None; row_table int [voxel_num / zdim, 3] or None.
    -> (labels uint8 [bs * voxel_num], count int32 [bs + 1], bad int32 [2]).
    Every voxel starts as ``classes``; a pair (v, c < classes) in range sets voxel v of its sample, the LARGEST class among
    several listings; c == classes writes nothing; anything else is skipped and counted in bad[0].  bad[1]: the pairs whose
    voxel ends up with another class than theirs.  count: the voxels that left the empty state per sample, then the total.
    Invalid voxels become 255 after all pairs; out-of-range ones count in bad[0]."""
    import numpy as np
    voxel_num, zdim, classes = int(voxel_num), int(zdim), int(classes)
    if not 1 <= classes < 255 or zdim < 1 or voxel_num < 0 or voxel_num % zdim:
        raise ValueError('occ_targets_host: voxel_num=%d zdim=%d classes=%d (1 <= classes < 255, voxel_num %% zdim == 0)'
                         % (voxel_num, zdim, classes))
    pairs = np.asarray(pairs).reshape(-1, 2).astype(np.int64)
    off = _occ_offsets(offsets, pairs.shape[0], 'offsets')
    bs = off.size - 1
    if bs * voxel_num >= 2 ** 31:
        raise ValueError('occ_targets_host: %d x %d labels do not fit 2^31' % (bs, voxel_num))
    rows = voxel_num // zdim
    where = None
    if row_table is not None:
        table = np.asarray(row_table).astype(np.int64)
        if table.shape != (rows, 3):
            raise ValueError('occ_targets_host: row_table must be [%d, 3], got %s' % (rows, table.shape))
        v = np.arange(voxel_num, dtype=np.int64)
        z, q = np.divmod(v, rows)
        # [bs, voxel_num]: byte of (sample, voxel)
        where = ((bs * table[q, 0])[None, :] + np.arange(bs, dtype=np.int64)[:, None] * table[q, 1][None, :]
                 + table[q, 2][None, :]) * zdim + z[None, :]
        if bs and voxel_num and not np.array_equal(np.sort(where.reshape(-1)), np.arange(bs * voxel_num)):
            raise ValueError('occ_targets_host: row_table is no permutation of the label bytes')
    vol = np.full((bs, voxel_num), classes, dtype=np.uint8)
    count = np.zeros(bs + 1, dtype=np.int32)
    bad = np.zeros(2, dtype=np.int32)
    for b in range(bs):
        p = pairs[off[b]:off[b + 1]]
        ok = (p[:, 0] >= 0) & (p[:, 0] < voxel_num) & (p[:, 1] >= 0) & (p[:, 1] <= classes)
        bad[0] += int((~ok).sum())
        p = p[ok & (p[:, 1] < classes)]
        best = np.full(voxel_num, -1, dtype=np.int64)
        np.maximum.at(best, p[:, 0], p[:, 1])
        vol[b] = np.where(best >= 0, best, classes).astype(np.uint8)
        count[b] = int((best >= 0).sum())
        bad[1] += int((best[p[:, 0]] != p[:, 1]).sum())
    count[bs] = int(count[:bs].sum())
    if invalid is not None:
        inv = np.asarray(invalid).reshape(-1).astype(np.int64)
        ioff = _occ_offsets(invalid_offsets, inv.size, 'invalid_offsets')
        if ioff.size != bs + 1:
            raise ValueError('occ_targets_host: invalid_offsets must be [%d]' % (bs + 1))
        for b in range(bs):
            i = inv[ioff[b]:ioff[b + 1]]
            ok = (i >= 0) & (i < voxel_num)
            bad[0] += int((~ok).sum())
            vol[b, i[ok]] = 255
    if where is None:
        return vol.reshape(-1), count, bad
    labels = np.empty(bs * voxel_num, dtype=np.uint8)
    labels[where.reshape(-1)] = vol.reshape(-1)
    return labels, count, bad


class PackedOccGts:
    """The occupancy annotation of a batch in ONE int32 buffer, ``[offsets (bs + 1) | invalid_offsets (bs + 1) | pairs
    (2 n_total) | invalid (n_invalid)]``, so that one copy moves all of it (``pack_occ_gts``).  ``pairs``, ``offsets``,
    ``invalid`` and ``invalid_offsets`` are views of ``buffer``; ``to(device)`` is that copy."""

    def __init__(self, buffer, bs, n_total, n_invalid, has_invalid, slot=None):
        self.buffer, self.bs, self.n_total, self.n_invalid, self.has_invalid = buffer, bs, n_total, n_invalid, has_invalid
        self._slot, self._generation = slot, (slot[2] if slot is not None else None)
        h = 2 * (bs + 1)
        self.offsets = buffer[:bs + 1]
        self.invalid_offsets = buffer[bs + 1:h] if has_invalid else None
        self.pairs = buffer[h:h + 2 * n_total].view(n_total, 2)
        self.invalid = buffer[h + 2 * n_total:h + 2 * n_total + n_invalid] if has_invalid else None

    def to(self, device):
        """On ``device``: one asynchronous copy on the current stream out of the (pinned) staging buffer, whose next
        ``pack_occ_gts`` waits for this copy's event before it rewrites the buffer."""
        device = torch.device(device)
        if self._slot is not None and self._slot[2] != self._generation:
            raise RuntimeError('PackedOccGts.to: the staging buffer of this size class was packed again since -- one pack is '
                               'outstanding per size class: copy it (.to) before the next pack_occ_gts, or pack with pinned=False')
        if device.type != 'cuda':
            return PackedOccGts(self.buffer.clone(), self.bs, self.n_total, self.n_invalid, self.has_invalid)
        dev = self.buffer.to(device, non_blocking=True)
        if self._slot is not None:
            done = torch.cuda.Event()
            done.record()
            self._slot[1] = done
        return PackedOccGts(dev, self.bs, self.n_total, self.n_invalid, self.has_invalid)


_OCC_STAGING = {}            # capacity in int32 elements (a power of two) -> [pinned host buffer, copy-done event or None, packs]


def pack_occ_gts(occ_gts, invalid=None, pinned=True):
    """Host half of ``occ_targets``: ``occ_gts[b]`` -- an integer [n, 2] array of (flat voxel index, class) pairs, or the
    reference's one-element list around it (``occ_gts[b][0]``) -- and optionally ``invalid[b]`` (integer voxel indices or
    None) of every sample, concatenated into one int32 staging buffer with their offsets -> ``PackedOccGts`` on the host.
    With ``pinned`` and a GPU present the buffer is pinned, kept per size class (the next power of two) and reused: its
    ``to(device)`` is ONE ``non_blocking`` copy, and the buffer is not rewritten before that copy's event has completed.
    A loader that wants the copy to overlap the previous step calls this and ``.to(device)`` ahead of time and hands the
    result to ``head.occupancy_targets_device``.  ONE pack is outstanding per size class: the next ``pack_occ_gts`` of that
    class rewrites the buffer, and ``to`` of the earlier object then raises instead of copying the other batch
    (``pinned=False`` gives an object with memory of its own).  Values outside int32 are saturated, so they stay out of range."""
    import numpy as np

    def arr(a, cols):
        if cols == 2 and isinstance(a, (list, tuple)):
            a = a[0]                                           # occ_gts[bs][queue_index], as head.occupancy_targets reads it
        if a is None:
            return np.zeros((0, 2) if cols == 2 else (0,), dtype=np.int32)
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if a.size == 0:
            return np.zeros((0, 2) if cols == 2 else (0,), dtype=np.int32)
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError('pack_occ_gts: integer arrays expected, got %s' % a.dtype)
        if cols == 2 and (a.ndim != 2 or a.shape[1] != 2):
            raise ValueError('pack_occ_gts: a sample is [n, 2] (voxel index, class) pairs, got %s' % (a.shape,))
        return a if cols == 2 else a.reshape(-1)

    gts = [arr(a, 2) for a in occ_gts]
    bs = len(gts)
    has_invalid = invalid is not None
    inv = [arr(a, 1) for a in invalid] if has_invalid else []
    if has_invalid and len(inv) != bs:
        raise ValueError('pack_occ_gts: %d invalid lists for %d samples' % (len(inv), bs))
    n_total, n_invalid = sum(a.shape[0] for a in gts), sum(a.size for a in inv)
    used = 2 * (bs + 1) + 2 * n_total + n_invalid
    if max(n_total, n_invalid) >= 2 ** 31 - 1 or used >= 2 ** 31:
        raise ValueError('pack_occ_gts: %d pairs / %d invalid voxels exceed the int32 offsets' % (n_total, n_invalid))
    slot = None
    if pinned and torch.cuda.is_available():
        cap = 1024
        while cap < used:
            cap *= 2
        slot = _OCC_STAGING.get(cap)
        if slot is None:
            slot = _OCC_STAGING[cap] = [torch.empty(cap, dtype=torch.int32, pin_memory=True), None, 0]
        elif slot[1] is not None:
            slot[1].synchronize()                              # the previous copy out of this buffer
        slot[2] += 1                                           # (an earlier pack of this size class is void from here on)
        host = slot[0][:used]
    else:
        host = torch.empty(used, dtype=torch.int32)
    hv = host.numpy()
    lim = np.iinfo(np.int32)

    def put(dst, a):
        if a.dtype.itemsize > 4 or a.dtype == np.uint32:
            np.clip(a, lim.min, lim.max, out=dst, casting='unsafe')
        else:
            dst[...] = a

    h = 2 * (bs + 1)
    hv[0] = 0
    hv[bs + 1] = 0
    if bs:
        hv[1:bs + 1] = np.cumsum([a.shape[0] for a in gts])
        hv[bs + 2:h] = np.cumsum([a.size for a in inv]) if has_invalid else 0
    pos = h
    for a in gts:
        put(hv[pos:pos + a.size].reshape(-1, 2), a)
        pos += a.size
    for a in inv:
        put(hv[pos:pos + a.size], a)
        pos += a.size
    return PackedOccGts(host, bs, n_total, n_invalid, has_invalid, slot)


def occ_targets(pairs, offsets, voxel_num, zdim, classes, row_table=None, invalid=None, invalid_offsets=None, out=None):
    """Byte labels and occupied counts of a batch from its sparse annotation (ver_occ_targets): pairs int32 | int64
    [n_total, 2] (flat voxel index, class) of all samples, offsets int32 [bs + 1], both on the GPU; ``row_table`` int32
    [voxel_num / zdim, 3] (``occ_proj_lattice.row_table``) writes the labels in the group-major row order of the occupancy
    GEMMs, None in the reference's voxel order; ``invalid`` int32 | int64 [n_invalid] with ``invalid_offsets`` int32
    [bs + 1]: voxels set to 255 after the pairs.  ``out``: ``(labels, count, bad)`` of an earlier call to write into.
    -> (labels uint8 [bs * voxel_num], count int32 [bs + 1], bad int32 [2]); semantics: ``occ_targets_host``.
    Four launches at most, no host synchronisation, capturable."""
    what = 'occ_targets'
    pairs = _gpu(pairs, 'pairs')
    dev = pairs.device
    if pairs.dtype not in (torch.int32, torch.int64) or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise TypeError('%s: pairs must be int32 or int64 [n_total, 2], got %s %s' % (what, pairs.dtype, tuple(pairs.shape)))

    def idx(t, name, shape):
        t = _gpu(t, name, torch.int32)
        if tuple(t.shape) != shape or t.device != dev:
            raise ValueError('%s: %s must be int32 %s on %s, got %s on %s' % (what, name, shape, dev, tuple(t.shape), t.device))
        return t

    if offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError('%s: offsets must be [bs + 1]' % what)
    bs = offsets.numel() - 1
    offsets = idx(offsets, 'offsets', (bs + 1,))
    voxel_num, zdim, classes = int(voxel_num), int(zdim), int(classes)
    if voxel_num < 0 or zdim < 1 or classes < 1:
        raise ValueError('%s: voxel_num=%d zdim=%d classes=%d' % (what, voxel_num, zdim, classes))
    if row_table is not None:
        row_table = idx(row_table, 'row_table', (voxel_num // zdim, 3))
    n_invalid = 0
    if (invalid is None) != (invalid_offsets is None):
        raise ValueError('%s: invalid and invalid_offsets come together' % what)
    if invalid is not None:
        invalid = _gpu(invalid, 'invalid')
        if invalid.dtype not in (torch.int32, torch.int64) or invalid.dim() != 1 or invalid.device != dev:
            raise TypeError('%s: invalid must be int32 or int64 [n_invalid] on %s' % (what, dev))
        invalid_offsets = idx(invalid_offsets, 'invalid_offsets', (bs + 1,))
        n_invalid = invalid.numel()
    total = bs * voxel_num
    padded = (total + 3) // 4 * 4
    if out is None:
        labels = torch.empty(padded, dtype=torch.uint8, device=dev)[:total]
        count = torch.empty(bs + 1, dtype=torch.int32, device=dev)
        bad = torch.empty(2, dtype=torch.int32, device=dev)
    else:
        labels, count, bad = out
        room = labels.untyped_storage().nbytes() - labels.storage_offset()
        if (labels.dtype != torch.uint8 or labels.numel() != total or not labels.is_contiguous() or labels.device != dev
                or room < padded):
            raise ValueError('%s: out labels must be %d contiguous uint8 on %s, allocated up to a multiple of 4 bytes' % (what, total, dev))
        labels = labels.view(-1)
        count, bad = idx(count, 'out count', (bs + 1,)), idx(bad, 'out bad', (2,))
    code = lambda t: 1 if t is not None and t.dtype == torch.int64 else 0
    _launch('ver_occ_targets', lambda: lib().ver_occ_targets(
        _p(pairs), code(pairs), _p(offsets), pairs.shape[0], _p(invalid), code(invalid), _p(invalid_offsets), n_invalid,
        _p(row_table), _p(labels), _p(count), _p(bad), voxel_num, zdim, classes, bs, _stream()))
    return labels, count, bad


# ------------------------------------------------------------------------------------------
# Occupancy pairs (ver_occ_pairs): byte labels of a batch -> per-sample sparse (voxel, class) pairs with offsets, the inverse
# of occ_targets, in fixed shapes and without a host read.
def occ_pairs_block_size():
    """Voxels of one sample a workgroup of ``ver_occ_pairs`` covers: its scratch holds one int32 per such block."""
    return int(lib().ver_occ_pairs_block_size())


def _occ_pairs_sizes(who, bs, voxel_num, zdim, classes, capacity, flat, int32_pairs):
    bs, voxel_num, zdim, classes = int(bs), int(voxel_num), int(zdim), int(classes)
    if bs < 0 or voxel_num < 0 or zdim < 1 or not 1 <= classes < 255 or voxel_num % zdim:
        raise ValueError('%s: bs=%d voxel_num=%d zdim=%d classes=%d (1 <= classes < 255, voxel_num %% zdim == 0)'
                         % (who, bs, voxel_num, zdim, classes))
    if bs * voxel_num >= 2 ** 31:
        raise ValueError('%s: %d x %d labels do not fit 2^31%s' % (who, bs, voxel_num, ' (nor do flattened-batch indices fit '
                                                                    'int32 pairs)' if flat and int32_pairs else ''))
    capacity = bs * voxel_num if capacity is None else int(capacity)
    if not 0 <= capacity < 2 ** 31:
        raise ValueError('%s: capacity=%d' % (who, capacity))
    return bs, voxel_num, zdim, classes, capacity


def occ_pairs_host(labels, bs, voxel_num, zdim, classes, row_table=None, capacity=None, flat=False, dtype=torch.int32):
    """The contract of ``ver_occ_pairs`` (include/ver_ops.h) in numpy, written from its semantics: the model the tests hold the
    kernel to, and the CPU route.  labels uint8 [bs * voxel_num] in the reference's (Z, X, Y) voxel order, or -- with
    ``row_table`` int [voxel_num / zdim, 3] -- in the group-major row order ``occ_targets_host`` writes.
    -> (pairs [capacity, 2] of ``dtype`` (int32 | int64), offsets int32 [bs + 1], count int32 [bs + 2]).
    A byte < ``classes`` is an occupied voxel; ``classes`` and anything above produce nothing.  pairs: (voxel index within
    the sample -- plus ``b * voxel_num`` with ``flat`` --, class), ascending within a sample, sample after sample; only the
    first ``min(total, capacity)`` are written (zeros behind them here).  offsets: exclusive prefix sums of the per-sample
    counts, each clamped to ``capacity``.  count: the true count of every sample, the true total, then 1 if the total
    exceeded ``capacity``.  ``capacity=None``: ``bs * voxel_num``, which no batch overflows."""
    import numpy as np
    np_dtype = {torch.int32: np.int32, torch.int64: np.int64}.get(dtype, dtype)
    if np_dtype not in (np.int32, np.int64):
        raise TypeError('occ_pairs_host: pairs are int32 or int64, got %s' % (dtype,))
    bs, voxel_num, zdim, classes, capacity = _occ_pairs_sizes('occ_pairs_host', bs, voxel_num, zdim, classes, capacity, flat,
                                                              np_dtype == np.int32)
    lab = np.asarray(labels).reshape(-1)
    if lab.dtype != np.uint8 or lab.size != bs * voxel_num:
        raise ValueError('occ_pairs_host: labels must be %d uint8, got %d %s' % (bs * voxel_num, lab.size, lab.dtype))
    rows = voxel_num // zdim
    if row_table is None:
        vol = lab.reshape(bs, voxel_num)
    else:
        table = np.asarray(row_table).astype(np.int64)
        if table.shape != (rows, 3):
            raise ValueError('occ_pairs_host: row_table must be [%d, 3], got %s' % (rows, table.shape))
        z, q = np.divmod(np.arange(voxel_num, dtype=np.int64), rows)
        # [bs, voxel_num]: byte of (sample, voxel), occ_targets_host's formula
        where = ((bs * table[q, 0])[None, :] + np.arange(bs, dtype=np.int64)[:, None] * table[q, 1][None, :]
                 + table[q, 2][None, :]) * zdim + z[None, :]
        inside = (where >= 0) & (where < bs * voxel_num)
        vol = np.where(inside, lab[np.where(inside, where, 0)], classes).astype(np.uint8) if lab.size else lab.reshape(bs, voxel_num)
    count = np.zeros(bs + 2, dtype=np.int32)
    found = []
    for b in range(bs):
        v = np.flatnonzero(vol[b] < classes)
        count[b] = v.size
        found.append(np.stack([v + (b * voxel_num if flat else 0), vol[b][v].astype(np.int64)], axis=1))
    total = int(count[:bs].sum())
    count[bs], count[bs + 1] = total, int(total > capacity)
    offsets = np.minimum(np.concatenate([[0], np.cumsum(count[:bs], dtype=np.int64)]), capacity).astype(np.int32)
    pairs = np.zeros((capacity, 2), dtype=np_dtype)
    if found:
        kept = np.concatenate(found)[:capacity]
        pairs[:kept.shape[0]] = kept
    return pairs, offsets, count


class OccPairsGts(PackedOccGts):
    """``(pairs, offsets)`` of ``occ_pairs`` (per-sample indices, ``flat=False``) as the ``PackedOccGts`` that ``occ_targets``
    and ``head.occupancy_targets_device`` take -- the round trip: ``occ_targets(g.pairs, g.offsets, ...)`` visits
    ``[offsets[b], offsets[b + 1])`` of every sample and nothing behind ``offsets[bs]``.  A view: no copy, no host read."""

    def __init__(self, pairs, offsets):
        if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype not in (torch.int32, torch.int64) or offsets.dim() != 1 \
                or offsets.dtype != torch.int32 or offsets.numel() < 1 or offsets.device != pairs.device:
            raise TypeError('OccPairsGts: pairs int32 | int64 [capacity, 2] and offsets int32 [bs + 1] on one device')
        self.buffer, self.bs, self.n_total, self.n_invalid, self.has_invalid = pairs, offsets.numel() - 1, pairs.shape[0], 0, False
        self._slot = self._generation = None
        self.pairs, self.offsets, self.invalid, self.invalid_offsets = pairs, offsets, None, None

    def to(self, device):
        return OccPairsGts(self.pairs.to(device), self.offsets.to(device))


def occ_pairs(labels, bs, voxel_num, zdim, classes, row_table=None, capacity=None, flat=False, dtype=torch.int32, out=None):
    """Per-sample sparse pairs of a batch of byte labels (ver_occ_pairs; semantics: ``occ_pairs_host``): labels uint8
    [bs * voxel_num] on the GPU (any shape with that many elements), in the reference's voxel order or -- with ``row_table``
    int32 [voxel_num / zdim, 3] (``occ_proj_lattice.row_table``) -- in the GEMMs' row order, e.g. as ``occ_mlp_classes`` leaves
    them.  -> (pairs ``dtype`` [capacity, 2], offsets int32 [bs + 1], count int32 [bs + 2]); ``capacity=None``:
    ``bs * voxel_num``.  ``flat``: voxel indices over the flattened batch, what ``occupancy_pairs_from_classes`` returns.
    ``out``: ``(pairs, offsets, count)`` of an earlier call with the same sizes to write into -- offsets, count and the
    kernel's scratch are one allocation, so such a call allocates nothing.  Three launches, no host synchronisation,
    capturable; sample b's pairs are ``pairs[offsets[b]:offsets[b + 1]]`` once the host knows the offsets."""
    what = 'occ_pairs'
    labels = _gpu(labels, 'labels', torch.uint8).reshape(-1)
    dev = labels.device
    if dtype not in (torch.int32, torch.int64):
        raise TypeError('%s: pairs are int32 or int64, got %s' % (what, dtype))
    bs, voxel_num, zdim, classes, capacity = _occ_pairs_sizes(what, bs, voxel_num, zdim, classes, capacity, flat,
                                                              dtype == torch.int32)
    if labels.numel() != bs * voxel_num:
        raise ValueError('%s: %d labels for %d x %d voxels' % (what, labels.numel(), bs, voxel_num))
    if row_table is not None:
        row_table = _gpu(row_table, 'row_table', torch.int32)
        if tuple(row_table.shape) != (voxel_num // zdim, 3) or row_table.device != dev:
            raise ValueError('%s: row_table must be int32 %s on %s' % (what, (voxel_num // zdim, 3), dev))
    nb = int(lib().ver_occ_pairs_blocks(bs, voxel_num))
    head = 2 * bs + 3
    if out is None:
        pairs = torch.empty(capacity, 2, dtype=dtype, device=dev)
        # (zeros: a call with bs == 0 or voxel_num == 0 launches nothing and still returns offsets and counts)
        meta = torch.zeros(head + nb, dtype=torch.int32, device=dev) if nb == 0 else torch.empty(head + nb, dtype=torch.int32, device=dev)
        offsets, count, work = meta[:bs + 1], meta[bs + 1:head], meta[head:]
    else:
        pairs, offsets, count = out
        if (pairs.dtype != dtype or tuple(pairs.shape) != (capacity, 2) or not pairs.is_contiguous() or pairs.device != dev):
            raise ValueError('%s: out pairs must be contiguous %s %s on %s' % (what, dtype, (capacity, 2), dev))
        for t, name, n in ((offsets, 'out offsets', bs + 1), (count, 'out count', bs + 2)):
            if t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_contiguous() or t.device != dev:
                raise ValueError('%s: %s must be contiguous int32 [%d] on %s' % (what, name, n, dev))
        room = offsets.untyped_storage().nbytes() // 4 - offsets.storage_offset()
        if count.data_ptr() == offsets.data_ptr() + 4 * (bs + 1) and room >= head + nb:
            work = offsets.as_strided((nb,), (1,), offsets.storage_offset() + head)       # the earlier call's scratch
        else:
            work = torch.empty(nb, dtype=torch.int32, device=dev)
    _launch('ver_occ_pairs', lambda: lib().ver_occ_pairs(
        _p(labels), _p(row_table), _p(pairs), 1 if dtype == torch.int64 else 0, _p(offsets), _p(count), _p(work), capacity,
        voxel_num, zdim, classes, bs, 1 if flat else 0, _stream()))
    return pairs, offsets, count


# ------------------------------------------------------------------------------------------
# A batch out of a device-resident viewpoint store (ver_fetch_batch): features, cameras, padded box tables and sparse pairs
# of the viewpoints an index vector names, written into buffers of fixed shapes without a host read (resident.ResidentStore).
def fetch_pair_tile():
    """Output pair slots one workgroup of ``ver_fetch_batch``'s pair copy covers."""
    return int(lib().ver_fetch_pair_tile())


def fetch_batch_host(index, V=None, feats=None, world2pixel=None, origin=None, boxes=None, labels=None, counts=None,
                     pairs=None, pair_offsets=None, out_cap=None, pair_capacity=None, out=None):
    """The contract of ``ver_fetch_batch`` (include/ver_ops.h) in numpy, written from its semantics: the model the tests hold
    the kernels to, and the CPU route of ``ResidentStore.fetch``.  ``index`` int [bs]; the store's tables as arrays, a group
    being absent when its tables are None: ``feats [V, Ncam, row]`` (any dtype: a pure copy); ``world2pixel [V, Ncam, 4, 4]``
    with ``origin [V, 3]``; ``boxes [V, store_cap, box_dim]``, ``labels [V, store_cap]``, ``counts [V]`` with ``out_cap``;
    ``pairs [total, 2]`` with ``pair_offsets [V + 1]`` (CSR) and ``pair_capacity``.  ``out``: a dict of earlier outputs
    (``boxes``, ``labels``, ``pairs``) whose contents past the counts / behind the live pairs are KEPT; zeros without it.
    -> dict of the present groups' outputs -- ``feats [Ncam, bs, row]``, ``world2pixel [bs, Ncam, 4, 4]``, ``origin [bs, 3]``,
    ``boxes f32 [bs, out_cap, box_dim]``, ``labels int64 [bs, out_cap]``, ``counts int32 [bs]``, ``offsets int32 [bs + 1]``,
    ``pairs int32 [pair_capacity, 2]`` -- and ``status`` int32 [4].
    A sample whose index is outside [0, V) is empty: zero features and cameras, count 0, no pairs.  A sample's first
    min(count, out_cap) box rows are copied and that minimum is its count.  offsets: exclusive prefix sums of the fetched
    pair lengths, each clamped to the capacity; pairs past the capacity are dropped.  status: samples with an index outside
    the store; samples whose count exceeded ``out_cap``; 1 if the pairs overflowed; the true pair total, saturated at
    2^31 - 1."""
    import numpy as np
    idx = np.asarray(index).reshape(-1).astype(np.int64)
    bs = idx.size
    for t in (feats, world2pixel, counts):
        if V is None and t is not None:
            V = t.shape[0]
    if V is None:
        V = (np.asarray(pair_offsets).size - 1) if pair_offsets is not None else 0
    V = int(V)
    ok = (idx >= 0) & (idx < V)
    safe = np.where(ok, idx, 0)
    out = dict(out or {})
    res = {}
    status = np.zeros(4, dtype=np.int32)
    status[0] = int((~ok).sum())
    if feats is not None:
        feats = np.asarray(feats)
        if feats.ndim != 3 or feats.shape[0] != V:
            raise ValueError('fetch_batch_host: feats must be [%d, Ncam, row], got %s' % (V, feats.shape))
        got = np.zeros((feats.shape[1], bs, feats.shape[2]), dtype=feats.dtype)
        if V and bs:
            got[:, ok] = feats[safe[ok]].transpose(1, 0, 2)
        res['feats'] = got
    if (world2pixel is None) != (origin is None):
        raise ValueError('fetch_batch_host: world2pixel and origin come together')
    if world2pixel is not None:
        w2p, org = np.asarray(world2pixel, dtype=np.float32), np.asarray(origin, dtype=np.float32)
        if w2p.ndim != 4 or w2p.shape[0] != V or w2p.shape[2:] != (4, 4) or org.shape != (V, 3):
            raise ValueError('fetch_batch_host: world2pixel [%d, Ncam, 4, 4] and origin [%d, 3], got %s and %s' % (V, V, w2p.shape, org.shape))
        res['world2pixel'] = np.zeros((bs,) + w2p.shape[1:], dtype=np.float32)
        res['origin'] = np.zeros((bs, 3), dtype=np.float32)
        if V and bs:
            res['world2pixel'][ok] = w2p[safe[ok]]
            res['origin'][ok] = org[safe[ok]]
    if counts is not None:
        boxes, labels, counts = np.asarray(boxes, dtype=np.float32), np.asarray(labels).astype(np.int64), np.asarray(counts).astype(np.int64)
        if boxes.ndim != 3 or boxes.shape[0] != V or labels.shape != boxes.shape[:2] or counts.shape != (V,) or out_cap is None:
            raise ValueError('fetch_batch_host: boxes [%d, cap, dim], labels [%d, cap], counts [%d] and out_cap' % (V, V, V))
        store_cap, dim, out_cap = boxes.shape[1], boxes.shape[2], int(out_cap)
        got_b = np.array(out['boxes'], dtype=np.float32) if 'boxes' in out else np.zeros((bs, out_cap, dim), dtype=np.float32)
        got_l = np.array(out['labels'], dtype=np.int64) if 'labels' in out else np.zeros((bs, out_cap), dtype=np.int64)
        got_c = np.zeros(bs, dtype=np.int32)
        for b in range(bs):
            if ok[b]:
                c = int(counts[idx[b]])
                status[1] += int(c > out_cap)
                n = min(max(c, 0), store_cap, out_cap)
                got_b[b, :n] = boxes[idx[b], :n]
                got_l[b, :n] = labels[idx[b], :n]
                got_c[b] = n
        res.update(boxes=got_b, labels=got_l, counts=got_c)
    if pair_offsets is not None:
        po = np.asarray(pair_offsets).astype(np.int64)
        pairs = np.asarray(pairs if pairs is not None else np.zeros((0, 2)), dtype=np.int32).reshape(-1, 2)
        if po.shape != (V + 1,) or pair_capacity is None:
            raise ValueError('fetch_batch_host: pair_offsets must be [%d] and pair_capacity given' % (V + 1))
        cap = int(pair_capacity)
        lo = np.clip(po[:-1], 0, pairs.shape[0])
        hi = np.clip(np.maximum(po[1:], lo), 0, pairs.shape[0])
        lens = np.where(ok, (hi - lo)[safe] if V else 0, 0).astype(np.int64)
        starts = np.concatenate([[0], np.cumsum(lens)])
        total = int(starts[-1])
        got_p = np.array(out['pairs'], dtype=np.int32) if 'pairs' in out else np.zeros((cap, 2), dtype=np.int32)
        for b in range(bs):
            n = max(0, min(int(starts[b + 1]), cap) - int(starts[b]))
            if n:
                got_p[starts[b]:starts[b] + n] = pairs[lo[idx[b]]:lo[idx[b]] + n]
        res.update(offsets=np.minimum(starts, cap).astype(np.int32), pairs=got_p)
        status[2], status[3] = int(total > cap), min(total, 2 ** 31 - 1)
    res['status'] = status
    return res


def fetch_batch(index, V, feats=None, cameras=None, boxes=None, pairs=None, status=None):
    """``ver_fetch_batch`` (semantics: ``fetch_batch_host``): ``index`` int32 [bs] ON THE GPU, read by the kernels alone; ``V``
    viewpoints in the store.  Each group is a tuple of GPU tensors or None (absent):
    ``feats = (store [V, Ncam, row] f32 | bf16, out [Ncam, bs, ...] of row elements per (camera, sample))``;
    ``cameras = (w2p_store [V, Ncam, 4, 4], origin_store [V, 3], w2p_out [bs, Ncam, 4, 4], origin_out [bs, 3])`` f32;
    ``boxes = (box_store f32 [V, store_cap, dim], label_store int64 [V, store_cap], count_store int32 [V], box_out f32
    [bs, out_cap, dim], label_out int64 [bs, out_cap], count_out int32 [bs])``;
    ``pairs = (pair_store int32 [total, 2], pair_offsets int64 [V + 1], offsets_out int32 [bs + 1], pairs_out int32
    [pair_capacity, 2])``.  ``status``: int32 [4] to write (allocated when None) -> status.  Every shape is checked here, on
    the host; at most four launches, no synchronisation, capturable."""
    what = 'fetch_batch'
    index = _gpu(index, 'index', torch.int32)
    dev = index.device
    if index.dim() != 1:
        raise ValueError('%s: index must be int32 [bs], got %s' % (what, tuple(index.shape)))
    bs, V = index.numel(), int(V)
    if V < 0:
        raise ValueError('%s: V=%d' % (what, V))

    def need(t, name, dtype, shape):
        if not torch.is_tensor(t) or not t.is_cuda or t.device != dev or t.dtype != dtype or tuple(t.shape) != tuple(shape) \
                or not t.is_contiguous():
            raise ValueError('%s: %s must be contiguous %s %s on %s, got %s' % (
                what, name, dtype, tuple(shape), dev,
                '%s %s on %s' % (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__))
        return t

    ncam = 0
    f_store = f_out = w_store = o_store = w_out = o_out = None
    b_store = l_store = c_store = b_out = l_out = c_out = p_store = p_off = off_out = p_out = None
    f_dtype, row, store_cap, out_cap, dim, total, cap = 0, 0, 0, 0, 0, 0, 0
    if feats is not None:
        f_store, f_out = feats
        if f_store.dim() != 3 or f_store.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError('%s: the feature store is f32 or bf16 [V, Ncam, row], got %s %s' % (what, f_store.dtype, tuple(f_store.shape)))
        ncam, row = int(f_store.shape[1]), int(f_store.shape[2])
        need(f_store, 'feat_store', f_store.dtype, (V, ncam, row))
        if f_out.dim() < 2 or f_out.numel() != ncam * bs * row:
            raise ValueError('%s: feat_out %s does not hold [%d, %d] rows of %d' % (what, tuple(f_out.shape), ncam, bs, row))
        need(f_out, 'feat_out', f_store.dtype, (ncam, bs) + tuple(f_out.shape[2:]))
        f_dtype = 1 if f_store.dtype == torch.bfloat16 else 0
    if cameras is not None:
        w_store, o_store, w_out, o_out = cameras
        if w_store.dim() != 4 or (feats is not None and w_store.shape[1] != ncam):
            raise ValueError('%s: w2p_store %s beside %d cameras of features' % (what, tuple(w_store.shape), ncam))
        ncam = int(w_store.shape[1])
        need(w_store, 'w2p_store', torch.float32, (V, ncam, 4, 4))
        need(o_store, 'origin_store', torch.float32, (V, 3))
        need(w_out, 'w2p_out', torch.float32, (bs, ncam, 4, 4))
        need(o_out, 'origin_out', torch.float32, (bs, 3))
    if boxes is not None:
        b_store, l_store, c_store, b_out, l_out, c_out = boxes
        if b_store.dim() != 3 or b_out.dim() != 3:
            raise ValueError('%s: box_store [V, store_cap, dim] and box_out [bs, out_cap, dim]' % what)
        store_cap, dim, out_cap = int(b_store.shape[1]), int(b_store.shape[2]), int(b_out.shape[1])
        need(b_store, 'box_store', torch.float32, (V, store_cap, dim))
        need(l_store, 'label_store', torch.int64, (V, store_cap))
        need(c_store, 'count_store', torch.int32, (V,))
        need(b_out, 'box_out', torch.float32, (bs, out_cap, dim))
        need(l_out, 'label_out', torch.int64, (bs, out_cap))
        need(c_out, 'count_out', torch.int32, (bs,))
    if pairs is not None:
        p_store, p_off, off_out, p_out = pairs
        total, cap = int(p_store.shape[0]), int(p_out.shape[0])
        need(p_store, 'pair_store', torch.int32, (total, 2))
        need(p_off, 'pair_offsets', torch.int64, (V + 1,))
        need(off_out, 'offsets_out', torch.int32, (bs + 1,))
        need(p_out, 'pairs_out', torch.int32, (cap, 2))
    status = torch.empty(4, dtype=torch.int32, device=dev) if status is None else need(status, 'status', torch.int32, (4,))
    if bs == 0:
        return status.zero_()
    # (an empty tensor's address is 0 = NULL, which the C side takes where a table has no rows)
    _launch('ver_fetch_batch', lambda: lib().ver_fetch_batch(
        _p(index), bs, V, ncam, _p(f_store), _p(f_out), f_dtype, row, _p(w_store), _p(o_store), _p(w_out), _p(o_out),
        _p(b_store), _p(l_store), _p(c_store), _p(b_out), _p(l_out), _p(c_out), store_cap, out_cap, dim,
        _p(p_store), _p(p_off), total, _p(off_out), _p(p_out), cap, _p(status), _stream()))
    return status


# ------------------------------------------------------------------------------------------
def wgrad_tn_supported(a, g):
    """Shapes / strides ``wgrad_tn`` takes: bf16 GPU matrices, unit column stride, 16-byte aligned rows."""
    return (a.is_cuda and g.is_cuda and a.dtype == torch.bfloat16 and g.dtype == torch.bfloat16 and a.dim() == 2
            and g.dim() == 2 and a.shape[0] == g.shape[0] and a.stride(1) == 1 and g.stride(1) == 1
            and a.stride(0) % 8 == 0 and g.stride(0) % 8 == 0 and a.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
            and g.shape[1] % 4 == 0)


def wgrad_tn(a, g, out_dtype=None, splits=0, flags=0, out=None):
    """``a.t() @ g`` for tall bf16 operands with the ROWS on the contraction axis (ver_wgrad_tn): a [M, Ka] (may be a
    column range of a wider row-major matrix), g [M, N] -> [Ka, N] in ``out_dtype`` (default: a's dtype; ``out``: a matrix
    of that dtype to write into, e.g. a row range of a stacked buffer), fp32 accumulation over all rows.  The weight gradient of a lattice layer / of occ_proj (dense_heads/upsample.py::rows_tn)."""
    if not wgrad_tn_supported(a, g):
        raise RuntimeError('wgrad_tn: unsupported operands %s %s / %s %s' % (tuple(a.shape), a.stride(), tuple(g.shape), g.stride()))
    m, ka = a.shape
    n = g.shape[1]
    out_dtype = out_dtype or a.dtype
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise TypeError('wgrad_tn: out_dtype must be bf16 or fp32')
    L = lib()
    if splits <= 0:
        splits = L.ver_wgrad_tn_splits_ld(m, ka, n, max(a.stride(0), g.stride(0)))
    nbytes = L.ver_wgrad_tn_workspace(m, ka, n, splits)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=a.device)
    if out is None:
        out = torch.empty(ka, n, dtype=out_dtype, device=a.device)
    elif not (out.is_cuda and out.shape == (ka, n) and out.dtype == out_dtype and out.stride(1) == 1):
        raise RuntimeError('wgrad_tn: out must be a [Ka, N] GPU matrix of out_dtype with unit column stride')
    _launch('ver_wgrad_tn', lambda: L.ver_wgrad_tn(
        _p(a), a.stride(0), _p(g), g.stride(0), m, ka, n, _p(out), out.stride(0), 1 if out_dtype == torch.bfloat16 else 0,
        splits, flags, _p(ws), nbytes, _stream()), meta=dict(flops=2.0 * m * ka * n))
    return out


def gemm_nn_supported(a, w):
    """Shapes / strides ``gemm_nn`` takes: bf16 GPU matrices, unit column stride, 16-byte aligned rows, K % 32 == 0."""
    return (a.is_cuda and w.is_cuda and a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and a.dim() == 2
            and w.dim() == 2 and a.shape[1] == w.shape[0] and a.stride(1) == 1 and w.stride(1) == 1
            and a.stride(0) % 8 == 0 and w.stride(0) % 8 == 0 and a.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
            and a.shape[1] % 32 == 0 and a.shape[1] >= 64)


def gemm_nn_splits(m, k, n):
    """K slices ``gemm_nn`` would cut an [m, k] x [k, n] product into (1: one pass, no workspace): > 1 for skinny operands."""
    return lib().ver_gemm_nn_splits(m, k, n)


def gemm_nn(a, w, bias=None, out=None, splits=None, timer_class='ver_gemm_nn'):
    """``a @ w (+ bias)`` on ver_gemm_nn: a bf16 [M, K] (may be a column range of a wider row-major matrix), w bf16 [K, N]
    row-major, bias fp32 [N] or None -> bf16 [M, N] (``out``: a bf16 matrix with unit column stride to write into).
    ``splits``: K slices (None: the library's choice -- 1 except for skinny operands; fp32 partial tiles, added up once).
    ``timer_class``: the name a KernelTimer files the launch under (bench.py's classes of the head's products)."""
    if not gemm_nn_supported(a, w):
        raise RuntimeError('gemm_nn: unsupported operands %s %s / %s %s' % (tuple(a.shape), a.stride(), tuple(w.shape), w.stride()))
    m, k = a.shape
    n = w.shape[1]
    if out is None:
        out = torch.empty(m, n, dtype=torch.bfloat16, device=a.device)
    if out.shape != (m, n) or out.dtype != torch.bfloat16 or out.stride(1) != 1 or not out.is_cuda:
        raise RuntimeError('gemm_nn: out must be a bf16 [M, N] GPU matrix with unit column stride')
    if bias is not None:
        bias = _gpu(bias, 'bias').float().contiguous()
    if splits is None:
        splits = gemm_nn_splits(m, k, n)
    if splits > 1 and (n % 4 or out.stride(0) % 4 or out.data_ptr() % 8):
        splits = 1
    ws = torch.empty(splits * m * n, dtype=torch.float32, device=a.device) if splits > 1 else None
    _launch(timer_class, lambda: lib().ver_gemm_nn_splitk(
        _p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0), m, k, n, splits, _p(ws),
        ws.numel() * 4 if ws is not None else 0, _stream()), meta=dict(flops=2.0 * m * k * n))
    return out


def gemm_nn_taps_supported(lattice, layout, w, c):
    """What ``gemm_nn_taps`` takes: a contiguous bf16 lattice below 2 GiB in layout 0 / 2 / 3 with C % 32 == 0, a bf16 weight
    matrix with 16-byte aligned rows (``w`` None: the lattice side only, before the weights exist).  Any 2 H W."""
    return (lattice.is_cuda and lattice.dtype == torch.bfloat16 and lattice.is_contiguous() and layout in (PLAIN, ZSPLIT, PLANAR_ZSPLIT)
            and lattice.numel() * 2 < 2 ** 31 - 1 and c % 32 == 0 and c >= 64
            and (w is None or (w.is_cuda and w.dtype == torch.bfloat16 and w.dim() == 2 and w.stride(1) == 1 and w.stride(0) % 8 == 0
                               and w.data_ptr() % 16 == 0)))


def gemm_nn_taps(lattice, layout, combined_hw, taps, w, rowpos=None, bias=None, out=None, const_rows=None, planes=None,
                 timer_class='ver_gemm_nn'):
    """ver_gemm_nn_segments: ``tap_matrix(lattice) @ w (+ rowpos by row position) (+ bias)`` without the tap matrix: lattice
    bf16 in layout 0 / 2 / 3 (see ``lattice_gather``), rows = the cells (b, zl, y, x) of the combined (H, W) lattice.  ``taps``:
    the segments of the K axis in order -- (dz in {0, 2}, dy, dx) = the C channels of that neighbouring cell, or ('c', block) =
    the columns of constant-pattern block ``block`` of ``const_rows`` bf16 [2 H W, blocks, width] (what ``lattice_gather``
    copies into every viewpoint's rows).  w bf16 [sum of the segment widths, N] -> bf16 [B * 2 * H * W, N].
    ``planes`` = list with the source plane of every tap: ``lattice`` is then [planes, ...] -- several lattices of one shape
    (the four class planes of a layer's output gradient), tap t reads ``lattice[planes[t]]``."""
    lat, w = _gpu(lattice, 'lattice'), _gpu(w, 'w')
    plane_elems = nplanes = 0
    if planes is not None:
        nplanes, plane_elems = int(lat.shape[0]), int(lat[0].numel())
        if len(planes) != len(taps) or not lat.is_contiguous():
            raise ValueError('gemm_nn_taps: one source plane per tap, contiguous planes')
    lat_one = lat[0] if planes is not None else lat
    B, H, W, C, const_rows, ncst, cw, kdim, arr, ntaps = _segment_args(lat_one, layout, combined_hw, taps, const_rows, 'gemm_nn_taps')
    if not gemm_nn_taps_supported(lat_one, int(layout), w, C):
        raise RuntimeError('gemm_nn_taps: unsupported operands %s layout %d / %s %s' % (tuple(lat.shape), layout, tuple(w.shape), w.stride()))
    m, n = B * 2 * H * W, w.shape[1]
    if w.shape[0] != kdim:
        raise ValueError('gemm_nn_taps: w has %d rows, the segments span %d columns' % (w.shape[0], kdim))
    if out is None:
        out = torch.empty(m, n, dtype=torch.bfloat16, device=lat.device)
    if out.shape != (m, n) or out.dtype != torch.bfloat16 or out.stride(1) != 1 or not out.is_cuda:
        raise RuntimeError('gemm_nn_taps: out must be a bf16 [M, N] GPU matrix with unit column stride')
    if rowpos is not None:
        rowpos = _gpu(rowpos, 'rowpos').float().contiguous()
        if tuple(rowpos.shape) != (2 * H * W, n):
            raise ValueError('gemm_nn_taps: rowpos must be [2 H W, N]')
    if bias is not None:
        bias = _gpu(bias, 'bias').float().contiguous()
    parr = (ctypes.c_int * ntaps)(*[int(v) for v in planes]) if planes is not None else None
    _launch(timer_class, lambda: lib().ver_gemm_nn_planes(
        _p(lat), layout, B, H, W, C, plane_elems, nplanes, parr, arr, ntaps, _p(const_rows), ncst, cw, _p(w), w.stride(0),
        _p(rowpos), _p(bias), _p(out), out.stride(0), n, _stream()), meta=dict(flops=2.0 * m * w.shape[0] * n))
    return out


def _segment_args(lat, layout, combined_hw, taps, const_rows, name):
    H, W = combined_hw
    B, _, C = _lattice_dims(lat, int(layout))
    ncst = cw = 0
    if const_rows is not None:
        const_rows = _gpu(const_rows, 'const_rows')
        if not (const_rows.is_contiguous() and const_rows.dtype == torch.bfloat16 and const_rows.dim() == 3 and const_rows.shape[0] == 2 * H * W):
            raise ValueError('%s: const_rows must be a contiguous bf16 [2 H W, blocks, width] table' % name)
        ncst, cw = int(const_rows.shape[1]), int(const_rows.shape[2])
    taps = [((-1 - int(t[1]), 0, 0) if t[0] == 'c' else t) for t in taps]
    kdim = sum(cw if t[0] < 0 else C for t in taps)
    flat = [int(v) for t in taps for v in t]
    return B, H, W, C, const_rows, ncst, cw, kdim, (ctypes.c_int * len(flat))(*flat), len(taps)


# rows per viewpoint (2 H W) ver_wgrad_tn_segments takes: its four per-wave offset tables of 2 H W ints sit next to the 128-KiB
# operand ring in LDS, and 128 KiB + 4 x 4 x 2 048 B is all of a gfx950 CU's 160 KiB (csrc/ver_wgrad.hip)
WGRAD_SEGMENTS_ROWS = (16, 2048)


def wgrad_tn_segments_supported(lattice, layout, combined_hw, c, const_width, g):
    """What ``wgrad_tn_segments`` takes -- the library's rules: 16 <= 2 H W <= 2 048 rows per viewpoint of the combined (H, W)
    lattice, segment widths multiples of 64, the lattice below 2 GiB; ``g`` None: the lattice side only (a layer's forward
    pass decides before its output gradient exists)."""
    H, W = combined_hw
    return (WGRAD_SEGMENTS_ROWS[0] <= 2 * H * W <= WGRAD_SEGMENTS_ROWS[1]
            and lattice.is_cuda and lattice.dtype == torch.bfloat16 and lattice.is_contiguous() and layout in (PLAIN, ZSPLIT, PLANAR_ZSPLIT)
            and lattice.numel() * 2 < 2 ** 31 - 1 and c % 64 == 0 and const_width % 64 == 0
            and (g is None or (g.is_cuda and g.dtype == torch.bfloat16 and g.dim() == 2 and g.stride(1) == 1 and g.stride(0) % 8 == 0
                               and g.data_ptr() % 16 == 0 and g.shape[1] % 4 == 0)))


def wgrad_tn_segments(lattice, layout, combined_hw, taps, g, out_dtype=None, out=None, const_rows=None, splits=0):
    """ver_wgrad_tn_segments: ``tap_matrix(lattice).t() @ g`` without the tap matrix (operands as ``gemm_nn_taps``): the weight
    gradient of a lattice layer's class GEMM, [sum of the segment widths, N] in ``out_dtype`` (``out``: a matrix to write into)."""
    lat, g = _gpu(lattice, 'lattice'), _gpu(g, 'g')
    B, H, W, C, const_rows, ncst, cw, ka, arr, nseg = _segment_args(lat, layout, combined_hw, taps, const_rows, 'wgrad_tn_segments')
    if not wgrad_tn_segments_supported(lat, int(layout), (H, W), C, cw, g):
        raise RuntimeError('wgrad_tn_segments: unsupported operands %s layout %d / %s %s' % (tuple(lat.shape), layout, tuple(g.shape), g.stride()))
    if g.shape[0] != B * 2 * H * W:
        raise ValueError('wgrad_tn_segments: g has %d rows, %d cells' % (g.shape[0], B * 2 * H * W))
    n = g.shape[1]
    out_dtype = out_dtype or (out.dtype if out is not None else lat.dtype)
    if out is None:
        out = torch.empty(ka, n, dtype=out_dtype, device=lat.device)
    elif not (out.is_cuda and out.shape == (ka, n) and out.dtype == out_dtype and out.stride(1) == 1):
        raise RuntimeError('wgrad_tn_segments: out must be a [Ka, N] GPU matrix of out_dtype with unit column stride')
    L = lib()
    if splits <= 0:
        splits = L.ver_wgrad_tn_segments_splits(B, H, W, ka, n, g.stride(0))
    ws = torch.empty(splits * ka * n, dtype=torch.float32, device=lat.device)
    _launch('ver_wgrad_tn', lambda: L.ver_wgrad_tn_segments(
        _p(lat), layout, B, H, W, C, arr, nseg, _p(const_rows), ncst, cw, _p(g), g.stride(0), n, _p(out), out.stride(0),
        1 if out_dtype == torch.bfloat16 else 0, splits, _p(ws), ws.numel() * 4, _stream()), meta=dict(flops=2.0 * g.shape[0] * ka * n))
    return out
