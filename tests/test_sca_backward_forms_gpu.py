"""Every launch form of ``ver_sca_backward`` (csrc/ver_sca.hip) against the oracle in float64, and hand-made hit tables
on the fast kernels (``k_sca_fwd_cs``, ``k_sca_bwd_mm``, the two-kernel fp32 backward).  Needs an MI355X: ``-m gpu``.

Reference: ``util.oracle_slots`` evaluated in float64 on the CPU and autograd of it.  bf16 cases feed it the SAME
bf16-rounded value and grad rows the kernel gets, so only the kernel's own arithmetic is measured.

d(offsets) is discontinuous where a sample's pixel coordinate crosses an integer (the bilinear cell changes), and an fp32
kernel may put such a sample into the neighbouring cell: the (voxel, head, point, camera) samples whose float64 pixel x or
y lies within 1e-4 of an integer are left out of the d(offsets) comparison -- nothing else is, and nothing is left out of
slots, d(value) or d(logits), which are continuous.  Their share is asserted <= 0.1 % in every case (expected 4e-4 with
offsets ~ 3 N(0,1): two coordinates x a window of 2e-4).

Bounds (the project's, by what the kernel computes in; none is fitted to a measured error):
  fp32 value tiles      slots max |d| < 2e-5; gradients ``close()`` at its defaults (1e-4 + 1e-5 |ref|).
  bf16 value tiles      the bounds of test_sca_gather_bf16_value: slots max |d| < 1e-2 and rel. L2 < 2e-3 (packed-fp16
                        accumulation of the corner-slot forward); d(value) -- rounded to bf16 once, at the end --
                        ``close(atol = 1e-3 max|ref|, rtol = 2^-8)`` and rel. L2 < 2e-3; d(offsets) / d(logits) ``close()``
                        at its defaults (fp32 grad rows split hi + lo: 16 mantissa bits).
  bf16 grad rows        VER_SCA_GRAD_SLOTS_BF16: the row is the matrix operand as given, one bf16 term per element, and the
                        fp32-row kernel's ``lo`` operand is zero on the same rows; adding exact zero products changes no
                        fp32 MFMA accumulation, so the three gradients must be ``torch.equal`` to those of the fp32-row
                        kernel run on the same bf16-representable rows, and hold the bf16-value bounds against float64 plus
                        rel. L2 < 2e-3 on every gradient -- with every visible voxel seen by 1, 2, 4 or 8 cameras and with
                        counts of 3, 5, 6 or 7 alike.  (These bounds are inside ``close(atol = 2^-8 max|ref|, rtol = 2^-8)``,
                        the element-wise allowance for one more bf16 rounding per grad element at the odd counts.  The
                        kernel used to need it: it scaled the ROW by 1 / count, which rounds in bf16 for 3, 5, 6, 7, and
                        d(value) -- already rounded once on the way out, rel. L2 1.65e-3 -- came to 2.03e-3 with every
                        voxel seen by 6 cameras and 1.83e-3 with counts of 3 and 5, past the 2e-3 of ONE rounding.  The
                        factor now rides on the sample's fp32 weight.)
Every case prints its measured figures, and all cases of a test are run and printed before the first assertion."""
import numpy as np
import pytest
import torch

from sca_modes_helper import random_sca_case
from util import close, maxdiff, oracle, oracle_slots, pkg, rel_l2

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda'
BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------ reference
def _near_integer(offsets, uv, mask, map_hw):
    """Samples at a cell edge.  offsets [B,Nq,heads,P,2] (pixels), uv [B,Ncam,Nq,D,2], mask bool [B,Ncam,Nq] (all CPU).
    Returns (bool [B,Nq,heads,P]: a visible camera's sample of this d(offsets) entry has its float64 pixel x or y within
    1e-4 of an integer; the share of such samples among the (voxel, head, point, visible camera) samples)."""
    mh, mw = map_hw
    heads, P, D = offsets.shape[2], offsets.shape[3], uv.shape[3]
    norm = torch.tensor([float(mw), float(mh)], dtype=torch.float64)
    u = uv.double()[:, :, :, torch.arange(P) % D, :]                       # point p samples around anchor p % D
    pix = (u[:, :, :, None] + offsets.double()[:, None] / norm) * norm - 0.5  # [B,Ncam,Nq,heads,P,2], as msda_core forms it
    near = ((pix - pix.round()).abs() < 1e-4).any(-1) & mask[:, :, :, None, None]
    samples = int(mask.sum()) * heads * P
    return near.any(1), float(near.sum()) / max(samples, 1)


def _reference(value, offsets, logits, uv, mask, map_hw, grads):
    """float64 oracle: slots and, per grad in ``grads``, (d value, d offsets, d logits).  value: CPU tensor holding exactly
    what the kernel reads (bf16-rounded for a bf16 case), reference layout [B,Ncam,Nk,heads,hd]."""
    vc = value.double().requires_grad_(True)
    oc = T(offsets).double().requires_grad_(True)
    lc = T(logits).double().requires_grad_(True)
    ref = oracle_slots(oracle(), vc, oc, lc, uv.double(), mask, map_hw)
    out = []
    for g in grads:
        gs = torch.autograd.grad(ref, (vc, oc, lc), g.double(), retain_graph=True, allow_unused=True)
        out.append(tuple(torch.zeros_like(x) if y is None else y for x, y in zip((vc, oc, lc), gs)))
    return ref.detach(), out


# ------------------------------------------------------------------------------------------ the code under test
def _run(hit, value, offsets, logits, grad, map_hw, head_major=False, lowp_out=False):
    """Forward and backward through ``hipops.sca_gather``.  value: device tensor, reference layout; grad: device tensor in
    the dtype the consumer hands back (bf16 with ``lowp_out``).  Returns slots, d(value) (reference layout), d(offsets),
    d(logits) on the CPU and the launch meta of the one ``ver_sca_backward`` call."""
    hip = pkg('hipops')
    v = (value.permute(3, 0, 1, 2, 4).contiguous() if head_major else value.clone()).requires_grad_(True)
    of = T(offsets).to(DEV).requires_grad_(True)
    lg = T(logits).to(DEV).requires_grad_(True)
    before, timer = hip.KERNEL_TIMER, hip.KernelTimer()
    hip.KERNEL_TIMER = timer
    try:
        slots = hip.sca_gather(v, of, lg, hit, map_hw[0], map_hw[1], None, head_major, lowp_out)
        slots.backward(grad)
        torch.cuda.synchronize()
    finally:
        hip.KERNEL_TIMER = before
    metas = [m for name, _, _, m in timer.records if name == 'ver_sca_backward']
    assert len(metas) == 1
    gv = v.grad.permute(1, 2, 3, 0, 4) if head_major else v.grad
    assert gv.dtype == value.dtype and gv.shape == value.shape
    return dict(slots=slots.detach().cpu(), gv=gv.cpu(), go=of.grad.cpu(), gl=lg.grad.cpu(), meta=metas[0])


def _abi_backward(hit, value, offsets, logits, grad, map_hw, gdt, flags, head_major=False):
    """``ver_sca_backward`` at the C ABI with d(value) pre-filled with NaN: every element must be written.  value in the
    reference layout (handed over head-major with ``head_major``); d(value) always comes back in the reference layout."""
    hip = pkg('hipops')
    lib, p = hip.lib(), hip._p
    B, ncam, _, heads, hd = value.shape
    if head_major:
        value, flags = value.permute(3, 0, 1, 2, 4).contiguous(), flags | 2
    of, lg = T(offsets).to(DEV), T(logits).to(DEV)
    gv = torch.full((B, ncam, map_hw[0] * map_hw[1], heads, hd), float('nan'), dtype=BF16 if gdt == 1 else F32, device=DEV)
    go, gl = torch.empty_like(of), torch.empty_like(lg)
    rc = lib.ver_sca_backward(p(value), 1 if value.dtype == BF16 else 0, p(of), p(lg), p(hit.uv), p(hit.vis), p(hit.vis_list),
                              p(hit.vis_cnt), p(hit.fwd_list), p(hit.fwd_cnt), p(grad), p(gv), gdt, p(go), p(gl), B, ncam,
                              hit.Nq, hit.D, heads, hd, logits.shape[-1], map_hw[0], map_hw[1], flags, hip._stream())
    assert rc == 0, lib.ver_last_error()
    torch.cuda.synchronize()
    return gv.cpu(), go.cpu(), gl.cpu()


# ------------------------------------------------------------------------------------------ judging
def _norm_err(a, b, atol, rtol):
    """max |a-b| / (atol + rtol |b|): <= 1 is ``close(a, b, atol, rtol)``."""
    a, b = a.double(), b.double()
    return float(((a - b).abs() / (atol + rtol * b.abs())).max())


class _Report:
    def __init__(self):
        self.bad = []

    def line(self, case, what, ok, text):
        print('%s %s: %s%s' % (case, what, text, '' if ok else '   <-- FAILS'))
        if not ok:
            self.bad.append('%s %s: %s' % (case, what, text))

    def judge(self, case, kind, got, ref, ref_grads, skip_off, unseen):
        """kind: 'f32' | 'bf16' (bf16 value, d(value) rounded to bf16 once) | 'bf16_rows' (the same bounds, and rel. L2 <
        2e-3 on every gradient).  skip_off: the d(offsets) entries with a sample at a cell edge."""
        rgv, rgo, rgl = ref_grads
        d, rel = maxdiff(got['slots'], ref), rel_l2(got['slots'], ref)
        ok = d < 2e-5 if kind == 'f32' else (d < 1e-2 and rel < 2e-3)
        self.line(case, 'slots', ok, 'max |d| %.3g, rel. L2 %.3g' % (d, rel))
        ggo = torch.where(skip_off[..., None], rgo.to(got['go'].dtype), got['go'])
        for what, g, r in (('d(value)', got['gv'].float(), rgv), ('d(offsets)', ggo, rgo), ('d(logits)', got['gl'], rgl)):
            d, rel, top = maxdiff(g, r), rel_l2(g, r), float(r.abs().max())
            if kind != 'f32' and what == 'd(value)':
                atol, rtol, l2 = 1e-3 * top, 2.0 ** -8, 2e-3
            else:
                atol, rtol, l2 = 1e-4, 1e-5, 2e-3 if kind == 'bf16_rows' else None
            ne = _norm_err(g, r, atol, rtol)
            ok = close(g, r, atol=atol, rtol=rtol) and (l2 is None or rel < l2)
            self.line(case, what, ok, 'max |d| %.3g, rel. L2 %.3g, worst |d| / (%.3g + %.3g |ref|) = %.3g'
                      % (d, rel, atol, rtol, ne))
        if bool(unseen.any()):
            z = max(float(got[k][unseen].abs().max()) for k in ('slots', 'go', 'gl'))
            self.line(case, 'unseen voxels', z == 0.0, 'max |slots|, |d(offsets)|, |d(logits)| %.3g' % z)

    def equal(self, case, a, b, why, rows=None):
        """torch.equal of the three gradients; rows (bool [B,Nq]): the voxels whose d(offsets) / d(logits) are compared."""
        for k in ('gv', 'go', 'gl'):
            x, y = (a[k], b[k]) if rows is None or k == 'gv' else (a[k][rows], b[k][rows])
            same = torch.equal(x, y)
            self.line(case, 'bit-equality of %s (%s)' % (k, why), same,
                      'equal' if same else 'max |d| %.3g' % maxdiff(x.float(), y.float()))


def _one_camera_of(hit, c):
    """The hit table with the work lists of every camera but ``c`` emptied; the visibility bytes (the camera counts) stay."""
    hip = pkg('hipops')
    one = hip.HitTable(hit.B, hit.Ncam, hit.Nq, hit.D, hit.vis.device)
    for k in hip.HitTable.__slots__[:8]:
        getattr(one, k).copy_(getattr(hit, k))
    keep = torch.zeros(hit.Ncam, dtype=torch.bool, device=hit.vis.device)
    keep[c] = True
    one.fwd_cnt[:, ~keep] = 0
    one.vis_cnt[:, ~keep] = 0
    return one


def _same_up_to_add_order(a, b, few):
    """Two runs of one kernel: d(offsets) / d(logits) rows of voxels seen by <= 2 cameras (``few`` bool [B,Nq]) bitwise, the
    others -- summed over the cameras by fp32 atomics in arrival order -- within the bound the determinism test of the
    forward holds such rows to (8 * 2^-24 * max |.|, test_sca_gather_three_camera_overlap_determinism_bound)."""
    return torch.equal(a[few], b[few]) and maxdiff(a, b) <= 8 * 2.0 ** -24 * float(b.abs().max())


def _counts_are_powers_of_two(mask):
    cnt = mask.sum(1)
    return bool(((cnt == 0) | (cnt == 1) | (cnt == 2) | (cnt == 4) | (cnt == 8)).all())


def _check_case(rep, case, hit, mask, value, offsets, logits, gslots, map_hw, vdtype, rows, head_major=False):
    """One gather problem on fp32 or bf16 value tiles.  rows: 'f32' -- full-precision fp32 grad rows; 'bf16' -- the grad
    comes back in bf16 (``lowp_out``), and the fp32-row kernel is run on the same rows as the bit-equality partner."""
    lib = pkg('hipops').lib()
    heads, hd, P = value.shape[3], value.shape[4], logits.shape[-1]
    uv = hit.uv.cpu()
    vdev = T(value).to(DEV).to(vdtype)
    g32 = T(gslots)
    gbf = g32.bfloat16()
    grads = [g32] * ('f32' in rows) + [gbf.float()] * ('bf16' in rows)
    ref, ref_grads = _reference(vdev.float().cpu(), offsets, logits, uv, mask, map_hw, grads)
    skip_off, share = _near_integer(T(offsets), uv, mask, map_hw)
    rep.line(case, 'd(offsets) samples at a cell edge', share <= 1e-3, 'share %.3g (%d entries left out)' % (share, int(skip_off.sum())))
    unseen = ~mask.any(1)
    gdt = lib.ver_sca_backward_grad_dtype(1 if vdtype == BF16 else 0, hd, P, map_hw[0], map_hw[1])
    kind = 'f32' if vdtype == F32 else 'bf16'
    if 'f32' in rows:
        got = _run(hit, vdev, offsets, logits, g32.to(DEV), map_hw, head_major)
        rep.line(case, 'fp32 rows: launch', got['meta']['grad_slots_bf16'] is False and got['slots'].dtype == F32, str(got['meta']))
        rep.judge(case + ' [fp32 rows]', kind, got, ref, ref_grads[0], skip_off, unseen)
    if 'bf16' in rows:
        assert vdtype == BF16 and gdt == 1
        rg = ref_grads[-1]
        got = _run(hit, vdev, offsets, logits, gbf.to(DEV), map_hw, head_major, lowp_out=True)
        part = _run(hit, vdev, offsets, logits, gbf.float().to(DEV), map_hw, head_major)
        rep.line(case, 'bf16 rows: launch', got['meta']['grad_slots_bf16'] is True and part['meta']['grad_slots_bf16'] is False
                 and got['slots'].dtype == BF16 and torch.equal(got['slots'], part['slots'].bfloat16()),
                 '%s, slots %s = the fp32 slots rounded' % (got['meta'], got['slots'].dtype))
        got['slots'] = part['slots']            # (judged in fp32: the bf16 copy is that tensor rounded, just asserted)
        pow2 = _counts_are_powers_of_two(mask)
        rep.judge(case + ' [fp32 kernel on the bf16 rows]', 'bf16', part, ref, rg, skip_off, unseen)
        rep.judge(case + ' [bf16 rows, camera counts %s]' % ('in {1,2,4,8}' if pow2 else 'include 3, 5, 6 or 7'),
                  'bf16_rows', got, ref, rg, skip_off, unseen)
        # Bit-equality, for every camera count.  d(value) is summed inside one workgroup, in list order.  d(offsets) /
        # d(logits) of a voxel are summed over its cameras by fp32 atomics from different workgroups (include/ver_ops.h:
        # reproducible up to two cameras, with more the last bit follows the arrival order): the voxels seen by <= 2 cameras
        # are compared in the full launch, and the contribution of every single camera -- at the full camera count -- with
        # the other cameras' lists emptied.
        few = mask.sum(1) <= 2
        rep.equal(case, got, part, 'bf16 rows against the fp32-row kernel on the same rows', few)
        if not bool(few.all()):
            for c in range(mask.shape[1]):
                one = _one_camera_of(hit, c)
                a = dict(zip(('gv', 'go', 'gl'), _abi_backward(one, vdev, offsets, logits, gbf.to(DEV), map_hw, 1, 4, head_major)))
                b = dict(zip(('gv', 'go', 'gl'), _abi_backward(one, vdev, offsets, logits, gbf.float().to(DEV), map_hw, 1, 0, head_major)))
                rep.equal(case, a, b, 'camera %d alone' % c)
    return gdt


# ------------------------------------------------------------------------------------------ A. forms by shape
# The forms of the backward's launcher, each reached by SHAPE (the kernel a row names is what one kernel trace over this
# file showed: profiles/README.md).  B = 2 viewpoints unless a grid needs one chunk boundary only; P = 8.
# name: (heads, head_dim, grid, B, map, value dtype, grad rows, head-major value, dtype of d(value) at the C ABI)
_SCA_BWD_FORMS = {
    # k_sca_bwd_mm<128, 196, bf16>: NT = 8, KS = 4, SEG = 16
    'mm_hd128': (1, 128, (2, 6, 5), 2, (14, 14), BF16, ('f32',), False, 1),
    # k_sca_bwd_mm<HD, 196, bf16, 4, bf16>: grad rows in bf16, single-term operands (what bf16 autocast runs)
    'mm_gbf_196_hd32': (2, 32, (3, 7, 6), 2, (14, 14), BF16, ('bf16',), False, 1),
    'mm_gbf_196_hd96': (8, 96, (3, 7, 6), 2, (14, 14), BF16, ('bf16',), False, 1),
    # ... on the head-major value layout: the benchmark's instantiation
    'mm_gbf_head_major': (8, 96, (4, 15, 15), 2, (14, 14), BF16, ('bf16',), True, 1),
    # k_sca_bwd_mm<HD, 0, ...>, run-time map size: 7 tile-row tiles with 13 slack rows; 16 tiles without slack; one tile
    'mm_rt_99': (2, 64, (2, 6, 5), 2, (9, 11), BF16, ('f32', 'bf16'), False, 1),
    'mm_rt_256_hd128': (1, 128, (2, 6, 5), 2, (16, 16), BF16, ('f32', 'bf16'), False, 1),
    'mm_rt_256_hd32': (2, 32, (2, 6, 5), 2, (16, 16), BF16, ('f32', 'bf16'), False, 1),
    'mm_rt_15': (2, 32, (2, 6, 5), 2, (3, 5), BF16, ('f32',), False, 1),
    # the matrix-core kernel's operand pipeline over ~20 chunks of 32 voxels per camera
    'mm_many_chunks': (2, 32, (5, 30, 30), 1, (14, 14), BF16, ('f32', 'bf16'), False, 1),
    # map beyond 256 rows, head_dim % 32 == 0: past both fast paths into k_sca_bwd<32, 16, 8, VT> (LDS atomics)
    'big_map_bf16': (2, 32, (2, 6, 5), 2, (17, 17), BF16, ('f32',), False, 0),
    'big_map_f32': (2, 32, (2, 6, 5), 2, (17, 17), F32, ('f32',), False, 0),
    # 4 500 voxels: k_sca_bwd_off over 3 list chunks of 2 048 + k_sca_bwd_val over 2 chunks of 4 096 (zero fill, atomic flush)
    'two_kernel_chunked': (2, 32, (5, 30, 30), 1, (14, 14), F32, ('f32',), False, 0),
    # k_sca_bwd<8, 4, 8, float> over 2 chunks
    'lds_atomic_chunked': (4, 8, (5, 30, 30), 1, (14, 14), F32, ('f32',), False, 0),
}


def test_sca_backward_forms_by_shape():
    """Forward and backward of every form of _SCA_BWD_FORMS through ``hipops.sca_gather`` against the float64 oracle,
    bounds as in the module docstring.  big_map_bf16 computes in fp32 from bf16 tiles and autograd rounds its fp32
    d(value) to the dtype of value: the bf16-value bounds apply to it as they do to the matrix-core kernel."""
    rep = _Report()
    for form, (heads, hd, grid, B, mhw, vdtype, rows, head_major, want_gdt) in _SCA_BWD_FORMS.items():
        # (the seed is one at which every form's share of cell-edge samples -- a property of the inputs alone -- is inside
        #  the 0.1 % cap: at the 60-voxel grids that cap is ONE sample, and at the expected 4e-4 a form often draws two)
        hit, value, offsets, logits, gslots = random_sca_case(54, B, grid, heads, hd, 8, map_hw=mhw)
        mask = hit.mask()[:, :, :, 0].permute(1, 0, 2).cpu()
        gdt = _check_case(rep, form, hit, mask, value, offsets, logits, gslots, mhw, vdtype, rows, head_major)
        rep.line(form, 'd(value) dtype at the C ABI', gdt == want_gdt, '%d' % gdt)
    assert not rep.bad, '\n'.join(rep.bad)


def test_sca_backward_beyond_lds_is_loud():
    """bf16 value, head_dim 128, 17x17 map, 8 points: the forward runs; the backward has no matrix-core form (19 tile-row
    tiles) and the LDS-atomic kernel would need 289 * 128 * 6 B > 160 KiB: VER_EUNSUPPORTED with a message, no launch."""
    hip = pkg('hipops')
    lib, p = hip.lib(), hip._p
    hit, value, offsets, logits, gslots = random_sca_case(5, 1, (2, 6, 5), 1, 128, 8, map_hw=(17, 17))
    vb, of, lg, gs = T(value).to(DEV).bfloat16(), T(offsets).to(DEV), T(logits).to(DEV), T(gslots).to(DEV)
    slots = hip.sca_gather(vb, of, lg, hit, 17, 17)
    assert bool(torch.isfinite(slots).all()) and float(slots.abs().max()) > 0.0
    assert lib.ver_sca_backward_grad_dtype(1, 128, 8, 17, 17) == 0
    gv, go, gl = torch.zeros(vb.shape, device=DEV), torch.empty_like(of), torch.empty_like(lg)
    rc = lib.ver_sca_backward(p(vb), 1, p(of), p(lg), p(hit.uv), p(hit.vis), p(hit.vis_list), p(hit.vis_cnt), p(hit.fwd_list),
                              p(hit.fwd_cnt), p(gs), p(gv), 0, p(go), p(gl), 1, 6, hit.Nq, 1, 1, 128, 8, 17, 17, 0, hip._stream())
    torch.cuda.synchronize()
    assert rc == -2                                                        # VER_EUNSUPPORTED
    assert b'exceed LDS' in lib.ver_last_error()
    assert float(gv.abs().max()) == 0.0                                    # nothing wrote d(value)


# ------------------------------------------------------------------------------------------ B. hand-made hit tables
def _mask_from_groups(ncam, nq, D, views, seed):
    """bev_mask bool [Ncam, B, Nq, D].  views: per viewpoint a list of (cameras, count): ``count`` voxels seen by exactly
    these cameras, so every per-camera count is exact by construction; voxel ids are dealt from a fixed permutation (the
    lists are built in ascending id order, not in group order).  D > 1: the anchors through which a (voxel, camera) pair
    is visible walk through the non-empty subsets of the anchors, so the mask differs per anchor."""
    mask = np.zeros((ncam, len(views), nq, D), dtype=bool)
    rng = np.random.default_rng(seed)
    k = 0
    for b, groups in enumerate(views):
        ids, at = rng.permutation(nq), 0
        for cams, cnt in groups:
            for n in ids[at:at + cnt]:
                for c in cams:
                    sub = 1 + k % (2 ** D - 1)
                    k += 1
                    mask[c, b, n] = [(sub >> d) & 1 for d in range(D)]
            at += cnt
        assert at <= nq
    return mask


def _fwd_counts(ncam, views):
    """[B][Ncam] (n_single, n_multi) of the groups."""
    return [[(sum(n for cams, n in groups if cams == (c,)), sum(n for cams, n in groups if c in cams and len(cams) > 1))
             for c in range(ncam)] for groups in views]


_ALL6, _ALL8 = tuple(range(6)), tuple(range(8))
# name: (Ncam, D, Nq, views)
_MASK_SETS = {
    # viewpoint 0: camera 0 sees nothing; camera 1 only voxels of its own (n_multi == 0); camera 2 only shared ones
    # (n_single == 0); n_single = 9, 1, 7, 8 on cameras 1, 3, 4, 5.  viewpoint 1: n_single rounded up to 8, plus n_multi,
    # = 32, 33, 64, 65 on cameras 0..3 (the boundaries of the operand pipeline: total > 32, e0 + 64 < total).
    # Every visible voxel is seen by 1, 2 or 4 cameras.
    'regions': (6, 1, 96, [
        [((1,), 9), ((3,), 1), ((4,), 7), ((5,), 8), ((2, 3, 4, 5), 20)],
        [((0,), 5), ((1,), 9), ((2,), 16), ((3,), 3), ((0, 1, 2, 3), 17), ((0, 2, 3, 4), 7), ((2, 3), 24), ((3, 5), 9)]]),
    # voxels seen by all 6 cameras, by 3 and by 5 (1/6, 1/3, 1/5 round in bf16); a viewpoint where every camera sees all
    'all_of_6': (6, 1, 80, [
        [(_ALL6, 20), ((0, 1, 2), 10), ((1, 2, 3, 4, 5), 10), ((0,), 5), ((3,), 7)],
        [(_ALL6, 80)]]),
    'one_camera': (1, 1, 80, [[((0,), 37)], [((0,), 80)]]),
    # bit 7 of the visibility byte: voxels only camera 7 sees, and voxels all 8 see (1/8 is exact)
    'eight_cameras': (8, 1, 88, [
        [(_ALL8, 24), ((7,), 11), ((6, 7), 10), ((0,), 5)],
        [(_ALL8, 40), ((7,), 3), ((0, 1, 2, 3), 9)]]),
    # anchors: point p samples around anchor p % D; viewpoint 1 of 'anchors_2' leaves cameras 1, 2, 3 blind
    'anchors_2': (6, 2, 80, [
        [((0,), 12), ((1, 2), 15), ((3,), 9), ((2, 4), 11), ((0, 1, 3, 5), 10)],
        [((5,), 20), ((0, 5), 13), ((4,), 1)]]),
    'anchors_4': (6, 4, 80, [
        [((0, 1, 2), 14), ((3,), 10), ((1, 4, 5), 9), ((2,), 12), ((0, 1, 2, 3, 4), 6)],
        [((0, 3), 21), ((1, 2, 4), 17)]]),
}


def test_mask_sets_hold_the_conditions_they_are_named_for():
    """The per-camera counts of _MASK_SETS, spelled out (the cases below rely on them)."""
    reg = _fwd_counts(6, _MASK_SETS['regions'][3])
    assert reg[0] == [(0, 0), (9, 0), (0, 20), (1, 20), (7, 20), (8, 20)]
    assert [((s + 7) & ~7) + m for s, m in reg[1][:4]] == [32, 33, 64, 65]
    assert _fwd_counts(8, _MASK_SETS['eight_cameras'][3])[0][7] == (11, 34)
    assert _fwd_counts(6, _MASK_SETS['all_of_6'][3])[1] == [(0, 80)] * 6
    for name, pow2 in (('regions', True), ('all_of_6', False), ('one_camera', True), ('eight_cameras', True),
                       ('anchors_2', True), ('anchors_4', False)):
        ncam, D, nq, views = _MASK_SETS[name]
        m = T(_mask_from_groups(ncam, nq, D, views, 3)).any(-1).permute(1, 0, 2)
        assert _counts_are_powers_of_two(m) == pow2, name


@pytest.mark.parametrize('name,mhw', [('regions', (14, 14)), ('regions', (9, 11)), ('all_of_6', (14, 14)),
                                      ('one_camera', (14, 14)), ('eight_cameras', (14, 14)), ('anchors_2', (14, 14)),
                                      ('anchors_4', (14, 14))])
def test_sca_gather_hand_made_hit_tables(name, mhw):
    """heads 2, head_dim 32, 8 points on the hit table of a mask set: fp32 value (k_sca_fwd_cs + the two-kernel backward),
    bf16 value with fp32 and with bf16 grad rows (k_sca_fwd_cs + k_sca_bwd_mm), forward and backward against float64; the
    lists hold the counts the set was built for; at the C ABI every element of a NaN-filled d(value) is written, the tile
    of a camera that sees nothing as exact zeros, and the numbers are those autograd hands back."""
    hip = pkg('hipops')
    ncam, D, nq, views = _MASK_SETS[name]
    heads, hd, P, B, nk = 2, 32, 8, len(views), mhw[0] * mhw[1]
    rng = np.random.default_rng(71)
    bev = _mask_from_groups(ncam, nq, D, views, 3)
    uv = rng.uniform(-0.1, 1.1, (ncam, B, nq, D, 2)).astype(np.float32)
    hit = hip.hits_from_mask(T(uv).to(DEV), T(bev).to(DEV))
    value = rng.standard_normal((B, ncam, nk, heads, hd)).astype(np.float32)
    offsets = (rng.standard_normal((B, nq, heads, P, 2)) * 3.0).astype(np.float32)
    logits = rng.standard_normal((B, nq, heads, P)).astype(np.float32)
    gslots = rng.standard_normal((B, nq, heads * hd)).astype(np.float32)
    mask = T(bev).any(-1).permute(1, 0, 2)
    want = _fwd_counts(ncam, views)
    assert hit.fwd_cnt.cpu().tolist() == [[list(sm) for sm in row] for row in want]
    assert maxdiff(hit.uv.cpu(), T(uv).permute(1, 0, 2, 3, 4)) == 0.0
    rep = _Report()
    case = '%s %dx%d' % (name, mhw[0], mhw[1])
    _check_case(rep, case + ' fp32 value', hit, mask, value, offsets, logits, gslots, mhw, F32, ('f32',))
    _check_case(rep, case + ' bf16 value', hit, mask, value, offsets, logits, gslots, mhw, BF16, ('f32', 'bf16'))
    # C ABI, NaN-filled d(value)
    blind = (~mask.any(2)).nonzero().tolist()                              # [viewpoint, camera] pairs
    gbf = T(gslots).bfloat16()
    for what, vdt, grad, gdt, flags in (('fp32 value', F32, T(gslots), 0, 0), ('bf16 value, fp32 rows', BF16, T(gslots), 1, 0),
                                        ('bf16 value, bf16 rows', BF16, gbf, 1, 4)):
        vdev = T(value).to(DEV).to(vdt)
        gv, go, gl = _abi_backward(hit, vdev, offsets, logits, grad.to(DEV), mhw, gdt, flags)
        via = _run(hit, vdev, offsets, logits, grad.to(DEV), mhw, lowp_out=bool(flags & 4))
        ok = bool(torch.isfinite(gv.float()).all()) and all(float(gv[b, c].float().abs().max()) == 0.0 for b, c in blind)
        rep.line(case, 'C ABI, %s: d(value) written in full, %d blind tiles zero' % (what, len(blind)), ok, str(ok))
        # (csrc/ver_sca.hip, head comment: the matrix-core kernel's d(value) is bitwise reproducible; the fp32 path's counting
        #  sort leaves the order of a tile row's events open, so its last bits may differ run to run: fp32 gradient tolerance)
        few = mask.sum(1) <= 2
        same = torch.equal(gv, via['gv']) if vdt == BF16 else close(gv, via['gv'])
        same = same and _same_up_to_add_order(go, via['go'], few) and _same_up_to_add_order(gl, via['gl'], few)
        rep.line(case, 'C ABI, %s: the numbers autograd hands back' % what, same, str(same))
    assert not rep.bad, '\n'.join(rep.bad)
