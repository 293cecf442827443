"""fp64 model and deterministic inputs for the four general-shape sampling kernels of csrc/ver_msda.hip (test_msda_forms_cpu.py,
test_msda_forms_gpu.py): ``k_msda_fwd`` / ``k_msda_bwd`` behind ``MultiScaleDeformableAttnFunction_fp32`` and ``k_msda3d_fwd`` /
``k_msda3d_bwd`` behind ``hipops.voxel_msda``.  Pure torch / numpy on the CPU; nothing here ever sees a kernel's output.

The model (``model``): ``oracle.ver_oracle.msda_core`` (dim 2) / ``voxel_msda_core`` (dim 3) and their autograd on ``.double()``
copies of the fp32 operands, then the kernels' strict gate on the location gradient: ``grad_loc`` of a sample is zero unless
``-1 < pixel < size`` on every axis (pixel = loc * size - 0.5).  The gate changes one point per axis only: at a pixel coordinate
of exactly -1 the corner at 0 has weight 0 and a non-zero location gradient, which the oracle's autograd (and, in 3-D,
``F.grid_sample``) returns and the kernels -- like mmcv's 2-D op -- do not (include/ver_ops.h at ``ver_msda3d_*``;
test_msda_forms_cpu.py holds both halves).  Everywhere else outside the gate every quantity is zero both ways.

The kernels come in eight lane forms, chosen by ``dispatch_group(head_dim)``; ``WIDTHS`` holds the last width of each form
and the first, ragged, width of the next (``form`` names the form of a width).

Inputs:
  * ``random_case``: 78 (batch, query, head) groups -- with 32, 16, 8 or 4 groups per 256-thread block every form runs several
    full blocks plus a ragged one, over two batches -- on three levels, one of them a single pixel.  Locations are uniform in
    [-0.25, 1.25] and GATE-STABLE: no fp64 pixel coordinate has a fractional part within ``MARGIN`` of 0 or 1 (those that
    had were moved by a quarter pixel), so the fp32 kernel and the fp64 model take the same ``floor`` and the same gate whether
    or not the compiler contracts ``loc * size - 0.5`` into one fused multiply-add.
  * ``edge_case``: levels with power-of-two sizes and ``loc = (t + 0.5) / size`` for pixel coordinates t that are multiples of
    1/4, so that loc, loc * size and t are exact in fp32 under either contraction (asserted).  The coordinate sets hold the
    integer coordinates (a corner of weight 0 with a non-zero gradient), both padding borders, the gate values -1 and
    ``size`` and the one-pixel axes.
  * ``collide_case``: one single-pixel level, so that every sample's ``grad_value`` atomics land on the one key of its head.

Bounds (the project's existing ones, tests/test_hip_ops_gpu.py): forward ``maxdiff < 2e-5``, gradients ``util.close`` (1e-4 +
1e-5 |b|).  ``ratios`` returns the worst ratio of each quantity to its bound; test_msda_forms_cpu.py checks that the fp32 CPU
oracle stays under a quarter of each on every input built here, so that the bounds measure the kernels and not the inputs."""
import functools
import importlib

import numpy as np
import torch

WIDTHS = (1, 8, 9, 16, 17, 32, 33, 64, 65, 96, 97, 128, 129, 192, 193, 256)
EDGE_WIDTHS = (5, 32, 96)
MARGIN = 1e-3
FWD_BOUND = 2e-5
ATOL, RTOL = 1e-4, 1e-5
LEVELS = {2: [[1, 1], [3, 5], [5, 4]], 3: [[1, 1, 1], [2, 3, 5], [1, 2, 2]]}          # (H, W) / (D, H, W)
EDGE_LEVELS = {2: [[4, 8], [1, 2]], 3: [[2, 4, 8], [1, 1, 2]]}
QUANTITIES = ('out', 'grad_value', 'grad_loc', 'grad_attn')


def oracle():
    return importlib.import_module('oracle.ver_oracle')


def form(head_dim):
    """(G, NC) of ``dispatch_group``: G lanes own one output row, each lane NC channels G apart."""
    for top, f in ((8, (8, 1)), (16, (16, 1)), (32, (32, 1)), (64, (64, 1)), (96, (32, 3)), (128, (64, 2)), (192, (64, 3)),
                   (256, (64, 4))):
        if head_dim <= top:
            return f
    raise ValueError(head_dim)


def sizes_of(dim, shapes):
    """[L, dim] float64: the size along x, y (, z) of every level -- shapes rows are (H, W) / (D, H, W)."""
    return torch.as_tensor(shapes, dtype=torch.float64).view(-1, dim).flip(-1)


def pixels(dim, shapes, loc):
    """fp64 pixel coordinates [B, Nq, heads, L, P, dim] of fp32 (or fp64) locations: loc * size - 0.5."""
    return loc.double() * sizes_of(dim, shapes)[:, None, :] - 0.5


def in_gate(dim, shapes, loc):
    """bool [B, Nq, heads, L, P]: -1 < pixel < size on every axis (false for a NaN)."""
    pix = pixels(dim, shapes, loc)
    size = sizes_of(dim, shapes)[:, None, :]
    return ((pix > -1.0) & (pix < size)).all(-1)


def core(dim):
    return oracle().msda_core if dim == 2 else oracle().voxel_msda_core


def autograd(dim, value, shapes, loc, attn, grad_out, dtype):
    """out and the three gradients of the oracle's core op with every operand cast to ``dtype``; no gate applied."""
    v, l, a = (t.detach().to(dtype).requires_grad_(True) for t in (value, loc, attn))
    out = core(dim)(v, [list(map(int, s)) for s in torch.as_tensor(shapes).tolist()], l, a)
    out.backward(grad_out.to(dtype))
    return dict(out=out.detach(), grad_value=v.grad, grad_loc=l.grad, grad_attn=a.grad)


def gated(dim, shapes, loc, res):
    """``res`` with the kernels' strict gate on grad_loc."""
    res = dict(res)
    res['grad_loc'] = torch.where(in_gate(dim, shapes, loc)[..., None], res['grad_loc'], torch.zeros((), dtype=res['grad_loc'].dtype))
    return res


def model(dim, value, shapes, loc, attn, grad_out):
    """float64 ``out``, ``grad_value``, ``grad_loc``, ``grad_attn`` of the op on the fp32 operands (module docstring)."""
    return gated(dim, shapes, loc, autograd(dim, value, shapes, loc, attn, grad_out, torch.float64))


def ratios(got, want):
    """{quantity: worst ratio to its bound} of ``got`` against the model ``want``: |out - model| / 2e-5 and, for the gradients,
    |a - b| / (1e-4 + 1e-5 |b|) -- a ratio below 1 is ``maxdiff < 2e-5`` / ``util.close``.  NaN if ``got`` holds one."""
    res = {}
    for k in QUANTITIES:
        a, b = torch.as_tensor(got[k]).detach().double().cpu(), want[k].double()
        assert a.shape == b.shape, (k, a.shape, b.shape)
        d = (a - b).abs()
        r = d / FWD_BOUND if k == 'out' else d / (ATOL + RTOL * b.abs())
        res[k] = float('nan') if bool(torch.isnan(r).any()) else float(r.max())
    return res


def _near_edge(pix):
    frac = pix - torch.floor(pix)
    return (frac < MARGIN) | (frac > 1.0 - MARGIN)


def gate_stable(dim, shapes, loc):
    """(fp32 locations with no pixel coordinate within MARGIN of an integer, the number of coordinates moved): a coordinate that
    was is moved by a quarter of a pixel."""
    size = sizes_of(dim, shapes)[:, None, :]
    near = _near_edge(pixels(dim, shapes, loc))
    out = torch.where(near, loc.double() + 0.25 / size, loc.double()).float()
    assert not bool(_near_edge(pixels(dim, shapes, out)).any())
    return out, int(near.sum())


def _operands(dim, shapes, loc, heads, head_dim, gen):
    """value and grad_out N(0,1), attn a softmax over L * P of N(0,1), the int64 shape / level-start tensors."""
    bsz, nq, _, nlev, npt, _ = loc.shape
    sh = torch.tensor(shapes, dtype=torch.int64).view(-1, dim)
    count = sh.prod(1)
    value = torch.randn(bsz, int(count.sum()), heads, head_dim, generator=gen)
    attn = torch.randn(bsz, nq, heads, nlev * npt, generator=gen).softmax(-1).view(bsz, nq, heads, nlev, npt)
    grad_out = torch.randn(bsz, nq, heads * head_dim, generator=gen)
    lsi = torch.cat([torch.zeros(1, dtype=torch.int64), count.cumsum(0)[:-1]])
    return dict(dim=dim, value=value, shapes=sh, level_start=lsi, loc=loc, attn=attn, grad_out=grad_out, head_dim=head_dim)


def with_model(c):
    c['model'] = model(c['dim'], c['value'], c['shapes'], c['loc'], c['attn'], c['grad_out'])
    c['gate'] = in_gate(c['dim'], c['shapes'], c['loc'])
    return c


@functools.lru_cache(maxsize=None)
def random_case(dim, head_dim, seed=0):
    """B = 2, Nq = 13, heads = 3, P = 4 on ``LEVELS[dim]`` (module docstring); computed once, shared, not to be modified."""
    gen = torch.Generator(device='cpu').manual_seed(1000 * seed + 10 * head_dim + dim)
    shapes = LEVELS[dim]
    loc = torch.rand(2, 13, 3, len(shapes), 4, dim, generator=gen) * 1.5 - 0.25
    loc, moved = gate_stable(dim, shapes, loc)
    assert moved < 0.05 * loc.numel(), '%d of %d coordinates moved' % (moved, loc.numel())
    c = _operands(dim, shapes, loc, 3, head_dim, gen)
    c['moved'] = moved
    return with_model(c)


def edge_coordinates(size, full):
    """pixel coordinates of one axis: every multiple of 1/4 from -1.25 to size + 0.25 (``full``) or the reduced set."""
    if full:
        return [k / 4.0 for k in range(-5, 4 * size + 2)]
    return sorted({-1.25, -1.0, -0.5, 0.0, 0.25, 1.0, size - 1.0, size - 0.75, size - 0.5, float(size), size + 0.25})


@functools.lru_cache(maxsize=None)
def edge_case(dim, head_dim=EDGE_WIDTHS[0]):
    """The product of the coordinate sets (x full, y and z reduced) of every level of ``EDGE_LEVELS[dim]``, packed into queries
    of P = 4; B = 1, heads = 2 (the second head takes the list one sample later, so that its queries pack other samples
    together).  A level with fewer products than the largest repeats its list.  Also returns ``pix``: the exact pixel coordinates [B, Nq, heads, L, P, dim]."""
    shapes = EDGE_LEVELS[dim]
    per_level = []
    for s in shapes:
        axes = [edge_coordinates(int(n), i == 0) for i, n in enumerate(reversed(s))]                # x, y (, z)
        grid = torch.cartesian_prod(*[torch.tensor(a, dtype=torch.float64) for a in axes]).view(-1, dim)
        per_level.append(grid)
    n = max(g.shape[0] for g in per_level)
    nq = (n + 3) // 4
    pix = torch.empty(1, nq, 2, len(shapes), 4, dim, dtype=torch.float64)
    for lvl, g in enumerate(per_level):
        for h in range(2):
            idx = (torch.arange(nq * 4) + h) % g.shape[0]
            pix[0, :, h, lvl] = g[idx].view(nq, 4, dim)
    size = sizes_of(dim, shapes)[:, None, :]
    loc = ((pix + 0.5) / size).float()
    # exact in fp32 either way: the product rounded and then the difference rounded, or one rounding of the fused multiply-add
    l32, s32 = loc.numpy(), size.float().numpy()
    two_step = (l32 * s32).astype(np.float32) - np.float32(0.5)
    fused = (l32.astype(np.float64) * s32.astype(np.float64) - 0.5).astype(np.float32)
    assert two_step.dtype == np.float32
    assert np.array_equal(two_step.astype(np.float64), pix.numpy()) and np.array_equal(fused.astype(np.float64), pix.numpy())
    assert np.array_equal(loc.double().numpy(), ((pix + 0.5) / size).numpy())
    gen = torch.Generator(device='cpu').manual_seed(77 + 10 * head_dim + dim)
    c = _operands(dim, shapes, loc, 2, head_dim, gen)
    c['pix'] = pix
    return with_model(c)


@functools.lru_cache(maxsize=None)
def collide_case(dim):
    """One single-pixel level, B = 1, Nq = 64, heads = 2, head_dim = 64, P = 4; pixel coordinates uniform in (-0.9, 0.9)."""
    gen = torch.Generator(device='cpu').manual_seed(300 + dim)
    shapes = [[1] * dim]
    loc = (torch.rand(1, 64, 2, 1, 4, dim, generator=gen) * 2.0 - 1.0) * 0.9 + 0.5
    loc, moved = gate_stable(dim, shapes, loc)
    assert moved < 0.05 * loc.numel()
    pix = pixels(dim, shapes, loc)
    assert float(pix.abs().max()) < 0.9 + 0.25 + 1e-6 and bool(in_gate(dim, shapes, loc).all())
    return with_model(_operands(dim, shapes, loc, 2, 64, gen))


def interior_integer(c):
    """bool [B, Nq, heads, L, P] of an ``edge_case``: the sample is inside the gate and has, on some axis, an integer pixel
    coordinate strictly inside the map (1 <= t <= size - 2): there the far corner of that axis has weight 0 and a non-zero
    gradient."""
    pix = c['pix']
    size = sizes_of(c['dim'], c['shapes'])[:, None, :]
    inner = (pix == torch.floor(pix)) & (pix >= 1.0) & (pix <= size - 2.0)
    return inner.any(-1) & c['gate']
