"""The host side of the flat gradient exchange (``ddp.GradExchange``, ``ver_grad_pack``, ``ver_clip_adamw_step_flat``): the
layout function, the numpy model of the bf16 wire rounding against torch's own conversion, the two prototypes and their
argument checks, and the claim the preset loss normalisers of ``graphs.GraphedTrainStep(exchange=)`` rest on."""
import ctypes
import re

import numpy as np
import pytest
import torch

from util import pkg

SIZES = (1, 7, 8, 9, 32769)


def test_flat_layout_aligns_and_does_not_overlap():
    ddp = pkg('ddp')
    for sizes in ([n] for n in SIZES):
        offsets, total = ddp.flat_layout(sizes)
        assert offsets == [0] and total == -(-sizes[0] // 8) * 8
    for sizes in (SIZES, SIZES[::-1], (9, 9, 9), (8, 1, 8)):
        offsets, total = ddp.flat_layout(sizes)
        assert len(offsets) == len(sizes) and offsets[0] == 0
        assert all(o % 8 == 0 for o in offsets) and total % 8 == 0
        ends = [o + n for o, n in zip(offsets, sizes)]
        assert all(e <= nxt for e, nxt in zip(ends, offsets[1:] + [total]))          # in order, no overlap
        assert all(nxt - e < 8 for e, nxt in zip(ends, offsets[1:] + [total]))        # and no more padding than needed
        assert total == sum(-(-n // 8) * 8 for n in sizes)
    assert ddp.flat_layout(SIZES) == ([0, 8, 16, 24, 40], 40 + 32776)
    assert ddp.flat_layout([]) == ([], 0)
    with pytest.raises(ValueError):
        ddp.flat_layout([4, -1])


def _specials():
    f32 = np.float32
    tiny = np.array([1, 2, 0x7fff, 0x8000, 0x8001, 0x007fffff, 0x00800000, 0x00017fff, 0x00018000], dtype=np.uint32).view(f32)
    values = np.concatenate([
        np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -9, 1 + 2.0 ** -7, 1 + 2.0 ** -8 + 2.0 ** -20,
                  1 + 2.0 ** -8 - 2.0 ** -20, 3.0, 1 / 3, 1e-3, 255.5, 256.5], dtype=f32),
        np.array([np.finfo(f32).max, 3.3895e38, 3.38e38, np.finfo(f32).tiny], dtype=f32), tiny,
        np.array([0.0, np.inf, np.nan], dtype=f32), np.random.default_rng(0).standard_normal(4096).astype(f32)])
    return np.concatenate([values, -values])


@pytest.mark.parametrize('scale', [1.0, 1 / 2, 1 / 3, 1 / 8])
def test_pack_host_rounds_as_torch_does(scale):
    hip = pkg('hipops')
    g = _specials()
    prod = torch.from_numpy(g) * torch.tensor(scale, dtype=torch.float32)
    got32 = hip.pack_host(g, scale, torch.float32)
    assert got32.dtype == np.float32 and np.array_equal(got32.view(np.uint32), prod.numpy().view(np.uint32))
    got = hip.pack_host(g, scale, torch.bfloat16)
    want = prod.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert got.dtype == np.uint16 and got.shape == want.shape
    nan = np.isnan(prod.numpy())
    assert nan.sum() == 2
    assert np.array_equal(got[~nan], want[~nan])                           # signed zeros, infinities, denormals: bit patterns
    assert np.all((got[nan] & 0x7fff) > 0x7f80) and np.all((want[nan] & 0x7fff) > 0x7f80)   # a NaN stays a NaN
    assert np.all(got[nan] == 0x7fc0)
    if scale == 1.0:                                                       # the named cases, spelled out
        one = lambda v: int(hip.pack_host(np.float32(v), 1.0, torch.bfloat16)[0])
        assert one(1 + 2.0 ** -8) == 0x3f80 and one(1 + 3 * 2.0 ** -8) == 0x3f82           # ties go to the even mantissa
        assert one(np.finfo(np.float32).max) == 0x7f80 and one(-np.finfo(np.float32).max) == 0xff80
        assert one(0.0) == 0 and one(-0.0) == 0x8000 and one(np.inf) == 0x7f80 and one(-np.inf) == 0xff80
        assert one(np.array([1], dtype=np.uint32).view(np.float32)[0]) == 0
    with pytest.raises(TypeError):
        hip.pack_host(g, 1.0, torch.float16)


def test_header_declares_both_entry_points_and_the_abi_stays_31():
    hip = pkg('hipops')
    text = open(hip.HEADER).read()
    assert re.search(r'#define\s+VER_ABI_VERSION\s+31\b', text)
    protos = hip.prototypes()
    p, i, f, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long
    assert protos['ver_grad_pack'] == (i, [p, p, p, p, p, i, i, i, f, p, i, p])
    assert protos['ver_clip_adamw_step_flat'] == (i, [p, p, p, p, p, p, p, p, i, i, i, i, p, p, f, p])
    assert 'ver_grad_pack' in hip.SYMBOLS and 'ver_clip_adamw_step_flat' in hip.SYMBOLS
    pkg('csrc.build').build_hip(verbose=False)
    lib = hip.lib()
    assert lib.ver_abi_version() == 31 == hip.ABI_VERSION


def test_argument_errors_without_a_gpu():
    hip = pkg('hipops')
    pkg('csrc.build').build_hip(verbose=False)
    lib = hip.lib()
    buf = (ctypes.c_char * 256)()
    a = ctypes.addressof(buf) & ~15                                        # any non-null address: rejected before any use
    a += 16
    pack = lambda flat, dtype, n=1, c=1, chunk=32768: lib.ver_grad_pack(a, a, a, a, a, n, c, chunk, 1.0, flat, dtype, None)
    flat = lambda flat, dtype, n=1, c=1, chunk=32768: lib.ver_clip_adamw_step_flat(a, a, a, a, a, a, a, flat, dtype, n, c, chunk,
                                                                                   a, None, 1.0, None)
    for call, name in ((pack, b'ver_grad_pack'), (flat, b'ver_clip_adamw_step_flat')):
        assert call(None, 0) == -1 and b'null' in lib.ver_last_error() and name in lib.ver_last_error()
        assert call(a, 2) == -1 and b'flat_dtype 2' in lib.ver_last_error() and name in lib.ver_last_error()
        assert call(a, -1) == -1 and b'flat_dtype' in lib.ver_last_error()
        assert call(a, 0, n=-1) == -1 and b'bad sizes' in lib.ver_last_error()
        assert call(a, 0, c=-1) == -1 and b'bad sizes' in lib.ver_last_error()
        assert call(a, 1, chunk=6) == -1 and b'bad sizes' in lib.ver_last_error()
        assert call(a + 4, 1) == -1 and b'16-byte' in lib.ver_last_error()
        assert call(None, 0, n=0) == 0 and call(None, 1, c=0) == 0          # nothing to do: VER_OK without a launch
    assert lib.ver_grad_pack(None, a, a, a, a, 1, 1, 32768, 1.0, a, 0, None) == -1 and b'null' in lib.ver_last_error()
    assert lib.ver_clip_adamw_step_flat(a, a, None, a, a, a, a, a, 0, 1, 1, 32768, a, None, 1.0, None) == -1
    assert b'null' in lib.ver_last_error()


def test_a_solved_problem_matches_min_count_queries():
    """What the preset normalisers of ``GraphedTrainStep(exchange=)`` count: a solved assignment problem with ``count`` boxes
    matches exactly ``min(count, Nq)`` queries, so ``clamp(counts, max=Nq).sum()`` IS the number of matches."""
    head_mod = pkg('dense_heads.voxelformer_occupancy_head')
    nq, layers = 6, 2
    counts = (0, 3, nq, nq + 5)
    cost = np.random.default_rng(1).standard_normal((layers, len(counts), nq, nq + 5))
    idx = head_mod.VoxelFormerOccupancyHead._solve_on_host(cost, list(counts))
    assert idx.shape == (layers, len(counts), nq)
    matched = (idx >= 0).sum(2)
    want = torch.tensor(counts).clamp(max=nq)
    assert np.array_equal(matched, np.broadcast_to(want.numpy(), matched.shape))
    assert int(matched[0].sum()) == int(want.sum()) == 0 + 3 + nq + nq
    for b, n in enumerate(counts):                                           # distinct boxes, all inside the count
        cols = idx[0, b][idx[0, b] >= 0]
        assert len(set(cols.tolist())) == len(cols) and (cols < max(n, 1)).all()
