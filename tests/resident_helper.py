"""Shared by tests/test_resident_cpu.py, tests/test_resident_gpu.py and tests/test_resident_graph_gpu.py: a tiny hand-made
viewpoint store, seeded random stores as plain numpy tables (the arguments of ``hipops.fetch_batch_host``), and the
comparison of a fetch against that model."""
import numpy as np
import torch

T = torch.from_numpy
SENTINEL = -77                                # what output tables are pre-filled with where a fetch must leave them alone
KEYS = ('feats', 'world2pixel', 'origin', 'boxes', 'labels', 'counts', 'pairs', 'pair_offsets')


def hand_store():
    """Three viewpoints, two cameras, rows of three: feats[v, c, r] = 100 v + 10 c + r; 3, 0 and 1 boxes of two numbers;
    3, 0 and 2 pairs."""
    v, c, r = np.meshgrid(np.arange(3), np.arange(2), np.arange(3), indexing='ij')
    feats = (100 * v + 10 * c + r).astype(np.float32)
    w2p = np.stack([np.stack([np.full((4, 4), 10 * a + b + 1, np.float32) for b in range(2)]) for a in range(3)])
    origin = np.array([[0, 0.5, -0.0], [1, 1.5, -1], [2, 2.5, -2]], np.float32)
    boxes = np.zeros((3, 3, 2), np.float32)
    labels = np.zeros((3, 3), np.int64)
    boxes[0] = [[0, -0.0], [1, -1], [2, -2]]
    labels[0] = [1, 2, 3]
    boxes[2, 0] = [20, -20]
    labels[2, 0] = 21
    counts = np.array([3, 0, 1], np.int32)
    pairs = np.array([[1, 1], [2, 2], [3, 3], [20, 5], [21, 6]], np.int32)
    pair_offsets = np.array([0, 3, 3, 5], np.int64)
    return dict(feats=feats, world2pixel=w2p, origin=origin, boxes=boxes, labels=labels, counts=counts, pairs=pairs,
                pair_offsets=pair_offsets)


def random_store(seed, V, ncam, row, bits=32, store_cap=5, box_dim=9, lens=None):
    """Seeded tables of ``V`` viewpoints.  The features are random BIT patterns (int32 for f32, int16 for bf16: the fetch is a
    pure copy, so NaN patterns are welcome and the comparison is on the integers); counts cover 0 .. store_cap; ``lens``:
    the pair count of every viewpoint (default: random below 40, one of them 0)."""
    rng = np.random.default_rng(seed)
    ftype = np.int32 if bits == 32 else np.int16
    info = np.iinfo(ftype)
    feats = rng.integers(info.min, info.max, size=(V, ncam, row), dtype=ftype, endpoint=True)
    counts = rng.integers(0, store_cap + 1, size=V).astype(np.int32)
    if store_cap and V > 1:
        counts[0], counts[1] = store_cap, 0
    boxes = rng.standard_normal((V, store_cap, box_dim)).astype(np.float32)
    labels = rng.integers(0, 17, size=(V, store_cap)).astype(np.int64)
    if lens is None:
        lens = rng.integers(1, 40, size=V)
        lens[rng.integers(V)] = 0
    lens = np.asarray(lens, dtype=np.int64)
    total = int(lens.sum())
    pairs = np.stack([rng.integers(0, 504000, size=total), rng.integers(0, 16, size=total)], axis=1).astype(np.int32)
    return dict(feats=feats, world2pixel=rng.standard_normal((V, ncam, 4, 4)).astype(np.float32),
                origin=rng.standard_normal((V, 3)).astype(np.float32), boxes=boxes, labels=labels, counts=counts,
                pairs=pairs, pair_offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))


def feature_tensor(bits_array, device, shift=0):
    """The feature bit patterns as an f32 / bf16 tensor on ``device``; ``shift``: elements the base address is moved by (out
    of a larger allocation), which takes the 16-byte alignment of the base away."""
    dtype = torch.float32 if bits_array.dtype == np.int32 else torch.bfloat16
    flat = torch.empty(bits_array.size + shift, dtype=dtype, device=device)
    view = flat[shift:].view(bits_array.shape)
    view.copy_(T(bits_array).view(dtype))
    return view


def bits(t):
    """A float tensor's bit patterns as a numpy integer array."""
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
