"""``ver_fetch_batch`` (csrc/ver_fetch.hip) and ``resident.ResidentStore`` on the GPU against the numpy model
``hipops.fetch_batch_host``, bit for bit: every access width of the feature copy (row bytes and base addresses that allow 16, 8,
4 and 2 bytes), permuted / repeated / out-of-range indices, absent groups, box tables and pair tables whose cells behind the
counts keep a sentinel, pair segments around the copy's tile, capacities around the total, element offsets and CSR offsets past
2^31, capture and replay with changing index contents, and the host-fed assembly of vocc-sized viewpoints."""
import warnings

import numpy as np
import pytest
import torch

import cases
from resident_helper import SENTINEL, T, bits, feature_tensor, random_store, same_bits
from util import pkg

warnings.filterwarnings('ignore')
pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
V = 7
INDEX_SETS = ([3], [6, -1, 0], [2, 2, V, 5, 0, 6, -1, 1])       # bs 1, 3, 8: a permutation with repeats, and -1 and V


def _device_tables(store, shift=0):
    d = {k: T(store[k]).to(DEV) for k in store if k != 'feats'}
    d['feats'] = feature_tensor(store['feats'], DEV, shift)
    return d


def _outputs(store, bs, out_cap, pair_cap, shift=0):
    """Output tensors of a fetch, the box and pair tables pre-filled with the sentinel; the feature output out of a larger
    allocation when ``shift`` moves its base."""
    ncam, row = store['feats'].shape[1:]
    fdt = torch.float32 if store['feats'].dtype == np.int32 else torch.bfloat16
    flat = torch.full((ncam * bs * row + shift,), float(SENTINEL), dtype=fdt, device=DEV)
    return dict(feats=flat[shift:].view(ncam, bs, row), world2pixel=torch.full((bs, ncam, 4, 4), float(SENTINEL), device=DEV),
                origin=torch.full((bs, 3), float(SENTINEL), device=DEV),
                boxes=torch.full((bs, out_cap, store['boxes'].shape[2]), float(SENTINEL), device=DEV),
                labels=torch.full((bs, out_cap), SENTINEL, dtype=torch.int64, device=DEV),
                counts=torch.full((bs,), SENTINEL, dtype=torch.int32, device=DEV),
                offsets=torch.full((bs + 1,), SENTINEL, dtype=torch.int32, device=DEV),
                pairs=torch.full((pair_cap, 2), SENTINEL, dtype=torch.int32, device=DEV),
                status=torch.full((4,), SENTINEL, dtype=torch.int32, device=DEV))


def _fetch(hip, index, dev, out, groups=('feats', 'cameras', 'boxes', 'pairs')):
    idx = torch.tensor(index, dtype=torch.int32, device=DEV)
    kw = {}
    if 'feats' in groups:
        kw['feats'] = (dev['feats'], out['feats'])
    if 'cameras' in groups:
        kw['cameras'] = (dev['world2pixel'], dev['origin'], out['world2pixel'], out['origin'])
    if 'boxes' in groups:
        kw['boxes'] = (dev['boxes'], dev['labels'], dev['counts'], out['boxes'], out['labels'], out['counts'])
    if 'pairs' in groups:
        kw['pairs'] = (dev['pairs'], dev['pair_offsets'], out['offsets'], out['pairs'])
    status = hip.fetch_batch(idx, dev['counts'].shape[0], status=out['status'], **kw)
    torch.cuda.synchronize()
    assert status is out['status']


def _model(hip, index, store, out_cap, pair_cap, groups=('feats', 'cameras', 'boxes', 'pairs')):
    """The model on the same tables, the box and pair tables starting from the sentinel as the device's do."""
    bs = len(index)
    kw = {}
    if 'feats' in groups:
        kw['feats'] = store['feats']
    if 'cameras' in groups:
        kw.update(world2pixel=store['world2pixel'], origin=store['origin'])
    if 'boxes' in groups:
        kw.update(boxes=store['boxes'], labels=store['labels'], counts=store['counts'], out_cap=out_cap)
    if 'pairs' in groups:
        kw.update(pairs=store['pairs'], pair_offsets=store['pair_offsets'], pair_capacity=pair_cap)
    prev = dict(boxes=np.full((bs, out_cap, store['boxes'].shape[2]), SENTINEL, np.float32),
                labels=np.full((bs, out_cap), SENTINEL, np.int64), pairs=np.full((pair_cap, 2), SENTINEL, np.int32))
    return hip.fetch_batch_host(index, V=store['counts'].shape[0], out=prev, **kw)


def _same(out, want, untouched=()):
    """Every output the model lists equals it bit for bit; the outputs named in ``untouched`` still hold the sentinel."""
    for k, w in want.items():
        got = bits(out[k]) if k == 'feats' else out[k].cpu().numpy()
        assert same_bits(got, w), (k, got, w)
    for k in untouched:
        assert k not in want and bool((out[k] == SENTINEL).all()), k


@pytest.mark.parametrize('bits_', [32, 16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('row', [1, 3, 4, 1000, 196 * 768])
@pytest.mark.parametrize('ncam', [1, 6])
def test_fetch_equals_the_model_for_every_row_width(ncam, row, bits_):
    """V = 7.  Row bytes 2 and 6 (bf16 rows of 1 and 3) allow 2-byte accesses only, 4 and 12 allow 4, 8 allows 8, 16 and the
    larger rows 16; a base moved by one element takes the wider accesses away from the rows that had them."""
    hip = pkg('hipops')
    store = random_store(1000 * ncam + row + bits_, V, ncam, row, bits_)
    total = int(store['pair_offsets'][-1])
    for shift in (0, 1):
        dev = _device_tables(store, shift)
        assert dev['feats'].data_ptr() % 16 == (shift * bits_ // 8)
        for index in INDEX_SETS:
            out = _outputs(store, len(index), 5, total, shift)
            _fetch(hip, index, dev, out)
            _same(out, _model(hip, index, store, 5, total))


@pytest.mark.parametrize('absent', ['feats', 'cameras', 'boxes', 'pairs'])
def test_an_absent_group_leaves_the_others_alone(absent):
    hip = pkg('hipops')
    store = random_store(5, V, 2, 24, 32)
    dev = _device_tables(store)
    index = INDEX_SETS[2]
    groups = tuple(g for g in ('feats', 'cameras', 'boxes', 'pairs') if g != absent)
    out = _outputs(store, len(index), 4, 50)
    _fetch(hip, index, dev, out, groups)
    want = _model(hip, index, store, 4, 50, groups)
    assert want['status'][0] == 2
    _same(out, want, untouched=dict(feats=['feats'], cameras=['world2pixel', 'origin'], boxes=['boxes', 'labels', 'counts'],
                                    pairs=['offsets', 'pairs'])[absent])


@pytest.mark.parametrize('out_cap', [3, 5, 8])
@pytest.mark.parametrize('store_cap', [0, 5])
def test_box_tables_keep_what_lies_behind_the_counts(store_cap, out_cap):
    hip = pkg('hipops')
    store = random_store(11 + store_cap, V, 1, 4, 32, store_cap=store_cap)
    dev = _device_tables(store)
    index = [0, 1, 4, V, 0, 3]
    out = _outputs(store, len(index), out_cap, 8)
    _fetch(hip, index, dev, out, ('boxes',))
    want = _model(hip, index, store, out_cap, 8, ('boxes',))
    _same(out, want)
    counts = want['counts']
    assert counts.tolist() == [min(int(store['counts'][v]), out_cap) if 0 <= v < V else 0 for v in index]
    assert want['status'].tolist() == [1, sum(int(store['counts'][v]) > out_cap for v in index if 0 <= v < V), 0, 0]
    boxes, labels = out['boxes'].cpu().numpy(), out['labels'].cpu().numpy()
    for b, n in enumerate(counts):
        assert (boxes[b, n:] == SENTINEL).all() and (labels[b, n:] == SENTINEL).all()
        if n:
            assert np.array_equal(boxes[b, :n], store['boxes'][index[b], :n]) and np.array_equal(labels[b, :n], store['labels'][index[b], :n])


def test_pair_segments_around_the_tile_and_capacities_around_the_total():
    hip = pkg('hipops')
    tile = hip.fetch_pair_tile()
    lens = [0, 1, tile - 1, tile, tile + 1, 3 * tile + 5, 2]
    store = random_store(17, V, 1, 4, 32, lens=lens)
    dev = _device_tables(store)
    for index in ([5, 0, 2, 1, 3, 4], [4, 4, -1, 3], [0], [1, 6, 5]):
        total = sum(lens[v] for v in index if 0 <= v < V)
        for cap in sorted({0, max(total - 1, 0), total, total + 7}):
            out = _outputs(store, len(index), 1, cap)
            _fetch(hip, index, dev, out, ('pairs',))
            want = _model(hip, index, store, 1, cap, ('pairs',))
            _same(out, want)
            offsets, live = want['offsets'], min(total, cap)
            assert offsets[-1] == live and offsets.max() <= cap and (np.diff(offsets) >= 0).all()
            assert bool((out['pairs'][live:] == SENTINEL).all())                       # behind the live pairs
            assert want['status'].tolist() == [sum(not 0 <= v < V for v in index), 0, int(total > cap), total]
            assert out['status'].tolist() == want['status'].tolist()


def test_offsets_past_two_to_the_31():
    """Feature element offsets and CSR positions beyond int32: 2 400 vocc-sized f32 viewpoints (8.7 GB, uninitialised but for
    the first and last two) and a CSR of 2^31 + 4 096 pairs (17.2 GB, uninitialised but for the last 4 096)."""
    free = torch.cuda.mem_get_info(DEV)[0]
    if free < 40 * 2 ** 30:
        pytest.skip('%.1f GB of device memory free; the 8.7 GB feature store and the 17.2 GB pair table want 40' % (free / 2 ** 30))
    hip = pkg('hipops')
    rng = np.random.default_rng(31)
    nv, ncam, row = 2400, 6, 196 * 768
    assert (nv - 2) * ncam * row > 2 ** 31
    feats = torch.empty(nv, ncam, row, dtype=torch.float32, device=DEV)
    picked = [nv - 1, 0, nv - 2, 1]
    host = {v: rng.integers(-2 ** 31, 2 ** 31 - 1, size=(ncam, row), dtype=np.int32) for v in picked}
    for v, a in host.items():
        feats[v].copy_(T(a).view(torch.float32))
    out = torch.empty(ncam, 4, row, dtype=torch.float32, device=DEV)
    status = hip.fetch_batch(torch.tensor(picked, dtype=torch.int32, device=DEV), nv, feats=(feats, out))
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0, 0]
    assert same_bits(bits(out), np.stack([host[v] for v in picked], axis=1))
    del feats, out
    torch.cuda.empty_cache()
    big = 2 ** 31
    lens = [big, 1000, 2000, 1096]                              # viewpoint 0 owns the uninitialised 2^31 pairs and is never fetched
    pair_offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pairs = torch.empty(big + 4096, 2, dtype=torch.int32, device=DEV)
    tail = np.stack([rng.integers(0, 504000, 4096), rng.integers(0, 16, 4096)], axis=1).astype(np.int32)
    pairs[big:].copy_(T(tail))
    index = [3, 1, 2, 3]
    offsets = torch.full((5,), SENTINEL, dtype=torch.int32, device=DEV)
    got = torch.full((6000, 2), SENTINEL, dtype=torch.int32, device=DEV)
    status = hip.fetch_batch(torch.tensor(index, dtype=torch.int32, device=DEV), 4,
                             pairs=(pairs, T(pair_offsets).to(DEV), offsets, got))
    torch.cuda.synchronize()
    # the model on the last 4 096 pairs alone, their CSR moved down by 2^31 (viewpoint 0 empty there)
    want = hip.fetch_batch_host(index, pairs=tail, pair_offsets=np.array([0, 0, 1000, 3000, 4096]), pair_capacity=6000,
                                out=dict(pairs=np.full((6000, 2), SENTINEL, np.int32)))
    assert want['offsets'].tolist() == [0, 1096, 2096, 4096, 5192]
    assert same_bits(offsets.cpu().numpy(), want['offsets']) and same_bits(got.cpu().numpy(), want['pairs'])
    assert status.tolist() == want['status'].tolist() == [0, 0, 0, 5192]


def _small_store(res, feat_dtype=torch.float32):
    """Five small viewpoints in a ``ResidentStore`` on the GPU and the same tables as numpy."""
    tables = random_store(23, 5, 2, 32, 32, store_cap=4, lens=[40, 0, 9, 25, 3])
    store = res.ResidentStore(device=DEV, feat_dtype=feat_dtype)
    for v in range(5):
        lo, hi = tables['pair_offsets'][v], tables['pair_offsets'][v + 1]
        n = int(tables['counts'][v])
        store.append('s_v%d' % v, T(tables['feats'][v]).view(torch.float32).view(2, 4, 8), tables['world2pixel'][v], tables['origin'][v],
                     tables['boxes'][v, :n], tables['labels'][v, :n], tables['pairs'][lo:hi].astype(np.int64))
    return store.freeze(), tables


def test_store_on_the_gpu_and_capture_with_changing_indices():
    """``store.fetch(index_static, out=batch)`` captured once; three replays with three index contents, the second shorter in
    pairs than the first: each equals the model, and ``out=`` allocates nothing."""
    hip, res = pkg('hipops'), pkg('resident')
    store, tables = _small_store(res)
    assert store.feats.is_cuda and same_bits(bits(store.feats), tables['feats']) and store.max_boxes == 4
    assert all(same_bits(getattr(store, k).cpu().numpy(), tables[k]) for k in ('world2pixel', 'origin', 'counts', 'pairs', 'pair_offsets'))
    cap, pcap = 4, store.max_pairs(3)
    assert pcap == 74
    first = store.fetch([0, 3, 2])                                # a host list: pinned, asynchronous
    torch.cuda.synchronize()
    assert first.index.tolist() == [0, 3, 2] and first.occ.pairs.shape == (pcap, 2) and store.check(first) == (0, 0, 0, 74)
    batch = store.new_batch(3, cap, pcap)
    batch.gts.boxes.fill_(SENTINEL); batch.gts.labels.fill_(SENTINEL); batch.occ.pairs.fill_(SENTINEL)
    index = torch.zeros(3, dtype=torch.int32, device=DEV)
    store.fetch(index, out=batch)                                 # (warm-up outside the capture: library load, first launch)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = store.fetch(index, out=batch)
    assert captured.feats is batch.feats and captured.index is index and captured.status is batch.status
    prev = dict(boxes=batch.gts.boxes.cpu().numpy(), labels=batch.gts.labels.cpu().numpy(), pairs=batch.occ.pairs.cpu().numpy())
    kw = {k: tables[k] for k in tables}
    for contents in ([0, 3, 2], [4, 1, 2], [3, 7, 0]):            # 74 pairs, then 12, then 65 with an index outside the store
        index.copy_(torch.tensor(contents, dtype=torch.int32))
        before = torch.cuda.memory_allocated(DEV)
        graph.replay()
        assert torch.cuda.memory_allocated(DEV) == before
        torch.cuda.synchronize()
        want = hip.fetch_batch_host(contents, out_cap=cap, pair_capacity=pcap, out=prev, **kw)
        got = dict(feats=bits(batch.feats.reshape(2, 3, 32)), world2pixel=batch.world2pixel.cpu().numpy(), origin=batch.origin.cpu().numpy(),
                   boxes=batch.gts.boxes.cpu().numpy(), labels=batch.gts.labels.cpu().numpy(), counts=batch.gts.counts.cpu().numpy(),
                   offsets=batch.occ.offsets.cpu().numpy(), pairs=batch.occ.pairs.cpu().numpy(), status=batch.status.cpu().numpy())
        for k in want:
            assert same_bits(got[k], want[k]), (contents, k)
        prev = dict(boxes=got['boxes'], labels=got['labels'], pairs=got['pairs'])
    assert want['status'].tolist() == [1, 0, 0, 65] and want['offsets'].tolist() == [0, 25, 25, 65]
    # an eager fetch with out= allocates nothing either
    before = torch.cuda.memory_allocated(DEV)
    store.fetch(index, out=batch)
    assert torch.cuda.memory_allocated(DEV) == before
    with pytest.raises(ValueError, match='outside the store'):
        store.check(batch)


def test_fetch_equals_the_host_fed_assembly_of_vocc_viewpoints():
    """Three ``synthetic`` vocc-sized viewpoints with ``detection_gt`` boxes and sparse pairs: ``store.fetch([2, 0])`` against
    the stacked features, ``head.pad_gts`` and ``pack_occ_gts(...).to(device)``, bit for bit."""
    from infer_helper import head
    hip, res, syn = pkg('hipops'), pkg('resident'), pkg('synthetic')
    h = head()
    w2p, org = syn.camera_batch(3, seed=1)
    feats = syn.vit_features(3, seed=0)
    rng = np.random.default_rng(9)
    gt = [cases.detection_gt(seed=60 + v, num_gt=(4, 0, 6)[v]) for v in range(3)]
    pairs = [np.stack([rng.choice(h.voxel_num, size=k, replace=False), rng.integers(0, 16, k)], axis=1).astype(np.int64)
             for k in (3000, 0, 5000)]
    store = res.ResidentStore(device=DEV, viewpoints=3)
    for v in range(3):
        store.append('scan_%d' % v, feats[v], w2p[v], org[v], gt[v][0][:, :7], gt[v][1], [pairs[v]])
    store.freeze()
    assert store.feats.shape == (3, 6, 196 * 768) and store.nbytes_by_table['feats'] == 3 * 3612672
    order = [2, 0]
    batch = store.fetch(order)
    host_feats = T(np.stack([feats[v] for v in order], axis=1)).to(DEV)                       # [Ncam, bs, Nk, C]
    gts = h.pad_gts([T(gt[v][0][:, :7]).to(DEV) for v in order], [T(gt[v][1]).to(DEV) for v in order])
    occ = hip.pack_occ_gts([[pairs[v]] for v in order], pinned=False).to(DEV)
    torch.cuda.synchronize()
    assert store.check(batch) == (0, 0, 0, 8000)
    assert batch.feats.shape == host_feats.shape and batch.feats.dtype == host_feats.dtype and torch.equal(batch.feats, host_feats)
    assert torch.equal(batch.world2pixel, T(w2p[order]).to(DEV)) and torch.equal(batch.origin, T(org[order]).to(DEV))
    for got, want in zip(batch.gts, gts):
        assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)
    assert batch.occ.n_total == occ.n_total == 8000 and batch.occ.offsets.dtype == occ.offsets.dtype
    assert torch.equal(batch.occ.offsets, occ.offsets) and torch.equal(batch.occ.pairs, occ.pairs)
