"""The resident viewpoint store without a GPU: the numpy model of ``ver_fetch_batch`` (``hipops.fetch_batch_host``) against
arrays written out by hand, ``resident.ResidentStore`` on CPU tensors against the host-fed assembly (stacking, ``head.pad_gts``,
``hipops.pack_occ_gts``), and the library's argument validation (which never touches the device)."""
import ctypes

import numpy as np
import pytest
import torch

import cases
from resident_helper import SENTINEL, T, hand_store, same_bits
from util import pkg


def test_host_model_against_arrays_written_by_hand():
    """Index [2, 0, 5, 0, 1] into the 3-viewpoint store: viewpoint 0 twice, 5 outside the store, viewpoint 1 without pairs or
    boxes; two box columns for the three boxes of viewpoint 0; room for six of the eight pairs."""
    hip = pkg('hipops')
    got = hip.fetch_batch_host([2, 0, 5, 0, 1], out_cap=2, pair_capacity=6, **hand_store())
    row = lambda v, c: [100 * v + 10 * c, 100 * v + 10 * c + 1, 100 * v + 10 * c + 2]
    zero = [0, 0, 0]
    feats = np.array([[row(2, 0), row(0, 0), zero, row(0, 0), row(1, 0)],
                      [row(2, 1), row(0, 1), zero, row(0, 1), row(1, 1)]], np.float32)
    assert got['feats'].dtype == np.float32 and np.array_equal(got['feats'], feats)
    w2p = np.zeros((5, 2, 4, 4), np.float32)
    for b, first in ((0, 21), (1, 1), (3, 1), (4, 11)):
        w2p[b, 0], w2p[b, 1] = first, first + 1
    assert np.array_equal(got['world2pixel'], w2p)
    assert np.array_equal(got['origin'], np.array([[2, 2.5, -2], [0, 0.5, 0], [0, 0, 0], [0, 0.5, 0], [1, 1.5, -1]], np.float32))
    boxes = np.zeros((5, 2, 2), np.float32)
    boxes[0, 0] = [20, -20]
    boxes[1] = boxes[3] = [[0, 0], [1, -1]]
    assert got['boxes'].dtype == np.float32 and np.array_equal(got['boxes'], boxes)
    assert got['labels'].dtype == np.int64 and np.array_equal(got['labels'], [[21, 0], [1, 2], [0, 0], [1, 2], [0, 0]])
    assert got['counts'].dtype == np.int32 and got['counts'].tolist() == [1, 2, 0, 2, 0]
    assert got['offsets'].dtype == np.int32 and got['offsets'].tolist() == [0, 2, 5, 5, 6, 6]
    assert got['pairs'].dtype == np.int32 and got['pairs'].tolist() == [[20, 5], [21, 6], [1, 1], [2, 2], [3, 3], [1, 1]]
    # one index outside; viewpoint 0 (twice) holds more boxes than two; eight pairs for six places
    assert got['status'].dtype == np.int32 and got['status'].tolist() == [1, 2, 1, 8]


def test_host_model_keeps_what_lies_behind_and_takes_absent_groups():
    hip = pkg('hipops')
    store = hand_store()
    prev = dict(boxes=np.full((2, 4, 2), SENTINEL, np.float32), labels=np.full((2, 4), SENTINEL, np.int64),
                pairs=np.full((7, 2), SENTINEL, np.int32))
    got = hip.fetch_batch_host([2, 1], out_cap=4, pair_capacity=7, out=prev, **store)
    assert got['counts'].tolist() == [1, 0] and got['boxes'][0, 0].tolist() == [20, -20] and got['labels'][0, 0] == 21
    assert (got['boxes'][0, 1:] == SENTINEL).all() and (got['boxes'][1] == SENTINEL).all() and (got['labels'][1] == SENTINEL).all()
    assert got['offsets'].tolist() == [0, 2, 2] and got['pairs'][:2].tolist() == [[20, 5], [21, 6]] and (got['pairs'][2:] == SENTINEL).all()
    assert got['status'].tolist() == [0, 0, 0, 2]
    assert (prev['pairs'] == SENTINEL).all()                    # (the model copies: the caller's arrays are not written)
    only = hip.fetch_batch_host([0, -1], feats=store['feats'])
    assert sorted(only) == ['feats', 'status'] and only['status'].tolist() == [1, 0, 0, 0] and not only['feats'][:, 1].any()
    cams = hip.fetch_batch_host([1], world2pixel=store['world2pixel'], origin=store['origin'])
    assert sorted(cams) == ['origin', 'status', 'world2pixel'] and cams['origin'].tolist() == [[1, 1.5, -1]]
    pairs = hip.fetch_batch_host([0, 0], pairs=store['pairs'], pair_offsets=store['pair_offsets'], pair_capacity=0)
    assert pairs['offsets'].tolist() == [0, 0, 0] and pairs['pairs'].shape == (0, 2) and pairs['status'].tolist() == [0, 0, 1, 6]
    empty = hip.fetch_batch_host([], out_cap=1, pair_capacity=3, **store)
    assert empty['feats'].shape == (2, 0, 3) and empty['offsets'].tolist() == [0] and empty['status'].tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        hip.fetch_batch_host([0], world2pixel=store['world2pixel'])


def _viewpoints(n, seed=3):
    """``n`` small viewpoints: feats [2, 4, 8], cameras, ``cases.detection_gt`` boxes (7 columns) and int64 pairs."""
    rng = np.random.default_rng(seed)
    out = []
    for v in range(n):
        boxes, labels = cases.detection_gt(seed=40 + v, num_gt=(3, 0, 5, 1)[v % 4])
        k = (12, 0, 30, 7)[v % 4]
        pairs = np.stack([rng.choice(504000, size=k, replace=False), rng.integers(0, 16, k)], axis=1).astype(np.int64)
        out.append(dict(key='scan%d_vp%d' % (v // 2, v), feats=rng.standard_normal((2, 4, 8)).astype(np.float32),
                        w2p=rng.standard_normal((2, 4, 4)).astype(np.float32), origin=rng.standard_normal(3).astype(np.float32),
                        boxes=boxes[:, :7], labels=labels, pairs=pairs))
    return out


def _store(vps, **kwargs):
    store = pkg('resident').ResidentStore(device='cpu', **kwargs)
    for i, v in enumerate(vps):
        assert store.append(v['key'], v['feats'], v['w2p'], v['origin'], v['boxes'], v['labels'], [v['pairs']]) == i
    return store


def test_store_fills_freezes_and_answers_lookups():
    res = pkg('resident')
    vps = _viewpoints(4)
    store = _store(vps)
    with pytest.raises(RuntimeError, match='freeze'):
        store.fetch([0])
    with pytest.raises(KeyError):
        store.append(vps[0]['key'], vps[0]['feats'], vps[0]['w2p'], vps[0]['origin'])
    with pytest.raises(ValueError, match='feats'):
        store.append('other_vp', np.zeros((2, 4, 9), np.float32), vps[0]['w2p'], vps[0]['origin'])
    assert store.freeze() is store and len(store) == 4
    with pytest.raises(RuntimeError, match='frozen'):
        store.append('late_vp', vps[0]['feats'], vps[0]['w2p'], vps[0]['origin'])
    assert store.keys == [v['key'] for v in vps] and store.index_of('scan1_vp2') == 2
    with pytest.raises(KeyError):
        store.index_of('scan9_vp9')
    assert store.num_cams == 2 and store.row == 32 and store.feat_tail == (4, 8) and store.max_boxes == 5
    assert store.feats.shape == (4, 2, 32) and store.feats.dtype == torch.float32
    assert store.pairs.dtype == torch.int32 and store.pair_offsets.tolist() == [0, 12, 12, 42, 49]
    assert store.counts.tolist() == [3, 0, 5, 1] and store.labels.dtype == torch.int64 and store.boxes.shape == (4, 5, 9)
    by = store.nbytes_by_table
    assert by == dict(feats=4 * 2 * 32 * 4, world2pixel=4 * 2 * 16 * 4, origin=4 * 3 * 4, boxes=4 * 5 * 9 * 4, labels=4 * 5 * 8,
                      counts=4 * 4, pairs=49 * 8, pair_offsets=5 * 8)
    assert store.nbytes == sum(by.values())
    assert [store.max_pairs(b) for b in (0, 1, 2, 3, 4, 5)] == [0, 30, 42, 49, 49, 79]
    half = _store(vps, feat_dtype=torch.bfloat16).freeze()
    assert half.feats.dtype == torch.bfloat16 and half.nbytes_by_table['feats'] == by['feats'] // 2
    assert torch.equal(half.feats, store.feats.to(torch.bfloat16))            # rounded once, to nearest-even
    with pytest.raises(TypeError):
        res.ResidentStore(device='cpu', feat_dtype=torch.float16)
    with pytest.raises(RuntimeError, match='empty'):
        res.ResidentStore(device='cpu').freeze()


def test_pairs_beyond_int32_saturate_as_pack_occ_gts_does():
    hip = pkg('hipops')
    vps = _viewpoints(2)
    wide = np.array([[2 ** 40, 3], [-2 ** 35, -2 ** 33], [17, 2 ** 31], [5, 4]], np.int64)
    vps[1]['pairs'] = wide
    store = _store(vps).freeze()
    want = hip.pack_occ_gts([wide], pinned=False)
    assert torch.equal(store.pairs[12:], want.pairs)
    assert store.pairs[12:].tolist() == [[2 ** 31 - 1, 3], [-2 ** 31, -2 ** 31], [17, 2 ** 31 - 1], [5, 4]]
    with pytest.raises(ValueError, match='occ_pairs'):
        _store(vps[:1]).append('x_y', vps[0]['feats'], vps[0]['w2p'], vps[0]['origin'], occ_pairs=np.zeros((3, 2), np.float32))


def _head():
    pkg()
    torch.manual_seed(3)
    return pkg('registry').build_head(dict(cases.vocc_head_cfg(), train_cfg=cases.VOCC_TRAIN_CFG)).eval()


def test_cpu_fetch_equals_the_host_fed_assembly():
    """``fetch`` on the CPU against stacking + ``head.pad_gts`` + ``pack_occ_gts`` of the same viewpoints: shapes, dtypes, values."""
    hip, res = pkg('hipops'), pkg('resident')
    vps = _viewpoints(4)
    store = _store(vps).freeze()
    order = [2, 0, 3]
    batch = store.fetch(order, box_capacity=6)
    assert isinstance(batch, res.ResidentBatch) and store.check(batch) == (0, 0, 0, 49)
    feats = torch.stack([T(vps[v]['feats']) for v in order], dim=1)              # [Ncam, bs, Nk, C]
    assert batch.feats.shape == feats.shape and batch.feats.dtype == feats.dtype and torch.equal(batch.feats, feats)
    assert torch.equal(batch.world2pixel, torch.stack([T(vps[v]['w2p']) for v in order]))
    assert torch.equal(batch.origin, torch.stack([T(vps[v]['origin']) for v in order]))
    gts = _head().pad_gts([T(vps[v]['boxes']) for v in order], [T(vps[v]['labels']) for v in order], capacity=6)
    for got, want in zip(batch.gts, gts):
        assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)
    occ = hip.pack_occ_gts([[vps[v]['pairs']] for v in order], pinned=False)
    assert isinstance(batch.occ, hip.PackedOccGts) and batch.occ.bs == 3 and not batch.occ.has_invalid
    assert batch.occ.offsets.dtype == occ.offsets.dtype and torch.equal(batch.occ.offsets, occ.offsets)
    assert batch.occ.n_total == store.max_pairs(3) == occ.n_total and torch.equal(batch.occ.pairs, occ.pairs)
    assert batch.index.tolist() == order and batch.index.dtype == torch.int32
    # out=: the same tensors are written; a shorter batch leaves the longer one's tail where it was
    before = [t.data_ptr() for t in (batch.feats, batch.gts.boxes, batch.occ.buffer, batch.status)]
    again = store.fetch(torch.tensor([1, 9, 3]), out=batch)
    assert [t.data_ptr() for t in (again.feats, again.gts.boxes, again.occ.buffer, again.status)] == before
    assert again.gts.counts.tolist() == [0, 0, 1] and again.occ.offsets.tolist() == [0, 0, 0, 7]
    assert torch.equal(again.occ.pairs[7:], occ.pairs[7:]) and torch.equal(again.gts.boxes[0], gts.boxes[0])
    assert not again.feats[:, 1].any() and not again.world2pixel[1].any() and again.status.tolist() == [1, 0, 0, 7]
    with pytest.raises(ValueError, match='1 sample.*outside the store'):
        store.check(again.status)
    tight = store.fetch([2, 0], box_capacity=2, pair_capacity=20)
    assert tight.status.tolist() == [0, 2, 1, 42] and tight.gts.counts.tolist() == [2, 2] and tight.occ.offsets.tolist() == [0, 20, 20]
    with pytest.raises(ValueError, match='2 sample.*more boxes.*42 pairs'):
        store.check(tight)
    with pytest.raises(ValueError, match='capacities'):
        store.fetch([0, 1], out=tight, pair_capacity=5)


def test_from_stores_reads_the_existing_stores(tmp_path):
    syn, res = pkg('synthetic'), pkg('resident')
    rng = np.random.default_rng(0)
    w2p, org = syn.camera_batch(2, seed=1)
    syn.write_camera_files(str(tmp_path), 'scanA', ['vp0', 'vp1'], w2p, org)
    feat_dir = tmp_path / 'feats'
    feat_dir.mkdir()
    maps = {}
    for vp in ('vp0', 'vp1'):
        for deg in range(6):
            maps['scanA_%s_i1_%d' % (vp, deg)] = rng.standard_normal((1, 5, 8)).astype(np.float32)       # CLS + 4 tokens
            np.save(str(feat_dir / ('scanA_%s_i1_%d.npy' % (vp, deg))), maps['scanA_%s_i1_%d' % (vp, deg)])
    fstore, cstore = pkg('volume_io').FeatureStore(str(feat_dir)), pkg('camera_store').CameraStore(str(tmp_path))
    ann = {'scanA_vp1': dict(occ_pairs=np.array([[4, 2]], np.int64))}
    store = res.ResidentStore.from_stores(fstore, cstore, ['scanA_vp1', 'scanA_vp0'], ann, device='cpu')
    assert store.frozen and store.keys == ['scanA_vp1', 'scanA_vp0'] and store.feat_tail == (4, 8) and not fstore._cache
    batch = store.fetch([store.index_of('scanA_vp0'), store.index_of('scanA_vp1')])
    want = np.stack([np.stack([maps['scanA_%s_i1_%d' % (vp, deg)][0, 1:] for vp in ('vp0', 'vp1')]) for deg in range(6)])
    assert same_bits(batch.feats.numpy(), want)
    assert same_bits(batch.world2pixel.numpy(), w2p) and same_bits(batch.origin.numpy(), org)
    assert batch.gts.boxes.shape == (2, 0, 9) and batch.occ.offsets.tolist() == [0, 0, 1] and batch.occ.pairs.tolist() == [[4, 2]]


def test_freeze_cuts_grown_tables_and_from_tables_takes_ready_ones():
    """A feature table that doubled as it filled is cut to what was appended, so ``nbytes`` is what the store holds; and a
    store built around ready tables fetches what the appended one does."""
    res = pkg('resident')
    vps = _viewpoints(3)
    grown, sized = _store(vps).freeze(), _store(vps, viewpoints=3).freeze()
    for store in (grown, sized):
        assert store.feats.shape[0] == 3 and store.feats.untyped_storage().nbytes() == store.nbytes_by_table['feats']
        assert store.pairs.untyped_storage().nbytes() == store.nbytes_by_table['pairs'] == 42 * 8
    assert torch.equal(grown.feats, sized.feats) and torch.equal(grown.pairs, sized.pairs)
    ready = res.ResidentStore.from_tables(grown.keys, grown.feats, grown.world2pixel, grown.origin, grown.boxes, grown.labels,
                                          grown.counts, grown.pairs, grown.pair_offsets, feat_tail=(4, 8))
    assert ready.frozen and ready.index_of(vps[2]['key']) == 2 and ready.max_pairs(2) == 42 and ready.max_boxes == 5
    a, b = grown.fetch([2, 0, 7]), ready.fetch([2, 0, 7])
    for x, y in zip((a.feats, a.world2pixel, a.origin) + tuple(a.gts) + (a.occ.buffer, a.status),
                    (b.feats, b.world2pixel, b.origin) + tuple(b.gts) + (b.occ.buffer, b.status)):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y)
    bare = res.ResidentStore.from_tables(['a', 'b', 'c'], grown.feats, grown.world2pixel, grown.origin)
    got = bare.fetch([1])
    assert got.feats.shape == (2, 1, 32) and got.gts.boxes.shape == (1, 0, 9) and got.occ.offsets.tolist() == [0, 0]
    with pytest.raises(ValueError, match='pair_offsets'):
        res.ResidentStore.from_tables(grown.keys, grown.feats, grown.world2pixel, grown.origin, pairs=grown.pairs,
                                      pair_offsets=grown.pair_offsets + 1)
    with pytest.raises(ValueError, match='world2pixel'):
        res.ResidentStore.from_tables(grown.keys, grown.feats, grown.world2pixel[:2], grown.origin)


def test_library_validates_arguments_without_a_gpu():
    hip = pkg('hipops')
    lib = hip.lib()
    i, l, ptr = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    assert hip.PROTOTYPES['ver_fetch_pair_tile'] == (l, [])
    assert hip.PROTOTYPES['ver_fetch_batch'] == (i, [ptr, i, l, i, ptr, ptr, i, l] + [ptr] * 10 + [i, i, i, ptr, ptr, l, ptr, ptr, l, ptr, ptr])
    assert lib.ver_fetch_pair_tile() == hip.fetch_pair_tile() >= 64
    buf = (ctypes.c_int64 * 8)()                              # a 16-byte aligned host address: the checks only look at pointer
    a = (ctypes.addressof(buf) + 15) & ~15                    # values, and every call below is refused before any launch
    groups = dict(feats=('feat_store', 'feat_out'), cams=('w2p_store', 'origin_store', 'w2p_out', 'origin_out'),
                  boxes=('box_store', 'label_store', 'count_store', 'box_out', 'label_out', 'count_out'),
                  pairs=('pair_store', 'pair_offsets', 'offsets_out', 'pairs_out'))
    order = ('index', 'bs', 'V', 'ncam') + groups['feats'] + ('feat_dtype', 'row') + groups['cams'] + groups['boxes'] + \
        ('store_cap', 'out_cap', 'box_dim', 'pair_store', 'pair_offsets', 'pair_total', 'offsets_out', 'pairs_out',
         'pair_capacity', 'status', 'stream')

    def call(**kw):
        args = dict(index=a, bs=2, V=7, ncam=6, feat_dtype=0, row=5, store_cap=3, out_cap=4, box_dim=9, pair_total=11,
                    pair_capacity=8, status=a, stream=None)
        args.update({name: a for names in groups.values() for name in names})
        args.update(kw)
        return lib.ver_fetch_batch(*[args[k] for k in order])

    OK, EINVAL, EUNSUPPORTED = 0, -1, -2
    nothing = {name: None for names in groups.values() for name in names}
    # bs == 0 launches nothing and looks at no pointer
    assert call(bs=0, index=None, status=None, **nothing) == OK
    for bad, word in ((dict(bs=-1), b'bs'), (dict(V=-1), b'V='), (dict(ncam=-1), b'ncam'), (dict(row=-1), b'row'),
                      (dict(store_cap=-1), b'store_cap'), (dict(out_cap=-2), b'out_cap'), (dict(box_dim=-1), b'box_dim'),
                      (dict(pair_total=-1), b'pair_total'), (dict(pair_capacity=-1), b'pair_capacity'),
                      (dict(feat_dtype=2), b'feat_dtype'), (dict(index=None), b'index'), (dict(index=a + 2), b'index'),
                      (dict(status=None), b'status'), (dict(status=a + 1), b'status')):
        assert call(**bad) == EINVAL, bad
        assert b'ver_fetch_batch' in lib.ver_last_error() and word in lib.ver_last_error(), (bad, lib.ver_last_error())
    for bad, word in ((dict(bs=65536), b'bs'), (dict(pair_capacity=2 ** 31), b'pair_capacity')):
        assert call(**bad) == EUNSUPPORTED, bad
        assert word in lib.ver_last_error(), (bad, lib.ver_last_error())
    # a present group with one pointer null, or misaligned
    for names in groups.values():
        for name in names:
            assert call(**{name: None}) == EINVAL, name
            assert name.encode() in lib.ver_last_error(), (name, lib.ver_last_error())
    for name, off in (('feat_store', 2), ('feat_out', 1), ('w2p_store', 2), ('origin_out', 1), ('box_store', 2), ('label_store', 4),
                      ('label_out', 4), ('count_out', 2), ('pair_store', 4), ('pair_offsets', 4), ('offsets_out', 2), ('pairs_out', 4)):
        assert call(**{name: a + off}) == EINVAL, name
        assert name.encode() in lib.ver_last_error(), (name, lib.ver_last_error())
    assert call(feat_dtype=1, feat_store=a + 1) == EINVAL
