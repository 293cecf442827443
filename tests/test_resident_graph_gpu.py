"""``GraphedInference.fetch`` and ``GraphedTrainStep.fetch``: a ``resident.ResidentStore`` feeding the captured steps' static
buffers by index, against the same steps fed from host tensors.  vocc.py's head and the shapes of
tests/test_train_graph_gpu.py (ONE viewpoint per step, box capacity 8, pair capacity 40 000).

Inference is held to the bound of tests/test_infer_graph_gpu.py for "same kernels, replayed": ``E_vol`` (relative L2 of the
volume) and ``E_cls`` (differing class bytes) are measured between two HOST-FED replays of the same viewpoint first; the
index-fed replay must then stay within max(4 E_vol, 2e-3 bf16 / 1e-5 fp32) and 4 E_cls + 8 voxels of the host-fed one.  The
static inputs after ``fetch`` equal the host tensors bit for bit, so nothing but the gather's atomics separates the two.

Printed, not asserted: the relative L2 distance of the occupancy logits between a bf16 store and an f32 store (bf16 autocast,
seeded head) on the two synthetic viewpoints -- the price of ``feat_dtype=torch.bfloat16`` (resident.ResidentStore)."""
import warnings

import numpy as np
import pytest
import torch

from infer_helper import head, threshold, viewpoints
from test_train_graph_gpu import CAP, PAIR_CAP, _boxes, _build, _freeze_unused, _optimizer, _viewpoints
from util import pkg, rel_l2

warnings.filterwarnings('ignore')
pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = torch.device('cuda', 0)
COUNTS, PAIRS = (4, 6), (30000, 12000)         # boxes and pairs of the two viewpoints


def _annotations(voxel_num):
    rng = np.random.default_rng(71)
    out = []
    for v in range(2):
        boxes, labels = _boxes(50 + v, COUNTS[v])
        pairs = np.stack([rng.choice(voxel_num, size=PAIRS[v], replace=False), rng.integers(0, 16, PAIRS[v])], axis=1).astype(np.int64)
        out.append((boxes, labels, pairs))
    return out


def _store(feat_dtype=torch.float32, annotations=None, feats=None):
    """The two synthetic viewpoints (those of ``infer_helper.viewpoints`` and of the training tests) in a store on the GPU."""
    syn, res = pkg('synthetic'), pkg('resident')
    w2p, org = syn.camera_batch(2, seed=1)
    feats = syn.vit_features(2, seed=0) if feats is None else feats
    store = res.ResidentStore(device=DEV, feat_dtype=feat_dtype, viewpoints=2)
    for v in range(2):
        ann = annotations[v] if annotations else (None, None, None)
        store.append('scan_vp%d' % v, feats[v], w2p[v], org[v], *ann)
    return store.freeze()


@pytest.mark.parametrize('autocast', [True, False], ids=['bf16', 'fp32'])
def test_inference_fed_by_index_follows_the_host_fed_replays(autocast):
    h = head()
    graphs = pkg('graphs')
    dtype = torch.bfloat16 if autocast else None
    thr = threshold()
    ins = [viewpoints(1), viewpoints(1, first=1)]
    store = _store()
    step = graphs.GraphedInference(h, *ins[0], autocast_dtype=dtype, occ_threshold=thr, pair_capacity=h.voxel_num)
    keep = lambda outs: (outs.volume.clone(), outs.classes.clone())
    host, e_vol, e_cls = [], 0.0, 0
    for k in range(2):
        first, twin = keep(step(*ins[k])), keep(step(*ins[k]))
        e_vol, e_cls = max(e_vol, rel_l2(twin[0], first[0])), max(e_cls, int((twin[1] != first[1]).sum()))
        host.append(first)
    floor = 2e-3 if autocast else 1e-5
    vol_bound, cls_bound = max(4 * e_vol, floor), 4 * e_cls + 8
    print('autocast=%s: E_vol %.3e E_cls %d -> bounds %.3e / %d voxels' % (autocast, e_vol, e_cls, vol_bound, cls_bound))
    outside = []
    for k in (1, 0, 1):
        status = step.fetch(store, [k])
        for got, want in zip(step.inputs, ins[k]):
            assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)      # bit for bit
        outs = step(*step.inputs)
        torch.cuda.synchronize()
        vol, cls = rel_l2(outs.volume, host[k][0]), int((outs.classes != host[k][1]).sum())
        print('  index-fed viewpoint %d: volume rel L2 %.3e, %d differing voxels' % (k, vol, cls))
        if vol > vol_bound or cls > cls_bound:
            outside.append((k, vol, cls))
        assert store.check(status) == (0, 0, 0, 0)
    assert not outside, outside
    # a device index is used as it is; an index outside the store is an empty viewpoint and is reported, not raised
    step.fetch(store, torch.tensor([1], dtype=torch.int32, device=DEV))
    assert torch.equal(step.inputs[0], ins[1][0])
    status = step.fetch(store, [2])
    assert not step.inputs[0].any() and not step.inputs[1].any() and status.tolist() == [1, 0, 0, 0]
    # a store of another row size or dtype is refused on host data, before any launch
    step.fetch(store, [0])
    small = _store(feats=np.zeros((2, 6, 4, 8), np.float32))
    with pytest.raises(ValueError, match=r'GraphedInference.fetch: .*\(6, 32\) torch.float32, captured with \(6, 150528\) torch.float32'):
        step.fetch(small, [1])
    with pytest.raises(ValueError, match='torch.bfloat16, captured with .*torch.float32'):
        step.fetch(_store(torch.bfloat16), [1])
    with pytest.raises(ValueError, match='2 indices for a captured batch of 1'):
        step.fetch(store, [0, 1])
    torch.cuda.synchronize()
    assert torch.equal(step.inputs[0], ins[0][0]) and torch.equal(step.inputs[2], ins[0][2])


def test_bf16_store_deviation_is_reported():
    """Not a bound: prints what ``feat_dtype=torch.bfloat16`` costs in the occupancy logits (bf16 autocast, both viewpoints)."""
    h = head()
    stores = {torch.float32: _store(), torch.bfloat16: _store(torch.bfloat16)}
    assert stores[torch.bfloat16].nbytes_by_table['feats'] * 2 == stores[torch.float32].nbytes_by_table['feats']
    logits = {}
    for dt, store in stores.items():
        batch = store.fetch([0, 1])
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            volume = h(batch.feats.float(), None, only_bev=True, world2pixel=batch.world2pixel, origin=batch.origin)
            logits[dt] = h.occupancy_from_volume(volume).float()
    twin = stores[torch.float32].fetch([0, 1])
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        again = h.occupancy_from_volume(h(twin.feats, None, only_bev=True, world2pixel=twin.world2pixel, origin=twin.origin)).float()
    dev, noise = rel_l2(logits[torch.bfloat16], logits[torch.float32]), rel_l2(again, logits[torch.float32])
    print('bf16 store vs f32 store, occupancy logits under bf16 autocast: relative L2 %.3e (two runs of the f32 store: %.3e)' % (dev, noise))
    assert np.isfinite(dev) and torch.isfinite(logits[torch.bfloat16]).all()


def test_training_step_fed_by_index():
    graphs, hip = pkg('graphs'), pkg('hipops')
    head_ = _build()
    model = graphs.MultiTaskStep(head_, torch.bfloat16).eval()
    ins = _viewpoints()
    ann = _annotations(head_.voxel_num)
    store = _store(annotations=[(b, l, p) for b, l, p in ann])
    assert store.max_boxes == 6 <= CAP and store.max_pairs(1) == 30000 <= PAIR_CAP
    gt = [(head_.pad_gts([T(b).to(DEV)], [T(l).to(DEV)], capacity=CAP), hip.pack_occ_gts([p], pinned=False).to(DEV)) for b, l, p in ann]
    _freeze_unused([head_], model, ins[0] + gt[0])
    opt, params = _optimizer(head_, lr=0.0, weight_decay=0.0)
    step = graphs.GraphedTrainStep(model, opt, *ins[0], *gt[0], pair_capacity=PAIR_CAP, warmup=1)
    for k in (1, 0):
        # host-fed: the call's own loading of the static buffers, cloned
        for dst, src in zip(step.inputs, ins[k]):
            dst.copy_(src)
        step._load_gts(*gt[k])
        n, live = COUNTS[k], PAIRS[k]
        want = [t.clone() for t in step.inputs + (step.gts.boxes[:, :n], step.gts.labels[:, :n], step.gts.counts,
                                                  step.occ.offsets, step.occ.pairs[:live])]
        # the other viewpoint's data in the buffers, then the fetch
        for dst, src in zip(step.inputs, ins[1 - k]):
            dst.copy_(src)
        step._load_gts(*gt[1 - k])
        status = step.fetch(store, [k])
        got = step.inputs + (step.gts.boxes[:, :n], step.gts.labels[:, :n], step.gts.counts, step.occ.offsets, step.occ.pairs[:live])
        for g, w in zip(got, want):
            assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w)
        assert step.occ.offsets.tolist() == [0, live] and status.tolist() == [0, 0, 0, live]
    hip.AssignmentFlag.of(DEV).reset()                          # (sticky and the process's: this replay's own are asked for)
    hip.LabelRangeFlag.of(DEV).reset()
    status = step.fetch(store, torch.tensor([1], dtype=torch.int32, device=DEV))
    losses = {k: float(v) for k, v in step(*step.inputs, step.gts, step.occ).items()}
    print('index-fed replay:', losses)
    assert len(losses) == 14 and all(np.isfinite(v) for v in losses.values()) and losses['loss_occupancy'] > 0 and losses['loss_bbox'] > 0
    assert set(step.flags().values()) == {0} and status.tolist() == [0, 0, 0, PAIRS[1]]
    # ... and the same losses as the host-fed replay of that viewpoint (same kernels, replayed: 2e-3 under bf16 autocast)
    host = {k: float(v) for k, v in step(*ins[1], *gt[1]).items()}
    for k in host:
        assert abs(losses[k] - host[k]) <= 2e-3 * abs(host[k]), (k, losses[k], host[k])
    small = _store(feats=np.zeros((2, 6, 4, 8), np.float32))
    with pytest.raises(ValueError, match=r'GraphedTrainStep.fetch: .*\(6, 32\) torch.float32, captured with \(6, 150528\)'):
        step.fetch(small, [0])
    with pytest.raises(ValueError, match='torch.bfloat16, captured with'):
        step.fetch(_store(torch.bfloat16), [0])
