"""``graphs.GraphedTrainStep`` without a GPU: the host-side size checks on host data, and the refusals that are decided before
anything touches a device -- CPU tensors, a solver other than 'fused', the head modes outside the default multi-task branch,
an optimizer whose step cannot be captured, a DistributedDataParallel model."""
import types

import numpy as np
import pytest
import torch

from util import pkg


def _stub_model(**head):
    """A module with a ``head`` that has just what the constructor's checks read (no parameters, nothing is ever run)."""
    fields = dict(assigner=types.SimpleNamespace(solver='fused'), add_layout=False, only_occ=False, only_det=False, getbev=None)
    fields.update(head)
    m = torch.nn.Module()
    m.__dict__['head'] = types.SimpleNamespace(**fields)
    return m


class _Capturable:
    def prepare_capture(self):
        raise AssertionError('no refusal may get as far as the optimizer')


def _sample(bs=1, cap=4, pairs=10):
    pkg()
    PaddedGts = pkg('dense_heads.voxelformer_occupancy_head').PaddedGts
    gts = PaddedGts(torch.zeros(bs, cap, 9), torch.zeros(bs, cap, dtype=torch.int64), torch.zeros(bs, dtype=torch.int32))
    rng = np.random.default_rng(0)
    occ = pkg('hipops').pack_occ_gts([np.stack([rng.integers(0, 1000, pairs), rng.integers(0, 16, pairs)], 1) for _ in range(bs)],
                                     pinned=False)
    return torch.zeros(6, bs, 196, 768), torch.zeros(bs, 6, 4, 4), torch.zeros(bs, 3), gts, occ


def test_size_checks_run_on_host_data():
    graphs = pkg('graphs')
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    boxes = (1, 'boxes per sample', 'box capacity')

    def sig(feats=(6, 1, 196, 768), dtype=f32, nbox=8, npairs=100, bs=1):
        return (('feats', feats, dtype, None), ('gts.boxes', (bs, nbox, 9), f32, boxes), ('gts.labels', (bs, nbox), i64, boxes),
                ('occ.pairs', (npairs, 2), i32, (0, 'pairs', 'pair capacity')), ('occ.offsets', (bs + 1,), i32, None))

    graphs.check_step_inputs('step', sig(), sig())
    graphs.check_step_inputs('step', sig(), sig(nbox=0, npairs=0))             # less than the capacity is what a step brings
    graphs.check_step_inputs('step', sig(), sig(nbox=8, npairs=100))
    with pytest.raises(ValueError, match='gts.boxes holds 9 boxes per sample, the box capacity captured is 8'):
        graphs.check_step_inputs('step', sig(), sig(nbox=9))
    with pytest.raises(ValueError, match='occ.pairs holds 101 pairs, the pair capacity captured is 100'):
        graphs.check_step_inputs('step', sig(), sig(npairs=101))
    with pytest.raises(ValueError, match=r'feats is \(6, 2, 196, 768\) torch.float32, captured with \(6, 1, 196, 768\)'):
        graphs.check_step_inputs('step', sig(), sig(feats=(6, 2, 196, 768)))
    with pytest.raises(ValueError, match='feats is .* torch.bfloat16, captured with .* torch.float32'):
        graphs.check_step_inputs('step', sig(), sig(dtype=torch.bfloat16))
    with pytest.raises(ValueError, match='captured with'):
        graphs.check_step_inputs('step', sig(), sig(feats=(6, 196, 768)))      # another rank
    with pytest.raises(ValueError, match=r'occ.offsets is \(3,\)'):
        graphs.check_step_inputs('step', sig(), sig()[:4] + sig(bs=2)[4:])


def test_refusals_decided_before_any_device_work():
    graphs = pkg('graphs')
    feats, w2p, org, gts, occ = _sample()
    with pytest.raises(RuntimeError, match='GPU tensors.*feats, world2pixel, origin, gts.boxes, gts.labels, gts.counts, occ.buffer'):
        graphs.GraphedTrainStep(_stub_model(), _Capturable(), feats, w2p, org, gts, occ)
    with pytest.raises(ValueError, match="solver is 'host'.*'fused'"):
        graphs.GraphedTrainStep(_stub_model(assigner=types.SimpleNamespace(solver='host')), _Capturable(), feats, w2p, org, gts, occ)
    with pytest.raises(ValueError, match="solver is 'device'"):
        graphs.GraphedTrainStep(_stub_model(assigner=types.SimpleNamespace(solver='device')), _Capturable(), feats, w2p, org, gts, occ)
    with pytest.raises(NotImplementedError, match='add_layout=True'):
        graphs.GraphedTrainStep(_stub_model(add_layout=True), _Capturable(), feats, w2p, org, gts, occ)
    with pytest.raises(NotImplementedError, match='getbev'):
        graphs.GraphedTrainStep(_stub_model(getbev=object()), _Capturable(), feats, w2p, org, gts, occ)
    with pytest.raises(TypeError, match='optimizer whose step\\(\\) can be captured'):
        graphs.GraphedTrainStep(_stub_model(), torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1), feats, w2p, org, gts, occ)
    ddp = torch.nn.parallel.DistributedDataParallel
    with pytest.raises(RuntimeError, match='DistributedDataParallel'):
        graphs.GraphedTrainStep(ddp.__new__(ddp), _Capturable(), feats, w2p, org, gts, occ)
    with pytest.raises(TypeError, match='PaddedGts'):
        graphs.GraphedTrainStep(_stub_model(), _Capturable(), feats, w2p, org, [gts.boxes[0]], occ)
    with pytest.raises(ValueError, match='holds 10 pairs, the pair capacity is 4'):
        graphs.GraphedTrainStep(_stub_model(), _Capturable(), feats, w2p, org, gts, occ, pair_capacity=4)
    both = pkg('hipops').pack_occ_gts([np.array([[1, 2]])], invalid=[np.array([5])], pinned=False)
    with pytest.raises(ValueError, match='invalid voxels'):
        graphs.GraphedTrainStep(_stub_model(), _Capturable(), feats, w2p, org, gts, both)
