"""Host side of the fixed-shape inference step: what ``VoxelFormerOccupancyHead.infer`` and ``graphs.GraphedInference`` refuse,
decided from host data alone (modes, branches, devices, shapes and dtypes), the ``check_step_inputs`` signatures of the
graphed step, and ``inference_results`` (the one host copy) on hand-made tables."""
import collections
import inspect
import warnings

import pytest
import torch

import cases
from util import pkg

warnings.filterwarnings('ignore')


@pytest.fixture(scope='module')
def head():
    pkg()
    return pkg('registry').build_head(dict(cases.vocc_head_cfg(), train_cfg=cases.VOCC_TRAIN_CFG)).eval()


def _inputs(bs=1):
    return torch.zeros(6, bs, 196, 768), torch.zeros(bs, 6, 4, 4), torch.zeros(bs, 3)


def test_infer_refuses_modes_and_branches_with_the_training_graph_wording(head):
    graphs = pkg('graphs')
    ins = _inputs()
    try:
        head.train()
        with pytest.raises(RuntimeError, match='training mode'):
            head.infer(*ins)
        with pytest.raises(RuntimeError, match='training mode'):
            graphs.GraphedInference(head, *ins)
        head.eval()
        for attr, value, wording in (('add_layout', True, 'add_layout=True: the room-layout terms are not part of the captured step'),
                                     ('only_occ', True, 'covers the default multi-task branch of the head (only_occ / only_det are set)'),
                                     ('only_det', True, 'covers the default multi-task branch of the head (only_occ / only_det are set)'),
                                     ('getbev', '/tmp/store', 'a head built with getbev=<store> writes volumes to the host inside forward')):
            before = getattr(head, attr)
            setattr(head, attr, value)
            try:
                for call in (lambda: head.infer(*ins), lambda: graphs.GraphedInference(head, *ins)):
                    with pytest.raises(NotImplementedError) as err:
                        call()
                    assert wording in str(err.value)
            finally:
                setattr(head, attr, before)
    finally:
        head.eval()


def test_graphed_inference_refuses_cpu_tensors_and_wrapped_heads(head):
    graphs = pkg('graphs')
    with pytest.raises(RuntimeError, match='GPU tensors.*feats, world2pixel, origin'):
        graphs.GraphedInference(head, *_inputs())

    class Wrapped(torch.nn.parallel.DistributedDataParallel):      # (an instance without a process group: the check is by type)
        def __init__(self):
            torch.nn.Module.__init__(self)

    with pytest.raises(RuntimeError, match='DistributedDataParallel'):
        graphs.GraphedInference(Wrapped(), *_inputs())


def test_step_signatures_decide_from_shapes_and_dtypes():
    graphs = pkg('graphs')
    GI = graphs.GraphedInference
    captured = GI._signature(*_inputs(1))
    assert [c[0] for c in captured] == ['feats', 'world2pixel', 'origin'] and all(c[3] is None for c in captured)
    graphs.check_step_inputs('GraphedInference', captured, GI._signature(*_inputs(1)))
    with pytest.raises(ValueError, match=r'GraphedInference: feats is \(6, 2, 196, 768\)'):
        graphs.check_step_inputs('GraphedInference', captured, GI._signature(*_inputs(2)))
    f, w, o = _inputs(1)
    with pytest.raises(ValueError, match='world2pixel'):
        graphs.check_step_inputs('GraphedInference', captured, GI._signature(f, w.double(), o))
    with pytest.raises(ValueError, match='origin'):
        graphs.check_step_inputs('GraphedInference', captured, GI._signature(f, w, o[:, :2]))


def test_no_host_read_is_spelled_in_the_step():
    """The step's own statements: no ``.item()`` / ``.tolist()`` / ``.cpu()`` / ``torch.where`` between inputs and outputs."""
    Head = pkg('dense_heads.voxelformer_occupancy_head').VoxelFormerOccupancyHead
    hip = pkg('hipops')
    for fn in (Head.infer, Head._infer_classes, Head.detect_from_volume, hip.occ_pairs, hip.occ_predict_classes, hip.occ_mlp_classes):
        src = inspect.getsource(fn)
        code = '\n'.join(ln.split('#')[0] for ln in src.split('"""')[-1].splitlines())
        for word in ('.item()', '.tolist()', '.cpu()', 'torch.where'):
            assert word not in code, (fn.__name__, word)
    assert pkg('detectors.voxelformer').VoxelFormer.device_inference is False


def test_results_make_the_reference_dicts_from_the_tables():
    mod = pkg('dense_heads.voxelformer_occupancy_head')
    Outs = mod.InferenceOutputs
    assert Outs._fields == ('volume', 'boxes', 'scores', 'labels', 'valid', 'classes', 'plan', 'occ_pairs', 'occ_offsets', 'occ_count')
    bs, k, dim = 2, 3, 9
    g = torch.Generator().manual_seed(0)
    boxes, scores = torch.randn(bs, k, dim, generator=g), torch.rand(bs, k, generator=g)
    labels = torch.tensor([[3, 1, 2], [0, 5, 4]], dtype=torch.int32)
    valid = torch.tensor([[1, 0, 1], [0, 0, 1]], dtype=torch.uint8)
    pairs = torch.tensor([[4, 1], [9, 0], [2, 15], [-7, -7]], dtype=torch.int32)
    outs = Outs(torch.zeros(bs, 5, 8), boxes, scores, labels, valid, None, None, pairs, torch.tensor([0, 2, 3], dtype=torch.int32),
                torch.tensor([2, 1, 3, 0], dtype=torch.int32))
    volume, bbox_list, occ = mod.inference_results(None, outs)
    assert volume.shape == (5, bs, 8) and occ['flow_preds'] is None and len(bbox_list) == bs
    for b in range(bs):
        r, keep = bbox_list[b]['pts_bbox'], valid[b].bool()
        assert torch.equal(r['boxes_3d'], boxes[b][keep]) and torch.equal(r['scores_3d'], scores[b][keep])
        assert r['labels_3d'].dtype == torch.int64 and torch.equal(r['labels_3d'], labels[b][keep].long())
    assert [p.tolist() for p in occ['occupancy_preds']] == [[[4, 1], [9, 0]], [[2, 15]]] and occ['occupancy_preds'][0].dtype == torch.int64
    Box = collections.namedtuple('Box', 'tensor dim')
    one = Outs(outs.volume[:1], boxes[:1], scores[:1], labels[:1], valid[:1], None, None, pairs, torch.tensor([0, 3], dtype=torch.int32),
               torch.tensor([3, 3, 0], dtype=torch.int32))
    _, bbox_list, occ = mod.inference_results(None, one, [dict(box_type_3d=Box)])
    assert isinstance(bbox_list[0]['pts_bbox']['boxes_3d'], Box) and bbox_list[0]['pts_bbox']['boxes_3d'].dim == dim
    assert torch.is_tensor(occ['occupancy_preds']) and occ['occupancy_preds'].tolist() == [[4, 1], [9, 0], [2, 15]]
    with pytest.raises(RuntimeError, match='pair capacity'):
        mod.inference_results(None, one._replace(occ_count=torch.tensor([9, 9, 1], dtype=torch.int32)))
