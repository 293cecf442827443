"""A training or evaluation split resident in device memory, and batches fetched out of it by index (``ResidentStore``).

After the captured steps (``graphs.GraphedTrainStep``, ``GraphedInference``) the largest remaining host cost of a step is the
data in front of the graph: features out of ``volume_io.FeatureStore``, stacked and copied; boxes padded by ``head.pad_gts``;
pairs packed by ``hipops.pack_occ_gts`` (one int64 -> int32 pass per step and sample).  The reference answers the same
problem with a host dict of the feature maps it has read (detectors/voxelformer.py:317-325) and re-reads the occupancy
annotation on every step.  On an MI355X the natural cache is HBM: one viewpoint is 6 x 196 x 768 fp32 = 3.6 MB of features,
ten thousand are 36 GB (18 GB in bf16) of 288 GB.  Once the split is resident, ``ver_fetch_batch`` (csrc/ver_fetch.hip)
writes a step's batch straight into the step's static buffers for a device-resident index vector, and the only per-step
host -> device traffic is that vector: ``4 * bs`` bytes.
"""
import collections

import numpy as np
import torch

from . import hipops
from .dense_heads.voxelformer_occupancy_head import PaddedGts

ResidentBatch = collections.namedtuple('ResidentBatch', 'feats world2pixel origin gts occ status index')
ResidentBatch.__doc__ = """What ``ResidentStore.fetch`` writes: ``feats [Ncam, bs, Nk, C]``, ``world2pixel [bs, Ncam, 4, 4]``,
``origin [bs, 3]``, ``gts`` (a ``PaddedGts``), ``occ`` (a ``hipops.PackedOccGts`` at the pair capacity), ``status`` int32 [4]
(``ResidentStore.check``) and the device ``index`` int32 [bs] it was fetched for.  ``gts`` / ``occ`` / the feature and camera
tensors may be None in a batch handed to ``fetch(out=)``: that group is then not fetched."""

BOX_DIM = 9                     # (cx, cy, cz, w, l, h, yaw, vx, vy): the padded tables of head.pad_gts


class _Grown:
    """Rows appended to one device table that grows geometrically (one device copy per doubling); ``rows=`` sizes it up
    front, and then nothing is ever copied."""

    def __init__(self, width, dtype, device, rows=None):
        self.width, self.dtype, self.device, self.n = tuple(width), dtype, device, 0
        self.table = torch.empty((int(rows or 0),) + self.width, dtype=dtype, device=device)

    def room(self, n):
        """A view of the next ``n`` rows (the table is grown to hold them)."""
        if self.n + n > self.table.shape[0]:
            grown = torch.empty((max(self.n + n, 2 * self.table.shape[0], 1),) + self.width, dtype=self.dtype, device=self.device)
            grown[:self.n].copy_(self.table[:self.n])
            self.table = grown
        view = self.table[self.n:self.n + n]
        self.n += n
        return view


class ResidentStore:
    """Viewpoints of a split in device memory, fetched by index.

    Filling: ``append(sample_idx, feats, world2pixel, origin, gt_boxes=None, gt_labels=None, occ_pairs=None)`` one
    viewpoint at a time, then ``freeze()``; or ``ResidentStore.from_stores(feature_store, camera_store, sample_ids,
    annotations)`` over the existing ``volume_io.FeatureStore`` / ``camera_store.CameraStore``.  The host stages ONE viewpoint
    (in pinned memory when the store is on a GPU); the split is never held on the host as a whole.  ``viewpoints=`` sizes
    the feature table up front (``from_stores`` does); without it the table doubles as it fills.

    ``feat_dtype=torch.float32`` (default): a fetched batch is bit-identical to the host-fed one.  ``torch.bfloat16`` is
    opt-in and halves the store; it rounds the FEATURES to bf16 (nearest-even, once, at ``append``), before the camera and
    level embeddings are added, whereas the head's ``_EmbedCast`` rounds after that add under bf16 autocast -- so a bf16
    store is NOT bit-identical to the host-fed path.  Measured on the two synthetic viewpoints (seeded vocc head, bf16
    autocast, one MI355X; tests/test_resident_graph_gpu.py prints it): the occupancy logits of a bf16 store differ from
    those of an f32 store by 5.06e-3 relative L2, where two runs of the f32 store differ by 0.

    Pairs are converted int64 -> int32 (saturating, as ``hipops.pack_occ_gts`` does) once per viewpoint at ``append``, not
    per step, and kept as CSR: ``pairs int32 [total, 2]`` with ``pair_offsets int64 [V + 1]``.  Boxes are kept as
    ``head.pad_gts`` pads them: f32 ``[V, max_boxes, 9]`` (velocity columns zero where a box brings 7), int64 labels, int32
    counts.

    After ``freeze()``: ``index_of('<scan>_<vp>')`` and ``keys``; ``nbytes`` (``nbytes_by_table`` per table); ``max_boxes``
    and ``max_pairs(bs)`` -- the largest pair total of any ``bs`` viewpoints -- from which a caller sizes the box
    ``capacity`` and the ``pair_capacity`` of a captured step; ``fetch`` and ``check``."""

    def __init__(self, device='cuda', feat_dtype=torch.float32, viewpoints=None):
        if feat_dtype not in (torch.float32, torch.bfloat16):
            raise TypeError('ResidentStore: feat_dtype is torch.float32 or torch.bfloat16, got %s' % (feat_dtype,))
        self.device, self.feat_dtype = torch.device(device), feat_dtype
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self._rows_hint = viewpoints
        self.keys, self._index = [], {}
        self.num_cams = self.row = self.feat_tail = None
        self._feats = None
        self._pairs = _Grown((2,), torch.int32, self.device)
        self._w2p, self._origin, self._boxes, self._labels, self._lens = [], [], [], [], []
        self._stage = self._stage_done = None
        self.frozen = False

    # ---- filling ------------------------------------------------------------------------------------------------------
    def _upload(self, dst, src):
        """``src`` (a host tensor; converted to ``dst``'s dtype on the way) -> ``dst`` on the device through the pinned
        one-viewpoint staging buffer, asynchronously; the buffer is rewritten only after its last copy has completed."""
        if self.device.type != 'cuda':
            dst.copy_(src.reshape(dst.shape))
            return
        n = dst.numel() * dst.element_size()
        if self._stage is None or self._stage.numel() < n:
            if self._stage_done is not None:
                self._stage_done.synchronize()
            self._stage = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        elif self._stage_done is not None:
            self._stage_done.synchronize()
        host = self._stage[:n].view(dst.dtype).view(dst.shape)
        host.copy_(src.reshape(dst.shape))
        dst.copy_(host, non_blocking=True)
        self._stage_done = torch.cuda.Event()
        self._stage_done.record()

    def append(self, sample_idx, feats, world2pixel, origin, gt_boxes=None, gt_labels=None, occ_pairs=None):
        """One viewpoint: ``feats [Ncam, Nk, C]`` (or ``[Ncam, 1, Nk, C]``, as ``FeatureStore.viewpoint`` returns it; or
        ``[Ncam, row]``), ``world2pixel [Ncam, 4, 4]``, ``origin [3]``; ``gt_boxes [G, 7..9]`` with ``gt_labels [G]``;
        ``occ_pairs`` an integer ``[n, 2]`` array of (flat voxel index, class) -- or the reference's one-element list around
        it -- saturated to int32 here.  -> the viewpoint's index."""
        if self.frozen:
            raise RuntimeError('ResidentStore.append: the store is frozen')
        sample_idx = str(sample_idx)
        if sample_idx in self._index:
            raise KeyError('ResidentStore.append: %r is in the store already' % sample_idx)
        as_host = lambda t: t.detach().cpu() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
        feats = as_host(feats)
        if feats.dim() == 4 and feats.shape[1] == 1:
            feats = feats[:, 0]
        if feats.dim() not in (2, 3) or not feats.is_floating_point():
            raise ValueError('ResidentStore.append: feats is floating point [Ncam, Nk, C] or [Ncam, row], got %s %s'
                             % (feats.dtype, tuple(feats.shape)))
        ncam, tail = int(feats.shape[0]), tuple(int(s) for s in feats.shape[1:])
        if self._feats is None:
            self.num_cams, self.feat_tail, self.row = ncam, tail, int(np.prod(tail))
            self._feats = _Grown((ncam, self.row), self.feat_dtype, self.device, self._rows_hint)
        elif (ncam, tail) != (self.num_cams, self.feat_tail):
            raise ValueError('ResidentStore.append: feats %s, the store holds %s per viewpoint'
                             % ((ncam,) + tail, (self.num_cams,) + self.feat_tail))
        w2p = np.asarray(as_host(world2pixel).numpy(), dtype=np.float32)
        org = np.asarray(as_host(origin).numpy(), dtype=np.float32).reshape(-1)
        if w2p.shape != (ncam, 4, 4) or org.shape != (3,):
            raise ValueError('ResidentStore.append: world2pixel [%d, 4, 4] and origin [3], got %s and %s' % (ncam, w2p.shape, org.shape))
        boxes, labels = np.zeros((0, BOX_DIM), dtype=np.float32), np.zeros(0, dtype=np.int64)
        if gt_boxes is not None:
            g = np.asarray(as_host(gt_boxes).numpy(), dtype=np.float32)
            lab = np.asarray(as_host(gt_labels).numpy()).reshape(-1).astype(np.int64)
            if g.ndim != 2 or g.shape[0] != lab.shape[0]:
                raise ValueError('ResidentStore.append: gt_boxes [G, dim] with gt_labels [G], got %s and %s' % (g.shape, lab.shape))
            width = min(g.shape[1], BOX_DIM)
            boxes = np.zeros((g.shape[0], BOX_DIM), dtype=np.float32)
            boxes[:, :width] = g[:, :width]
            labels = lab
        pairs = self._int32_pairs(occ_pairs)
        # every check has passed: from here on the tables change
        self._upload(self._feats.room(1)[0], feats)
        if pairs.shape[0]:
            self._upload(self._pairs.room(pairs.shape[0]), torch.from_numpy(pairs))
        self._w2p.append(w2p)
        self._origin.append(org)
        self._boxes.append(boxes)
        self._labels.append(labels)
        self._lens.append(pairs.shape[0])
        self._index[sample_idx] = len(self.keys)
        self.keys.append(sample_idx)
        return len(self.keys) - 1

    @staticmethod
    def _int32_pairs(occ_pairs):
        """(voxel, class) pairs of one viewpoint as int32 [n, 2], values beyond int32 saturated (``pack_occ_gts``'s rule)."""
        a = occ_pairs
        if isinstance(a, (list, tuple)):
            a = a[0] if len(a) else None                       # occ_gts[b][queue_index], as the head reads it
        if a is None:
            return np.zeros((0, 2), dtype=np.int32)
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if a.size == 0:
            return np.zeros((0, 2), dtype=np.int32)
        if not np.issubdtype(a.dtype, np.integer) or a.ndim != 2 or a.shape[1] != 2:
            raise ValueError('ResidentStore.append: occ_pairs is an integer [n, 2] array, got %s %s' % (a.dtype, a.shape))
        if a.dtype.itemsize > 4 or a.dtype == np.uint32:
            lim = np.iinfo(np.int32)
            return np.clip(a, lim.min, lim.max).astype(np.int32)
        return np.ascontiguousarray(a, dtype=np.int32)

    def freeze(self):
        """Close the store: the small tables (cameras, padded boxes, counts, CSR offsets) go to the device, the feature and
        pair tables are cut to what was appended.  -> self."""
        if self.frozen:
            return self
        V = len(self.keys)
        if V == 0:
            raise RuntimeError('ResidentStore.freeze: the store is empty')
        dev = self.device
        counts = np.array([b.shape[0] for b in self._boxes], dtype=np.int32)
        self.max_boxes = int(counts.max())
        boxes = np.zeros((V, self.max_boxes, BOX_DIM), dtype=np.float32)
        labels = np.zeros((V, self.max_boxes), dtype=np.int64)
        for i, (b, lab) in enumerate(zip(self._boxes, self._labels)):
            boxes[i, :counts[i]] = b
            labels[i, :counts[i]] = lab
        self._pair_lens = np.asarray(self._lens, dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(self._pair_lens)]).astype(np.int64)
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        cut = lambda grown, n: grown.table if grown.table.shape[0] == n else grown.table[:n].clone()
        self.feats = cut(self._feats, V)                      # (a table that doubled as it filled is cut to size: nbytes is what is held)
        self.world2pixel, self.origin = to_dev(np.stack(self._w2p)), to_dev(np.stack(self._origin))
        self.boxes, self.labels, self.counts = to_dev(boxes), to_dev(labels), to_dev(counts)
        self.pairs, self.pair_offsets = cut(self._pairs, int(offsets[-1])), to_dev(offsets)
        if dev.type == 'cuda':
            torch.cuda.current_stream(dev).synchronize()       # (the last staged upload: the staging buffer is dropped now)
        self._feats = self._pairs = self._stage = self._stage_done = None
        self._w2p = self._origin = self._boxes = self._labels = self._lens = None
        self.frozen = True
        return self

    @classmethod
    def from_stores(cls, feature_store, camera_store, sample_ids, annotations=None, device='cuda', feat_dtype=torch.float32):
        """A frozen store of ``sample_ids`` ('<scan>_<vp>') out of a ``volume_io.FeatureStore`` and a
        ``camera_store.CameraStore``.  ``annotations``: None, or a mapping / callable ``sample_idx -> dict`` with any of
        ``gt_boxes``, ``gt_labels``, ``occ_pairs``.  The feature store's own host cache is emptied viewpoint by viewpoint, so
        the split is never on the host as a whole."""
        sample_ids = list(sample_ids)
        store = cls(device=device, feat_dtype=feat_dtype, viewpoints=len(sample_ids))
        for sid in sample_ids:
            ann = {} if annotations is None else (annotations(sid) if callable(annotations) else annotations.get(sid)) or {}
            w2p, org = camera_store.lookup(sid)
            store.append(sid, feature_store.viewpoint(sid), w2p, org, ann.get('gt_boxes'), ann.get('gt_labels'), ann.get('occ_pairs'))
            cache = getattr(feature_store, '_cache', None)
            if isinstance(cache, dict):
                cache.clear()
        return store.freeze()

    @classmethod
    def from_tables(cls, keys, feats, world2pixel, origin, boxes=None, labels=None, counts=None, pairs=None, pair_offsets=None,
                    feat_tail=None):
        """A frozen store around tables that ARE on their device already (a split assembled there, a benchmark's random
        one), used as they are: ``feats [V, Ncam, row]`` f32 | bf16, ``world2pixel [V, Ncam, 4, 4]``, ``origin [V, 3]``,
        ``boxes f32 [V, cap, 9]`` with ``labels int64 [V, cap]`` and ``counts int32 [V]`` (default: no boxes), ``pairs int32
        [total, 2]`` with ``pair_offsets int64 [V + 1]`` (default: no pairs).  ``feat_tail``: the shape a fetched row is
        viewed as (default ``(row,)``; vocc.py: ``(196, 768)``).  One host read, of the CSR offsets, for ``max_pairs``."""
        keys = [str(k) for k in keys]
        V, dev = len(keys), feats.device
        store = cls(device=dev, feat_dtype=feats.dtype)
        if feats.dim() != 3 or feats.shape[0] != V or V == 0 or len(set(keys)) != V:
            raise ValueError('ResidentStore.from_tables: %d distinct keys for feats %s ([V, Ncam, row])' % (len(set(keys)), tuple(feats.shape)))
        ncam, row = int(feats.shape[1]), int(feats.shape[2])
        tail = (row,) if feat_tail is None else tuple(int(s) for s in feat_tail)
        if int(np.prod(tail)) != row:
            raise ValueError('ResidentStore.from_tables: feat_tail %s for rows of %d' % (tail, row))
        if boxes is None:
            boxes = torch.zeros(V, 0, BOX_DIM, dtype=torch.float32, device=dev)
            labels, counts = torch.zeros(V, 0, dtype=torch.int64, device=dev), torch.zeros(V, dtype=torch.int32, device=dev)
        if pairs is None:
            pairs, pair_offsets = torch.zeros(0, 2, dtype=torch.int32, device=dev), torch.zeros(V + 1, dtype=torch.int64, device=dev)
        cap, total = int(boxes.shape[1]), int(pairs.shape[0])
        for t, name, dtype, shape in ((feats, 'feats', feats.dtype, (V, ncam, row)), (world2pixel, 'world2pixel', torch.float32, (V, ncam, 4, 4)),
                                      (origin, 'origin', torch.float32, (V, 3)), (boxes, 'boxes', torch.float32, (V, cap, BOX_DIM)),
                                      (labels, 'labels', torch.int64, (V, cap)), (counts, 'counts', torch.int32, (V,)),
                                      (pairs, 'pairs', torch.int32, (total, 2)), (pair_offsets, 'pair_offsets', torch.int64, (V + 1,))):
            if t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
                raise ValueError('ResidentStore.from_tables: %s must be contiguous %s %s on %s, got %s %s on %s'
                                 % (name, dtype, shape, dev, t.dtype, tuple(t.shape), t.device))
        offsets = pair_offsets.cpu().numpy()
        if offsets[0] != 0 or offsets[-1] != total or (np.diff(offsets) < 0).any():
            raise ValueError('ResidentStore.from_tables: pair_offsets must ascend from 0 to %d' % total)
        store.keys, store._index = keys, {k: i for i, k in enumerate(keys)}
        store.num_cams, store.row, store.feat_tail = ncam, row, tail
        store.feats, store.world2pixel, store.origin = feats, world2pixel, origin
        store.boxes, store.labels, store.counts, store.max_boxes = boxes, labels, counts, cap
        store.pairs, store.pair_offsets, store._pair_lens = pairs, pair_offsets, np.diff(offsets).astype(np.int64)
        store._feats = store._pairs = None
        store._w2p = store._origin = store._boxes = store._labels = store._lens = None
        store.frozen = True
        return store

    # ---- lookups ------------------------------------------------------------------------------------------------------
    def _need_frozen(self, who):
        if not self.frozen:
            raise RuntimeError('ResidentStore.%s: call freeze() first' % who)

    def __len__(self):
        return len(self.keys)

    def index_of(self, sample_idx):
        """The index of viewpoint '<scan>_<vp>' (``KeyError`` when it is not in the store)."""
        return self._index[str(sample_idx)]

    @property
    def nbytes_by_table(self):
        self._need_frozen('nbytes')
        names = ('feats', 'world2pixel', 'origin', 'boxes', 'labels', 'counts', 'pairs', 'pair_offsets')
        return {k: getattr(self, k).numel() * getattr(self, k).element_size() for k in names}

    @property
    def nbytes(self):
        return sum(self.nbytes_by_table.values())

    def max_pairs(self, bs):
        """The largest pair total of any ``bs`` different viewpoints -- the sum of the ``bs`` longest: the ``pair_capacity`` no
        batch of distinct viewpoints overflows.  (Past ``len(store)`` samples the longest one is counted again; an index
        vector that repeats long viewpoints can still overflow, which ``status`` reports.)"""
        self._need_frozen('max_pairs')
        bs, lens = int(bs), np.sort(self._pair_lens)[::-1]
        return int(lens[:bs].sum() + max(0, bs - lens.size) * lens[0]) if bs > 0 else 0

    # ---- fetching -----------------------------------------------------------------------------------------------------
    def _device_index(self, index, out):
        """The device int32 index vector of a call: a device tensor as it is; host data through pinned memory and one
        asynchronous copy (into ``out.index`` when there is one) out of a pinned staging buffer the store keeps, with no
        synchronisation."""
        if torch.is_tensor(index) and index.is_cuda and index.device == self.device:
            if index.dtype != torch.int32 or index.dim() != 1:
                raise TypeError('ResidentStore.fetch: a device index is int32 [bs], got %s %s' % (index.dtype, tuple(index.shape)))
            return index
        host = torch.as_tensor(index, device='cpu').to(torch.int32).reshape(-1)
        if self.device.type != 'cuda':
            return host
        # the store's ONE pinned index buffer, kept and reused from call to call.  Nothing here waits: should the previous
        # copy out of it still be in flight (the host ran a whole step ahead), this call takes pinned memory of its own.
        n = host.numel()
        slot = getattr(self, '_index_stage', None)
        if slot is None or slot[0].numel() < n:
            slot = self._index_stage = [torch.empty(max(n, 64), dtype=torch.int32, pin_memory=True), None]
        busy = slot[1] is not None and not slot[1].query()
        staged = host.pin_memory() if busy else slot[0][:n].copy_(host)
        if out is not None and out.index is not None and out.index.shape == staged.shape:
            dev = out.index.copy_(staged, non_blocking=True)
        else:
            dev = staged.to(self.device, non_blocking=True)
        if not busy:
            slot[1] = torch.cuda.Event()
            slot[1].record()                                   # behind the copy: the buffer is free once it has passed
        return dev

    def new_batch(self, bs, box_capacity=None, pair_capacity=None):
        """Buffers of a ``ResidentBatch`` of ``bs`` samples (box tables and pair table start as zeros); ``box_capacity``
        defaults to ``max_boxes``, ``pair_capacity`` to ``max_pairs(bs)``."""
        self._need_frozen('new_batch')
        dev, bs = self.device, int(bs)
        cap = self.max_boxes if box_capacity is None else int(box_capacity)
        pcap = self.max_pairs(bs) if pair_capacity is None else int(pair_capacity)
        if cap < 0 or not 0 <= pcap < 2 ** 31:
            raise ValueError('ResidentStore: box_capacity=%d pair_capacity=%d' % (cap, pcap))
        gts = PaddedGts(torch.zeros(bs, cap, BOX_DIM, dtype=torch.float32, device=dev),
                        torch.zeros(bs, cap, dtype=torch.int64, device=dev), torch.zeros(bs, dtype=torch.int32, device=dev))
        occ = hipops.PackedOccGts(torch.zeros(2 * (bs + 1) + 2 * pcap, dtype=torch.int32, device=dev), bs, pcap, 0, False)
        return ResidentBatch(torch.empty((self.num_cams, bs) + self.feat_tail, dtype=self.feat_dtype, device=dev),
                             torch.empty(bs, self.num_cams, 4, 4, dtype=torch.float32, device=dev),
                             torch.empty(bs, 3, dtype=torch.float32, device=dev), gts, occ,
                             torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(bs, dtype=torch.int32, device=dev))

    def fetch(self, index, out=None, box_capacity=None, pair_capacity=None):
        """The batch of the viewpoints ``index`` names -> ``ResidentBatch``.  ``index``: a device int32 tensor [bs], used as it
        is (the kernels read it; the host never does), or a host list / CPU tensor, copied asynchronously through pinned
        memory with no synchronisation.  An index outside the store gives an EMPTY sample (zero features and cameras, no
        boxes, no pairs) and is counted in ``status``; nothing is raised here -- ``check(status)`` reads the status on demand.
        ``out``: an earlier batch (or a ``ResidentBatch`` around a captured step's static buffers) to write into; nothing is
        allocated then, and a group whose tensors are None in it is not fetched.  Box columns at or past a sample's count and
        pairs behind ``occ.offsets[bs]`` are left as they were.  ``box_capacity`` / ``pair_capacity``: the sizes of a new
        batch's tables (default: ``max_boxes``, ``max_pairs(bs)``).  On the GPU: ``ver_fetch_batch``, at most four launches
        on the current stream, capturable; CPU stores go through ``hipops.fetch_batch_host``."""
        self._need_frozen('fetch')
        index = self._device_index(index, out)
        bs = index.numel()
        if out is None:
            out = self.new_batch(bs, box_capacity, pair_capacity)
        elif box_capacity is not None or pair_capacity is not None:
            raise ValueError('ResidentStore.fetch: the capacities of out= are those of its tables')
        out = out._replace(index=index)
        V = len(self.keys)
        gts, occ = out.gts, out.occ
        if (out.world2pixel is None) != (out.origin is None):
            raise ValueError('ResidentStore.fetch: out.world2pixel and out.origin come together')
        if occ is not None and (occ.has_invalid or occ.bs != bs):
            raise ValueError('ResidentStore.fetch: out.occ holds %d samples%s, the index %d'
                             % (occ.bs, ' and invalid voxels' if occ.has_invalid else '', bs))
        if self.device.type == 'cuda':
            hipops.fetch_batch(
                index, V,
                feats=None if out.feats is None else (self.feats, out.feats),
                cameras=None if out.world2pixel is None else (self.world2pixel, self.origin, out.world2pixel, out.origin),
                boxes=None if gts is None else (self.boxes, self.labels, self.counts, gts.boxes, gts.labels, gts.counts),
                pairs=None if occ is None else (self.pairs, self.pair_offsets, occ.offsets, occ.pairs), status=out.status)
            return out
        return self._fetch_host(index, out)

    def _fetch_host(self, index, out):
        """The CPU route: ``hipops.fetch_batch_host`` on numpy views of the tables, written back into ``out``."""
        raw = lambda t: t.view(torch.int16).numpy() if t.dtype == torch.bfloat16 else t.numpy()
        gts, occ = out.gts, out.occ
        kw, prev = {}, {}
        if out.feats is not None:
            kw['feats'] = raw(self.feats)
        if out.world2pixel is not None:
            kw.update(world2pixel=self.world2pixel.numpy(), origin=self.origin.numpy())
        if gts is not None:
            kw.update(boxes=self.boxes.numpy(), labels=self.labels.numpy(), counts=self.counts.numpy(), out_cap=gts.boxes.shape[1])
            prev.update(boxes=gts.boxes.numpy(), labels=gts.labels.numpy())
        if occ is not None:
            kw.update(pairs=self.pairs.numpy(), pair_offsets=self.pair_offsets.numpy(), pair_capacity=occ.pairs.shape[0])
            prev['pairs'] = occ.pairs.numpy()
        got = hipops.fetch_batch_host(index.numpy(), V=len(self.keys), out=prev, **kw)
        put = lambda dst, a: dst.copy_(torch.from_numpy(a).view(dst.dtype).reshape(dst.shape))
        if out.feats is not None:
            put(out.feats, got['feats'])
        if out.world2pixel is not None:
            put(out.world2pixel, got['world2pixel'])
            put(out.origin, got['origin'])
        if gts is not None:
            put(gts.boxes, got['boxes'])
            put(gts.labels, got['labels'])
            put(gts.counts, got['counts'])
        if occ is not None:
            put(occ.offsets, got['offsets'])
            put(occ.pairs, got['pairs'])
        put(out.status, got['status'])
        return out

    @staticmethod
    def check(status):
        """Read the four status words of a fetch (ONE synchronisation, only when asked) and raise ``ValueError`` with a
        sentence per non-zero word; -> the words as a tuple when all is well.  ``status``: the tensor or a ``ResidentBatch``."""
        if isinstance(status, ResidentBatch):
            status = status.status
        outside, cut, overflow, total = (int(v) for v in status.tolist())
        said = []
        if outside:
            said.append('%d sample(s) had an index outside the store and were fetched as empty samples.' % outside)
        if cut:
            said.append('%d sample(s) hold more boxes than the box capacity; the surplus was dropped.' % cut)
        if overflow:
            said.append('The batch holds %s%d pairs, more than the pair capacity; the surplus was dropped.'
                        % ('at least ' if total == 2 ** 31 - 1 else '', total))
        if said:
            raise ValueError('ResidentStore.check: ' + ' '.join(said))
        return outside, cut, overflow, total
