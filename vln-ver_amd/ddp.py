"""Data-parallel training of the lifting path: one process per GPU, viewpoints sharded across
ranks, gradients summed with one bucketed all-reduce (RCCL over xGMI through
``torch.distributed``; ``gloo`` on CPU for the logic tests).

The path shards by independent units (a viewpoint = 6 views -> one volume); there is no data-path
collective, only the gradient sum.  Reference behaviour being mirrored:
* ``MMDistributedDataParallel(model, broadcast_buffers=False, find_unused_parameters=True)``
  (apis/mmdet_train.py:71-80) -> torch DDP; we freeze what the step does not touch instead of
  paying ``find_unused_parameters``;
* ``DistributedGroupSampler`` (datasets/samplers/group_sampler.py:62-103): every rank derives the
  same seed+epoch permutation and takes its contiguous slice -> :func:`shard_indices`;
* ``reduce_mean`` of the loss normalisers (mmdet, head:954,964) -> :func:`reduce_mean`.

``GradExchange`` is the second route for the gradient sum, for steps that are replayed as hipGraphs
(``graphs.GraphedLiftStep(..., exchange=)``): no DistributedDataParallel wrapper, one launch packs every gradient into
one flat buffer (``ver_grad_pack``, fp32 or bf16 on the wire), ONE eager all-reduce exchanges it, and
``optim.ClipAdamW.step(exchange)`` reads the gradients from that buffer.
"""
import math

import numpy as np
import torch
import torch.distributed as dist


def shard_indices(group_flags, world_size, rank, samples_per_gpu=1, seed=0, epoch=0):
    """Indices this rank visits in ``epoch`` -- same rule as the reference sampler: per group a
    ``torch.randperm`` (generator seeded with epoch+seed), padded by repetition to a multiple of
    samples_per_gpu*world_size, then a permutation of the samples_per_gpu-sized chunks, then the
    rank's contiguous slice."""
    flags = torch.as_tensor(group_flags, dtype=torch.long)
    sizes = torch.bincount(flags)
    g = torch.Generator()
    g.manual_seed(epoch + seed)
    num_samples = sum(int(math.ceil(int(s) / samples_per_gpu / world_size)) * samples_per_gpu for s in sizes)
    indices = []
    for i, size in enumerate(sizes.tolist()):
        if size == 0:
            continue
        where = torch.nonzero(flags == i).squeeze(1)
        ind = where[torch.randperm(size, generator=g)].tolist()
        extra = int(math.ceil(size / samples_per_gpu / world_size)) * samples_per_gpu * world_size - len(ind)
        tmp = list(ind)
        for _ in range(extra // size):
            ind.extend(tmp)
        ind.extend(tmp[:extra % size])
        indices.extend(ind)
    assert len(indices) == num_samples * world_size
    chunks = torch.randperm(len(indices) // samples_per_gpu, generator=g).tolist()
    indices = [indices[j] for c in chunks for j in range(c * samples_per_gpu, (c + 1) * samples_per_gpu)]
    off = num_samples * rank
    return indices[off:off + num_samples]


def reduce_mean(t):
    """mmdet.core.reduce_mean: all-reduce(sum)/world (identity when not distributed)."""
    if not (dist.is_available() and dist.is_initialized()):
        return t
    t = t.clone()
    dist.all_reduce(t.div_(dist.get_world_size()), op=dist.ReduceOp.SUM)
    return t


def wrap_ddp(module, device=None, bucket_cap_mb=200, bf16_gradients=True):
    """DDP wrapper used by bench.py.  bf16-compressed buckets halve the bytes on the xGMI links
    (ring all-reduce time is set by one 153 GB/s link: 2*(N-1)/N * bytes / link_bw); 200 MB
    buckets keep each of the three 88 MB (bf16) up_sample gradients in its own reduce so the
    first ones overlap the rest of the backward."""
    ids = [device.index] if (device is not None and device.type == 'cuda') else None
    ddp = torch.nn.parallel.DistributedDataParallel(module, device_ids=ids, gradient_as_bucket_view=True,
                                                    bucket_cap_mb=bucket_cap_mb, broadcast_buffers=False)
    if bf16_gradients and ids is not None:
        from torch.distributed.algorithms.ddp_comm_hooks import default_hooks
        ddp.register_comm_hook(None, default_hooks.bf16_compress_hook)
    return ddp


def flat_layout(sizes, align=8):
    """Where ``GradExchange`` puts tensors of ``sizes`` elements in its flat buffer -> (offsets, total): the running sum of
    the sizes, each rounded up to ``align`` = 8 elements (16 bytes of bf16, 32 of fp32), so that every tensor starts on a
    vector boundary in either wire dtype.  Pure host arithmetic."""
    offsets, total = [], 0
    for n in sizes:
        n = int(n)
        if n < 0:
            raise ValueError('flat_layout: a negative size')
        offsets.append(total)
        total += -(-n // align) * align
    return offsets, total


class GradExchange:
    """The gradients of a FIXED, ordered list of dense fp32 GPU parameters, exchanged through one flat buffer.

    ``params``: parameters, or ``(name, parameter)`` pairs as ``module.named_parameters()`` yields them (the names appear in
    error messages); ``wire_dtype``: ``torch.bfloat16`` (half the bytes; every gradient rounded once to nearest-even before
    the sum) or ``torch.float32``; ``group``: the process group, default the world.  Without an initialised process group
    the exchange still packs (scale 1) and ``all_reduce`` does nothing -- one rank, the same code path.

    The object owns the flat buffer (zero-filled once; the padding between tensors is never written, so it stays zero
    through every sum), the device tables ``ver_grad_pack`` reads and the pinned staging buffer of the pointer upload.  A
    step is ``pack()`` -> ``all_reduce()`` -> ``optimizer.step(exchange)``; ``p.grad`` is left as it was.

    Under stream capture ``pack()`` follows the rules of ``optim.ClipAdamW._upload``: the staging buffer is pinned by
    ``prepare_capture()`` BEFORE the capture, the copy of the pointer table becomes a graph node that re-runs on every replay
    (the replay therefore always packs the capture's own gradient buffers), and every buffer a graph reads by raw address
    stays referenced for the life of this object.  ``replayed()`` after a replay forgets the host's record of the device
    table, so that the next eager ``pack()`` uploads its pointers again."""

    def __init__(self, params, wire_dtype=torch.bfloat16, group=None):
        from .optim import ClipAdamW
        if wire_dtype not in (torch.bfloat16, torch.float32):
            raise TypeError('GradExchange: wire_dtype torch.bfloat16 or torch.float32, got %s' % (wire_dtype,))
        named = [q if isinstance(q, (tuple, list)) else (None, q) for q in params]
        self.params = [p for _, p in named]
        self.names = [k if k is not None else 'parameter %d %s' % (i, tuple(p.shape)) for i, (k, p) in enumerate(named)]
        if not self.params:
            raise ValueError('GradExchange: an empty parameter list')
        if len({id(p) for p in self.params}) != len(self.params):
            raise ValueError('GradExchange: a parameter appears twice')
        for k, p in zip(self.names, self.params):
            if not (torch.is_tensor(p) and p.is_cuda and p.dtype == torch.float32 and not p.is_sparse and p.is_contiguous()):
                raise TypeError('GradExchange: dense fp32 GPU parameters only (%s)' % k)
        dev = self.params[0].device
        if any(p.device != dev for p in self.params):
            raise ValueError('GradExchange: parameters on more than one device')
        self.device, self.wire_dtype, self.group = dev, wire_dtype, group
        self.distributed = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if self.distributed else 1
        self.chunk = ClipAdamW.CHUNK
        self.sizes = [p.numel() for p in self.params]
        self.offsets, self.total = flat_layout(self.sizes)
        self.flat = torch.zeros(max(self.total, 8), dtype=wire_dtype, device=dev)
        tensor, index = [], []
        for t, n in enumerate(self.sizes):
            c = -(-n // self.chunk)
            tensor += [t] * c
            index += list(range(c))
        self._sizes_dev = torch.tensor(self.sizes, dtype=torch.int64, device=dev)
        self.offsets_dev = torch.tensor(self.offsets, dtype=torch.int64, device=dev)
        self._chunk_tensor = torch.tensor(tensor, dtype=torch.int32, device=dev)
        self._chunk_index = torch.tensor(index, dtype=torch.int32, device=dev)
        self._table = torch.zeros(len(self.params), dtype=torch.int64, device=dev)
        self._ptrs = None            # what the device table holds, while its last writer was an eager pack()
        self._stage = None
        self._keep = []              # pinned sources of captured copies

    @property
    def scale(self):
        return 1.0 / self.world

    def prepare_capture(self):
        """Call right before capturing a graph that contains ``pack()``: pins the staging buffer the captured ``pack()`` fills
        with the addresses of the capture's own gradient buffers (no host allocation inside the capture)."""
        self._stage = torch.empty(len(self.params), dtype=torch.int64).pin_memory()

    def replayed(self):
        """A graph holding ``pack()`` was replayed: its copy node has rewritten the device table behind the host's back."""
        self._ptrs = None

    @torch.no_grad()
    def pack(self):
        """``flat[offsets[t] :] = p_t.grad / world`` for every parameter of the list, one launch on the current stream."""
        from . import hipops
        grads = []
        for k, p in zip(self.names, self.params):
            g = p.grad
            if g is None:
                raise RuntimeError('GradExchange.pack(): %s has no gradient (every parameter of the list takes part in '
                                   'every exchange; freeze it and leave it out, or give it one)' % k)
            if not (g.is_cuda and g.dtype == torch.float32 and not g.is_sparse and g.numel() == p.numel()):
                raise TypeError('GradExchange.pack(): dense fp32 GPU gradients only (%s: %s on %s)' % (k, g.dtype, g.device))
            grads.append(g if g.is_contiguous() else g.contiguous())
        ptrs = [g.data_ptr() for g in grads]
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing or ptrs != self._ptrs:
            array = np.asarray(ptrs, dtype=np.int64)
            if capturing:
                if self._stage is None:
                    raise RuntimeError('GradExchange.pack() inside a graph capture: call `prepare_capture()` right before '
                                       'capturing')
                src, self._stage = self._stage, None
                src.numpy()[:] = array
                self._keep.append(src)
            else:
                src = torch.from_numpy(array).pin_memory()
            self._table.copy_(src, non_blocking=True)
            # (a captured copy has not run, and every replay runs it without the host: no record of it)
            self._ptrs = None if capturing else ptrs
        L = hipops.lib()
        hipops._launch('ver_grad_pack', lambda: L.ver_grad_pack(
            hipops._p(self._table), hipops._p(self._sizes_dev), hipops._p(self.offsets_dev), hipops._p(self._chunk_tensor),
            hipops._p(self._chunk_index), len(self.params), self._chunk_tensor.numel(), self.chunk, self.scale,
            hipops._p(self.flat), 1 if self.wire_dtype == torch.bfloat16 else 0, hipops._stream()))
        # (contiguous copies may go out of scope: the allocator reuses their blocks only behind this launch on the stream)

    def all_reduce(self):
        """ONE ``all_reduce(SUM)`` of the flat buffer (the scale 1 / world is already in it); nothing without a group."""
        if self.distributed:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group)

    @torch.no_grad()
    def broadcast_parameters(self, src=0):
        """Every rank takes rank ``src``'s parameter values -- once, eagerly: what DistributedDataParallel does when it is
        constructed."""
        if self.distributed:
            for p in self.params:
                dist.broadcast(p.data, src=src, group=self.group)

    @torch.no_grad()
    def grads(self):
        """fp32 copies of the exchanged gradients, one per parameter in its shape (tests, debugging)."""
        return [self.flat[o:o + n].to(torch.float32, copy=True).reshape(p.shape) for o, n, p in zip(self.offsets, self.sizes, self.params)]
