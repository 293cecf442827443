"""hipGraph replay of the head (``GraphedHead``), of the whole lifting step (``GraphedLiftStep``) and of the whole multi-task
training step with fresh ground truth per replay (``GraphedTrainStep``) for small, launch-bound batches; both steps also
under data parallelism, as two graphs around one eager all-reduce of a flat gradient buffer (``exchange=``).  Inference --
boxes, per-sample occupancy pairs and the volume of a viewpoint -- replays as one graph too (``GraphedInference``).

At the reference's own batch point (vocc.py: ``samples_per_gpu=1``) the full multi-task step is bound by the HOST: ~1 500
module calls forward and as many autograd nodes backward, 13-16 ms + 23-28 ms of Python / dispatcher time around ~20 ms of
GPU work (scratch/r03/full_step_host_profile.py).  ``GraphedHead`` records the head's forward and its backward once, for
one fixed batch shape, as two HIP graphs (``torch.cuda.make_graphed_callables``) and replays them: the Hungarian assignment,
the loss terms, gradient clipping and the optimizer stay eager between the two.  Everything the graphs contain is what the
eager path launches -- same kernels, same arithmetic, fresh dropout seeds per replay (they come from the device generator).

Nothing per step may change shape: one ``GraphedHead`` per (batch size, dtype); the cameras and features are copied into
the graphs' static inputs on every call.  Build it BEFORE wrapping the head in DistributedDataParallel (PyTorch's rule
for graphed callables).  ``bench.py`` uses it for the ``config.latency`` records of the full multi-task workload on one
rank (``graphed: true`` in the record); the headline step is always eager.

One rule found the hard way (ROCm 7.2 / PyTorch 2.10): NO loss of an earlier eager step may still be referenced when the
graphs are captured.  A live scalar with a spent autograd graph behind it (``last = step()`` kept around for logging) makes
``hipStreamEndCapture`` of the backward graph crash the process -- a segmentation fault, not an exception
(scratch/r03/graphed_full_step.py reproduces it with LIKE_BENCH=3, and not with DEL_LAST=1).  ``GraphedHead`` therefore
looks for such tensors first and refuses with an error that says what to drop.
"""
import gc

import torch


def _live_losses():
    """0-dim tensors that still carry an autograd graph: what a training loop keeps of its previous steps."""
    found = []
    for obj in gc.get_objects():
        try:
            if isinstance(obj, torch.Tensor) and obj.dim() == 0 and obj.grad_fn is not None:
                found.append(obj)
        except Exception:                                  # objects that do not like being inspected
            continue
    return found


class _HeadForward(torch.nn.Module):
    """Tensor-in / tensor-out view of ``VoxelFormerOccupancyHead.forward`` (graphed callables take and return tensors)."""

    def __init__(self, head, autocast_dtype, occupancy_rows):
        super().__init__()
        self.head = head
        self.autocast_dtype = autocast_dtype
        self.occupancy_rows = occupancy_rows
        self.row_plan = None

    def forward(self, feats, world2pixel, origin):
        with torch.autocast('cuda', dtype=self.autocast_dtype or torch.bfloat16, enabled=self.autocast_dtype is not None,
                            cache_enabled=False):
            outs = self.head(feats, None, world2pixel=world2pixel, origin=origin, occupancy_rows=self.occupancy_rows)
        occ = outs['occupancy_preds']
        if isinstance(occ, tuple):                       # (logits in GEMM row order, plan, bs): the plan is host data
            occ, plan, bs = occ
            self.row_plan = (plan, bs)
        return outs['all_cls_scores'].float(), outs['all_bbox_preds'].float(), occ, outs['bev_embed']


class GraphedHead:
    """``outs = GraphedHead(head, feats, w2p, org)(feats, w2p, org)``: the dict ``head.loss`` takes, produced by graph replay.

    feats [Ncam, B, Nk, C], world2pixel [B, Ncam, 4, 4], origin [B, 3] on the GPU are the SAMPLE inputs that fix the
    shapes; ``autocast_dtype=torch.bfloat16`` (default) runs the head under bf16 autocast as ``bench.py`` does, None in
    fp32.  The head must be in the mode (train / eval) and have the ``requires_grad`` flags it will be used with (checked
    on every call).  Outputs are valid until the next call (they alias the graphs' static buffers)."""

    def __init__(self, head, feats, world2pixel, origin, autocast_dtype=torch.bfloat16, occupancy_rows=True,
                 check_live_losses=True):
        if not feats.is_cuda:
            raise RuntimeError('GraphedHead needs GPU tensors (HIP graphs)')
        if head.only_occ or head.only_det or head.add_layout:
            raise NotImplementedError('GraphedHead covers the default multi-task branch of the head')
        if getattr(head, 'getbev', None) is not None:
            raise NotImplementedError('GraphedHead: a head built with getbev=<store> writes volumes to the host inside '
                                      'forward (device -> host copies and file I/O), which cannot be captured')
        self.head, self.training = head, head.training
        self.grad_flags = [p.requires_grad for p in head.parameters()]
        if check_live_losses:
            gc.collect()
            n = len(_live_losses())
            if n:
                raise RuntimeError(
                    'GraphedHead: %d scalar tensor(s) with an autograd graph are still alive (losses of earlier eager '
                    'steps?).  Drop them (`loss = None`, or keep `loss.detach()` / `float(loss)`) before building the '
                    'graphs: with one alive, ending the capture of the backward graph crashes the process on this '
                    'ROCm / PyTorch build (vln-ver_amd/graphs.py).' % n)
        self.module = _HeadForward(head, autocast_dtype, occupancy_rows)
        self.graphed = torch.cuda.make_graphed_callables(self.module, (feats, world2pixel, origin), allow_unused_input=True)

    def __call__(self, feats, world2pixel, origin):
        """NOTE: the returned tensors ALIAS the graph's static output buffers -- ``bev_embed``, the class scores and the
        boxes are overwritten by the next call; clone what has to survive it."""
        if self.head.training != self.training or [p.requires_grad for p in self.head.parameters()] != self.grad_flags:
            raise RuntimeError('GraphedHead: head.training / requires_grad flags differ from capture time; build a new '
                               'GraphedHead for the new mode')
        cls, box, occ, bev = self.graphed(feats, world2pixel, origin)
        if self.module.row_plan is not None:
            occ = (occ,) + self.module.row_plan
        return dict(bev_embed=bev, all_cls_scores=cls, all_bbox_preds=box, all_layout_preds=None, occupancy_preds=occ,
                    flow_preds=None, enc_cls_scores=None, enc_bbox_preds=None, enc_occupancy_preds=None)


def _check_exchange(who, optimizer, exchange):
    """An exchange for a captured step covers exactly the optimizer's trainable parameters (the order is the exchange's)."""
    mine = {id(p) for group in optimizer.param_groups for p in group['params'] if p.requires_grad}
    theirs = {id(p) for p in exchange.params}
    if mine != theirs:
        raise ValueError('%s: the exchange lists %d parameters, the optimizer trains %d, %d in common; the captured update '
                         'reads every gradient from the exchange, so the two lists must hold the same parameters'
                         % (who, len(theirs), len(mine), len(mine & theirs)))


def _exchanged_update(optimizer, exchange):
    """The eager tail of a data-parallel step: pack, ONE all-reduce, clipped AdamW from the flat buffer -> clip norm."""
    exchange.pack()
    exchange.all_reduce()
    return optimizer.step(exchange=exchange)


class GraphedLiftStep:
    """One training step of the lifting path -- forward, occupancy loss, backward, gradient clipping + AdamW -- for ONE fixed
    batch shape, captured as a single hipGraph and replayed: the reference's own operating point (vocc.py:222
    ``samples_per_gpu=1``) is bound by the host in the eager step (~450 launches behind ~9 ms of Python / dispatcher time for
    ~4 ms of GPU work).  Same kernels, same arithmetic as the eager step; dropout seeds come from the device generator and
    advance per replay; ``optim.ClipAdamW`` keeps its pointer table, hyper-parameters and per-tensor update counts on the
    device, so the captured update uses the right bias corrections on every replay (``optimizer.replayed()`` keeps the host's
    counts in step, ``optimizer.refresh()`` uploads a learning rate a scheduler has moved).

    Eager steps of the same optimizer may run between the calls (the ragged last batch of an epoch), with either
    ``zero_grad`` mode: every replay rewrites the optimizer's device pointer table to this capture's gradient buffers, so
    ``replayed()`` drops the host's record of that table and the next eager step uploads its own pointers again.  The graph
    reads the optimizer's device buffers by raw address: ``optimizer.load_state_dict``, unpickling, or an eager step over
    another set of tensors (a parameter whose first gradient arrives after the capture) replaces them and makes this object
    unusable -- ``refresh()`` raises at the top of the next call, before the replay; build a new GraphedLiftStep then.

    ``model(feats, w2p, org, gt) -> scalar loss`` (bench.py's LiftTrainer); ``optimizer``: a ClipAdamW over the model's trainable
    parameters.  Construction runs ``warmup`` REAL eager steps on the sample inputs (allocator, AdamW state, library
    heuristics) before the capture -- they train the model like any other step.  One rank only: the gradient all-reduce of
    DistributedDataParallel is not part of the graph.  ``loss = step(feats, w2p, org, gt)`` copies the inputs into the graph's
    static buffers (unless they ARE those buffers: ``step.inputs``) and returns the graph's loss tensor, overwritten by the
    next call.

    ``exchange``: a ``ddp.GradExchange`` over the optimizer's trainable parameters -- the step under data parallelism, with
    no DistributedDataParallel wrapper around the model.  Construction first broadcasts rank 0's parameters (when a process
    group exists); the warm-up steps are eager exchanged steps (backward, ``exchange.pack()``, ``exchange.all_reduce()``,
    ``optimizer.step(exchange)``); then TWO graphs are captured on one stream, the second in the memory pool of the first:
    A = forward + loss + backward + ``exchange.pack()``, B = ``optimizer.step(exchange)``.  A call replays A, all-reduces the
    ONE flat buffer eagerly (the collective is not part of a graph) and replays B.  Without a process group the all-reduce
    is nothing and the scale is 1: the same two graphs on one rank."""

    def __init__(self, model, optimizer, feats, world2pixel, origin, gt, warmup=3, check_live_losses=True, exchange=None):
        if not feats.is_cuda:
            raise RuntimeError('GraphedLiftStep needs GPU tensors (HIP graphs)')
        if not hasattr(optimizer, 'prepare_capture'):
            raise TypeError('GraphedLiftStep needs an optimizer whose step() can be captured (optim.ClipAdamW)')
        self.model, self.optimizer, self.exchange = model, optimizer, exchange
        if exchange is not None:
            _check_exchange('GraphedLiftStep', optimizer, exchange)
            exchange.broadcast_parameters()
        self.inputs = tuple(t.detach().clone() for t in (feats, world2pixel, origin, gt))
        self.training = model.training
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            norm = None
            for _ in range(max(1, warmup)):                 # (at least one: the optimizer state must exist before the capture)
                optimizer.zero_grad(set_to_none=True)
                loss = model(*self.inputs)
                loss.backward()
                norm = optimizer.step() if exchange is None else _exchanged_update(optimizer, exchange)
            self._clean_warmup = norm is not None and bool(torch.isfinite(norm))
            self._unchecked = 3
            loss = None
            optimizer.zero_grad(set_to_none=True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if check_live_losses:
            gc.collect()
            n = len(_live_losses())
            if n:
                raise RuntimeError('GraphedLiftStep: %d scalar tensor(s) with an autograd graph are still alive (losses of '
                                   'earlier eager steps?); drop them before building the graph (see GraphedHead)' % n)
        optimizer.prepare_capture()
        self.graph = torch.cuda.CUDAGraph()
        if exchange is None:
            with torch.cuda.graph(self.graph):
                loss = model(*self.inputs)
                loss.backward()
                self.grad_norm = optimizer.step()
                self.loss = loss.detach()
        else:
            exchange.prepare_capture()
            stream = torch.cuda.Stream()
            with torch.cuda.graph(self.graph, stream=stream):
                loss = model(*self.inputs)
                loss.backward()
                exchange.pack()
                self.loss = loss.detach()
            self.update_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.update_graph, pool=self.graph.pool(), stream=stream):
                self.grad_norm = optimizer.step(exchange=exchange)
        loss = None

    def __call__(self, feats, world2pixel, origin, gt):
        if self.model.training != self.training:
            raise RuntimeError('GraphedLiftStep: model.training differs from capture time')
        for dst, src in zip(self.inputs, (feats, world2pixel, origin, gt)):
            if src is not dst:
                if src.shape != dst.shape or src.dtype != dst.dtype:
                    raise RuntimeError('GraphedLiftStep: input %s %s, captured with %s %s' % (tuple(src.shape), src.dtype, tuple(dst.shape), dst.dtype))
                dst.copy_(src, non_blocking=True)
        self.optimizer.refresh()
        self.graph.replay()
        if self.exchange is not None:
            self.exchange.all_reduce()
            self.update_graph.replay()
            self.exchange.replayed()
        self.optimizer.replayed()
        if self._unchecked:
            # the first replays are checked (one synchronisation each): a replay that leaves a non-finite gradient norm behind
            # after a clean capture step is the runtime's memset-node problem (vln-ver_amd/__init__.py), not the model's
            self._unchecked -= 1
            if not bool(torch.isfinite(self.grad_norm)) and self._clean_warmup:
                raise RuntimeError(
                    'GraphedLiftStep: the gradient norm of a replayed step is not finite although the eager warm-up steps were '
                    'clean.  On ROCm 7.2 hipGraph replay needs DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 in the environment BEFORE the '
                    'first GPU call of the process (memset nodes are not ordered against the kernels behind them otherwise); '
                    'importing vln-ver_amd sets it, but only takes effect if HIP was not initialised earlier.')
        return self.loss


class MultiTaskStep(torch.nn.Module):
    """The full multi-task training step's forward, from tensors of fixed shapes to the loss dict, through the head's public
    API alone: ``head(..., occupancy_rows=True)``, ``head.occupancy_targets_device`` on the packed sparse pairs
    (``ver_occ_targets``: byte labels in the GEMMs' row order) and ``head.loss`` with a ``PaddedGts`` -- with
    ``train_cfg.assigner.solver = 'fused'`` nothing in it touches the host after its first call, so ``GraphedTrainStep`` can
    capture it; called eagerly it is that step's twin.  ``autocast_dtype``: torch.bfloat16 as ``bench.py`` trains, None =
    fp32.  ``targets`` holds the ``OccupancyTargets`` of the last call (its ``bad`` counters: ``GraphedTrainStep.flags``)."""

    def __init__(self, head, autocast_dtype=torch.bfloat16):
        super().__init__()
        self.head, self.autocast_dtype = head, autocast_dtype
        self.targets = None

    def forward(self, feats, world2pixel, origin, gts, occ):
        """feats [Ncam, B, Nk, C], world2pixel [B, Ncam, 4, 4], origin [B, 3]; gts: ``PaddedGts`` (``head.pad_gts``); occ:
        ``hipops.PackedOccGts`` on the GPU -- pairs at or past ``occ.offsets[B]`` belong to no sample."""
        head = self.head
        with torch.autocast('cuda', dtype=self.autocast_dtype or torch.bfloat16, enabled=self.autocast_dtype is not None,
                            cache_enabled=False):
            outs = head(feats, None, world2pixel=world2pixel, origin=origin, occupancy_rows=True)
        outs = {k: (v.float() if torch.is_tensor(v) and k != 'occupancy_preds' else v) for k, v in outs.items()}
        self.targets = head.occupancy_targets_device(occ, device=feats.device)
        return head.loss(gts, None, self.targets, outs)


def check_step_inputs(who, captured, offered):
    """The host-side size checks of ``GraphedTrainStep``, on host data alone: ``captured`` and ``offered`` are sequences of
    ``(name, shape, dtype, ragged)`` of the static buffers and of a call's tensors.  ``ragged`` names the axis along which
    a call may bring LESS than the buffer holds (boxes per sample, pairs) and the limit's name; every other axis, and the
    dtype, must be what was captured.  Raises ``ValueError``."""
    for (name, shape, dtype, ragged), (_, got, got_dtype, _) in zip(captured, offered):
        shape, got = tuple(shape), tuple(got)
        if ragged is not None and len(got) == len(shape) and got[ragged[0]] > shape[ragged[0]]:
            raise ValueError('%s: %s holds %d %s, the %s captured is %d' % (who, name, got[ragged[0]], ragged[1], ragged[2],
                                                                            shape[ragged[0]]))
        same = len(got) == len(shape) and all(a == b or (ragged is not None and i == ragged[0]) for i, (a, b) in enumerate(zip(got, shape)))
        if not same or got_dtype != dtype:
            raise ValueError('%s: %s is %s %s, captured with %s %s' % (who, name, got, got_dtype, shape, dtype))


def _fetch_into(who, step, store, index, gts, occ):
    """``store.fetch`` (``resident.ResidentStore``) straight into a captured step's static buffers: eager launches on the
    current stream, in front of the replay.  The store's camera count, row size and dtype are held against the captured
    feature buffer first, on host data alone and before any launch.  -> the status tensor (``store.check`` reads it)."""
    from .resident import ResidentBatch
    feats = step.inputs[0]
    if store.device != feats.device:
        raise RuntimeError('%s: the store lives on %s, the captured buffers on %s' % (who, store.device, feats.device))
    row = 1
    for s in feats.shape[2:]:
        row *= int(s)
    check_step_inputs(who, (('the store\'s viewpoint features [Ncam, row]', (feats.shape[0], row), feats.dtype, None),),
                      (('', (store.num_cams, store.row), store.feat_dtype, None),))
    batch = getattr(step, '_resident', None)
    if batch is None:
        dev = feats.device
        batch = step._resident = ResidentBatch(*step.inputs, gts, occ, torch.zeros(4, dtype=torch.int32, device=dev),
                                               torch.zeros(feats.shape[1], dtype=torch.int32, device=dev))
    n = index.numel() if torch.is_tensor(index) else len(index)
    if n != feats.shape[1]:
        raise ValueError('%s: %d indices for a captured batch of %d' % (who, n, feats.shape[1]))
    return store.fetch(index, out=batch).status


class GraphedTrainStep:
    """One training step of the WHOLE head -- encoder, detection decoder, cls / reg branches, coarse-to-fine occupancy,
    occupancy targets from the sparse pairs, the set loss of every decoder layer, the occupancy focal loss, backward, gradient
    clipping + AdamW -- for one fixed batch shape and one rank, captured as a SINGLE hipGraph and replayed with fresh ground
    truth: nothing between the inputs and the updated parameters runs on the host (``GraphedHead`` replays two graphs around
    a host-side Hungarian solve, eager loss terms and an eager optimizer).  Same kernels, same arithmetic as the eager step.

    ``model``: a ``MultiTaskStep`` (or a module with its signature and a ``head``); its head must use
    ``train_cfg.assigner.solver = 'fused'`` -- costs, ``ver_lsa_solve``, normalisers and the set loss on the device -- and be
    the default multi-task head (no ``add_layout``, ``only_occ``, ``only_det``, ``getbev``); ``optimizer``: an
    ``optim.ClipAdamW`` over the trainable parameters.  The sample inputs fix every shape:

    * ``feats [Ncam, B, Nk, C]``, ``world2pixel [B, Ncam, 4, 4]``, ``origin [B, 3]``;
    * ``gts``: a ``PaddedGts`` as ``head.pad_gts(..., capacity=)`` makes it; its width is the box ``capacity`` of every later
      call, which may bring a narrower one (copied into the leading columns; the counts bound what is read);
    * ``occ``: a ``hipops.PackedOccGts`` on the GPU without invalid voxels; ``pair_capacity`` (default: its pair count) is the
      most pairs a later call may bring.  ``ver_occ_targets`` runs inside the graph over the whole pair buffer with the
      offsets delimiting the live pairs: every sample visits ``[offsets[b], offsets[b + 1])`` and nothing else, so the
      stale pairs past ``offsets[B]`` of a longer earlier step are applied to no sample.

    Construction follows ``GraphedLiftStep``: ``warmup`` REAL eager steps on a side stream (they train the model; the
    first-call host checks -- label range, ``OccupancyTargets.check``, the assignment flag -- the library handles and the row
    plan happen there and never under capture), the live-loss check, ``optimizer.prepare_capture()``, one capture on one
    stream.  Everything said there about eager steps of the same optimizer between replays and about replaced optimizer
    buffers holds here.

    ``losses = step(feats, w2p, origin, gts, occ)`` copies the inputs into the static buffers (unless they ARE those buffers:
    ``step.inputs``, ``step.gts``, ``step.occ``) and returns the loss dict: STATIC tensors, overwritten by the next call
    (``float()`` or clone what has to survive it); ``step.total`` is their sum, ``step.grad_norm`` the clip norm.  Refusals are
    decided from sizes the host knows, never from a device read; what only the device knows -- an assignment problem, a pair
    with a class or voxel out of range, a label outside [0, C] -- is not read in the call: ``flags()`` reads it on demand.

    ``exchange``: a ``ddp.GradExchange`` over the optimizer's trainable parameters -- the step under data parallelism, as in
    ``GraphedLiftStep``: rank 0's parameters broadcast first, eager exchanged warm-up steps, graph A (forward, losses,
    backward, ``exchange.pack()``) and graph B (``optimizer.step(exchange)``) with the one eager all-reduce between them.  The
    head's two loss normalisers are all-reduced too, which cannot happen inside graph A; so every call forms them BEFORE
    the replay, on the device and without a host read: positives per layer = ``clamp(gts.counts, max=Nq).sum()``, through
    ``head._device_normalisers`` (its all-reduce included) into a static ``[2, L]`` buffer that the captured
    ``_set_loss_fused`` reads (``head.preset_normalisers``, set for the capture alone) instead of counting matches.  The
    two agree whenever every assignment problem was solved -- a solved problem matches exactly ``min(Nq, count)`` queries
    -- which is exactly the case in which ``AssignmentFlag`` stays clear; a flagged problem leaves its queries unmatched
    while its count still enters the preset normaliser, and ``flags()['assignment']`` reports that case.  A model wrapped
    in DistributedDataParallel is refused with or without an exchange."""

    def __init__(self, model, optimizer, feats, world2pixel, origin, gts, occ, pair_capacity=None, warmup=3,
                 check_live_losses=True, exchange=None):
        from .dense_heads.voxelformer_occupancy_head import PaddedGts
        from .hipops import PackedOccGts
        who = 'GraphedTrainStep'
        if isinstance(model, torch.nn.parallel.DistributedDataParallel) or \
                isinstance(getattr(model, 'head', None), torch.nn.parallel.DistributedDataParallel):
            raise RuntimeError('%s: a DistributedDataParallel model: its bucket hooks and reducer cannot live inside a capture '
                               '(one rank only); for data parallelism pass the UNWRAPPED model and `exchange=` '
                               'ddp.GradExchange(parameters)' % who)
        if not hasattr(optimizer, 'prepare_capture'):
            raise TypeError('%s needs an optimizer whose step() can be captured (optim.ClipAdamW)' % who)
        head = model.head
        self._check_head(head)
        if not isinstance(gts, PaddedGts) or not isinstance(occ, PackedOccGts):
            raise TypeError('%s: gts is a PaddedGts (head.pad_gts), occ a hipops.PackedOccGts' % who)
        if occ.has_invalid:
            raise ValueError('%s: a PackedOccGts with invalid voxels (evaluation labels) is not a training target' % who)
        bs = feats.shape[1]
        pair_capacity = occ.n_total if pair_capacity is None else int(pair_capacity)
        if occ.n_total > pair_capacity:
            raise ValueError('%s: occ holds %d pairs, the pair capacity is %d' % (who, occ.n_total, pair_capacity))
        if occ.bs != bs or gts.boxes.shape[0] != bs:
            raise ValueError('%s: %d samples of features, %d of boxes, %d of pairs' % (who, bs, gts.boxes.shape[0], occ.bs))
        self._need_gpu(feats, world2pixel, origin, gts, occ)
        self.model, self.optimizer, self.exchange = model, optimizer, exchange
        if exchange is not None:
            _check_exchange(who, optimizer, exchange)
            exchange.broadcast_parameters()
        self.capacity, self.pair_capacity = int(gts.boxes.shape[1]), pair_capacity
        self.inputs = tuple(t.detach().clone() for t in (feats, world2pixel, origin))
        self.gts = PaddedGts(*(t.detach().clone() for t in gts))
        # the layout of a PackedOccGts at the pair capacity; pairs past the live ones start out as (0, 0) and belong to no sample
        buffer = torch.zeros(2 * (bs + 1) + 2 * pair_capacity, dtype=torch.int32, device=feats.device)
        self.occ = PackedOccGts(buffer, bs, pair_capacity, 0, False)
        self._load_gts(gts, occ)
        self.training = model.training
        static = self.inputs + (self.gts, self.occ)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            norm = None
            shapes = []                                     # [L, B, Nq, C] of the class scores, for the preset normalisers
            hook = exchange is not None and head.register_forward_hook(
                lambda mod, args, kwargs, outs: shapes.append(tuple(outs['all_cls_scores'].shape)), with_kwargs=True)
            for _ in range(max(1, warmup)):                 # (at least one: the optimizer state must exist before the capture)
                optimizer.zero_grad(set_to_none=True)
                total = sum(model(*static).values())
                total.backward()
                norm = optimizer.step() if exchange is None else _exchanged_update(optimizer, exchange)
            if hook:
                hook.remove()
            self._clean_warmup = norm is not None and bool(torch.isfinite(norm))
            self._unchecked = 3
            total = None
            optimizer.zero_grad(set_to_none=True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if check_live_losses:
            gc.collect()
            n = len(_live_losses())
            if n:
                raise RuntimeError('%s: %d scalar tensor(s) with an autograd graph are still alive (losses of earlier eager '
                                   'steps?); drop them before building the graph (see GraphedHead)' % (who, n))
        optimizer.prepare_capture()
        self.graph = torch.cuda.CUDAGraph()
        if exchange is None:
            with torch.cuda.graph(self.graph):
                losses = model(*static)
                total = sum(losses.values())
                total.backward()
                self.grad_norm = optimizer.step()
                self.losses = {k: v.detach() for k, v in losses.items()}
                self.total = total.detach()
        else:
            self._layers, self._queries = shapes[0][0], shapes[0][2]
            self._normalisers = torch.ones(2, self._layers, dtype=torch.float32, device=feats.device)
            self._load_normalisers()
            exchange.prepare_capture()
            stream = torch.cuda.Stream()
            head.preset_normalisers = self._normalisers
            try:
                with torch.cuda.graph(self.graph, stream=stream):
                    losses = model(*static)
                    total = sum(losses.values())
                    total.backward()
                    exchange.pack()
                    self.losses = {k: v.detach() for k, v in losses.items()}
                    self.total = total.detach()
            finally:
                head.preset_normalisers = None
            self.update_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.update_graph, pool=self.graph.pool(), stream=stream):
                self.grad_norm = optimizer.step(exchange=exchange)
        self._targets = model.targets                      # the capture's OccupancyTargets: static tensors the replays rewrite
        losses = total = None

    @staticmethod
    def _check_head(head):
        who = 'GraphedTrainStep'
        solver = getattr(getattr(head, 'assigner', None), 'solver', 'host')
        if solver != 'fused':
            raise ValueError("%s: train_cfg.assigner.solver is %r; the captured step needs 'fused' (costs, assignment and set "
                             'loss on the device, nothing solved on the host)' % (who, solver))
        if head.add_layout:
            raise NotImplementedError('%s: add_layout=True: the room-layout terms are not part of the captured step' % who)
        if head.only_occ or head.only_det:
            raise NotImplementedError('%s covers the default multi-task branch of the head (only_occ / only_det are set)' % who)
        if getattr(head, 'getbev', None) is not None:
            raise NotImplementedError('%s: a head built with getbev=<store> writes volumes to the host inside forward (device '
                                      '-> host copies and file I/O), which cannot be captured' % who)

    @staticmethod
    def _need_gpu(feats, world2pixel, origin, gts, occ):
        named = (('feats', feats), ('world2pixel', world2pixel), ('origin', origin), ('gts.boxes', gts.boxes),
                 ('gts.labels', gts.labels), ('gts.counts', gts.counts), ('occ.buffer', occ.buffer))
        cpu = [k for k, t in named if not t.is_cuda]
        if cpu:
            raise RuntimeError('GraphedTrainStep needs GPU tensors (HIP graphs); on the CPU: %s' % ', '.join(cpu))

    @staticmethod
    def _signature(feats, world2pixel, origin, gts, n_pairs, n_offsets):
        boxes = ('boxes per sample', 'box capacity')
        return (('feats', feats.shape, feats.dtype, None), ('world2pixel', world2pixel.shape, world2pixel.dtype, None),
                ('origin', origin.shape, origin.dtype, None), ('gts.boxes', gts.boxes.shape, gts.boxes.dtype, (1,) + boxes),
                ('gts.labels', gts.labels.shape, gts.labels.dtype, (1,) + boxes),
                ('gts.counts', gts.counts.shape, gts.counts.dtype, None),
                ('occ.pairs', (n_pairs, 2), torch.int32, (0, 'pairs', 'pair capacity')),
                ('occ.offsets', (n_offsets,), torch.int32, None))

    def _load_gts(self, gts, occ):
        """Ground truth of a call into the static buffers: the leading columns of the box tables, the counts, the live pairs
        and their offsets (what lies behind them is never read: the counts and the offsets bound every kernel's loops)."""
        if gts is not self.gts:
            n = gts.boxes.shape[1]
            self.gts.boxes[:, :n].copy_(gts.boxes, non_blocking=True)
            self.gts.labels[:, :n].copy_(gts.labels, non_blocking=True)
            self.gts.counts.copy_(gts.counts, non_blocking=True)
        if occ is not self.occ:
            self.occ.offsets.copy_(occ.offsets, non_blocking=True)
            self.occ.pairs[:occ.n_total].copy_(occ.pairs, non_blocking=True)

    @torch.no_grad()
    def _load_normalisers(self):
        """The two loss normalisers of the step whose counts sit in ``self.gts``, into the static buffer graph A reads: eager
        device work (and, with a process group, the head's one all-reduce), no host read."""
        head = self.model.head
        bs = self.gts.counts.shape[0]
        positives = self.gts.counts.clamp(max=self._queries).sum().to(torch.int64).expand(self._layers)
        self._normalisers.copy_(head._device_normalisers(positives, bs * self._queries))

    def __call__(self, feats, world2pixel, origin, gts, occ):
        who = 'GraphedTrainStep'
        if self.model.training != self.training:
            raise RuntimeError('%s: model.training differs from capture time; build a new one for the new mode' % who)
        if not isinstance(gts, type(self.gts)) or not isinstance(occ, type(self.occ)):
            raise TypeError('%s: gts is a PaddedGts (head.pad_gts), occ a hipops.PackedOccGts' % who)
        self._need_gpu(feats, world2pixel, origin, gts, occ)
        if occ is not self.occ and occ.has_invalid:
            raise ValueError('%s: a PackedOccGts with invalid voxels (evaluation labels) is not a training target' % who)
        check_step_inputs(who, self._signature(*self.inputs, self.gts, self.pair_capacity, self.occ.bs + 1),
                          self._signature(feats, world2pixel, origin, gts, occ.n_total, occ.bs + 1))
        for dst, src in zip(self.inputs, (feats, world2pixel, origin)):
            if src is not dst:
                dst.copy_(src, non_blocking=True)
        self._load_gts(gts, occ)
        self.optimizer.refresh()
        if self.exchange is None:
            self.graph.replay()
        else:
            self._load_normalisers()
            self.graph.replay()
            self.exchange.all_reduce()
            self.update_graph.replay()
            self.exchange.replayed()
        self.optimizer.replayed()
        if self._unchecked:
            # as GraphedLiftStep: the first replays are checked (one synchronisation each) for the runtime's memset-node problem
            self._unchecked -= 1
            if not bool(torch.isfinite(self.grad_norm)) and self._clean_warmup:
                raise RuntimeError(
                    '%s: the gradient norm of a replayed step is not finite although the eager warm-up steps were clean.  On '
                    'ROCm 7.2 hipGraph replay needs DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 in the environment BEFORE the first GPU '
                    'call of the process (memset nodes are not ordered against the kernels behind them otherwise); importing '
                    'vln-ver_amd sets it, but only takes effect if HIP was not initialised earlier.' % who)
        return self.losses

    def fetch(self, store, index):
        """The ground truth and inputs of the next step out of a ``resident.ResidentStore``, written by the device into
        ``self.inputs``, ``self.gts`` and the ``offsets`` / ``pairs`` views of ``self.occ`` (at ``self.pair_capacity``):
        ``step.fetch(store, idx); step(*step.inputs, step.gts, step.occ)`` is a step whose only host -> device traffic is
        the ``4 * bs`` bytes of a host ``idx`` (none for a device tensor).  A store with another camera count, row size or
        feature dtype is refused before any launch.  -> the status tensor of the fetch (``store.check(status)``)."""
        return _fetch_into('GraphedTrainStep.fetch', self, store, index, self.gts, self.occ)

    def flags(self):
        """What the replayed steps could only report on the device, read now (ONE synchronisation): ``assignment`` -- the
        sticky ``AssignmentFlag`` (a cost matrix ``lsa_solve`` could not assign); ``label_range`` -- the sticky
        ``LabelRangeFlag`` (a label outside [0, C] reached the focal loss); ``rejected_pairs`` / ``lost_listings`` -- ``bad``
        of the LAST step's occupancy targets (pairs with a voxel or class out of range; listings of a voxel that lost to a
        larger class).  All zero for clean steps; nothing is raised or reset here."""
        from .hipops import AssignmentFlag, LabelRangeFlag
        dev = self.total.device
        values = torch.cat([AssignmentFlag.of(dev).dev, LabelRangeFlag.of(dev).dev, self._targets.bad]).tolist()
        return dict(zip(('assignment', 'label_range', 'rejected_pairs', 'lost_listings'), values))


class GraphedInference:
    """One inference step of the whole head -- ``head.infer``: encoder, detection decoder, fused box decode, occupancy class
    bytes and per-sample (voxel, class) pairs -- for one fixed batch shape, captured as a SINGLE hipGraph and replayed: what
    an agent pays per navigation step at the reference's batch point.  Same kernels, same arithmetic as the eager call; every
    output has a fixed shape (``InferenceOutputs``: padded box tables with ``valid``, pairs with offsets and counts), so
    nothing between the inputs and the outputs runs on, or waits for, the host.

    The sample inputs fix every shape: ``feats [Ncam, B, Nk, C]``, ``world2pixel [B, Ncam, 4, 4]``, ``origin [B, 3]`` on the
    GPU.  ``autocast_dtype``: torch.bfloat16 (default; the occupancy classes come from the classifying MLP launch, no logits)
    or None = fp32.  ``pair_capacity``: the most occupied voxels of the batch the pair table holds (None: ``B * voxel_num``,
    which cannot overflow; a smaller table makes the one host copy of ``results()`` smaller, and an overflow is reported in
    ``occ_count[B + 1]`` and raised by ``results()``).  Construction follows ``GraphedTrainStep``: ``warmup`` eager calls on a
    side stream (library handles, the row plan and its table, the packed MLP image are built there and never under capture),
    then one capture of ``head.infer`` on one stream.

    ``outs = step(feats, w2p, origin)`` checks shapes and dtypes on the host, copies the inputs into the static buffers
    (unless they ARE those buffers: ``step.inputs``), replays and returns the STATIC ``InferenceOutputs``, overwritten by the
    next call.  ``step.results(img_metas=None)`` makes the single device -> host copy and returns what
    ``VoxelFormer.simple_test`` returns (``inference_results``).  The head must be in eval mode, at capture time and at every
    call; a head wrapped in DistributedDataParallel, or a CPU tensor, is refused."""

    def __init__(self, head, feats, world2pixel, origin, autocast_dtype=torch.bfloat16, occ_threshold=0.25, pair_capacity=None,
                 warmup=2):
        who = 'GraphedInference'
        if isinstance(head, torch.nn.parallel.DistributedDataParallel):
            raise RuntimeError('%s: a DistributedDataParallel head: inference needs no gradient exchange; pass the unwrapped '
                               'module (head.module)' % who)
        if head.training:
            raise RuntimeError('%s: the head is in training mode; inference is captured in eval mode (head.eval())' % who)
        head._check_infer()
        self._need_gpu(feats, world2pixel, origin)
        self.head, self.autocast_dtype, self.occ_threshold = head, autocast_dtype, float(occ_threshold)
        self.pair_capacity = None if pair_capacity is None else int(pair_capacity)
        self.inputs = tuple(t.detach().clone() for t in (feats, world2pixel, origin))
        call = lambda out=None: head.infer(*self.inputs, occ_threshold=self.occ_threshold, pair_capacity=self.pair_capacity,
                                           autocast_dtype=self.autocast_dtype, out=out)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):                 # (at least one: handles, plan and tables must exist before the capture)
                outs = call()
            self._clean_warmup = bool(torch.isfinite(outs.volume).all())
            self._unchecked = 3
            outs = None
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.outputs = call()

    @staticmethod
    def _need_gpu(feats, world2pixel, origin):
        cpu = [k for k, t in (('feats', feats), ('world2pixel', world2pixel), ('origin', origin)) if not t.is_cuda]
        if cpu:
            raise RuntimeError('GraphedInference needs GPU tensors (HIP graphs); on the CPU: %s' % ', '.join(cpu))

    @staticmethod
    def _signature(feats, world2pixel, origin):
        return (('feats', feats.shape, feats.dtype, None), ('world2pixel', world2pixel.shape, world2pixel.dtype, None),
                ('origin', origin.shape, origin.dtype, None))

    def __call__(self, feats, world2pixel, origin):
        who = 'GraphedInference'
        if self.head.training:
            raise RuntimeError('%s: the head is in training mode; it was captured in eval mode (head.eval())' % who)
        self._need_gpu(feats, world2pixel, origin)
        check_step_inputs(who, self._signature(*self.inputs), self._signature(feats, world2pixel, origin))
        for dst, src in zip(self.inputs, (feats, world2pixel, origin)):
            if src is not dst:
                dst.copy_(src, non_blocking=True)
        self.graph.replay()
        if self._unchecked:
            # as the training graphs: the first replays are checked (one synchronisation each) for the runtime's memset-node problem
            self._unchecked -= 1
            if not bool(torch.isfinite(self.outputs.volume).all()) and self._clean_warmup:
                raise RuntimeError(
                    '%s: the volume of a replayed step is not finite although the eager warm-up calls were clean.  The '
                    "package's import-time environment handling (vln-ver_amd/__init__.py) only takes effect if vln-ver_amd was "
                    'imported BEFORE the first GPU call of the process; see GraphedTrainStep for the same check.' % who)
        return self.outputs

    def fetch(self, store, index):
        """The inputs of the next call out of a ``resident.ResidentStore`` (features and cameras; no ground truth), written
        by the device into ``self.inputs``: ``step.fetch(store, idx); step(*step.inputs)``.  A store with another camera
        count, row size or feature dtype is refused before any launch.  -> the status tensor (``store.check(status)``)."""
        return _fetch_into('GraphedInference.fetch', self, store, index, None, None)

    def results(self, img_metas=None):
        """The last replay's outputs as ``VoxelFormer.simple_test`` returns them: ONE device -> host copy of all tables."""
        from .dense_heads.voxelformer_occupancy_head import inference_results
        return inference_results(self.head, self.outputs, img_metas)
