"""The optimizer step the reference configures for vocc.py -- gradient clipping by the global L2 norm in front of AdamW
(projects/configs/verformer/vocc.py:260-274: ``optimizer=dict(type='AdamW', ..., paramwise_cfg=...)``,
``optimizer_config=dict(grad_clip=dict(max_norm=..., norm_type=2))``, run by mmcv's OptimizerHook as ``clip_grad_norm_`` +
``optimizer.step()``) -- as ONE C-ABI call over all parameters: ``ver_clip_adamw_step_tensors`` (csrc/ver_optim.hip; two
launches, 32 bytes per parameter).  ``step(exchange)`` is the same update with the gradients read from the flat buffer of a
``ddp.GradExchange`` (``ver_clip_adamw_step_flat``; fp32 or bf16 on the wire) -- data-parallel steps without a
DistributedDataParallel wrapper, bit for bit the update ``step()`` applies to fp32 gradient tensors of the same values.

``ClipAdamW`` keeps torch.optim.AdamW's state layout (``exp_avg`` / ``exp_avg_sq`` / ``step`` per parameter) and arithmetic
(decoupled weight decay, bias corrections from the PARAMETER's own step count, amsgrad off).  Any number of parameter groups
(mmcv's ``paramwise_cfg`` builds one per parameter: vocc.py gives ``img_backbone`` lr_mult 0.1) with their own lr / betas /
eps / weight decay; the clip norm is global over every parameter that has a gradient, as in ``clip_grad_norm_``, and a
non-finite norm poisons every gradient the way ``clip_grad_norm_`` does.  Parameters and gradients are dense fp32 GPU tensors.
There is no CPU path here: CPU tensors raise, as every product path of this package does without its HIP library.

What a launch reads lives on the device -- a pointer table (parameter, gradient, both moments per tensor), the per-tensor
hyper-parameters and the per-tensor update counts, which the kernel advances itself -- so a hipGraph that contains
``step()`` replays correctly (``vln-ver_amd/graphs.py``).  The host keeps what those buffers SHOULD hold and compares on
every call: a changed gradient / moment / parameter pointer (``zero_grad(set_to_none=True)``, ``load_state_dict``,
``model.to()``), a changed lr (schedulers) or a step count that was set from outside is uploaded again before the launch --
nothing is cached by object identity.

Two rules tie that host record to captured graphs (tests/test_optim_graph_gpu.py):

* The record of the pointer table holds only while the last writer of the table was an EAGER step.  A captured ``step()``
  turns its table copy into a graph node, so every replay rewrites the device table to the capture's own gradient buffers
  behind the host's back: the capture and ``replayed()`` forget the record, and the next eager step uploads its pointers
  again even when its gradients sit where they sat before the replay.  Any number of graphs may share one optimizer: each
  replay restores its own table.
* A graph reads the table / hyper-parameter / count buffers (and the chunk tables) by raw address.  They are kept referenced
  for as long as the optimizer lives, and whatever replaces or drops them once a ``step()`` has been captured --
  ``load_state_dict``, ``__setstate__``, an eager step over another set of tensors (a parameter whose first gradient
  arrives after the capture) -- makes every earlier capture INVALID: ``refresh()`` and ``replayed()``, which a replay passes
  through (``graphs.GraphedLiftStep.__call__``), raise until ``prepare_capture()`` and a new capture.
"""

import numpy as np
import torch


class ClipAdamW(torch.optim.Optimizer):
    CHUNK = 32768            # elements per workgroup

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=0.0):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError('ClipAdamW: hyper-parameters out of range')
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, max_norm=max_norm))
        self._tables = {}
        self._dev = None             # what the device buffers hold: dict(ptrs, hyper, steps, n) + the buffers themselves
        self._keep = []              # what captured graphs read by raw address: pinned staging buffers, device tables
        self._captured = None        # per-parameter states of the captured step(), while that capture may be replayed
        self._stale = None           # why the earlier captures may not be replayed any more

    # ------------------------------------------------------------------ host-side bookkeeping
    def _chunk_tables(self, sizes, device):
        key = (tuple(sizes), str(device))
        hit = self._tables.get(key)
        if hit is None:
            tensor, index = [], []
            for t, n in enumerate(sizes):
                c = -(-n // self.CHUNK)
                tensor += [t] * c
                index += list(range(c))
            hit = self._tables[key] = (
                torch.tensor(list(sizes), dtype=torch.int64, device=device), torch.tensor(tensor, dtype=torch.int32, device=device),
                torch.tensor(index, dtype=torch.int32, device=device), torch.empty(len(tensor), dtype=torch.float32, device=device))
            if len(self._tables) > 8:
                self._tables.pop(next(iter(self._tables)))
        return hit

    def _collect(self, exchange=None):
        """-> (parameters with a gradient, their gradients, hyper rows [n][6], max_norm): state created on first sight, ``step``
        normalised to an int (a torch AdamW checkpoint holds one tensor per parameter).  With an exchange: its parameter
        list in ITS order (the order of the flat buffer), every one of which must be ours; ``p.grad`` is not looked at and no
        gradients are returned."""
        ps, gs, hyper = [], [], []
        max_norm = None
        rows = {}
        for group in self.param_groups:
            mn = float(group.get('max_norm') or 0.0)
            if max_norm is None:
                max_norm = mn
            elif mn != max_norm:
                raise ValueError('ClipAdamW: one max_norm for all parameter groups (the clip norm is global)')
            b1, b2 = group['betas']
            if not (group['lr'] >= 0 and 0 <= b1 < 1 and 0 <= b2 < 1 and group['eps'] >= 0 and group['weight_decay'] >= 0):
                raise ValueError('ClipAdamW: hyper-parameters out of range in a parameter group')
            row = (float(group['lr']), float(b1), float(b2), float(group['eps']), float(group['weight_decay']), 0.0)
            for p in group['params']:
                if exchange is not None:
                    rows[id(p)] = row
                    continue
                g = p.grad
                if g is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32 and not g.is_sparse and p.is_contiguous()):
                    raise TypeError('ClipAdamW: dense fp32 GPU parameters and gradients only (got %s %s on %s)' % (p.dtype, g.dtype, p.device))
                st = self.state[p]
                if not st:
                    st['step'] = 0
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif not isinstance(st['step'], int):
                    st['step'] = int(st['step'])
                ps.append(p)
                gs.append(g if g.is_contiguous() else g.contiguous())
                hyper.append(row)
        if exchange is not None:
            for k, p in zip(exchange.names, exchange.params):
                if id(p) not in rows:
                    raise ValueError('ClipAdamW.step(exchange): %s of the exchange is not a parameter of this optimizer' % k)
                st = self.state[p]
                if not st:
                    st['step'] = 0
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif not isinstance(st['step'], int):
                    st['step'] = int(st['step'])
                ps.append(p)
                hyper.append(rows[id(p)])
        return ps, gs, hyper, max_norm or 0.0

    def _upload(self, ptrs, hyper, steps, dev, capturing):
        """Bring the device buffers to (ptrs, hyper, steps).  In place whenever the tensor count is unchanged: a captured
        graph keeps reading the same addresses.  While a graph is being captured only the pointer table may move (the copy
        becomes a graph node that re-copies the same values on every replay); hyper-parameters and update counts must
        already be resident -- they change between replays, from outside the graph."""
        d = self._dev
        n = len(steps)
        fresh = d is None or d['n'] != n or d['device'] != dev
        if fresh:
            if capturing:
                raise RuntimeError('ClipAdamW: the first step() for this set of parameters inside a graph capture; run '
                                   '`prepare_capture()` (or one eager step) before capturing')
            if d is not None:
                self._invalidate('an eager step() over %d tensors replaced the device buffers of %d' % (n, d['n']))
            d = self._dev = dict(n=n, device=dev, ptrs=None, hyper=None, steps=None,
                                 table=torch.empty(4 * n, dtype=torch.int64, device=dev),
                                 hyper_dev=torch.empty(n, 6, dtype=torch.float32, device=dev),
                                 steps_dev=torch.empty(n, dtype=torch.int32, device=dev))

        def push(dst, array):
            stage = getattr(self, '_stage', None)
            if capturing and stage is not None and stage.numel() == array.size and array.dtype == np.int64:
                src = stage                               # (pinned before the capture: no host allocation inside it)
                src.numpy()[:] = array
                self._stage = None
            else:
                src = torch.from_numpy(array).pin_memory()
            if capturing:
                self._keep.append(src)
            dst.copy_(src.view(dst.shape), non_blocking=True)
        if capturing or d['ptrs'] != ptrs:
            push(d['table'], np.asarray(ptrs, dtype=np.int64))
            # (a captured copy has not run, and every replay runs it without the host: no record of it)
            d['ptrs'] = None if capturing else ptrs
        if d['hyper'] != hyper or d['steps'] != steps:
            if capturing:
                raise RuntimeError('ClipAdamW: hyper-parameters / step counts changed inside a graph capture; call '
                                   '`prepare_capture()` right before capturing and `refresh()` between replays')
            if d['hyper'] != hyper:
                push(d['hyper_dev'], np.asarray(hyper, dtype=np.float32).reshape(n, 6))
                d['hyper'] = hyper
            if d['steps'] != steps:
                push(d['steps_dev'], np.asarray(steps, dtype=np.int32))
                d['steps'] = steps
        return d

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None, exchange=None):
        """One clipped AdamW update of every parameter that has a gradient.  Returns the gradient norm before clipping
        (a device scalar, like ``clip_grad_norm_``).

        ``exchange``: a ``ddp.GradExchange`` -- the update of ITS parameter list (all of them parameters of this optimizer)
        from the gradients in its flat buffer, as ``pack()`` and ``all_reduce()`` left them; ``p.grad`` is not consulted.
        Capture support is the same: ``prepare_capture``, ``replayed``, ``refresh`` and the invalidation rules above."""
        from . import hipops
        from .ddp import GradExchange
        if exchange is None and isinstance(closure, GradExchange):         # ``step(exchange)``
            closure, exchange = None, closure
        if closure is not None:
            raise NotImplementedError('ClipAdamW: no closure')
        if exchange is not None and not isinstance(exchange, GradExchange):
            raise TypeError('ClipAdamW.step(exchange): a ddp.GradExchange, got %s' % type(exchange).__name__)
        ps, gs, hyper, max_norm = self._collect(exchange)
        if not ps:
            return torch.zeros(())
        dev = ps[0].device
        capturing = torch.cuda.is_current_stream_capturing()
        n = len(ps)
        states = [self.state[p] for p in ps]
        if exchange is not None:
            if exchange.device != dev or exchange.chunk != self.CHUNK:
                raise ValueError('ClipAdamW.step(exchange): the exchange lives on %s with chunks of %d' % (exchange.device, exchange.chunk))
            gs = [None] * n                                # (the gradient row of the table is not read: zeros)
        ptrs = ([p.data_ptr() for p in ps] + [0 if g is None else g.data_ptr() for g in gs] + [st['exp_avg'].data_ptr() for st in states]
                + [st['exp_avg_sq'].data_ptr() for st in states])
        steps = [st['step'] for st in states]
        if not capturing and self._captured and [id(st) for st in states] != [id(st) for st in self._captured]:
            self._invalidate('an eager step() ran over other tensors than the captured one')
        d = self._upload(ptrs, hyper, steps, dev, capturing)
        norm = torch.zeros((), dtype=torch.float32, device=dev)
        tables = self._chunk_tables([p.numel() for p in ps], dev)
        sizes, chunk_tensor, chunk_index, partial = tables
        L = hipops.lib()
        if exchange is None:
            hipops._launch('ver_clip_adamw_step', lambda: L.ver_clip_adamw_step_tensors(
                hipops._p(d['table']), hipops._p(sizes), hipops._p(chunk_tensor), hipops._p(chunk_index), hipops._p(d['hyper_dev']),
                hipops._p(d['steps_dev']), n, chunk_tensor.numel(), self.CHUNK, hipops._p(partial), hipops._p(norm), max_norm,
                hipops._stream()))
        else:
            hipops._launch('ver_clip_adamw_step', lambda: L.ver_clip_adamw_step_flat(
                hipops._p(d['table']), hipops._p(sizes), hipops._p(exchange.offsets_dev), hipops._p(chunk_tensor),
                hipops._p(chunk_index), hipops._p(d['hyper_dev']), hipops._p(d['steps_dev']), hipops._p(exchange.flat),
                1 if exchange.wire_dtype == torch.bfloat16 else 0, n, chunk_tensor.numel(), self.CHUNK, hipops._p(partial),
                hipops._p(norm), max_norm, hipops._stream()))
        if capturing:
            # nothing has run: the replays advance the device counts, ``replayed()`` the host's
            self._captured, self._stale = states, None
            self._keep.append((d['table'], d['hyper_dev'], d['steps_dev'], tables, exchange))
        else:
            for st in states:
                st['step'] += 1
            d['steps'] = [s + 1 for s in steps]       # (the kernel advanced the device counts)
        # (contiguous gradient copies may go out of scope: the caching allocator reuses their blocks only behind this
        #  launch on the same stream)
        return norm

    # ------------------------------------------------------------------ hipGraph support
    @torch.no_grad()
    def prepare_capture(self):
        """Call right before capturing a graph that contains ``step()``, after at least one eager step over the same set of
        parameters (their state, hyper-parameters and update counts are then resident on the device): pins the staging
        buffer the captured ``step()`` fills with the pointer table of the capture's own gradient buffers."""
        n = sum(1 for group in self.param_groups for p in group['params'] if self.state.get(p))
        if not n or self._dev is None or self._dev['n'] != n:
            raise RuntimeError('ClipAdamW.prepare_capture(): run one eager step over the parameters of the step first')
        self._stage = torch.empty(4 * n, dtype=torch.int64).pin_memory()

    def _invalidate(self, why):
        """The buffers the captured graphs read are being replaced or dropped (they stay referenced in ``_keep``, so a replay
        that slips past the guard still reads memory of its own): no replay until a new capture."""
        if self.__dict__.get('_captured'):
            self._captured, self._stale = None, why

    def _live_capture(self, who):
        states = self.__dict__.get('_captured')
        if not states:
            raise RuntimeError('ClipAdamW.%s(): no captured step() may be replayed (%s); a new capture is needed -- one eager '
                               'step, `prepare_capture()`, then capture `step()` again'
                               % (who, self.__dict__.get('_stale') or 'none has been captured'))
        return states

    def replayed(self, times=1):
        """A graph holding ``step()`` was replayed ``times`` times: advance the host's step counts to what the device holds,
        and forget the record of the pointer table -- the replay has rewritten it to the capture's gradient buffers."""
        states = self._live_capture('replayed')
        for st in states:
            st['step'] += times
        d = self._dev
        d['ptrs'] = None
        if d['steps'] is not None:
            d['steps'] = [s + times for s in d['steps']]

    @torch.no_grad()
    def refresh(self):
        """Between replays: upload hyper-parameters that changed (a scheduler moved lr) into the buffers the graph reads."""
        states = self._live_capture('refresh')
        d = self._dev
        hyper = []
        ids = {id(st) for st in states}
        for group in self.param_groups:
            b1, b2 = group['betas']
            row = (float(group['lr']), float(b1), float(b2), float(group['eps']), float(group['weight_decay']), 0.0)
            hyper += [row for p in group['params'] if id(self.state.get(p)) in ids]
        if len(hyper) == d['n'] and hyper != d['hyper']:
            src = torch.from_numpy(np.asarray(hyper, dtype=np.float32).reshape(d['n'], 6)).pin_memory()
            d['hyper_dev'].copy_(src, non_blocking=True)
            d['hyper'] = hyper

    def load_state_dict(self, state_dict):
        """A torch.optim.AdamW checkpoint loads too (per-parameter step tensors become ints on the next step); its
        parameter groups carry no ``max_norm`` -- the groups REPLACE ours in torch's loader -- so keys a group lost get this
        optimizer's constructor values back."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            for k, v in self.defaults.items():
                group.setdefault(k, v)
        self._invalidate('load_state_dict() replaced the state the capture was made with')
        self._dev = None             # (pointers and counts are compared on every step anyway; drop the buffers with the old state)

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault('_tables', {})
        self.__dict__.setdefault('_keep', [])
        self.__dict__.setdefault('_captured', None)
        self.__dict__.setdefault('_stale', None)
        self._invalidate('__setstate__() replaced the state the capture was made with')
        self.__dict__['_dev'] = None
