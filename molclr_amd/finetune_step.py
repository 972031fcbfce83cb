"""The fine-tuning train and evaluation steps captured as HIP graphs.

The reference's fine-tuning loop (finetune.py:89-102 per training batch,
finetune.py:259-317 per evaluation pass) enqueues ~105 launches for a batch of
32 molecules whose kernels are nearly empty grids: the step is bound by the
host.  As molclr_amd.graph_step does for pre-training, this module captures
the step once per capacity bucket and replays it; the host cost per batch is
one staging launch (``molclr_stage_task``: the batch and its targets into
fixed buffers) and one graph launch.

* :class:`CapturedFinetuneStep` -- ``step(data) -> loss``: the graph build,
  ``zero_grad`` of every optimizer, ``model.loss_staged``, the backward, every
  FusedAdam update and one closing launch (``molclr_task_step_tail``).
* :class:`CapturedEval` -- ``run(loader) -> (mean_loss, predictions,
  labels)`` under ``eval()`` / ``no_grad``: every batch is staged and replayed,
  the graph's closing launch (``molclr_eval_tail``) gathers predictions,
  targets and the loss sum on the device, and the pass ends with ONE
  synchronisation and ONE device-to-host copy.  Its graphs are its own:
  eval-mode BatchNorm records other kernels than the training step's.

Both reuse graph_step's machinery: StagedPairGraph with one segment, the
device-sized graph build and BatchNorm, padding rows that carry no gradient, a
dry run before and a private memory pool for every capture, and dropout keys
drawn from a device counter so replays get fresh masks.  State that crosses
replays lives outside the pools: parameters, moments, the loss / status /
gather buffers, the staged targets and the task head's ticket word
(ops.CAPTURE_HEAD_SYNC: one per step object, made before the capture -- the
capture stream is not the stream the dry run ran on).

The motif model (ginet_finetune_mp) is taken too.  Its item count varies per
batch, so its graphs run the device-sized pool (ops.motif_pool_staged) over an
item capacity: a second staging launch (``molclr_stage_motif``) puts the
batch's ``(mol_idx, clique_idx)`` into fixed buffers with ``mol_ptr`` and the
stable sort by motif id the pool's backward reads, and the bucket key gets a
fourth term, the item capacity (``item_quantum``).  ``step`` and ``run`` take
the items next to the batch.  The trainer opts in with ``hip_graph_motif:
True`` next to ``hip_graph: True``; ``hip_graph: True`` alone keeps warning
and training the motif model eagerly, as before.

Single process only: fine-tuning has no data-parallel path.
"""
from __future__ import annotations

import contextlib
import ctypes
from collections import OrderedDict

import torch

from . import _lib, ops
from .data import _num_graphs_of, raise_for_status
from .graph_step import StagedPairGraph, _Captured, _round_up


def unsupported_reason(model, motif_items: bool = False) -> str | None:
    """Why the captured steps cannot take ``model`` (None: they can).  The
    motif model is taken only by a caller that hands over every batch's items
    (``motif_items=True``: ``step(data, mol_idx, clique_idx)``, ``run(loader,
    motif=...)``); asked without, the answer names the items, as it did before
    the pool had a device-sized form."""
    from .ginet_finetune import FinetuneReadout
    from .ginet_finetune_mp import GINet as MotifGINet
    if not isinstance(model, FinetuneReadout):
        return "the model has no loss_staged"
    if not model.use_executor or model.num_layer > 16:
        return "the encoder executor is off"
    if model._dim_pad():
        return f"emb_dim {model.emb_dim} needs padding to the kernels' width"
    if isinstance(model, MotifGINet) and not motif_items:
        return ("the motif model's item count varies per batch: its captured steps take the "
                "batch's items (motif_items)")
    lins, _ = model._head_layers()
    if isinstance(model, MotifGINet):
        # three chains: feat_lin, motif_lin, and pred_head over cat(h, hp)
        if not ops.MOTIF_POOL:
            return ("MOLCLR_MOTIF_POOL=0 composes the motif pool from torch ops, which has no "
                    "device-sized form")
        chains = [[model.emb_dim, model.feat_dim], [model.feat_dim, model.feat_dim],
                  [2 * model.feat_dim] + [m.out_features for m in lins]]
    else:
        chains = [[model.emb_dim, model.feat_dim] + [m.out_features for m in lins]]
    for dims in chains:
        if not ops.task_head_fused(dims):
            return (f"a task head of widths {dims} is composed from separate launches "
                    f"(fused up to {_lib.TASK_HEAD_MAX_DIM})")
    return None


def _is_motif(model) -> bool:
    from .ginet_finetune_mp import GINet as MotifGINet
    return isinstance(model, MotifGINet)


class _IdsBatch:
    """A batch named by its molecule ids in a task_store.DeviceTaskStore:
    what the captured steps take in place of a collated batch.  ``need``:
    (nodes, edges, molecules[, motif items]) from the store's host counts."""

    def __init__(self, store, dev_ids, host_ids):
        self.store, self.dev_ids, self.host_ids = store, dev_ids, host_ids
        self.sizes = store.sizes(host_ids)
        self.need = self.sizes[:2] + (int(dev_ids.shape[0]),) + self.sizes[2:]


class StagedTaskGraph(StagedPairGraph):
    """A one-segment StagedPairGraph with the batch's targets: ``target`` is
    int64 [B] (class labels) or fp32 [B, C], written by ``stage_task``."""

    def __init__(self, device, node_cap: int, edge_cap: int, graphs: int, labels: bool, cols: int):
        super().__init__(device, node_cap, edge_cap, [graphs])
        self.labels, self.cols = bool(labels), 1 if labels else int(cols)
        if labels:
            self.target = torch.zeros(graphs, dtype=torch.long, device=device)
        else:
            self.target = torch.zeros(graphs, self.cols, dtype=torch.float32, device=device)

    def stage_task(self, data) -> None:
        """The batch's x / edge_index / edge_attr / batch and ``data.y`` in, one
        launch on the current stream; the inputs stay alive until the next."""
        B = self.graphs_per_segment[0]
        if _num_graphs_of(data) != B:
            raise ValueError(f"StagedTaskGraph: {_num_graphs_of(data)} molecules, built for {B}")
        if data.x.device.type != "cuda" or data.y.device.type != "cuda":
            raise RuntimeError("StagedTaskGraph: the batch must be on the GPU")
        x = data.x.to(torch.long).contiguous()
        ei = data.edge_index.to(torch.long).contiguous()
        ea = data.edge_attr.to(torch.long).contiguous()
        b = getattr(data, "batch", None)
        if b is None:
            b = torch.zeros(x.shape[0], dtype=torch.long, device=x.device)
        b = b.to(torch.long).contiguous()
        if self.labels:
            y = data.y.reshape(B).to(torch.long).contiguous()
        else:
            y = data.y.reshape(B, self.cols).to(torch.float32).contiguous()
        src = _lib.StageSourceC(x.data_ptr(), ei.data_ptr(), ea.data_ptr(), b.data_ptr(),
                                int(x.shape[0]), int(ei.shape[1]))
        _lib.call("molclr_stage_task", ctypes.addressof(src), ctypes.addressof(self._dst),
                  self.x.data_ptr(), self.num_nodes, self.num_edges, self.counts.data_ptr(),
                  y.data_ptr(), self.target.data_ptr(), B, self.cols, int(not self.labels),
                  _lib.stream_of(self.device))
        self._keep = [x, ei, ea, b, y]

    def stage_task_ids(self, store, dev_ids, host_ids, sizes=None) -> None:
        """The batch of the molecules ``dev_ids`` (int64, on the device) of a
        task_store.DeviceTaskStore in -- what ``stage_task`` writes for the
        collated batch, gathered from the store by ``molclr_stage_task_ids``
        with no collated copy in between.  ``host_ids`` (or ``sizes``, from
        ``store.sizes``) size the batch; ``ids_status`` gets the launch's
        validity word (task_store.raise_for_collate_status)."""
        B = self.graphs_per_segment[0]
        if dev_ids.dim() != 1 or int(dev_ids.shape[0]) != B:
            raise ValueError(f"StagedTaskGraph: {tuple(dev_ids.shape)} molecule ids, built for {B}")
        if dev_ids.device.type != "cuda" or dev_ids.dtype != torch.long:
            raise RuntimeError("StagedTaskGraph: the molecule ids must be int64 on the GPU")
        if store.labels != self.labels or (not self.labels and store.cols != self.cols):
            raise ValueError("StagedTaskGraph: the store's targets do not match the graph's "
                             f"(labels {store.labels} / {self.labels}, columns {store.cols} / "
                             f"{self.cols})")
        n, e = (sizes if sizes is not None else store.sizes(host_ids))[:2]
        if getattr(self, "ids_status", None) is None:
            self.ids_status = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._ids_ws_bytes = _lib.query("molclr_collate_task_workspace_bytes", B)
            self._ids_ws = torch.empty(self._ids_ws_bytes, dtype=torch.uint8, device=self.device)
        dev_ids = dev_ids.contiguous()
        _lib.call("molclr_stage_task_ids", store.x.data_ptr(), store.atom_ptr.data_ptr(),
                  store.edge_index.data_ptr(), store.edge_attr.data_ptr(),
                  store.bond_ptr.data_ptr(), store.num_molecules, int(store.edge_index.shape[1]),
                  dev_ids.data_ptr(), B, store.y.data_ptr(), self.cols, int(not self.labels),
                  int(n), int(e), ctypes.addressof(self._dst), self.x.data_ptr(), self.num_nodes,
                  self.num_edges, self.counts.data_ptr(), self.target.data_ptr(),
                  self.ids_status.data_ptr(), self._ids_ws.data_ptr(), self._ids_ws_bytes,
                  _lib.stream_of(self.device))
        self._keep = [dev_ids]


class StagedMotifGraph(StagedTaskGraph):
    """A StagedTaskGraph that also holds the motif model's items in buffers of
    ``item_cap`` entries, written by ``stage_items``: ``clique`` (the ids,
    then _lib.MOTIF_PAD), ``mol_ptr`` int32 [B + 1] (the item count on the
    device: ``mol_ptr[B]``), ``sorted_idx`` / ``order`` (the stable sort by
    id, padding last).  ``item_status`` ORs the staging's refusal bits."""

    def __init__(self, device, node_cap: int, edge_cap: int, graphs: int, labels: bool, cols: int,
                 item_cap: int):
        super().__init__(device, node_cap, edge_cap, graphs, labels, cols)
        self.item_cap = int(item_cap)
        i64 = dict(dtype=torch.long, device=device)
        self.clique = torch.full((self.item_cap,), _lib.MOTIF_PAD, **i64)
        self.sorted_idx = torch.full((self.item_cap,), _lib.MOTIF_PAD, **i64)
        self.order = torch.arange(self.item_cap, **i64)
        self.mol_ptr = torch.zeros(graphs + 1, dtype=torch.int32, device=device)
        self.item_status = torch.zeros(1, dtype=torch.int32, device=device)
        self._keep_items = []

    def stage_items(self, mol_idx, clique_idx) -> None:
        """The batch's ``mol_idx`` [T + B] and ``clique_idx`` [T] in, one launch
        on the current stream; the inputs stay alive until the next."""
        B = self.graphs_per_segment[0]
        if mol_idx.dim() != 1 or clique_idx.dim() != 1 or \
                mol_idx.shape[0] != clique_idx.shape[0] + B:
            raise ValueError(f"mol_idx must be [T + B] and clique_idx [T] with B = {B}; got "
                             f"{tuple(mol_idx.shape)} and {tuple(clique_idx.shape)}")
        T = int(clique_idx.shape[0])
        if T > self.item_cap:
            raise ValueError(f"StagedMotifGraph: {T} items, built for {self.item_cap}")
        mol_idx = mol_idx.to(self.device, torch.long).contiguous()
        clique_idx = clique_idx.to(self.device, torch.long).contiguous()
        _lib.call("molclr_stage_motif", mol_idx.data_ptr(), clique_idx.data_ptr(), T, B,
                  self.item_cap, self.clique.data_ptr(), self.mol_ptr.data_ptr(),
                  self.sorted_idx.data_ptr(), self.order.data_ptr(), self.item_status.data_ptr(),
                  _lib.stream_of(self.device))
        self._keep_items = [mol_idx, clique_idx]

    def stage_items_ids(self, store, dev_ids, host_ids, sizes=None) -> None:
        """The items of the molecules ``dev_ids`` from the store's motif CSR
        (``store.set_motifs``): exactly what ``stage_items`` writes for
        ``motifs.motif_batch(ids, assignments)``, expanded on the device
        (``molclr_stage_motif_ids``).  More items than ``item_cap`` are refused
        on the device (``item_status``: STATUS_ITEM_OVERFLOW)."""
        B = self.graphs_per_segment[0]
        if store.motif_ptr is None:
            raise RuntimeError("StagedMotifGraph: the store holds no motifs (set_motifs)")
        if dev_ids.dim() != 1 or int(dev_ids.shape[0]) != B:
            raise ValueError(f"StagedMotifGraph: {tuple(dev_ids.shape)} molecule ids, built for {B}")
        if dev_ids.device.type != "cuda" or dev_ids.dtype != torch.long:
            raise RuntimeError("StagedMotifGraph: the molecule ids must be int64 on the GPU")
        T = (sizes if sizes is not None else store.sizes(host_ids))[2]
        if getattr(self, "_items_ws", None) is None:
            self._items_ws_bytes = _lib.query("molclr_stage_motif_ids_workspace_bytes", B,
                                              self.item_cap)
            self._items_ws = torch.empty(self._items_ws_bytes, dtype=torch.uint8,
                                         device=self.device)
        dev_ids = dev_ids.contiguous()
        _lib.call("molclr_stage_motif_ids", store.motif_ptr.data_ptr(), store.motif_ids.data_ptr(),
                  store.num_molecules, dev_ids.data_ptr(), B, int(T), self.item_cap,
                  self.clique.data_ptr(), self.mol_ptr.data_ptr(), self.sorted_idx.data_ptr(),
                  self.order.data_ptr(), self.item_status.data_ptr(), self._items_ws.data_ptr(),
                  self._items_ws_bytes, _lib.stream_of(self.device))
        self._keep_items = [dev_ids]


class _CapturedTask:
    """What the two step objects share: the buckets, their lookup and the
    capture discipline of graph_step.CapturedTrainStep (dry run first, a
    private pool per capture, CAPTURE_SCOPE / CAPTURE_KEEP, the plane
    generation bumped before and after)."""

    def __init__(self, model, criterion, normalizer, node_quantum, edge_quantum, max_graphs,
                 node_slack, edge_headroom, device=None, item_quantum: int = 256):
        from .ginet_finetune import TASK_LOSS
        if not hasattr(model, "loss_staged"):
            raise TypeError(f"{type(self).__name__}: the model has no loss_staged")
        self.model = model
        self.criterion = criterion or TASK_LOSS[model.task]
        if self.criterion not in ("cross_entropy", "mse", "l1"):
            raise ValueError(f"criterion {criterion!r}: 'cross_entropy', 'mse' or 'l1'")
        self.labels = self.criterion == "cross_entropy"
        self.normalizer = None if self.labels else normalizer
        self.node_quantum, self.edge_quantum = int(node_quantum), int(edge_quantum)
        self.node_slack = 2 * self.node_quantum if node_slack is None else int(node_slack)
        self.edge_headroom = float(edge_headroom)
        # the motif model: keys carry a fourth term, the item capacity
        self.motif = _is_motif(model)
        self.item_quantum = int(item_quantum)
        self.max_graphs = int(max_graphs)
        self._graphs: OrderedDict = OrderedDict()
        self.captures = 0
        self.replays = 0
        self.last_graph: StagedTaskGraph | None = None
        self.device = device
        self._made = False

    # -- device state, made on first use (the arithmetic above needs no GPU) ----
    def _make_state(self) -> None:
        if self._made:
            return
        if self.device is None:
            self.device = next(self.model.parameters()).device
        self.out_dim = int(self.model._head_layers()[0][-1].out_features)
        self._head_sync = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._alloc()
        self._made = True

    def _alloc(self) -> None:
        raise NotImplementedError

    # -- buckets ---------------------------------------------------------------
    def _need(self, data, items=None) -> tuple:
        """(nodes, edges, molecules) of a batch, or of a size tuple; for the
        motif model a fourth term, the number of motif items (``items``: the
        count, ``(mol_idx, clique_idx)``, or the size tuple's fourth term)."""
        if isinstance(data, _IdsBatch):  # the size tuple of store.sizes, and the ids' count
            if self.motif and len(data.need) != 4:
                raise TypeError("the motif model's step needs the store's motifs (set_motifs)")
            need = data.need
        elif isinstance(data, tuple):
            need = tuple(int(v) for v in data)
        else:
            need = (int(data.x.shape[0]), int(data.edge_index.shape[1]), _num_graphs_of(data))
        if not self.motif:
            return need[:3]
        if len(need) == 4:
            return need
        if items is None:
            raise TypeError("the motif model's step needs the batch's items "
                            "(mol_idx, clique_idx)")
        t = items if isinstance(items, int) else int(items[1].shape[0])
        return need + (int(t),)

    def bucket(self, data, items=None) -> tuple:
        """(node_cap, edge_cap, molecules) a new capture for this batch gets;
        (node_cap, edge_cap, molecules, item_cap) for the motif model."""
        n, e, g, *t = self._need(data, items)
        e_cap = _round_up(int(e * (1.0 + self.edge_headroom)) + 1, self.edge_quantum)
        key = (_round_up(n, self.node_quantum), e_cap, g)
        return key + (_round_up(t[0], self.item_quantum),) if t else key

    def pick(self, keys, data, items=None):
        """Of the captured ``keys`` (node_cap, edge_cap, molecules[, item_cap]),
        the one this batch replays on: the smallest that holds it with the same
        molecule count (a partial last batch is a bucket of its own) and a
        node capacity within ``node_slack`` rows of the batch's own rounded
        size; None when none does.  The motif model's item capacity must hold
        the batch's items; among keys equal in nodes and edges the smallest
        does."""
        n, e, g, *t = self._need(data, items)
        limit = _round_up(n, self.node_quantum) + self.node_slack
        best = None
        for k in keys:
            if k[0] >= n and k[1] >= e and k[0] <= limit and k[2] == g:
                if t and k[3] < t[0]:
                    continue
                if best is None or k[:2] + k[3:] < best[:2] + best[3:]:
                    best = k
        return best

    def lookup(self, data, items=None):
        """The captured entry this batch would replay on, or None."""
        k = self.pick(list(self._graphs), data, items)
        return None if k is None else self._graphs[k]

    def _insert(self, key, ent) -> None:
        self._graphs[key] = ent
        if len(self._graphs) > self.max_graphs:
            self._graphs.popitem(last=False)

    def _entry(self, data, items=None):
        self._make_state()
        k = self.pick(list(self._graphs), data, items)
        if k is None:
            k = self.bucket(data, items)
            self._insert(k, self._capture(k, data, items))  # stages this batch too
            return self._graphs[k], True
        self._graphs.move_to_end(k)  # least-recently-replayed eviction
        return self._graphs[k], False

    def prepare(self, batches, motif=None) -> int:
        """Capture (without running) every graph the given batches need;
        returns the number of new captures.  ``motif`` (the motif model): a
        callable from a host batch to its ``(mol_idx, clique_idx)``."""
        before = self.captures
        with self._mode():
            for data in batches:
                items = motif(data) if self.motif else None
                self._entry(data.to(self.device) if self.device is not None else data, items)
        return self.captures - before

    def _mode(self):
        """The context captures and replays run in."""
        return contextlib.nullcontext()

    @property
    def buckets(self) -> list:
        """(node_cap, edge_cap, molecules[, item_cap]) of every live capture."""
        return list(self._graphs)

    # -- capture ---------------------------------------------------------------
    def _optimizers(self) -> tuple:
        return ()

    def _body(self, graph):
        """The step through the Python layer (the dry run and the capture run
        the same code); returns what must stay alive until it is recorded."""
        raise NotImplementedError

    def _target(self, graph):
        """The head's target: the staged one, normalised with the torch ops the
        eager loop uses (FineTune._step) -- the same arithmetic by construction."""
        return self.normalizer.norm(graph.target) if self.normalizer else graph.target

    def _stage(self, graph, data, items) -> None:
        if isinstance(data, _IdsBatch):
            graph.stage_task_ids(data.store, data.dev_ids, data.host_ids, data.sizes)
            torch.bitwise_or(self.collate_status, graph.ids_status, out=self.collate_status)
            if self.motif:
                graph.stage_items_ids(data.store, data.dev_ids, data.host_ids, data.sizes)
            return
        graph.stage_task(data)
        if self.motif:
            graph.stage_items(*items)

    def _capture(self, key, data=None, items=None) -> _Captured:
        reason = unsupported_reason(self.model, motif_items=self.motif)
        if reason is None and not self.model._executor_ok():
            reason = "the encoder executor does not take the model's BatchNorm / dropout settings"
        if reason:
            raise NotImplementedError(f"{type(self).__name__}: {reason}")
        ops._check_no_timer()
        if self.motif:
            graph = StagedMotifGraph(self.device, key[0], key[1], key[2], self.labels,
                                     self.out_dim, key[3])
        else:
            graph = StagedTaskGraph(self.device, key[0], key[1], key[2], self.labels, self.out_dim)
        if data is not None:
            self._stage(graph, data, items)
        for opt in self._optimizers():
            opt.sync_lr()
        # the capture must record the weight-plane regeneration: make every
        # cached image stale so the forward's first lookup refreshes them all
        ops.bump_param_generation()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize(self.device)
        ops.CAPTURE_HEAD_SYNC = self._head_sync
        try:
            # dry run: every library call skipped; what it leaves behind (the
            # weight images, the dropout state) is what the capture must not
            # allocate from its pool
            with _lib.dry_run():
                held = self._body(graph)
            del held
            ops.bump_param_generation()
            torch.cuda.synchronize(self.device)
            ops.CAPTURE_SCOPE = {id(p) for p in self.model.parameters()}
            ops.CAPTURE_KEEP = keep = []
            # a private pool per capture (graph_step.CapturedTrainStep)
            with torch.cuda.graph(g, pool=torch.cuda.graph_pool_handle()):
                graph.build()
                held = self._body(graph)
            del held
        finally:
            ops.CAPTURE_SCOPE = None
            ops.CAPTURE_KEEP = None
            ops.CAPTURE_HEAD_SYNC = None
        self.captures += 1
        # a capture only records: the cached images must be regenerated by the
        # next eager use as well
        ops.bump_param_generation()
        ent = _Captured(graph, g, keep)
        ent.bn_mode = self._bn_mode()
        return ent

    def _bn_mode(self) -> tuple:
        """What a capture is valid for besides its capacities: the model's
        training flag (the dropout) and each BatchNorm's (batch or running
        statistics) -- the recorded kernels differ."""
        return (bool(self.model.training),) + tuple(bool(bn.training)
                                                    for bn in self.model.batch_norms)

    def _replay(self, data, items=None):
        ent, fresh = self._entry(data, items)
        if ent.bn_mode != self._bn_mode():
            raise RuntimeError(
                f"{type(self).__name__}: the model's BatchNorm / training mode changed after "
                "this bucket was captured (freeze_bn or a BatchNorm's train() / eval()); "
                "close() the captured graphs and capture again")
        if not fresh:
            self._stage(ent.graph, data, items)
            for opt in self._optimizers():
                opt.sync_lr()
        ent.cuda_graph.replay()
        self.replays += 1
        self.last_graph = ent.graph
        return ent

    def check(self) -> None:
        """Raise ValueError if any replayed batch so far had invalid inputs."""
        self._make_state()
        st = int(self.status.item())
        if self.motif:  # the item staging's own refusals
            for ent in self._graphs.values():
                st |= int(ent.graph.item_status.item())
        raise_for_status(st)
        from .task_store import raise_for_collate_status
        raise_for_collate_status(int(self.collate_status.item()))  # step_ids' batches

    def close(self) -> None:
        """Release every captured graph (and its pool's memory) now."""
        if self.device is not None:
            torch.cuda.synchronize(self.device)
        self._graphs.clear()
        self.last_graph = None
        import gc
        gc.collect()
        if self.device is not None:
            torch.cuda.synchronize(self.device)


class CapturedFinetuneStep(_CapturedTask):
    """``step(data) -> loss``: one fine-tuning step (finetune.py:89-102 with
    the trainer's zero_grad / backward / Adam around it) replayed from a HIP
    graph captured per capacity bucket; ``data`` is a labelled batch on the
    GPU (``.y``: int64 class labels or float targets [B, C]).

    ``optimizers``: one FusedAdam or two (GCN's base and ``pred_lin`` groups);
    each keeps its own learning rate on the device, synced before every
    replay.  ``criterion``: 'cross_entropy', 'mse', 'l1' or None (by the
    model's task); ``normalizer`` (finetune.Normalizer) is applied to float
    targets inside the graph.  Buckets are keyed (node capacity, edge
    capacity, molecules): lookup as graph_step.CapturedTrainStep's, and a
    partial last batch gets a bucket of its own.  The motif model's step is
    ``step(data, mol_idx, clique_idx)`` and its keys carry a fourth term, the
    item capacity (``item_quantum``): a batch with more items than a bucket
    holds replays on a larger one or captures it.

    The returned loss is this object's own buffer, overwritten by the next
    step.  ``status`` ORs every replayed batch's validity word -- graph
    indices, atom features and the head's class-label bit -- and ``check()``
    raises for an invalid batch at any earlier step."""

    def __init__(self, model, optimizers, criterion=None, normalizer=None, node_quantum: int = 256,
                 edge_quantum: int = 2048, max_graphs: int = 16, node_slack: int | None = None,
                 edge_headroom: float = 0.04, item_quantum: int = 256):
        from .optim import FusedAdam
        if isinstance(optimizers, FusedAdam):
            optimizers = [optimizers]
        optimizers = list(optimizers)
        if not 1 <= len(optimizers) <= 2 or not all(isinstance(o, FusedAdam) for o in optimizers):
            raise TypeError("CapturedFinetuneStep needs one or two molclr_amd.optim.FusedAdam "
                            "(learning rate and step counter on the device)")
        super().__init__(model, criterion, normalizer, node_quantum, edge_quantum, max_graphs,
                         node_slack, edge_headroom, optimizers[0].flat.device, item_quantum)
        self.optimizers = optimizers

    def _optimizers(self):
        return self.optimizers

    def _alloc(self) -> None:
        self.loss = torch.zeros((), dtype=torch.float32, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        # sticky OR of every stage_task_ids' validity word (step_ids)
        self.collate_status = torch.zeros(1, dtype=torch.int32, device=self.device)
        # d loss / d loss from a tensor made before any capture: no fill
        # kernel in the graph for autograd's ones_like(loss)
        self._one = torch.ones((), dtype=torch.float32, device=self.device)

    def _body(self, graph):
        opts = self.optimizers
        for opt in opts:
            opt.zero_grad()
        _, pred, loss = self.model.loss_staged(graph, self._target(graph), self.criterion)
        loss.backward(self._one)
        for opt in opts:
            opt.step(sync_lr=False, tick=False)
        # one closing launch: both step counters, the loss into this object's
        # buffer, the batch's validity bits into the sticky status word
        _lib.call("molclr_task_step_tail", opts[0]._step_dev.data_ptr(),
                  opts[1]._step_dev.data_ptr() if len(opts) > 1 else None, loss.data_ptr(),
                  self.loss.data_ptr(), graph.status.data_ptr(), self.status.data_ptr(),
                  _lib.stream_of(self.device))
        return pred, loss

    def step(self, data, mol_idx=None, clique_idx=None) -> torch.Tensor:
        if not self.model.training:
            raise RuntimeError("CapturedFinetuneStep: the model must be in training mode")
        if self.motif and (mol_idx is None or clique_idx is None):
            raise TypeError("CapturedFinetuneStep: the motif model's step takes "
                            "(data, mol_idx, clique_idx)")
        self._replay(data, (mol_idx, clique_idx) if self.motif else None)
        # the replay's Adam steps changed the weights behind Python's back
        ops.bump_param_generation()
        return self.loss

    def step_ids(self, store, dev_ids, host_ids) -> torch.Tensor:
        """``step`` of the batch of the molecules ``dev_ids`` (int64, on the
        device; ``host_ids``: their host copy, which sizes the batch) of a
        task_store.DeviceTaskStore: the batch is gathered from the store
        straight into the graph's buffers, and the motif model's items from the
        store's motif CSR."""
        if not self.model.training:
            raise RuntimeError("CapturedFinetuneStep: the model must be in training mode")
        self._replay(_IdsBatch(store, dev_ids, host_ids))
        ops.bump_param_generation()
        return self.loss

    __call__ = step


class CapturedEval(_CapturedTask):
    """``run(loader) -> (mean_loss, predictions, labels)``: an evaluation pass
    (finetune.py:259-317) with every batch replayed from a HIP graph.

    Where the eager loop synchronises three times per batch (``loss.item()``
    and two ``.cpu()`` copies), the graph's closing launch appends the batch's
    predictions and staged targets to device buffers behind a device cursor
    and adds ``loss * B`` to an fp64 sum in the loop's order; the pass ends
    with one synchronisation and one device-to-host copy.  Predictions are
    de-normalised after the copy.  ``predictions`` is float32 [n, C],
    ``labels`` the flattened targets (int64 or float32), both numpy.  For the
    motif model ``run(loader, motif=fn)`` takes a callable from a host batch to
    its ``(mol_idx, clique_idx)``.

    ``capacity``: rows the gather buffers hold.  None (the default) sizes them
    by the loader and grows them when a larger one comes (the graphs are
    captured again: they hold the buffers' addresses); a given capacity is
    kept, and rows past it are refused on the device (no store; the status
    bit STATUS_EVAL_OVERFLOW makes ``run`` raise)."""

    _HEADER = 64  # bytes: cursor int64, loss sum fp64, status int32, collate status int32

    def __init__(self, model, criterion=None, normalizer=None, capacity: int | None = None,
                 node_quantum: int = 256, edge_quantum: int = 2048, max_graphs: int = 16,
                 node_slack: int | None = None, edge_headroom: float = 0.04,
                 item_quantum: int = 256):
        super().__init__(model, criterion, normalizer, node_quantum, edge_quantum, max_graphs,
                         node_slack, edge_headroom, None, item_quantum)
        self.fixed = capacity is not None
        self.capacity = int(capacity) if self.fixed else 0
        self._sticky = 0  # status bits of earlier passes (check())
        self._collate_sticky = 0  # and of their device collates (a DeviceTaskLoader's)

    @contextlib.contextmanager
    def _mode(self):
        self._make_state()
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                yield
        finally:
            self.model.train(was_training)

    def _alloc(self) -> None:
        # the normalizer's constants on the host, once: run() copies nothing else
        n = self.normalizer
        self._denorm = None if n is None else (n.std.detach().cpu(), n.mean.detach().cpu())
        self._alloc_rows(self.capacity if self.fixed else max(self.capacity, 1024))

    def _alloc_rows(self, rows: int) -> None:
        """One buffer, so that one copy brings everything to the host: header,
        pred_all [rows, C] fp32, target_all [rows] int64 or [rows, C] fp32."""
        self._graphs.clear()  # they hold the old buffers' addresses
        self.capacity = int(rows)
        C = self.out_dim
        pred_bytes = (rows * C * 4 + 15) // 16 * 16
        tgt_bytes = rows * (8 if self.labels else 4 * C)
        self._buf = torch.zeros(self._HEADER + pred_bytes + tgt_bytes, dtype=torch.uint8,
                                device=self.device)
        self._layout = (self._HEADER, self._HEADER + pred_bytes)
        self.cursor, self.loss_acc, self.status, self.pred_all, self.target_all = \
            self._views(self._buf)
        self.collate_status = self._buf[20:24].view(torch.int32)

    def _views(self, buf):
        p0, t0 = self._layout
        rows, C = self.capacity, self.out_dim
        cursor = buf[0:8].view(torch.long)
        loss_acc = buf[8:16].view(torch.float64)
        status = buf[16:20].view(torch.int32)
        pred = buf[p0:p0 + rows * C * 4].view(torch.float32).view(rows, C)
        if self.labels:
            tgt = buf[t0:t0 + rows * 8].view(torch.long)
        else:
            tgt = buf[t0:t0 + rows * C * 4].view(torch.float32).view(rows, C)
        return cursor, loss_acc, status, pred, tgt

    def _body(self, graph):
        _, pred, loss = self.model.loss_staged(graph, self._target(graph), self.criterion)
        B, C = graph.graphs_per_segment[0], self.out_dim
        _lib.call("molclr_eval_tail", pred.data_ptr(), graph.target.data_ptr(), B, C,
                  2 if self.labels else C, loss.data_ptr(), self.pred_all.data_ptr(),
                  self.target_all.data_ptr(), self.capacity, self.cursor.data_ptr(),
                  self.loss_acc.data_ptr(), graph.status.data_ptr(), self.status.data_ptr(),
                  _lib.stream_of(self.device))
        return pred, loss

    @staticmethod
    def _rows_of(loader):
        for obj in (getattr(loader, "sampler", None), loader):
            if isinstance(obj, (list, tuple)):
                return sum(_num_graphs_of(d) for d in obj)
        s = getattr(loader, "sampler", None)
        return len(s) if s is not None and hasattr(s, "__len__") else None

    def run(self, loader, motif=None):
        from .task_store import DeviceTaskLoader, raise_for_collate_status
        by_ids = isinstance(loader, DeviceTaskLoader)  # staged by ids, items from the store
        if self.motif and motif is None and not by_ids:
            raise TypeError("CapturedEval: the motif model's pass takes motif=callable, from a "
                            "host batch to its (mol_idx, clique_idx)")
        self._make_state()
        if not self.fixed:
            rows = self._rows_of(loader)
            if rows is None:  # unknown length: read it once
                loader = list(loader)
                rows = self._rows_of(loader)
            if rows > self.capacity:
                self._alloc_rows(rows)
        self._buf[:self._HEADER].zero_()
        with self._mode():
            if by_ids:
                for dev_ids, host_ids in loader.ids():
                    self._replay(_IdsBatch(loader.store, dev_ids, host_ids))
            else:
                for data in loader:
                    items = motif(data) if self.motif else None
                    self._replay(data.to(self.device), items)
        host = self._buf.cpu()  # the pass's one synchronisation and one copy
        cursor, loss_acc, status, pred, tgt = self._views(host)
        self._sticky |= int(status.item())
        self._collate_sticky |= int(host[20:24].view(torch.int32).item())
        raise_for_status(self._sticky)
        raise_for_collate_status(self._collate_sticky)
        n = int(cursor.item())
        pred, tgt = pred[:n], tgt[:n]
        if self._denorm is not None:  # Normalizer.denorm, after the copy
            pred = pred * self._denorm[0] + self._denorm[1]
        mean_loss = float(loss_acc.item()) / max(n, 1)
        return mean_loss, pred.numpy().copy(), tgt.reshape(-1).numpy().copy()

    def check(self) -> None:
        from .task_store import raise_for_collate_status
        raise_for_status(self._sticky)
        raise_for_collate_status(self._collate_sticky)


__all__ = ["CapturedEval", "CapturedFinetuneStep", "StagedMotifGraph", "StagedTaskGraph",
           "unsupported_reason"]
