"""What the four model classes share: the encoder's constructor and the code
that drives the native encoder executor (ops.gin_encoder / ops.gcn_encoder).

``Encoder`` is the base of ginet_molclr.GINet and gcn_molclr.GCN, and through
them of the two fine-tuning classes.  A kind supplies its conv class
(``_make_conv``), its pad multiple (``_pad_multiple``), its per-layer
parameters with their pads (``_layer_params`` / ``_LAYER_PADS``), its executor
call (``_executor``) and its per-op layer step (``_layer_step``); everything
else is here once.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .data import DeviceGraph, device_graph, pair_graph

num_atom_type = 119  # including the extra mask tokens
num_chirality_tag = 3

num_bond_type = 5  # including aromatic and self-loop edge
num_bond_direction = 3


def dropout_seed(generator: torch.Generator | None = None, rank: int = 0) -> int:
    """The seed of an encoder's dropout stream: one draw from ``generator``
    (torch's default CPU generator when None, so torch.manual_seed makes runs
    repeatable), xor-ed with rank * 0x9E3779B97F4A7C15 so that the ranks of a
    data-parallel run draw different masks.  Returned as a signed 64-bit
    value (the stream takes its bit pattern)."""
    draw = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.long,
                             generator=generator).item())
    seed = (draw ^ (int(rank) * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF
    return seed - (1 << 64) if seed >= 1 << 63 else seed


def _rank() -> int:
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


class Encoder(nn.Module):
    """Atom embeddings, ``num_layer`` x (conv, BatchNorm), pooling, feat_lin
    (models/ginet_molclr.py:50-117, models/gcn_molclr.py:94-158) and the
    projection head's forward of the two pre-training models."""

    precision = 'fp32'  # GINet and GCN set 'fp32' | 'bf16' per instance

    # F.pad of each _layer_params entry in units of the pad p; None: not padded
    _LAYER_PADS: tuple = ()

    def _make_conv(self, emb_dim) -> nn.Module:
        raise NotImplementedError

    def _pad_multiple(self) -> int:
        """The multiple of emb_dim the kind's kernels take."""
        raise NotImplementedError

    def _layer_params(self, conv, bn) -> list:
        """One layer's parameters in the order its executor takes them."""
        raise NotImplementedError

    def _executor(self, x, graph, bns, params):
        """The kind's ops.*_encoder call."""
        raise NotImplementedError

    def _layer_step(self, graph):
        """``step(layer, h)``: the conv of one layer of the per-op path."""
        raise NotImplementedError

    def _init_encoder(self, num_layer, emb_dim, feat_dim, drop_ratio, pool):
        """The encoder's attributes and modules in the reference's creation
        order (hence its seeded initialisation), up to feat_lin; the caller
        creates its head (out_lin, pred_head, pred_lin) after it."""
        self.num_layer = num_layer
        self.emb_dim = emb_dim
        self.feat_dim = feat_dim
        self.drop_ratio = drop_ratio
        # int64 [seed, call counter] of the executor's dropout stream on the
        # parameters' device, made by the first training forward that needs it
        # (_dropout_state).  A plain attribute, not a buffer: no part of
        # state_dict().  dropout_state[1] = k replays call k's masks.
        self.dropout_state = None

        self.x_embedding1 = nn.Embedding(num_atom_type, emb_dim)
        self.x_embedding2 = nn.Embedding(num_chirality_tag, emb_dim)
        nn.init.xavier_uniform_(self.x_embedding1.weight.data)
        nn.init.xavier_uniform_(self.x_embedding2.weight.data)
        self._init_after_atom_embeddings()

        self.gnns = nn.ModuleList()
        for _ in range(num_layer):
            self.gnns.append(self._make_conv(emb_dim))

        self.batch_norms = nn.ModuleList()
        for _ in range(num_layer):
            self.batch_norms.append(nn.BatchNorm1d(emb_dim))

        # The reference leaves self.pool unset for an unknown name and fails at
        # forward time (ginet_molclr.py:83-88); fail at construction instead.
        if pool not in ('mean', 'add', 'max'):
            raise ValueError('Not defined pooling!')
        self.pool = pool

        self.feat_lin = nn.Linear(self.emb_dim, self.feat_dim)

    def _init_after_atom_embeddings(self):
        """Modules a model creates between the atom embeddings and the GIN /
        GCN layers (the motif model's motif_embedding); none by default."""

    def _init_projection_head(self):
        """out_lin of the pre-training models (ginet_molclr.py:92-96)."""
        self.out_lin = nn.Sequential(
            nn.Linear(self.feat_dim, self.feat_dim),
            nn.ReLU(inplace=True),
            nn.Linear(self.feat_dim, self.feat_dim // 2),
        )

    # Run the node-embedding stack through the native encoder executor (one
    # host call per direction) when its BatchNorm and dropout settings are the
    # ones it implements (dropout: any drop_ratio < 1, the masks drawn inside
    # the executor's kernels); else op by op.
    use_executor = True

    # Frozen BatchNorm: every BatchNorm1d of the encoder stays in eval mode
    # (running statistics, nothing updated) whatever train() is called with, so
    # a trainer's per-epoch model.train() does not undo it; the dropout still
    # follows the model's own flag.  Putting the BatchNorm modules into eval
    # mode by hand gives the same step until the next train() call.
    _freeze_bn = False

    @property
    def freeze_bn(self) -> bool:
        return self._freeze_bn

    @freeze_bn.setter
    def freeze_bn(self, value):
        self._freeze_bn = bool(value)
        self.train(self.training)

    def train(self, mode: bool = True):
        super().train(mode)
        if self._freeze_bn:
            for bn in self.batch_norms:
                bn.eval()
        return self

    def bn_frozen(self) -> bool:
        """Whether this forward differentiates through running statistics
        while the model trains (the executor's MODE_FROZEN_BN)."""
        return self.training and not any(bn.training for bn in self.batch_norms)

    def _executor_ok(self) -> bool:
        # any emb_dim: the executor runs on the width padded to the kernels'
        # multiple (_dim_pad) with zero columns
        if not self.use_executor or self.num_layer > 16:
            return False
        if self.drop_ratio >= 1 and self.training:  # F.dropout's all-zero output: per op
            return False
        bn0 = self.batch_norms[0]
        return all(bn.track_running_stats and bn.affine and bn.momentum is not None
                   and bn.training == bn0.training and bn.momentum == bn0.momentum
                   and bn.eps == bn0.eps for bn in self.batch_norms)

    def _dim_pad(self) -> int:
        """Zero columns that bring emb_dim to the kernels' multiple."""
        return (-self.emb_dim) % self._pad_multiple()

    def _encoder_params(self):
        params = [self.x_embedding1.weight, self.x_embedding2.weight]
        for conv, bn in zip(self.gnns, self.batch_norms):
            params += self._layer_params(conv, bn)
        p = self._dim_pad()
        if not p:
            return params
        # emb_dim D -> D + p with zero rows / columns (F.pad: the gradients of
        # the real entries flow back, the pads' drop).  A zero column stays
        # zero through every layer: embeddings and GIN's edge tables add 0, the
        # weights' zero rows / columns keep it out of the real columns, and
        # BatchNorm with gamma = beta = 0 maps it (and GCN's scalar edge terms,
        # which do reach the pad columns) to 0.
        pads = ((0, 1), (0, 1)) + self._LAYER_PADS * self.num_layer
        return [t if m is None else F.pad(t, tuple(k * p for k in m))
                for t, m in zip(params, pads)]

    def _dropout_state(self):
        """dropout_state for this forward: None when no dropout applies."""
        if not (self.training and self.drop_ratio > 0):
            return None
        dev = self.x_embedding1.weight.device
        if self.dropout_state is None:
            self.dropout_state = torch.tensor([dropout_seed(rank=_rank()), 0], dtype=torch.long)
        if self.dropout_state.device != dev:
            self.dropout_state = self.dropout_state.to(dev)
        return self.dropout_state

    def _run_encoder(self, x, graph):
        """The executor on the (padded) width; returns h [N, emb_dim + pad]."""
        p = self._dim_pad()
        bns = list(self.batch_norms)
        if p:  # running statistics on the padded width, copied back after the call
            bns = [_PaddedBatchNorm(bn, p) for bn in bns]
        h = self._executor(x, graph, bns, self._encoder_params())
        if p:
            for pb in bns:
                pb.copy_back()
        return h

    def encode(self, data, graph: DeviceGraph | None = None):
        """Node embeddings after the last layer (ginet_molclr.py:103-111)."""
        graph = graph or device_graph(data)
        if self._executor_ok():
            h = self._run_encoder(data.x, graph)
            return (h[:, :self.emb_dim] if self._dim_pad() else h), graph
        if self.precision != 'fp32':
            raise NotImplementedError("bf16 runs through the encoder executor only "
                                      "(tracked BatchNorm statistics)")
        if self._dim_pad():
            raise NotImplementedError("emb_dim % 4 != 0 runs through the encoder executor only "
                                      "(tracked BatchNorm statistics)")
        h = ops.atom_embed(data.x, self.x_embedding1.weight, self.x_embedding2.weight,
                           graph.status)
        step = self._layer_step(graph)
        for layer in range(self.num_layer):
            h = step(layer, h)
            last = layer == self.num_layer - 1
            h = ops.batch_norm(h, self.batch_norms[layer], relu=not last)
            if self.drop_ratio > 0 and self.training:
                h = F.dropout(h, self.drop_ratio, training=True)
        return h, graph

    def _embed(self, data):
        """encode(), but the executor's output keeps its padded width (the
        readout takes it as it is)."""
        graph = device_graph(data)
        if self._executor_ok():
            return self._run_encoder(data.x, graph), graph
        return self.encode(data, graph)

    def _pool(self, h, graph):
        """Pooled node embeddings and feat_lin's weight at their width."""
        h = ops.segment_pool(h, graph, self.pool)
        W = self.feat_lin.weight
        if h.shape[1] != W.shape[1]:  # padded width: zero weight columns for the pads
            W = F.pad(W, (0, h.shape[1] - W.shape[1]))
        return h, W

    def _readout(self, h, graph):
        h, W = self._pool(h, graph)
        h = ops.linear(h, W, self.feat_lin.bias, side=True)
        out = ops.projection_head(h, self.out_lin[0].weight, self.out_lin[0].bias,
                                  self.out_lin[2].weight, self.out_lin[2].bias, side=True)
        return h, out

    def forward(self, data):
        """``(h [B, feat_dim], out [B, feat_dim // 2])``."""
        return self._readout(*self._embed(data))

    def forward_staged(self, graph):
        """forward_pair over a StagedPairGraph (molclr_amd.graph_step): the
        views' atoms are graph.x, fixed-capacity buffers whose padding rows
        carry no gradient -- the capturable form of the paired pass."""
        if not self._executor_ok() or self._dim_pad():
            raise NotImplementedError("forward_staged needs the encoder executor at a width "
                                      "the kernels take unpadded")
        return self._readout(self._run_encoder(graph.x, graph), graph)

    def forward_pair(self, xi, xj):
        """Both contrastive views of a step in ONE pass: ``(h, out)`` with the
        rows of ``forward(xi)`` followed by those of ``forward(xj)``
        (molclr.py:57,60).  The views' graphs are built as one
        (molclr_graph_build_multi) and every BatchNorm keeps per-view batch
        statistics, updating its running statistics for view i, then view j
        (molclr_batchnorm_seg_fwd) -- the two-call semantics, with half the
        launches and twice the rows per GEMM / aggregation launch."""
        if not self._executor_ok():
            hi, oi = self(xi)
            hj, oj = self(xj)
            return torch.cat([hi, hj], 0), torch.cat([oi, oj], 0)
        graph = pair_graph(xi, xj)
        x = torch.cat([xi.x, xj.x], 0)
        return self._readout(self._run_encoder(x, graph), graph)


class _PaddedBatchNorm:
    """A BatchNorm1d's settings and running statistics on the padded width
    (Encoder._run_encoder); copy_back() writes the real columns back."""

    def __init__(self, bn: nn.BatchNorm1d, p: int):
        self.bn = bn
        self.training, self.momentum, self.eps = bn.training, bn.momentum, bn.eps
        self.num_batches_tracked = bn.num_batches_tracked
        self.running_mean = F.pad(bn.running_mean, (0, p))
        self.running_var = F.pad(bn.running_var, (0, p), value=1.0)

    def copy_back(self):
        D = self.bn.running_mean.shape[0]
        self.bn.running_mean.copy_(self.running_mean[:D])
        self.bn.running_var.copy_(self.running_var[:D])
