"""GCN encoder + projection head — drop-in for models/gcn_molclr.py.

Same names, constructor arguments, parameter-creation order and state_dict
keys as the reference (models/gcn_molclr.py:39-158; keys verified against the
shipped ``ckpt/pretrained_gcn/checkpoints/model.pth``):
``gnns.{l}.{weight,bias,edge_embedding1.weight,edge_embedding2.weight}``.

The reference computes ``gcn_norm`` and discards the result
(gcn_molclr.py:74), so it has no effect on outputs and is not computed; the
``torch_sparse`` ``message_and_aggregate`` path (gcn_molclr.py:90-91) is dead
for dense ``edge_index`` input and is not provided.
"""
from __future__ import annotations

import math

import torch
from torch import nn
from torch.nn import Parameter

from . import ops
from .data import DeviceGraph
from .encoder import (Encoder, num_atom_type, num_bond_direction,  # noqa: F401
                      num_bond_type, num_chirality_tag)
from .ginet_molclr import check_precision


class GCNConv(nn.Module):
    """models/gcn_molclr.py:39-91:
    ``out_i = Σ_{j→i} (e_ji + (xW)_j) + (e_self + (xW)_i) + b``, scalar e."""

    def __init__(self, emb_dim, aggr="add"):
        super().__init__()
        if aggr != "add":
            raise NotImplementedError("molclr_amd GCNConv supports aggr='add' (the reference's)")
        self.emb_dim = emb_dim
        self.aggr = aggr

        self.weight = Parameter(torch.Tensor(emb_dim, emb_dim))
        self.bias = Parameter(torch.Tensor(emb_dim))
        self.reset_parameters()

        self.edge_embedding1 = nn.Embedding(num_bond_type, 1)
        self.edge_embedding2 = nn.Embedding(num_bond_direction, 1)

        nn.init.xavier_uniform_(self.edge_embedding1.weight.data)
        nn.init.xavier_uniform_(self.edge_embedding2.weight.data)

    def reset_parameters(self):
        stdv = math.sqrt(6.0 / (self.weight.size(-2) + self.weight.size(-1)))
        self.weight.data.uniform_(-stdv, stdv)
        self.bias.data.fill_(0)

    def conv(self, x, graph: DeviceGraph):
        return ops.gcn_conv(x, self.weight, self.bias, self.edge_embedding1.weight,
                            self.edge_embedding2.weight, graph)

    def forward(self, x, edge_index, edge_attr, graph: DeviceGraph | None = None):
        if graph is None:
            graph = DeviceGraph(edge_index, edge_attr, x.shape[0])
        return self.conv(x, graph)


class GCN(Encoder):
    """models/gcn_molclr.py:94-158; constructor and forward plumbing: Encoder."""

    def __init__(self, num_layer=5, emb_dim=300, feat_dim=256, drop_ratio=0, pool='mean',
                 precision='fp32'):
        super().__init__()
        # 'bf16': the reference's fp16_precision switch for the GCN
        # (molclr.py:16-24,93-96): bf16 node features, x W and dxw W^T as bf16
        # MFMA products with fp32 accumulation; fp32 master weights, edge
        # scalars, bias, BatchNorm statistics, pooled features, heads, NT-Xent
        self.precision = check_precision(precision)
        self._init_encoder(num_layer, emb_dim, feat_dim, drop_ratio, pool)
        self._init_projection_head()

    def _init_encoder(self, num_layer, *args):
        if num_layer < 2:
            raise ValueError("Number of GNN layers must be greater than 1.")
        super()._init_encoder(num_layer, *args)

    def _make_conv(self, emb_dim):
        return GCNConv(emb_dim, aggr="add")

    def _pad_multiple(self):
        return 8 if self.precision == 'bf16' else 4

    def _layer_params(self, g, bn):
        return [g.weight, g.bias, g.edge_embedding1.weight, g.edge_embedding2.weight,
                bn.weight, bn.bias]

    # the scalar edge embeddings [5, 1] / [3, 1] have no width to pad
    _LAYER_PADS = ((0, 1, 0, 1), (0, 1), None, None, (0, 1), (0, 1))

    def _executor(self, x, graph, bns, params):
        return ops.gcn_encoder(x, graph, bns, params, drop_ratio=self.drop_ratio,
                               drop_state=self._dropout_state(), precision=self.precision,
                               drop_training=self.training)

    def _layer_step(self, graph):
        return lambda l, h: self.gnns[l].conv(h, graph)
