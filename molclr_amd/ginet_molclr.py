"""GIN-E encoder + projection head — drop-in for models/ginet_molclr.py.

Same class names, constructor arguments, parameter-creation order (hence the
same seeded initialisation) and ``state_dict`` keys as the reference
(models/ginet_molclr.py:16-117): ``x_embedding{1,2}.weight``,
``gnns.{l}.mlp.{0,2}.{weight,bias}``, ``gnns.{l}.edge_embedding{1,2}.weight``,
``batch_norms.{l}.*``, ``feat_lin.*``, ``out_lin.{0,2}.*``.  The forward runs
entirely on the HIP kernels of libmolclr_hip.so (see molclr_amd.ops).
"""
from __future__ import annotations

from torch import nn

from . import ops
from .data import DeviceGraph
from .encoder import (Encoder, num_atom_type, num_bond_direction,  # noqa: F401
                      num_bond_type, num_chirality_tag)


class GINEConv(nn.Module):
    """GIN-E convolution, models/ginet_molclr.py:16-47.

    ``out_i = MLP( Σ_{j→i} (x_j + e_ji) + (x_i + e_self) )`` with
    ``e = E1[bond type] + E2[bond dir]`` and the self loop (type 4, dir 0).
    """

    def __init__(self, emb_dim):
        super().__init__()
        self.mlp = nn.Sequential(
            nn.Linear(emb_dim, 2 * emb_dim),
            nn.ReLU(),
            nn.Linear(2 * emb_dim, emb_dim),
        )
        self.edge_embedding1 = nn.Embedding(num_bond_type, emb_dim)
        self.edge_embedding2 = nn.Embedding(num_bond_direction, emb_dim)
        nn.init.xavier_uniform_(self.edge_embedding1.weight.data)
        nn.init.xavier_uniform_(self.edge_embedding2.weight.data)

    def aggregate(self, x, graph: DeviceGraph, Ec=None):
        """Ec: this layer's combined edge table (ops.edge_tables_combine), or None."""
        return ops.gine_aggregate(x, self.edge_embedding1.weight, self.edge_embedding2.weight,
                                  graph, Ec)

    def update(self, aggr_out):
        return ops.gin_mlp(aggr_out, self.mlp[0].weight, self.mlp[0].bias, self.mlp[2].weight,
                           self.mlp[2].bias)

    def forward(self, x, edge_index, edge_attr, graph: DeviceGraph | None = None):
        if graph is None:
            graph = DeviceGraph(edge_index, edge_attr, x.shape[0])
        return self.update(self.aggregate(x, graph))




def check_precision(precision):
    if precision not in ('fp32', 'bf16'):
        raise ValueError(f"precision {precision!r}: 'fp32' or 'bf16'")
    return precision


class GINet(Encoder):
    """models/ginet_molclr.py:50-117.  ``forward(data) -> (h [B, feat_dim],
    out [B, feat_dim // 2])``; constructor and forward plumbing: Encoder."""

    def __init__(self, num_layer=5, emb_dim=300, feat_dim=256, drop_ratio=0, pool='mean',
                 precision='fp32'):
        super().__init__()
        # 'bf16': the c5 configuration (BASELINE.json) / the reference's
        # fp16_precision switch (molclr.py:16-24,93-96): bf16 node features and
        # bf16 MFMA GEMMs with fp32 accumulation; fp32 master weights, BatchNorm
        # statistics, pooled features, heads and NT-Xent
        self.precision = check_precision(precision)
        self._init_encoder(num_layer, emb_dim, feat_dim, drop_ratio, pool)
        self._init_projection_head()

    def _make_conv(self, emb_dim):
        return GINEConv(emb_dim)

    def _pad_multiple(self):
        return 8 if self.precision == 'bf16' else 4

    def _layer_params(self, g, bn):
        return [g.mlp[0].weight, g.mlp[0].bias, g.mlp[2].weight, g.mlp[2].bias,
                g.edge_embedding1.weight, g.edge_embedding2.weight, bn.weight, bn.bias]

    # emb_dim D -> D + p, the MLP's hidden width 2D -> 2D + 2p
    _LAYER_PADS = ((0, 1, 0, 2), (0, 2), (0, 2, 0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1))

    def _executor(self, x, graph, bns, params):
        return ops.gin_encoder(x, graph, bns, params, self.precision,
                               drop_ratio=self.drop_ratio, drop_state=self._dropout_state(),
                               drop_training=self.training)

    def _layer_step(self, graph):
        # per-edge embeddings E1[bt] + E2[bd] of every layer, tabulated in one launch
        Ec = ops.edge_tables_combine([g.edge_embedding1.weight for g in self.gnns],
                                     [g.edge_embedding2.weight for g in self.gnns])
        return lambda l, h: self.gnns[l].update(self.gnns[l].aggregate(h, graph, Ec[l]))
