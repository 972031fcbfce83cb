"""GCN encoder + supervised task head — drop-in for models/gcn_finetune.py.

Same class name, constructor arguments, parameter-creation order and
``state_dict`` keys as the reference (models/gcn_finetune.py:94-174): the
pre-training GCN encoder and ``feat_lin``, then ``pred_lin.{0,2}.*`` =
Linear(feat, feat/2), Softplus, Linear(feat/2, 2 | 1); no ``out_lin``.  The
encoder runs as gcn_molclr.GCN's does; everything after the pooling is one
ops.task_head call (see ginet_finetune).
"""
from __future__ import annotations

from torch import nn

from . import gcn_molclr
from .gcn_molclr import GCNConv, num_atom_type, num_chirality_tag
from .ginet_finetune import FinetuneReadout, task_out_dim


class GCN(FinetuneReadout, gcn_molclr.GCN):
    """models/gcn_finetune.py:94-174."""

    def __init__(self, task='classification', num_layer=5, emb_dim=300, feat_dim=256,
                 drop_ratio=0, pool='mean'):
        # The parent's __init__ is NOT called (it would create out_lin, see
        # ginet_finetune.GINet).  COUPLING: whatever gcn_molclr.GCN.__init__
        # sets that its encoder methods read must be set here too;
        # tests/test_finetune_cpu.py compares the two classes' attributes.
        nn.Module.__init__(self)
        self.num_layer = num_layer
        self.emb_dim = emb_dim
        self.feat_dim = feat_dim
        self.drop_ratio = drop_ratio
        self.task = task
        out_dim = task_out_dim(task)

        if self.num_layer < 2:
            raise ValueError("Number of GNN layers must be greater than 1.")

        self.x_embedding1 = nn.Embedding(num_atom_type, emb_dim)
        self.x_embedding2 = nn.Embedding(num_chirality_tag, emb_dim)
        nn.init.xavier_uniform_(self.x_embedding1.weight.data)
        nn.init.xavier_uniform_(self.x_embedding2.weight.data)

        self.gnns = nn.ModuleList()
        for _ in range(num_layer):
            self.gnns.append(GCNConv(emb_dim, aggr="add"))

        self.batch_norms = nn.ModuleList()
        for _ in range(num_layer):
            self.batch_norms.append(nn.BatchNorm1d(emb_dim))

        if pool in ('mean', 'add', 'max'):
            self.pool = pool
        else:
            raise ValueError('Not defined pooling!')

        self.feat_lin = nn.Linear(self.emb_dim, self.feat_dim)

        self.pred_lin = nn.Sequential(
            nn.Linear(self.feat_dim, self.feat_dim // 2),
            nn.Softplus(),
            nn.Linear(self.feat_dim // 2, out_dim),
        )

    def _head_layers(self):
        return [self.pred_lin[0], self.pred_lin[2]], ['softplus', None]
