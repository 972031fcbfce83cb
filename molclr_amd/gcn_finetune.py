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
from .gcn_molclr import GCNConv, num_atom_type, num_chirality_tag  # noqa: F401
from .ginet_finetune import FinetuneReadout, task_out_dim


class GCN(FinetuneReadout, gcn_molclr.GCN):
    """models/gcn_finetune.py:94-174."""

    def __init__(self, task='classification', num_layer=5, emb_dim=300, feat_dim=256,
                 drop_ratio=0, pool='mean', precision='fp32'):
        # The parent's __init__ is NOT called (it would create out_lin, see
        # ginet_finetune.GINet).
        nn.Module.__init__(self)
        self.precision = gcn_molclr.check_precision(precision)
        self.task = task
        out_dim = task_out_dim(task)
        self._init_encoder(num_layer, emb_dim, feat_dim, drop_ratio, pool)

        self.pred_lin = nn.Sequential(
            nn.Linear(self.feat_dim, self.feat_dim // 2),
            nn.Softplus(),
            nn.Linear(self.feat_dim // 2, out_dim),
        )

    def _head_layers(self):
        return [self.pred_lin[0], self.pred_lin[2]], ['softplus', None]
