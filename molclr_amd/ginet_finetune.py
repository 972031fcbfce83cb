"""GIN-E encoder + supervised task head — drop-in for models/ginet_finetune.py.

Same class name, constructor arguments, parameter-creation order (hence the
same seeded initialisation) and ``state_dict`` keys as the reference
(models/ginet_finetune.py:52-157): the pre-training encoder and ``feat_lin``,
then ``pred_head.{0,2,...}.*`` = Linear(feat, feat/2), act, (Linear(feat/2,
feat/2), act) x (pred_n_layer - 1), Linear(feat/2, 2 | 1) with act Softplus or
ReLU; no ``out_lin``.  ``load_my_state_dict`` copies the entries of a
pre-training checkpoint the model has and skips the rest (``out_lin.*``).

The encoder is ginet_molclr.GINet's, run as it runs there (the executor,
which draws the dropout masks of ``drop_ratio`` inside its kernels); everything
after the pooling -- feat_lin, the head and, through :meth:`GINet.loss`, the
criterion -- is ONE ops.task_head call (task_head.hip).
"""
from __future__ import annotations

from torch import nn

from . import ginet_molclr, ops
from .ginet_molclr import (GINEConv, num_atom_type, num_bond_direction,  # noqa: F401
                           num_bond_type, num_chirality_tag)

TASK_LOSS = {'classification': 'cross_entropy', 'regression': 'mse'}


def task_out_dim(task: str) -> int:
    if task not in TASK_LOSS:
        raise ValueError(f"task {task!r}: 'classification' or 'regression'")
    return 2 if task == 'classification' else 1


class FinetuneReadout:
    """Pooling + feat_lin + task head of both fine-tuning models (mixin over a
    pre-training encoder class)."""

    def _head_layers(self):
        raise NotImplementedError

    def _task(self, data, loss=None, target=None):
        return self._head(*self._embed(data), loss, target)

    def _head(self, h, graph, loss=None, target=None):
        h, W = self._pool(h, graph)
        lins, acts = self._head_layers()
        return ops.task_head(h, [W] + [m.weight for m in lins],
                             [self.feat_lin.bias] + [m.bias for m in lins], [None] + acts,
                             loss, target, graph.status)

    def forward(self, data):
        """``(h [B, feat_dim], pred [B, 2 | 1])``; pred stays differentiable, so
        a criterion applied to it in user code trains as in the reference."""
        h, pred, _ = self._task(data)
        return h, pred

    def loss(self, data, target, criterion=None):
        """``(h, pred, loss)`` with the criterion computed inside the head's
        launch: ``criterion`` 'cross_entropy' (int64 labels), 'mse' or 'l1'
        (float targets [B, 1]); default by task (cross-entropy / MSE)."""
        return self._task(data, criterion or TASK_LOSS[self.task], target)

    def loss_staged(self, graph, target, criterion=None):
        """:meth:`loss` over a staged graph (molclr_amd.graph_step.StagedPairGraph
        of one segment): the atoms are ``graph.x``, fixed-capacity buffers whose
        padding rows lie outside every molecule and carry no gradient -- the
        capturable form of the step (molclr_amd.finetune_step)."""
        if not self._executor_ok() or self._dim_pad():
            raise NotImplementedError("loss_staged needs the encoder executor at a width "
                                      "the kernels take unpadded")
        return self._head(self._run_encoder(graph.x, graph), graph,
                          criterion or TASK_LOSS[self.task], target)

    def load_my_state_dict(self, state_dict):
        """Copy every entry whose name the model has (a shape mismatch raises
        in copy_), skip the rest (ginet_finetune.py:149-157)."""
        own_state = self.state_dict()
        for name, param in state_dict.items():
            if name not in own_state:
                continue
            if isinstance(param, nn.parameter.Parameter):
                param = param.data
            own_state[name].copy_(param)

    def forward_pair(self, xi, xj):
        raise NotImplementedError("the fine-tuning models take one view (forward / loss)")

    forward_staged = forward_pair


class GINet(FinetuneReadout, ginet_molclr.GINet):
    """models/ginet_finetune.py:52-157."""

    def __init__(self, task='classification', num_layer=5, emb_dim=300, feat_dim=512,
                 drop_ratio=0, pool='mean', pred_n_layer=2, pred_act='softplus',
                 precision='fp32'):
        # The parent's __init__ is NOT called: it would create out_lin, whose
        # initialisation draws from the RNG between feat_lin and pred_head and
        # whose keys the fine-tuning state_dict must not have.
        nn.Module.__init__(self)
        self.precision = ginet_molclr.check_precision(precision)
        self.task = task
        out_dim = task_out_dim(task)
        self._init_encoder(num_layer, emb_dim, feat_dim, drop_ratio, pool)

        self.pred_n_layer = max(1, pred_n_layer)
        if pred_act == 'relu':
            act = lambda: nn.ReLU(inplace=True)  # noqa: E731
        elif pred_act == 'softplus':
            act = nn.Softplus
        else:
            raise ValueError('Undefined activation function')
        self.pred_act = pred_act
        pred_head = [nn.Linear(self.feat_dim, self.feat_dim // 2), act()]
        for _ in range(self.pred_n_layer - 1):
            pred_head.extend([nn.Linear(self.feat_dim // 2, self.feat_dim // 2), act()])
        pred_head.append(nn.Linear(self.feat_dim // 2, out_dim))
        self.pred_head = nn.Sequential(*pred_head)

    def _head_layers(self):
        lins = [m for m in self.pred_head if isinstance(m, nn.Linear)]
        return lins, [self.pred_act] * (len(lins) - 1) + [None]
