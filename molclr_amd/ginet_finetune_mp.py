"""GIN-E encoder + motif readout + task head — drop-in for
models/ginet_finetune_mp.py, the model the reference's finetune.py trains
when ``model_type`` is ``gin``.

Same class name, constructor arguments, parameter-creation order (hence the
same seeded initialisation) and ``state_dict`` keys as the reference
(models/ginet_finetune_mp.py:52-175): the atom embeddings,
``motif_embedding.weight`` [num_motifs, feat_dim], the GIN layers, the
BatchNorms and ``feat_lin``, then ``motif_lin.*`` (Xavier-uniform weight),
``motif_pool.gate_nn.0.*`` (PyG's GlobalAttention draws its gate Linear a
second time in ``reset_parameters``; restated) and ``pred_head.*``, whose
first Linear is ``2 * feat_dim -> feat_dim // 2``.

``forward(data, mol_idx, clique_idx)`` takes the reference's layout
(finetune.py:202-210): ``clique_idx`` [T] are the motif indices of the batch's
molecules, ``mol_idx`` [T + B] the molecule of each (ascending) followed by
``0 .. B - 1`` for the molecules' own rows.  After the segment pool:
``h = feat_lin(pooled)``, ``a = ops.motif_pool(h, motif_embedding, ...)``
(motif_pool.hip), ``hp = motif_lin(a)``, and ``cat(h, hp)`` through the
``pred_head`` chain with -- through :meth:`GINet.loss` -- the criterion in ONE
ops.task_head call.  Nothing synchronises with the host.
"""
from __future__ import annotations

import torch
from torch import nn

from . import ginet_molclr, ops
from .ginet_finetune import TASK_LOSS, FinetuneReadout, task_out_dim
from .ginet_molclr import (GINEConv, num_atom_type, num_bond_direction,  # noqa: F401
                           num_bond_type, num_chirality_tag)


class GlobalAttention(nn.Module):
    """The parameters of PyG's GlobalAttention(gate_nn) (``gate_nn.0.*``); the
    pool itself is ops.motif_pool."""

    def __init__(self, gate_nn):
        super().__init__()
        self.gate_nn = gate_nn
        self.nn = None
        self.reset_parameters()

    def reset_parameters(self):
        # torch_geometric.nn.inits.reset: every child that can, redraws itself
        for item in self.gate_nn.children():
            if hasattr(item, 'reset_parameters'):
                item.reset_parameters()


class GINet(FinetuneReadout, ginet_molclr.GINet):
    """models/ginet_finetune_mp.py:52-175."""

    def __init__(self, num_motifs, task='classification', num_layer=5, emb_dim=300, feat_dim=512,
                 drop_ratio=0, pool='mean', pred_n_layer=2, pred_act='softplus',
                 precision='fp32'):
        # as ginet_finetune.GINet: the parent's __init__ would create out_lin
        nn.Module.__init__(self)
        self.precision = ginet_molclr.check_precision(precision)
        self.num_motifs = num_motifs
        self.task = task
        out_dim = task_out_dim(task)
        self._init_encoder(num_layer, emb_dim, feat_dim, drop_ratio, pool)

        self.motif_lin = nn.Linear(self.feat_dim, self.feat_dim)
        nn.init.xavier_uniform_(self.motif_lin.weight.data)
        self.motif_pool = GlobalAttention(gate_nn=nn.Sequential(nn.Linear(feat_dim, 1)))

        self.pred_n_layer = max(1, pred_n_layer)
        if pred_act == 'relu':
            act = lambda: nn.ReLU(inplace=True)  # noqa: E731
        elif pred_act == 'softplus':
            act = nn.Softplus
        else:
            raise ValueError('Undefined activation function')
        self.pred_act = pred_act
        pred_head = [nn.Linear(2 * self.feat_dim, self.feat_dim // 2), act()]
        for _ in range(self.pred_n_layer - 1):
            pred_head.extend([nn.Linear(self.feat_dim // 2, self.feat_dim // 2), act()])
        pred_head.append(nn.Linear(self.feat_dim // 2, out_dim))
        self.pred_head = nn.Sequential(*pred_head)
        self._segment_values = {}

    def _init_after_atom_embeddings(self):
        # nn.Embedding's N(0, 1) draw, between the atom embeddings and the GIN layers
        self.motif_embedding = nn.Embedding(self.num_motifs, self.feat_dim)

    def init_motif_emb(self, init):
        """Set the motif table (finetune.py:161: the plain model's ``h`` of the
        vocabulary's graphs); the Parameter and its storage stay."""
        with torch.no_grad():
            self.motif_embedding.weight.copy_(init)

    def _head_layers(self):
        lins = [m for m in self.pred_head if isinstance(m, nn.Linear)]
        return lins, [self.pred_act] * (len(lins) - 1) + [None]

    def _mol_ptr(self, mol_idx, T, B):
        """int32 [B + 1] first item of every molecule from the ascending
        mol_idx[:T] (a mol_idx that does not ascend gives a pointer the pool
        flags in the status word)."""
        key = (B, mol_idx.device)
        values = self._segment_values.get(key)
        if values is None:
            values = self._segment_values[key] = torch.arange(B + 1, device=mol_idx.device)
        return torch.searchsorted(mol_idx[:T].contiguous(), values).to(torch.int32)

    def _motif_readout(self, h, graph, pool, loss=None, target=None):
        """Everything after the encoder: pooling + feat_lin, the attention pool
        ``pool(h)``, motif_lin and ``cat(h, hp)`` through the pred_head chain."""
        pooled, W = self._pool(h, graph)
        h = ops.task_head(pooled, [W], [self.feat_lin.bias], [None])[0]
        a = pool(h)
        hp = ops.task_head(a, [self.motif_lin.weight], [self.motif_lin.bias], [None])[0]
        x = torch.cat((h, hp), dim=1)
        lins, acts = self._head_layers()
        _, pred, loss = ops.task_head(x, [m.weight for m in lins], [m.bias for m in lins], acts,
                                      loss, target, graph.status)
        return x, pred, loss

    def _task(self, data, mol_idx, clique_idx, loss=None, target=None):
        h, graph = self._embed(data)
        B, T = graph.num_graphs, clique_idx.shape[0]
        if mol_idx.dim() != 1 or clique_idx.dim() != 1 or mol_idx.shape[0] != T + B:
            raise ValueError(f"mol_idx must be [T + B] = [{T} + {B}] and clique_idx [T]; got "
                             f"{tuple(mol_idx.shape)} and {tuple(clique_idx.shape)}")
        mol_idx = mol_idx.to(h.device, torch.long)
        clique_idx = clique_idx.to(h.device, torch.long)
        gate = self.motif_pool.gate_nn[0]

        def pool(hm):
            return ops.motif_pool(hm, self.motif_embedding.weight, clique_idx,
                                  self._mol_ptr(mol_idx, T, B), gate.weight, gate.bias,
                                  graph.status)
        return self._motif_readout(h, graph, pool, loss, target)

    def forward(self, data, mol_idx, clique_idx):
        """``(cat(h, hp) [B, 2 * feat_dim], pred [B, 2 | 1])``; pred stays
        differentiable for a criterion applied in user code."""
        x, pred, _ = self._task(data, mol_idx, clique_idx)
        return x, pred

    def loss(self, data, mol_idx, clique_idx, target, criterion=None):
        """``(cat(h, hp), pred, loss)`` with the criterion computed inside the
        head's launch, for both tasks (the reference's regression branch calls
        ``model(data)`` without the motif arguments and cannot run)."""
        return self._task(data, mol_idx, clique_idx, criterion or TASK_LOSS[self.task], target)

    def loss_staged(self, graph, target, criterion=None):
        """:meth:`loss` over a staged graph that also carries the batch's items
        (molclr_amd.finetune_step.StagedMotifGraph): ``graph.clique`` /
        ``mol_ptr`` / ``sorted_idx`` / ``order`` are buffers of a fixed item
        capacity, the item count stays on the device, and the pool is
        ops.motif_pool_staged -- no sort, no searchsorted and no shape that
        follows the batch, so the step can be captured."""
        if not self._executor_ok() or self._dim_pad():
            raise NotImplementedError("loss_staged needs the encoder executor at a width "
                                      "the kernels take unpadded")
        if getattr(graph, "clique", None) is None:
            raise NotImplementedError("the motif model has no staged form without the batch's "
                                      "items in the graph (finetune_step.StagedMotifGraph)")
        gate = self.motif_pool.gate_nn[0]

        def pool(hm):
            return ops.motif_pool_staged(hm, self.motif_embedding.weight, graph.clique,
                                         graph.mol_ptr, graph.sorted_idx, graph.order,
                                         gate.weight, gate.bias, graph.status)
        return self._motif_readout(self._run_encoder(graph.x, graph), graph, pool,
                                   criterion or TASK_LOSS[self.task], target)
