"""Restatements the motif-model tests compare against (no product code):

* ``MotifGINetLayout``: models/ginet_finetune_mp.py:62-135's modules in the
  reference's creation order with its initialisation calls, PyG 1.6.3's
  GlobalAttention.__init__ -> reset_parameters() (the gate Linear is drawn
  twice) included;
* ``pool_ref``: PyG 1.6.3's GlobalAttention(gate_nn=Linear(F, 1)) forward --
  softmax(src, index) = exp(src - scatter_max[index]) / (scatter_add[index] +
  1e-16), then scatter_add(gate * x) -- on the CPU in a chosen dtype, with the
  rows in the reference's order cat(motif rows, h rows), and its gradients;
* ``RefMotifGINet``: the oracle's GIN encoder with that readout;
* ``reference_motif_batch``: the loop of finetune.py:202-210, literally.
"""
import torch
import torch.nn.functional as F
from torch import nn

from oracle.reference_cpu import (RefGINet, num_atom_type, num_bond_direction, num_bond_type,
                                  num_chirality_tag)


class _GINEConvLayout(nn.Module):
    def __init__(self, emb_dim):  # ginet_finetune_mp.py:17-28
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(emb_dim, 2 * emb_dim), nn.ReLU(),
                                 nn.Linear(2 * emb_dim, emb_dim))
        self.edge_embedding1 = nn.Embedding(num_bond_type, emb_dim)
        self.edge_embedding2 = nn.Embedding(num_bond_direction, emb_dim)
        nn.init.xavier_uniform_(self.edge_embedding1.weight.data)
        nn.init.xavier_uniform_(self.edge_embedding2.weight.data)


class _GlobalAttentionLayout(nn.Module):
    def __init__(self, gate_nn):  # torch_geometric/nn/glob/attention.py (1.6.3)
        super().__init__()
        self.gate_nn = gate_nn
        for item in self.gate_nn.children():  # reset_parameters() -> inits.reset
            item.reset_parameters()


def _head(feat_in, feat_dim, out_dim, pred_n_layer, pred_act):
    act = {"relu": lambda: nn.ReLU(inplace=True), "softplus": nn.Softplus}[pred_act]
    head = [nn.Linear(feat_in, feat_dim // 2), act()]
    for _ in range(max(1, pred_n_layer) - 1):
        head += [nn.Linear(feat_dim // 2, feat_dim // 2), act()]
    head.append(nn.Linear(feat_dim // 2, out_dim))
    return nn.Sequential(*head)


class MotifGINetLayout(nn.Module):
    def __init__(self, num_motifs, task="classification", num_layer=5, emb_dim=300, feat_dim=512,
                 pred_n_layer=2, pred_act="softplus"):
        super().__init__()
        self.x_embedding1 = nn.Embedding(num_atom_type, emb_dim)
        self.x_embedding2 = nn.Embedding(num_chirality_tag, emb_dim)
        nn.init.xavier_uniform_(self.x_embedding1.weight.data)
        nn.init.xavier_uniform_(self.x_embedding2.weight.data)
        self.motif_embedding = nn.Embedding(num_motifs, feat_dim)
        self.gnns = nn.ModuleList([_GINEConvLayout(emb_dim) for _ in range(num_layer)])
        self.batch_norms = nn.ModuleList([nn.BatchNorm1d(emb_dim) for _ in range(num_layer)])
        self.feat_lin = nn.Linear(emb_dim, feat_dim)
        self.motif_lin = nn.Linear(feat_dim, feat_dim)
        nn.init.xavier_uniform_(self.motif_lin.weight.data)
        self.motif_pool = _GlobalAttentionLayout(nn.Sequential(nn.Linear(feat_dim, 1)))
        self.pred_head = _head(2 * feat_dim, feat_dim, 2 if task == "classification" else 1,
                               pred_n_layer, pred_act)


def global_attention(x, index, size, w, c):
    """PyG 1.6.3 GlobalAttention.forward with nn=None; ``(out, gate logits)``."""
    g = x @ w.reshape(-1) + c.reshape(())
    m = torch.full((size,), float("-inf"), dtype=x.dtype).scatter_reduce(
        0, index, g, "amax", include_self=True)
    e = (g - m[index]).exp()
    s = torch.zeros(size, dtype=x.dtype).index_add(0, index, e)  # scatter_add: row order
    gate = e / (s[index] + 1e-16)
    return torch.zeros(size, x.shape[1], dtype=x.dtype).index_add(0, index, gate[:, None] * x), g


def segments_of(ptr):
    """item -> molecule for mol_ptr [B + 1]."""
    ptr = torch.as_tensor(ptr, dtype=torch.long)
    return torch.repeat_interleave(torch.arange(len(ptr) - 1), ptr[1:] - ptr[:-1])


def pool_ref(h, E, idx, ptr, w, c, da, dtype):
    """a and the gradients (dh, dE, dw, dc) of sum(a * da), on the CPU in
    ``dtype``; ``absdgate`` = sum |d/dgate| (dc is its signed sum: exactly 0)."""
    h, E, w, c = (t.detach().to(dtype).clone().requires_grad_(True) for t in (h, E, w, c))
    B = h.shape[0]
    index = torch.cat([segments_of(ptr), torch.arange(B)])
    x = torch.cat([E[idx], h], 0)
    a, g = global_attention(x, index, B, w, c)
    g.retain_grad()
    a.backward(da.to(dtype))
    return {"a": a.detach(), "dh": h.grad, "dE": E.grad, "dw": w.grad, "dc": c.grad,
            "absdgate": g.grad.abs().sum().item()}


class RefMotifGINet(RefGINet):
    """The oracle's encoder and feat_lin with ginet_finetune_mp.py:137-165's
    readout, under the product's parameter names."""

    def __init__(self, num_motifs, task, num_layer, emb_dim, feat_dim, pred_n_layer=2,
                 pred_act="softplus"):
        super().__init__(num_layer, emb_dim, feat_dim)
        del self.out_lin
        self.motif_embedding = nn.Embedding(num_motifs, feat_dim)
        self.motif_lin = nn.Linear(feat_dim, feat_dim)
        self.motif_pool = _GlobalAttentionLayout(nn.Sequential(nn.Linear(feat_dim, 1)))
        self.pred_head = _head(2 * feat_dim, feat_dim, 2 if task == "classification" else 1,
                               pred_n_layer, pred_act)

    def forward(self, data, mol_idx, clique_idx):
        h = self.x_embedding1(data.x[:, 0]) + self.x_embedding2(data.x[:, 1])
        for l in range(self.num_layer):
            h = self.batch_norms[l](self.gnns[l](h, data.edge_index, data.edge_attr))
            if l != self.num_layer - 1:
                h = F.relu(h)
        h = self.feat_lin(self.pool(h, data.batch))
        hp = torch.cat((self.motif_embedding(clique_idx), h), dim=0)
        gate = self.motif_pool.gate_nn[0]
        hp, g = global_attention(hp, mol_idx, h.shape[0], gate.weight, gate.bias)
        if g.requires_grad:  # d loss / d gate logits: their signed sum is the bias gradient
            g.retain_grad()
            self.gate_logits = g
        hp = self.motif_lin(hp)
        h = torch.cat((h, hp), dim=1)
        return h, self.pred_head(h)


def reference_motif_batch(mol_indices, mol_to_clique, clique_list):
    """finetune.py:202-210 over a batch's dataset indices."""
    mol_idx, clique_idx = [], []
    for i, d in enumerate(mol_indices):
        for clique in mol_to_clique[d].keys():
            mol_idx.append(i)
            clique_idx.append(clique_list.index(clique))
    mol_idx.extend([i for i in range(max(mol_idx) + 1)])
    return torch.tensor(mol_idx), torch.tensor(clique_idx)
