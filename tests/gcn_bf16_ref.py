"""The oracle's GCN with the rounding points of the HIP bf16 storage path
(molclr_gcn_encoder with MOLCLR_DTYPE_BF16), for tests/test_gpu_gcn_bf16.py.

``EmuGCNConv`` is oracle.reference_cpu.RefGCNConv with the two tensors the
kernels store in bf16 -- xw = x W and the convolution's output z -- rounded
through ``_StoreBF16`` (value forward, gradient backward) and W taken as a bf16
GEMM operand through ``_OperandBF16``.  ``emu_gcn`` builds a RefGCN of such
layers with ``emulate_bf16 = True``: its forward is RefGINet.forward, which
then also rounds the atom embedding and every BatchNorm (+ReLU, dropout)
output, as the kernels' stores do.  Everything else (edge scalars, bias,
BatchNorm statistics, pooling, heads) stays in the module's dtype.
"""
from __future__ import annotations

import torch

from oracle.reference_cpu import (RefGCN, RefGCNConv, _OperandBF16, _StoreBF16, add_self_loops,
                                  propagate_add)


class EmuGCNConv(RefGCNConv):
    def forward(self, x, edge_index, edge_attr):  # RefGCNConv.forward with the stores
        st, op = _StoreBF16.apply, _OperandBF16.apply
        N = x.size(0)
        edge_index = add_self_loops(edge_index, N)
        self_loop_attr = torch.zeros(N, 2)
        self_loop_attr[:, 0] = 4
        self_loop_attr = self_loop_attr.to(edge_attr.device).to(edge_attr.dtype)
        edge_attr = torch.cat((edge_attr, self_loop_attr), dim=0)
        edge_embeddings = self.edge_embedding1(edge_attr[:, 0]) + self.edge_embedding2(edge_attr[:, 1])
        xw = st(x @ op(self.weight))
        out = propagate_add(xw, edge_index, N, lambda x_j: edge_embeddings + x_j)
        return st(out + self.bias)


def emu_gcn(base=RefGCN, *args, **kw):
    """``base(*args, **kw)`` (RefGCN or a subclass) with EmuGCNConv layers
    holding the same parameters, and ``emulate_bf16`` set."""
    model = base(*args, **kw)
    for l, conv in enumerate(model.gnns):
        emu = EmuGCNConv(conv.emb_dim, aggr=conv.aggr)
        emu.load_state_dict(conv.state_dict())
        model.gnns[l] = emu
    model.emulate_bf16 = True
    return model
