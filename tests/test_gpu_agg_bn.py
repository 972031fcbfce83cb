"""GINE aggregation with a BatchNorm source (molclr_gine_aggregate_bn_fwd[_bf16]
after molclr_batchnorm_seg_coeffs[_dev]) == the two existing calls
(molclr_batchnorm_seg_fwd[_dev], then molclr_gine_aggregate_fwd[_rowmax | _bf16]
on its stored output), bit for bit: the aggregation, its row maxima and max
slot, save_mean / save_invstd, the running statistics and num_batches_tracked.

Shapes: D = 300 (D/4 >= 64: per-wave-pair row maxima) and 16 (row parts) in
fp32; D = 64 (16-byte units) and 72 (float4 units) in bf16.  Segments of 37
and 90 rows put a segment boundary inside a wave; every segment holds a node
of degree 0, one of degree exactly 4 (the last slot) and one of degree 6 (the
CSR walk).  gamma has both signs, so the ReLU cuts on either side of the mean.
"""
import ctypes
from ctypes import c_void_p

import pytest
import torch

from molclr_amd import _lib, ops
from molclr_amd.data import DeviceGraph

pytestmark = pytest.mark.gpu

PAD = 21  # padding rows of the device-sized case


def _segment(n, seed):
    """(edge_index, edge_attr, batch, n, graphs) of n >= 15 nodes in 4 molecules:
    a hub of in-degree 6, a centre of in-degree exactly 4, an isolated atom and
    a chain."""
    pairs = [(0, k) for k in range(1, 7)] + [(7, k) for k in range(8, 12)]
    pairs += [(k, k + 1) for k in range(13, n - 1)]
    ei = []
    for a, b in pairs:
        ei += [(a, b), (b, a)]
    ei = torch.tensor(ei, dtype=torch.long).t().contiguous()
    g = torch.Generator().manual_seed(seed)
    E = ei.shape[1]
    ea = torch.stack([torch.randint(0, 4, (E,), generator=g),
                      torch.randint(0, 3, (E,), generator=g)], 1)
    batch = torch.tensor([0] * 7 + [1] * 5 + [2] + [3] * (n - 13), dtype=torch.long)
    return ei, ea, batch, n, 4


_GRAPHS = {}


def _graph(rows, dev):
    """The union graph of the segments (built once per segment split), with its
    neighbour slots and row pointers extended by PAD padding rows as
    molclr_graph_build_dev leaves them: no edges."""
    if rows not in _GRAPHS:
        parts = [tuple(t.to(dev) if torch.is_tensor(t) else t for t in _segment(n, 11 + s))
                 for s, n in enumerate(rows)]
        g = DeviceGraph.union(parts)
        g.check()
        deg = g.nbr.view(-1, 4)[:, 0].to(torch.int64).bitwise_and(0xFFFFFFFF) >> 29
        for s0 in torch.tensor((0,) + rows[:-1]).cumsum(0).tolist():
            assert deg[s0].item() == 7 and deg[s0 + 7].item() == 4 and deg[s0 + 12].item() == 0
        nbr = torch.cat([g.nbr, torch.zeros(4 * PAD, dtype=torch.int32, device=dev)])
        rowptr = torch.cat([g.rowptr, g.rowptr[-1:].expand(PAD)]).contiguous()
        _GRAPHS[rows] = (g, nbr, rowptr)
    return _GRAPHS[rows]


@pytest.mark.parametrize("mode", ["train", "eval", "dev"])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("rows", [(37, 90), (127,)])
@pytest.mark.parametrize("dtype,D", [("fp32", 300), ("fp32", 16), ("bf16", 64), ("bf16", 72)])
def test_aggregate_bn_source_matches_apply_then_gather(dev, dtype, D, rows, relu, mode):
    lib = _lib.load()
    st = _lib.stream_of(dev)
    g, nbr, rowptr = _graph(rows, dev)
    S, n = len(rows), sum(rows)
    on_dev = mode == "dev"
    cap = n + PAD if on_dev else n  # rows of every buffer
    training = 0 if mode == "eval" else 1
    bf = dtype == "bf16"
    tdt = torch.bfloat16 if bf else torch.float32
    dt = _lib.DTYPE_BF16 if bf else _lib.DTYPE_F32
    gen = torch.Generator().manual_seed(D + 7 * relu + n)
    z = (torch.randn(cap, D, generator=gen) * 2 + 0.5).to(dev).to(tdt)
    if on_dev:
        z[n:] = float("nan")  # padding rows are never read as values
    gamma, beta = torch.randn(D, generator=gen).to(dev), torch.randn(D, generator=gen).to(dev)
    assert bool((gamma < 0).any()) and bool((gamma > 0).any())
    E1, E2 = torch.randn(5, D, generator=gen).to(dev), torch.randn(3, D, generator=gen).to(dev)
    Ec = torch.empty(15, D, device=dev)
    arr = lambda t: (c_void_p * 1)(t.data_ptr())  # noqa: E731
    assert lib.molclr_edge_tables_combine(1, arr(E1), arr(E2), Ec.data_ptr(), D, st) == 0
    rm0, rv0 = torch.randn(D, generator=gen).to(dev), (torch.rand(D, generator=gen) + 0.5).to(dev)
    seg = (ctypes.c_int64 * S)(*rows)
    drows = torch.tensor(rows, dtype=torch.long, device=dev)
    wsb = (lib.molclr_batchnorm_seg_dev_workspace_bytes(S, cap, D) if on_dev
           else lib.molclr_batchnorm_seg_workspace_bytes(S, seg, D))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rowmax = not bf
    rmx_bytes = lib.molclr_rowmax_bytes(cap, D)
    graph = (rowptr.data_ptr(), g.col.data_ptr(), g.ecode.data_ptr(), nbr.data_ptr(), Ec.data_ptr())

    def run(fused):
        r = dict(rm=rm0.clone(), rv=rv0.clone(), nbt=torch.zeros(1, dtype=torch.long, device=dev),
                 sm=torch.full((S, D), 7.0, device=dev), si=torch.full((S, D), 7.0, device=dev),
                 agg=torch.full((cap, D), 7.0, device=dev).to(tdt))
        if rowmax:
            r["agg_rm"] = torch.full((cap, D), 7.0, device=dev)
            r["parts"] = torch.full((rmx_bytes // 4,), -1.0, device=dev)
            r["slot"] = torch.zeros(ops.MAX_SLOT, device=dev)
        stats = (z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), r["rm"].data_ptr(),
                 r["rv"].data_ptr(), r["nbt"].data_ptr())
        tail = (D, dt, 0.1, 1e-5, training)
        if fused:
            coef = torch.full((2, S, D), 7.0, device=dev)
            save = (r["sm"].data_ptr(), r["si"].data_ptr(), coef.data_ptr(), S)
            if on_dev:
                assert lib.molclr_batchnorm_seg_coeffs_dev(*stats, *save, drows.data_ptr(), cap,
                                                           *tail, ws.data_ptr(), wsb, st) == 0
            else:
                assert lib.molclr_batchnorm_seg_coeffs(*stats, *save, seg, *tail, ws.data_ptr(),
                                                       wsb, st) == 0
            ws.fill_(0x7F)  # the coefficients live in `coef`, not in the workspace
            src = (z.data_ptr(), coef.data_ptr(), relu, S, None if on_dev else seg,
                   drows.data_ptr() if on_dev else None)
            if bf:
                assert lib.molclr_gine_aggregate_bn_fwd_bf16(*src, *graph, r["agg"].data_ptr(),
                                                             cap, D, st) == 0
            else:
                assert lib.molclr_gine_aggregate_bn_fwd(*src, *graph, r["agg"].data_ptr(), cap, D,
                                                        None, None, st) == 0
                assert lib.molclr_gine_aggregate_bn_fwd(*src, *graph, r["agg_rm"].data_ptr(), cap,
                                                        D, r["parts"].data_ptr(),
                                                        r["slot"].data_ptr(), st) == 0
        else:
            y = torch.full((cap, D), 7.0, device=dev).to(tdt)
            save = (y.data_ptr(), r["sm"].data_ptr(), r["si"].data_ptr(), S)
            if on_dev:
                assert lib.molclr_batchnorm_seg_fwd_dev(*stats, *save, drows.data_ptr(), cap, *tail,
                                                        relu, ws.data_ptr(), wsb, st) == 0
            else:
                assert lib.molclr_batchnorm_seg_fwd(*stats, *save, seg, *tail, relu, ws.data_ptr(),
                                                    wsb, st) == 0
            if bf:
                assert lib.molclr_gine_aggregate_fwd_bf16(y.data_ptr(), *graph, r["agg"].data_ptr(),
                                                          cap, D, st) == 0
            else:
                assert lib.molclr_gine_aggregate_fwd(y.data_ptr(), *graph, r["agg"].data_ptr(), cap,
                                                     D, st) == 0
                assert lib.molclr_gine_aggregate_fwd_rowmax(y.data_ptr(), *graph,
                                                            r["agg_rm"].data_ptr(), cap, D,
                                                            r["parts"].data_ptr(),
                                                            r["slot"].data_ptr(), st) == 0
        torch.cuda.synchronize()
        return r

    ref, got = run(False), run(True)
    assert not bool(torch.isnan(ref["agg"].float()).any())
    assert bool((ref["agg"].float() != 7.0).any())
    for k in ref:
        assert torch.equal(ref[k], got[k]), k
    assert int(ref["nbt"]) == (S if training else 0)
    if rowmax:
        assert torch.equal(got["agg_rm"], got["agg"])
        assert bool((got["parts"] >= 0).all()), "a row-max entry was left unwritten"
        assert got["slot"].max().item() == got["agg"].abs().max().item()
