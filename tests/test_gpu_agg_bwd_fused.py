"""GINE aggregation backward in one pass over g (molclr_gine_aggregate_bwd_impl,
impl = 1: k_gather_ecount) == the transposed gather followed by the edge-table
partials (impl = 0), bit for bit: dx, dE1 and dE2.

Shapes (fp32).  D = 300: a partition is band x 8 = 24 rows, so N = 113 has a
short last partition and N = 1113 many partitions; N = 1024 * 24 + 1 puts the
1024-partition cap on (25 rows per partition: a second, ragged trip of the row
loop, a last partition of two rows, and forty partitions past N that hold no
row at all).  D = 8, N = 5: one block, two column units, most threads idle.
Every graph of 13 rows or more holds a node of out-degree 6 (the CSC walk),
one of exactly 4 (the last slot) and an isolated one; `pad` rows follow the
last molecule with no edges and zero bond counts, as a captured step's
padding.  dx starts as NaN: a row the kernel left out would stay NaN.
"""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from molclr_amd import _lib
from molclr_amd.data import DeviceGraph

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _band(D):
    """molclr::make_band(D).band (common.h)."""
    d4 = D // 4
    band = max(256 // d4, 1)
    if band * d4 < 192 and (band + 1) * d4 <= 1024:
        band += 1
    while band * d4 > 1024:
        band -= 1
    return band


def _edges(n, seed):
    """Undirected bonds of n atoms in molecules of about 20: a hub of degree 6,
    a centre of degree exactly 4 and an isolated atom first (n >= 13), then
    random trees (an atom bonds to one of the three before it)."""
    g = torch.Generator().manual_seed(seed)
    pairs, batch = [], []
    if n >= 13:
        pairs += [(0, k) for k in range(1, 7)] + [(7, k) for k in range(8, 12)]
        batch += [0] * 7 + [1] * 5 + [2]
    mol, start = (batch[-1] + 1 if batch else 0), len(batch)
    back = torch.randint(1, 4, (n,), generator=g).tolist()
    for i in range(len(batch), n):
        if i - start >= 20:
            mol, start = mol + 1, i
        if i > start:
            pairs.append((max(start, i - back[i]), i))
        batch.append(mol)
    ei = [e for a, b in pairs for e in ((a, b), (b, a))]
    ei = torch.tensor(ei, dtype=torch.long).reshape(-1, 2).t().contiguous()
    E = ei.shape[1]
    ea = torch.stack([torch.randint(0, 4, (E,), generator=g),
                      torch.randint(0, 3, (E,), generator=g)], 1)
    return ei, ea, torch.tensor(batch, dtype=torch.long), mol + 1


_CASES = {}


def _case(n, pad, D, dev):
    """(graph tensors extended by `pad` padding rows, g), built once per shape."""
    key = (n, pad, D)
    if key not in _CASES:
        ei, ea, batch, G = _edges(n, 5 + n)
        gr = DeviceGraph.union([(ei.to(dev), ea.to(dev), batch.to(dev), n, G)])
        gr.check()
        deg = gr.nbr_t.view(-1, 4)[:, 0].to(torch.int64).bitwise_and(0xFFFFFFFF) >> 29
        if n >= 13:
            assert deg[0].item() == 7 and deg[7].item() == 4 and deg[12].item() == 0
        z = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)  # noqa: E731
        nbr_t = torch.cat([gr.nbr_t[:4 * n], z(4 * pad)])
        ecount = torch.cat([gr.ecount[:8 * n], z(8 * pad)])
        rowptr_t = torch.cat([gr.rowptr_t, gr.rowptr_t[-1:].expand(pad)]).contiguous()
        gen = torch.Generator().manual_seed(D + n)
        g = torch.randn(n + pad, D, generator=gen).to(dev)
        _CASES[key] = (rowptr_t, gr.col_t, nbr_t, ecount, g)
    return _CASES[key]


def _run(dev, case, D, impl, accumulate, tables=(True, True)):
    lib = _lib.load()
    rowptr_t, col_t, nbr_t, ecount, g = case
    N = g.shape[0]
    wsb = lib.molclr_gine_aggregate_bwd_workspace_bytes(N, D)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    dx = torch.full((N, D), float("nan"), device=dev)
    gen = torch.Generator().manual_seed(3)
    fill = (lambda r: torch.randn(r, D, generator=gen).to(dev)) if accumulate else \
        (lambda r: torch.full((r, D), float("nan"), device=dev))
    dE1, dE2 = fill(5), fill(3)
    assert lib.molclr_gine_aggregate_bwd_impl(
        g.data_ptr(), rowptr_t.data_ptr(), col_t.data_ptr(), nbr_t.data_ptr(), ecount.data_ptr(),
        dx.data_ptr(), dE1.data_ptr() if tables[0] else None,
        dE2.data_ptr() if tables[1] else None, N, D, accumulate, ws.data_ptr(), wsb,
        _lib.stream_of(dev), impl) == 0, _lib.last_error()
    torch.cuda.synchronize()
    return dx, dE1, dE2


RAGGED = 1024 * _band(300) * 8 + 1


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("D,n,pad", [(300, 113, 0), (300, 1100, 13), (8, 5, 0), (300, RAGGED, 0)])
def test_fused_matches_split(dev, D, n, pad, accumulate):
    lib = _lib.load()
    if D == 300:  # the plan this file's shapes are chosen for
        part = 8 * D * 8
        rows = _band(D) * 8
        assert rows == 24
        assert (lib.molclr_gine_aggregate_bwd_workspace_bytes(3 * rows, D) - 256) // part == 3
        assert (lib.molclr_gine_aggregate_bwd_workspace_bytes(3 * rows + 1, D) - 256) // part == 4
        assert (lib.molclr_gine_aggregate_bwd_workspace_bytes(RAGGED, D) - 256) // part == 1024
    case = _case(n, pad, D, dev)
    split = _run(dev, case, D, 0, accumulate)
    fused = _run(dev, case, D, 1, accumulate)
    for name, a, b in zip(("dx", "dE1", "dE2"), split, fused):
        assert not bool(torch.isnan(b).any()), name + ": left unwritten"
        assert torch.equal(a, b), name
    g = case[4]
    if pad:  # a padding row comes out as its own g row
        assert torch.equal(fused[0][n:], g[n:])
    if n >= 13:  # the isolated atom too; the hub is the sum of its six and itself
        assert torch.equal(fused[0][12], g[12])
        hub = torch.zeros(D, device=dev)
        for k in range(1, 7):
            hub = hub + g[k]
        assert torch.equal(fused[0][0], hub + g[0])


def test_default_routing_and_one_table(dev):
    """impl = -1 takes the fused kernel unless the environment turns it off
    (either way the same bits); one table gradient alone still fuses; dx alone
    and tables alone run the two kernels under every impl."""
    D = 300
    case = _case(1100, 13, D, dev)
    ref = _run(dev, case, D, 0, 1)
    for a, b in zip(ref, _run(dev, case, D, -1, 1)):
        assert torch.equal(a, b)
    for tables in ((True, False), (False, True), (False, False)):
        a, b = _run(dev, case, D, 0, 1, tables), _run(dev, case, D, 1, 1, tables)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        assert torch.equal(a[0], ref[0])
        for t in (0, 1):
            if tables[t]:
                assert torch.equal(a[1 + t], ref[1 + t])
    lib = _lib.load()
    assert lib.molclr_gine_aggregate_bwd_impl(None, None, None, None, None, None, None, None, 0, D,
                                              0, None, 0, _lib.stream_of(dev), 2) != 0


_CHILD = """
import sys, torch
from molclr_amd.dataset import SyntheticPairBatches
from molclr_amd.ginet_molclr import GINet
dev = torch.device("cuda", 0)
torch.manual_seed(1)
m = GINet(2, 300, 256).to(dev)
assert m._executor_ok()
xi, _ = SyntheticPairBatches(8, seed=2).next()
xi = xi.to(dev)
g = torch.randn(xi.x.shape[0], 300, generator=torch.Generator().manual_seed(4)).to(dev)
h, _ = m.encode(xi)
(h * g).sum().backward()
grads = [p.grad.reshape(-1) for _, p in sorted(m.named_parameters()) if p.grad is not None]
assert len(grads) == 2 + 8 * 2
flat = torch.cat(grads + [h.detach().reshape(-1)]).cpu()
assert bool(torch.isfinite(flat).all())
open(sys.argv[1], "wb").write(flat.numpy().tobytes())
"""


def test_executor_gradients_same_with_switch_off(dev, tmp_path):
    """The GIN encoder executor, forward and backward (L = 2, D = 300, B = 8),
    in two fresh processes (the switch is read once per process): the flat
    gradients are the same bytes with the fused kernel on and off."""
    outs = []
    for val in ("1", "0"):
        out = tmp_path / f"grads_{val}.bin"
        env = dict(os.environ, MOLCLR_AGG_BWD_FUSED=val)
        r = subprocess.run([sys.executable, "-c", _CHILD, str(out)], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs.append(out.read_bytes())
    assert len(outs[0]) > 4 * 300 * 300 and outs[0] == outs[1]
