"""The device-sized motif pool (molclr_motif_pool_{fwd,bwd}_cap: an item
capacity in place of the item count, the count read on the device as
mol_ptr[B]) against the host-sized form on the same items -- exact equality of
a, alpha, dh, dE, dw and dc -- and the item staging (molclr_stage_motif).

Cases of tests/test_gpu_motif_pool.py: segments of 0, 1, 63..65 and 130 items
(above the kernels' 128-row LDS bound), a motif id shared by every molecule and
one that sits twice in a molecule, gates from -80 to +90."""
import pytest
import torch

from .test_gpu_motif_pool import NUM, USED, make_case

pytestmark = pytest.mark.gpu

UNUSED = USED + 20  # a valid id that no item of make_case uses
GUARD = 64


def pad_values():
    from molclr_amd import _lib
    return (_lib.MOTIF_PAD, 0, UNUSED)


def run_pool(case, dev, cap, pad, acc, dE0):
    """One forward and backward through the C entry points: the host-sized
    form (cap None) or the device-sized one with ``cap - T`` padding items of
    id ``pad``.  dE starts from dE0 with ``acc``, from NaN without (so every
    row must be written)."""
    from molclr_amd import _lib
    B, F = case["h"].shape
    T = case["idx"].shape[0]
    n = T if cap is None else cap
    clique = torch.cat([case["idx"], torch.full((n - T,), pad, dtype=torch.long)]).to(dev)
    sorted_idx, order = torch.sort(clique, stable=True)
    h, E, w, c, da = (case[k].to(dev).contiguous() for k in ("h", "E", "w", "c", "da"))
    ptr = case["ptr"].to(dev)
    a = torch.full((B, F), float("nan"), device=dev)
    alpha = torch.full((n + B,), float("nan"), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    st = _lib.stream_of(dev)
    sfx = "" if cap is None else "_cap"
    _lib.call("molclr_motif_pool_fwd" + sfx, h.data_ptr(), E.data_ptr(), clique.data_ptr(),
              ptr.data_ptr(), w.data_ptr(), c.data_ptr(), B, n, F, NUM, a.data_ptr(),
              alpha.data_ptr(), status.data_ptr(), st)
    dh = torch.full((B, F), float("nan"), device=dev)
    dE = dE0.to(dev).clone() if acc else torch.full((NUM, F), float("nan"), device=dev)
    dw = torch.full((F,), float("nan"), device=dev)
    dc = torch.full((1,), float("nan"), device=dev)
    query = "molclr_motif_pool_workspace_bytes" if cap is None else \
        "molclr_motif_pool_cap_workspace_bytes"
    ws_bytes = _lib.query(query, B, n, F)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    _lib.call("molclr_motif_pool_bwd" + sfx, da.data_ptr(), h.data_ptr(), E.data_ptr(),
              clique.data_ptr(), ptr.data_ptr(), sorted_idx.data_ptr(), order.data_ptr(),
              w.data_ptr(), a.data_ptr(), alpha.data_ptr(), B, n, F, NUM, dh.data_ptr(),
              dE.data_ptr(), dw.data_ptr(), dc.data_ptr(), acc, 0, 0, ws.data_ptr(), ws_bytes, st)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return {"a": a, "alpha_items": alpha[:T], "alpha_h": alpha[n:], "dh": dh, "dE": dE, "dw": dw,
            "dc": dc}


def caps_of(T):
    return (T, T + 1, (T + 255) // 256 * 256 + 512)


@pytest.mark.parametrize("B", (1, 5, 33))
@pytest.mark.parametrize("F", (6, 44, 128))
def test_device_sized_equals_host_sized(dev, F, B):
    case = make_case(F, B)
    T = case["idx"].shape[0]
    assert max(case["counts"]) == 130 or B == 5
    dE0 = torch.randn(NUM, F, generator=torch.Generator().manual_seed(4))
    for acc in (0, 1):
        host = run_pool(case, dev, None, 0, acc, dE0)
        assert all(torch.isfinite(v).all() for v in host.values())
        for cap in caps_of(T):
            for pad in pad_values():
                out = run_pool(case, dev, cap, pad, acc, dE0)
                for k in host:
                    assert torch.equal(out[k], host[k]), (k, acc, cap, pad)
                # a row that only padding names: 0, or unchanged when accumulating
                want = dE0[UNUSED].to(dev) if acc else torch.zeros(F, device=dev)
                assert torch.equal(out["dE"][UNUSED], want), (acc, cap, pad)


@pytest.mark.parametrize("F", (6, 128))
def test_no_items_with_a_capacity(dev, F):
    """T = 0, T_cap > 0: every molecule pools its own row, dE is 0."""
    B = 5
    case = make_case(F, B)
    case["idx"] = case["idx"][:0]
    case["ptr"] = torch.zeros(B + 1, dtype=torch.int32)
    dE0 = torch.randn(NUM, F, generator=torch.Generator().manual_seed(4))
    for acc in (0, 1):
        host = run_pool(case, dev, None, 0, acc, dE0)
        assert torch.equal(host["a"].cpu(), case["h"])
        for cap in (1, 256):
            for pad in pad_values():
                out = run_pool(case, dev, cap, pad, acc, dE0)
                for k in host:
                    assert torch.equal(out[k], host[k]), (k, acc, cap, pad)
                assert torch.equal(out["dE"].cpu(), dE0 if acc else torch.zeros(NUM, F))


def mol_idx_of(case):
    B = len(case["counts"])
    return torch.cat([torch.repeat_interleave(torch.arange(B), torch.tensor(case["counts"])),
                      torch.arange(B)])


def stage(dev, mol_idx, clique_idx, B, cap, T=None):
    """molclr_stage_motif into buffers with GUARD sentinel entries behind them;
    returns (clique, mol_ptr, sorted_idx, order, status, guards unchanged)."""
    from molclr_amd import _lib
    T = clique_idx.shape[0] if T is None else T
    mol_idx, clique_idx = mol_idx.to(dev), clique_idx.to(dev)
    bufs = [torch.full((cap + GUARD,), -7, dtype=torch.long, device=dev) for _ in range(3)]
    ptr = torch.full((B + 1 + GUARD,), -7, dtype=torch.int32, device=dev)
    status = torch.zeros(1 + GUARD, dtype=torch.int32, device=dev)
    _lib.call("molclr_stage_motif", mol_idx.data_ptr(), clique_idx.data_ptr(), T, B, cap,
              bufs[0].data_ptr(), ptr.data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
              status.data_ptr(), _lib.stream_of(dev))
    torch.cuda.synchronize()
    kept = all(bool((b[cap:] == -7).all()) for b in bufs) and bool((ptr[B + 1:] == -7).all()) \
        and bool((status[1:] == 0).all())
    return bufs[0][:cap], ptr[:B + 1], bufs[1][:cap], bufs[2][:cap], int(status[0]), kept


@pytest.mark.parametrize("B", (1, 5, 33))
def test_staging_equals_searchsorted_and_stable_sort(dev, B):
    from molclr_amd import _lib
    case = make_case(6, B)
    T = case["idx"].shape[0]
    mol_idx = mol_idx_of(case)
    for cap in caps_of(T):
        clique, ptr, sorted_idx, order, status, kept = stage(dev, mol_idx, case["idx"], B, cap)
        assert status == 0 and kept
        want = torch.cat([case["idx"], torch.full((cap - T,), _lib.MOTIF_PAD)]).to(dev)
        assert torch.equal(clique, want)
        assert torch.equal(ptr.cpu(), case["ptr"])
        assert torch.equal(ptr, torch.searchsorted(mol_idx[:T].to(dev).contiguous(),
                                                   torch.arange(B + 1, device=dev)).to(torch.int32))
        s, o = torch.sort(want, stable=True)
        assert torch.equal(sorted_idx, s) and torch.equal(order, o)
    # no items at all
    clique, ptr, sorted_idx, order, status, kept = stage(dev, torch.arange(B), case["idx"][:0], B,
                                                         256)
    assert status == 0 and kept and int(ptr.abs().sum()) == 0
    assert bool((clique == _lib.MOTIF_PAD).all()) and torch.equal(order.cpu(), torch.arange(256))


def test_staging_refusals(dev):
    from molclr_amd import _lib
    from molclr_amd.data import raise_for_status
    B = 5
    case = make_case(6, B)
    T = case["idx"].shape[0]
    mol_idx = mol_idx_of(case)

    def refused(out, bit, match):
        clique, ptr, sorted_idx, order, status, kept = out
        assert status == bit and kept
        assert bool((ptr == -1).all())  # the pool flags every molecule
        with pytest.raises(ValueError, match=match):
            raise_for_status(status)

    refused(stage(dev, mol_idx, case["idx"], B, T - 1), _lib.STATUS_ITEM_OVERFLOW, "capacity")
    refused(stage(dev, mol_idx, case["idx"], B, 0), _lib.STATUS_ITEM_OVERFLOW, "capacity")
    swapped = mol_idx.clone()
    swapped[3], swapped[70] = mol_idx[70], mol_idx[3]
    assert int(swapped[3]) > int(swapped[4])
    refused(stage(dev, swapped, case["idx"], B, T + 9), _lib.STATUS_ITEM_ORDER, "ascending")
    for pos, value in ((T - 1, B), (0, -1), (T + 2, B + 3)):
        bad = mol_idx.clone()
        bad[pos] = value
        refused(stage(dev, bad, case["idx"], B, T + 9), _lib.STATUS_ITEM_MOL, "mol_idx outside")


def run_staged(case, dev, cap, idx=None, status=None):
    """ops.motif_pool_staged over freshly staged items."""
    from molclr_amd import ops
    B = len(case["counts"])
    idx = case["idx"] if idx is None else idx
    clique, ptr, sorted_idx, order, st, kept = stage(dev, mol_idx_of(case), idx, B, cap)
    assert st == 0 and kept
    h, E, w, c = (case[k].to(dev).requires_grad_(True) for k in ("h", "E", "w", "c"))
    a = ops.motif_pool_staged(h, E, clique.contiguous(), ptr.contiguous(), sorted_idx.contiguous(),
                              order.contiguous(), w, c, status)
    a.backward(case["da"].to(dev))
    return {"a": a.detach(), "dh": h.grad, "dE": E.grad, "dw": w.grad, "dc": c.grad}


def test_staged_op_equals_motif_pool(dev):
    from .test_gpu_motif_pool import run_gpu
    case = make_case(44, 33)
    ref = run_gpu(case, dev)
    assert case["idx"].shape[0] < 1280
    out = run_staged(case, dev, 1280)
    for k in ref:
        assert torch.equal(out[k], ref[k]), k


@pytest.mark.parametrize("value", (-1, NUM))
def test_bad_motif_id_in_a_segment_sets_status(dev, value):
    from molclr_amd import _lib
    case = make_case(6, 5)
    idx = case["idx"].clone()
    idx[int(case["ptr"][2]) + 5] = value  # inside molecule 2
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = run_staged(case, dev, 512, idx=idx, status=status)
    assert int(status.item()) == _lib.STATUS_MOTIF_RANGE
    ok = [0, 1, 3, 4]
    assert torch.isnan(out["a"][2]).all() and torch.isfinite(out["a"][ok]).all()
    assert torch.isfinite(out["dh"][ok]).all()
    status.zero_()
    run_staged(case, dev, 512, status=status)
    assert int(status.item()) == 0


def test_staged_op_refuses_the_composed_switch(dev, monkeypatch):
    from molclr_amd import ops
    monkeypatch.setattr(ops, "MOTIF_POOL", False)
    with pytest.raises(NotImplementedError, match="MOLCLR_MOTIF_POOL"):
        run_staged(make_case(6, 5), dev, 512)
