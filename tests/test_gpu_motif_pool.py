"""ops.motif_pool (motif_pool.hip) against PyG's GlobalAttention restated in
fp64 on the CPU (tests/motif_ref.pool_ref), at the project's bound:
forward 1e-5 norm-wise; each gradient max(1e-5 ||g64||, 2 err32) with err32
the error of the same restatement run in fp32 on the CPU; dc, exactly 0
mathematically, 2 err32 + 1e-6 sum |dgate|."""
import pytest
import torch

from .motif_ref import pool_ref

pytestmark = pytest.mark.gpu

NUM, USED = 200, 150  # rows of E; rows USED.. are never indexed
SHARED, TWICE = 7, 11  # motif 7 opens every non-empty molecule; 11 sits twice in one
EXTREME = (140, 141, 142)  # rows whose gates are about +90, +90 and -80
COUNTS = {1: [130], 5: [0, 1, 63, 64, 65], 33: [0, 1, 63, 64, 65, 130, 3, 8, 4, 2, 9]}


def make_case(F, B, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * F + B)
    counts = [COUNTS[B][b % len(COUNTS[B])] for b in range(B)]
    ptr = torch.tensor([0] + counts).cumsum(0)
    idx = torch.randint(0, EXTREME[0], (int(ptr[-1]),), generator=g)
    for b, n in enumerate(counts):
        p = int(ptr[b])
        if n >= 1:
            idx[p] = SHARED
        if n >= 4:
            idx[p + 2] = idx[p + 3] = TWICE
    w = torch.randn(F, generator=g) / F ** 0.5
    E = torch.randn(NUM, F, generator=g)
    # the longest segment holds gates from -80 to +90 (HIGH twice over, so two rows
    # share the weight): exp overflows there without the max subtraction
    # (not in the one-molecule batches: its h row's weight is e^-90 there, and the
    # whole of dh would be fp32 subnormals, which hold no relative precision)
    last = max(range(B), key=lambda b: counts[b])
    if B > 1:
        for m, gate in zip(EXTREME, (90.0, 90.0, -80.0)):
            E[m] += w * ((gate - E[m].dot(w)) / w.dot(w))
            E[m] += 0.3 * torch.randn(F, generator=g)
        idx[int(ptr[last]) + 5:int(ptr[last]) + 8] = torch.tensor(EXTREME)
    return {"h": torch.randn(B, F, generator=g), "E": E, "idx": idx, "ptr": ptr.to(torch.int32),
            "w": w.reshape(1, F), "c": torch.randn(1, generator=g),
            "da": torch.randn(B, F, generator=g), "counts": counts}


_REF = {}


def refs(F, B):
    """(fp64 result, fp32 result) of the restatement, computed once per case."""
    if (F, B) not in _REF:
        c = make_case(F, B)
        args = (c["h"], c["E"], c["idx"], c["ptr"], c["w"], c["c"], c["da"])
        _REF[(F, B)] = (pool_ref(*args, torch.float64), pool_ref(*args, torch.float32))
    return _REF[(F, B)]


def run_gpu(case, dev, params=None, status=None, idx=None, ptr=None):
    from molclr_amd import ops
    h = case["h"].to(dev).requires_grad_(True)
    E, w, c = params or [case[k].to(dev).requires_grad_(True) for k in ("E", "w", "c")]
    a = ops.motif_pool(h, E, (case["idx"] if idx is None else idx).to(dev),
                       (case["ptr"] if ptr is None else ptr).to(dev), w, c, status)
    a.backward(case["da"].to(dev))
    return {"a": a.detach(), "dh": h.grad, "dE": E.grad, "dw": w.grad, "dc": c.grad}


def check(out, r64, r32, what):
    def err(a, b):
        return (a.detach().double().cpu().reshape(-1) - b.double().reshape(-1)).norm().item()

    bad = {}
    e = err(out["a"], r64["a"])
    print(what, "a", e / r64["a"].norm().item())
    if e > 1e-5 * r64["a"].norm().item():
        bad["a"] = e / r64["a"].norm().item()
    for k in ("dh", "dE", "dw"):
        e, e32, n = err(out[k], r64[k]), err(r32[k], r64[k]), r64[k].norm().item()
        print(what, k, e / n, "err32", e32 / n)
        if e > max(1e-5 * n, 2 * e32):
            bad[k] = (e / n, e32 / n)
    e, e32 = err(out["dc"], r64["dc"]), err(r32["dc"], r64["dc"])
    print(what, "dc", e, "err32", e32, "sum|dgate|", r64["absdgate"])
    if e > 2 * e32 + 1e-6 * r64["absdgate"]:
        bad["dc"] = (e, e32)
    assert not bad, (what, bad)


@pytest.mark.parametrize("B", (1, 5, 33))
@pytest.mark.parametrize("F", (4, 6, 44, 512))
def test_motif_pool_matches_fp64(dev, F, B):
    case = make_case(F, B)
    r64, r32 = refs(F, B)
    out = run_gpu(case, dev)
    check(out, r64, r32, f"F{F} B{B}")
    # rows of E that no item uses: exactly zero
    assert (out["dE"][USED:] == 0).all()
    used = torch.zeros(NUM, dtype=torch.bool)
    used[case["idx"]] = True
    assert (out["dE"].cpu()[~used] == 0).all()


def test_a_molecule_without_motifs_pools_its_own_row(dev):
    case = make_case(44, 5)
    out = run_gpu(case, dev)
    assert case["counts"][0] == 0 and torch.equal(out["a"][0].cpu(), case["h"][0])


@pytest.mark.parametrize("F,B", [(6, 5), (512, 33)])
def test_bit_identical_from_run_to_run(dev, F, B):
    case = make_case(F, B)
    a, b = run_gpu(case, dev), run_gpu(case, dev)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_accumulate_into_fused_adam_grads(dev):
    """E, the gate weight and bias owned by a FusedAdam: the kernels add into
    the flat gradient buffer; two passes leave exactly twice one pass."""
    from molclr_amd.optim import FusedAdam
    case = make_case(44, 33)
    params = [torch.nn.Parameter(case[k].to(dev)) for k in ("E", "w", "c")]
    opt = FusedAdam(params, 1e-3)
    opt.zero_grad()
    run_gpu(case, dev, params=params)
    once = opt.flat_grad.clone()
    assert once.abs().sum().item() > 0
    free = run_gpu(case, dev)
    for p, k in zip(params, ("dE", "dw", "dc")):
        assert torch.equal(p.grad, free[k]), k
    run_gpu(case, dev, params=params)
    eps = 2.0 ** -24
    assert ((opt.flat_grad - 2 * once).abs() <= eps * (2 * once).abs()).all()


@pytest.mark.parametrize("value", (-1, NUM))
def test_motif_out_of_range_sets_status(dev, value):
    from molclr_amd import _lib
    from molclr_amd.data import raise_for_status
    case = make_case(6, 5)
    idx = case["idx"].clone()
    idx[int(case["ptr"][2]) + 5] = value  # inside molecule 2
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = run_gpu(case, dev, status=status, idx=idx)
    assert int(status.item()) == _lib.STATUS_MOTIF_RANGE == 32
    with pytest.raises(ValueError, match="motif index"):
        raise_for_status(int(status.item()))
    ok = [0, 1, 3, 4]
    assert torch.isnan(out["a"][2]).all() and torch.isfinite(out["a"][ok]).all()
    assert torch.isfinite(out["dh"][ok]).all()
    status.zero_()
    run_gpu(case, dev, status=status)
    assert int(status.item()) == 0


def test_non_monotone_mol_ptr_sets_status(dev):
    from molclr_amd import _lib
    case = make_case(6, 5)
    ptr = case["ptr"].clone()
    ptr[2], ptr[3] = case["ptr"][3], case["ptr"][2]  # segment 2 runs backwards
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = run_gpu(case, dev, status=status, ptr=ptr)
    assert int(status.item()) == _lib.STATUS_MOTIF_RANGE
    assert torch.isnan(out["a"][2]).all() and torch.isfinite(out["a"][[0, 4]]).all()


def test_argument_errors(dev):
    from molclr_amd import ops
    c = make_case(6, 5)
    h, E, idx, ptr, w, b = (c[k].to(dev) for k in ("h", "E", "idx", "ptr", "w", "c"))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.motif_pool(h, E, idx.cpu(), ptr, w, b)
    with pytest.raises(ValueError, match="mol_ptr"):
        ops.motif_pool(h, E, idx, ptr[:-1], w, b)
    with pytest.raises(ValueError, match="clique_idx"):
        ops.motif_pool(h, E, idx.to(torch.int32), ptr, w, b)
    with pytest.raises(ValueError):
        ops.motif_pool(h, E[:, :4], idx, ptr, w, b)


@pytest.mark.parametrize("F,B", [(6, 5), (44, 1), (512, 33)])
def test_composed_path_within_the_same_bound(dev, F, B, monkeypatch):
    from molclr_amd import _lib, ops
    monkeypatch.setattr(ops, "MOTIF_POOL", False)
    case = make_case(F, B)
    check(run_gpu(case, dev), *refs(F, B), f"composed F{F} B{B}")
    idx = case["idx"].clone()
    idx[0] = NUM  # the first item: of the first molecule that has one
    first = next(b for b, n in enumerate(case["counts"]) if n)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = run_gpu(case, dev, status=status, idx=idx)
    assert int(status.item()) == _lib.STATUS_MOTIF_RANGE
    nan_rows = torch.isnan(out["a"]).all(1).cpu()
    assert nan_rows.tolist() == [b == first for b in range(B)]
