"""ops.topk_dot (molclr_topk_dot) on the device: exact integer cases against
the int64 numpy reference, random unit rows against fp64 scores with the
derived dot-product bound, the shard identity that pins the summation order,
run-to-run bits and graph capture."""
import numpy as np
import pytest
import torch

from .retrieval_ref import int_case, topk_ref, unit_rows
from .rounding import rne_bf16

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
NS = (0, 1, 9, 10, 257, 5000)
NQS = (1, 5, 33)
KS = (1, 10, 64)


def _dev(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dev).to(dtype)


def _same(got, want_s, want_i, what):
    s, i = got
    assert s.dtype == torch.float32 and i.dtype == torch.int64
    s, i = s.cpu().numpy().astype(np.float64), i.cpu().numpy()
    assert np.array_equal(i, want_i), (what, i, want_i)
    assert np.array_equal(s, want_s), (what, s, want_s)


@pytest.fixture(scope="module")
def int_cases():
    """One integer case per C at the largest nq and n; smaller ones are slices."""
    return {C: int_case(max(NQS), max(NS), C, seed=C) for C in (4, 44, 512)}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [4, 44, 512])
def test_exact_integer_cases(dev, int_cases, C, dtype):
    from molclr_amd import ops
    q, db, s = int_cases[C]
    qd, dbd = _dev(q, dev), _dev(db, dev, dtype)
    for n in NS:
        for nq in NQS:
            for k in KS:
                want = topk_ref(s[:nq, :n], k)
                _same(ops.topk_dot(qd[:nq], dbd[:n], k), *want, what=(C, n, nq, k))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_strides_offsets_and_exclusions(dev, int_cases, dtype):
    from molclr_amd import ops
    q, db, s = int_cases[44]
    nq, n = 5, 257
    # ldq > C and lddb > C: column slices of wider buffers
    qw = torch.full((nq, 64), 7.0, device=dev)
    dbw = torch.full((n, 56), 7.0, device=dev).to(dtype)
    qw[:, 8:52] = _dev(q[:nq], dev)
    dbw[:, 8:52] = _dev(db[:n], dev, dtype)
    qs, dbs = qw[:, 8:52], dbw[:, 8:52]
    assert qs.stride(0) == 64 and dbs.stride(0) == 56
    _same(ops.topk_dot(qs, dbs, 10), *topk_ref(s[:nq, :n], 10), what="strided")
    # idx_base beyond 2^32 and an exclude that names every query's best row
    base = 10 ** 10
    _, top = topk_ref(s[:nq, :n], 1)
    ex = top[:, 0] + base
    want = topk_ref(s[:nq, :n], 10, exclude=ex, idx_base=base)
    assert (want[1] != ex[:, None]).all()
    got = ops.topk_dot(_dev(q[:nq], dev), _dev(db[:n], dev, dtype), 10,
                       exclude=torch.from_numpy(ex).to(dev), idx_base=base)
    _same(got, *want, what="idx_base / exclude")
    # exclude on n == k: exactly one -inf / -1 entry per row
    k = 10
    ex = np.arange(nq, dtype=np.int64)
    want = topk_ref(s[:nq, :k], k, exclude=ex)
    assert (want[1] == -1).sum(1).tolist() == [1] * nq and np.isneginf(want[0][:, -1]).all()
    got = ops.topk_dot(_dev(q[:nq], dev), _dev(db[:k], dev, dtype), k,
                       exclude=torch.from_numpy(ex).to(dev))
    _same(got, *want, what="n == k with exclude")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_zero_signs_and_nan_rows(dev, dtype):
    from molclr_amd import ops
    C, n = 8, 40
    rng = np.random.default_rng(5)
    db = rng.integers(-2, 3, size=(n, C)).astype(np.float64)
    db[7] = 0.0                    # an all-zero row: +0.0 or -0.0 by the query's signs
    db[[3, 30]] = np.nan           # NaN rows rank last
    q = rng.integers(-2, 3, size=(3, C)).astype(np.float64)
    q[0] = -np.abs(q[0]) - 1       # all negative: the zero row's products are all -0.0
    q[1, ::2] = -1.0               # mixed signs
    q[1, 1::2] = 1.0
    with np.errstate(invalid="ignore"):
        s = q @ db.T
    dbz = db.copy()
    dbz[7, ::3] = -0.0             # and signed zeros in the row itself
    for k in (10, n):
        want_s, want_i = topk_ref(s, k)
        got_s, got_i = ops.topk_dot(_dev(q, dev), _dev(dbz, dev, dtype), k)
        _same((got_s, got_i), want_s, want_i, what=("zeros / NaN", k))
        assert not torch.signbit(got_s[got_i == 7]).any()  # the zero row scores +0.0
    assert want_i[:, -2:].tolist() == [[3, 30]] * 3 and np.isneginf(want_s[:, -2:]).all()


RANDOM_SHAPES = [(1, 1000, 512, 10), (17, 4097, 256, 64), (33, 5000, 44, 10)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_unit_rows_against_fp64(dev, shape, dtype):
    """tol = 2 C 2^-24: the dot-product bound gamma_C |q| |d| for unit vectors,
    with a factor 2 for the rows' own normalisation (derived, not measured).
    (a) every returned score is within tol of the fp64 score of its row; (b)
    rows sorted by the kernel's own (-score, idx), indices distinct, in range,
    the excluded row absent; (c) every row NOT returned has an fp64 score of
    at most the k-th returned one's + 2 tol."""
    from molclr_amd import ops
    nq, n, C, k = shape
    q, db = unit_rows(nq, C, seed=nq), unit_rows(n, C, seed=n)
    dbd = torch.from_numpy(db).to(dev).to(dtype)
    db64 = db.astype(np.float64)
    if dtype == torch.bfloat16:  # the fp64 scores of the bf16-rounded rows
        db64 = rne_bf16(torch.from_numpy(db64)).numpy()
        assert np.array_equal(dbd.float().cpu().numpy().astype(np.float64), db64)
    s64 = q.astype(np.float64) @ db64.T
    tol = 2 * C * 2.0 ** -24
    ex = np.argmax(s64, 1).astype(np.int64)  # leave every query's best row out
    gs, gi = ops.topk_dot(torch.from_numpy(q).to(dev), dbd, k,
                          exclude=torch.from_numpy(ex).to(dev))
    gs, gi = gs.cpu().numpy().astype(np.float64), gi.cpu().numpy()
    assert ((gi >= 0) & (gi < n)).all()
    ref = np.take_along_axis(s64, gi, 1)
    err = np.abs(gs - ref).max()
    print(f"shape {shape} {dtype}: max |score - s64| {err:.3e}, tol {tol:.3e}")
    assert err <= tol                                                   # (a)
    for i in range(nq):
        assert len(set(gi[i].tolist())) == k and ex[i] not in gi[i]     # (b)
        order = np.lexsort((gi[i], -gs[i]))
        assert np.array_equal(order, np.arange(k)), (i, gs[i], gi[i])
        rest = np.ones(n, dtype=bool)
        rest[gi[i]] = False
        rest[ex[i]] = False
        over = s64[i, rest].max() - ref[i, k - 1]
        assert over <= 2 * tol, (i, over)                               # (c)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_shard_identity(dev, dtype):
    """The top-k of the whole database equals, bit for bit, merge_topk of the
    top-k of db[:m] and db[m:] (idx_base = m): the summation order of a pair
    does not depend on its position, and the total order is the kernel's."""
    from molclr_amd import ops
    from molclr_amd.retrieval import merge_topk
    n, m, k, C = 5000, 1234, 10, 256
    q = torch.from_numpy(unit_rows(33, C, seed=1)).to(dev)
    db = torch.from_numpy(unit_rows(n, C, seed=2)).to(dev).to(dtype)
    ws, wi = ops.topk_dot(q, db, k)
    ms, mi = merge_topk([ops.topk_dot(q, db[:m], k), ops.topk_dot(q, db[m:], k, idx_base=m)])
    assert torch.equal(wi, mi) and torch.equal(ws.view(torch.int32), ms.view(torch.int32))
    # a query's result does not depend on its block: 40 queries at once
    # against 7 + 33 of them (the integer case: ties everywhere)
    qi, dbi, _ = int_case(40, 5000, 44, seed=9)
    qd, dbd = _dev(qi, dev), _dev(dbi, dev, dtype)
    ws, wi = ops.topk_dot(qd, dbd, k)
    for lo, hi in ((0, 7), (7, 40)):
        ps, pi = ops.topk_dot(qd[lo:hi], dbd, k)
        assert torch.equal(wi[lo:hi], pi) and torch.equal(ws[lo:hi], ps)
    # and the integer case through the shards
    ms, mi = merge_topk([ops.topk_dot(qd, dbd[:m], k), ops.topk_dot(qd, dbd[m:], k, idx_base=m)])
    assert torch.equal(wi, mi) and torch.equal(ws, ms)


def test_run_to_run_bits(dev):
    from molclr_amd import ops
    q = torch.from_numpy(unit_rows(33, 256, seed=3)).to(dev)
    db = torch.from_numpy(unit_rows(5000, 256, seed=4)).to(dev)
    a, b = ops.topk_dot(q, db, 64), ops.topk_dot(q, db, 64)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def test_refusals_on_the_device(dev):
    from molclr_amd import ops
    q, db = torch.zeros(2, 8, device=dev), torch.zeros(5, 8, device=dev)
    with pytest.raises(TypeError):
        ops.topk_dot(q.double(), db, 3)
    with pytest.raises(TypeError):
        ops.topk_dot(q, db.half(), 3)
    with pytest.raises(RuntimeError):
        ops.topk_dot(q, db, 65)
    with pytest.raises(ValueError):
        ops.topk_dot(q, db[:, :4], 3)
    s, i = ops.topk_dot(q[:0], db, 3)
    assert s.shape == (0, 3) and i.shape == (0, 3)


def test_capture_and_replay(dev):
    """One captured call, replayed on new contents of the same buffers."""
    from molclr_amd import ops
    nq, n, C, k = 5, 1000, 64, 10
    q = torch.from_numpy(unit_rows(nq, C, seed=5)).to(dev)
    db = torch.from_numpy(unit_rows(n, C, seed=6)).to(dev)
    ex = torch.arange(nq, device=dev)
    ops.topk_dot(q, db, k, exclude=ex)  # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cs, ci = ops.topk_dot(q, db, k, exclude=ex)
    q.copy_(torch.from_numpy(unit_rows(nq, C, seed=7)).to(dev))
    db.copy_(torch.from_numpy(unit_rows(n, C, seed=8)).to(dev))
    ex.copy_(torch.arange(nq, device=dev) + 100)
    g.replay()
    torch.cuda.synchronize()
    es, ei = ops.topk_dot(q, db, k, exclude=ex)
    assert torch.equal(ci, ei) and torch.equal(cs.view(torch.int32), es.view(torch.int32))
