"""Retrieval without a device: the top-k entry points' exports, refusals and
workspace query (argument validation returns before any HIP call), the numpy
reference the GPU tests compare against, merge_topk's order, and the index
files."""
import json

import numpy as np
import pytest
import torch

from .retrieval_ref import topk_ref


@pytest.fixture(scope="module")
def lib():
    from molclr_amd import _lib
    from molclr_amd.build import build
    build()
    return _lib.load()


def test_library_exports_the_topk_symbols(lib):
    from molclr_amd._lib import SIGNATURES
    for name in ("molclr_topk_dot_workspace_bytes", "molclr_topk_dot"):
        assert name in SIGNATURES and hasattr(lib, name)


def _call(lib, nq=4, n=100, C=8, k=3, ldq=None, lddb=None, bf16=0, ws_bytes=1 << 30):
    """molclr_topk_dot on null pointers: only a refusal can come back."""
    return lib.molclr_topk_dot(None, C if ldq is None else ldq, None, C if lddb is None else lddb,
                               bf16, nq, n, C, k, None, 0, None, None, None, ws_bytes, None)


@pytest.mark.parametrize("kwargs,word", [
    (dict(k=0), b"k 0"),
    (dict(k=65), b"k 65"),
    (dict(C=6), b"C 6"),
    (dict(C=2052), b"C 2052"),
    (dict(C=8, lddb=4), b"lddb 4"),
    (dict(n=-1), b"n -1"),
    (dict(ws_bytes=0), b"workspace_bytes 0"),
])
def test_refusals_before_any_hip_call(lib, kwargs, word):
    assert _call(lib, **kwargs) == -1
    msg = lib.molclr_last_error()
    assert b"molclr_topk_dot" in msg and word in msg, msg


def test_more_refusals(lib):
    assert _call(lib, C=8, ldq=4) == -1 and b"ldq 4" in lib.molclr_last_error()
    # bf16 rows of 12 values are 24 bytes: not 16-byte aligned
    assert _call(lib, C=12, lddb=12, bf16=1) == -1 and b"lddb 12" in lib.molclr_last_error()
    assert _call(lib, nq=-1) == -1 and b"nq -1" in lib.molclr_last_error()
    # an empty query set is a valid call and touches nothing
    assert _call(lib, nq=0, ws_bytes=0) == 0


def test_workspace_query(lib):
    ws = lib.molclr_topk_dot_workspace_bytes
    assert ws(1, 1, 4, 1) > 0 and ws(1024, 10 ** 7, 512, 10) > 0
    assert ws(0, 100, 4, 1) == 0 and ws(1, 0, 4, 1) == 0
    for n in (1, 257, 5000, 10 ** 6, 10 ** 7):
        for k in (1, 10, 64):
            sizes = [ws(nq, n, 512, k) for nq in (1, 5, 31, 32, 33, 64, 65, 96, 97, 1000, 1024,
                                                  8192, 8193, 20000)]
            assert sizes == sorted(sizes), (n, k, sizes)
        for nq in (1, 33, 1024):
            sizes = [ws(nq, n, 512, k) for k in range(1, 65)]
            assert sizes == sorted(sizes), (n, nq, sizes)
    # the candidates of the flagship shape stay small next to the database
    assert ws(1024, 10 ** 7, 512, 10) < 4 << 20


def test_reference_on_a_hand_written_case():
    """3 queries x 6 rows with ties, by hand."""
    s = np.array([[5, 7, 7, 1, 7, 0],
                  [0, 0, 0, 0, 0, 0],
                  [-3, 2, -3, 2, 9, 2]], dtype=np.int64)
    sc, ix = topk_ref(s, 4)
    assert ix.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3], [4, 1, 3, 5]]
    assert sc.tolist() == [[7, 7, 7, 5], [0, 0, 0, 0], [9, 2, 2, 2]]
    # exclude (in idx_base terms) and the index offset
    sc, ix = topk_ref(s, 3, exclude=[101, 100, 104], idx_base=100)
    assert ix.tolist() == [[102, 104, 100], [101, 102, 103], [101, 103, 105]]
    assert sc.tolist() == [[7, 7, 5], [0, 0, 0], [2, 2, 2]]
    # fewer rows than k: -inf / -1
    sc, ix = topk_ref(s[:, :2], 3, exclude=[0, 5, 1])
    assert ix.tolist() == [[1, -1, -1], [0, 1, -1], [0, -1, -1]]
    assert sc[0, 0] == 7 and np.isneginf(sc[0, 1:]).all() and np.isneginf(sc[1, 2])
    # NaN ranks as -inf (after every finite score, before nothing), -0.0 == +0.0
    f = np.array([[np.nan, -1.0, -0.0, 0.0, -np.inf]])
    sc, ix = topk_ref(f, 5)
    assert ix.tolist() == [[2, 3, 1, 0, 4]]
    assert sc[0, :3].tolist() == [0.0, 0.0, -1.0] and np.isneginf(sc[0, 3:]).all()
    assert not np.signbit(sc[0, 0])


def test_merge_topk_order_on_cpu_tensors():
    from molclr_amd.retrieval import merge_topk
    inf = float("inf")
    a = (torch.tensor([[3.0, 1.0, 1.0], [2.0, -inf, -inf]]),
         torch.tensor([[4, 0, 2], [1, 3, -1]]))
    b = (torch.tensor([[3.0, 3.0, 1.0], [-inf, -inf, -inf]]),
         torch.tensor([[10, 12, 11], [7, -1, -1]]))
    s, i = merge_topk([a, b])
    assert i.tolist() == [[4, 10, 12], [1, 3, 7]]
    assert s[0].tolist() == [3.0, 3.0, 3.0] and s[1].tolist() == [2.0, -inf, -inf]
    s, i = merge_topk([b, a], k=7)  # the order of the parts does not matter; padding last
    assert i.tolist() == [[4, 10, 12, 0, 2, 11, -1], [1, 3, 7, -1, -1, -1, -1]]
    assert s[0].tolist() == [3.0, 3.0, 3.0, 1.0, 1.0, 1.0, -inf]
    # against the reference on a random tied case split in two
    rng = np.random.default_rng(3)
    sc = rng.integers(-3, 4, size=(5, 40)).astype(np.int64)
    rs, ri = topk_ref(sc, 6)
    parts = []
    for lo, hi in ((0, 17), (17, 40)):
        ps, pi = topk_ref(sc[:, lo:hi], 6, idx_base=lo)
        parts.append((torch.from_numpy(ps), torch.from_numpy(pi)))
    s, i = merge_topk(parts)
    assert np.array_equal(i.numpy(), ri) and np.array_equal(s.numpy(), rs)


def test_index_files_round_trip(tmp_path):
    from molclr_amd.retrieval import MoleculeIndex
    g = torch.Generator().manual_seed(0)
    emb = torch.randn(7, 12, generator=g)
    for dtype, np_dtype in ((torch.float32, np.float32), (torch.bfloat16, np.uint16)):
        e = emb.to(dtype)
        path = tmp_path / f"lib_{np_dtype.__name__}.npy"
        MoleculeIndex(e, normalized=False, which='out').save(path)
        arr = np.load(path, allow_pickle=False)
        assert arr.dtype == np_dtype and arr.shape == (7, 12)
        if dtype == torch.bfloat16:  # the bit patterns: the upper half of the fp32 of the value
            bits = e.float().numpy().view(np.uint32) >> 16
            assert np.array_equal(arr, bits.astype(np.uint16))
        meta = json.loads((tmp_path / (path.name + ".json")).read_text())
        assert meta == {"dtype": str(dtype).replace("torch.", ""), "normalized": False,
                        "which": "out", "count": 7, "dim": 12}
        back = MoleculeIndex.load(path)
        assert back.embeddings.dtype == dtype and torch.equal(back.embeddings, e)
        assert (back.normalized, back.which, len(back), back.dim) == (False, "out", 7, 12)
    # a sidecar that disagrees with the matrix is refused
    (tmp_path / (path.name + ".json")).write_text(json.dumps(dict(meta, count=8)))
    with pytest.raises(ValueError):
        MoleculeIndex.load(path)


def test_cpu_tensors_are_refused():
    from molclr_amd import ops
    with pytest.raises(RuntimeError):
        ops.topk_dot(torch.zeros(2, 8), torch.zeros(5, 8), 3)
