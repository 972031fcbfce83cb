"""numpy reference of the exact top-k search (molclr_topk_dot's contract) and
the inputs the CPU and GPU retrieval tests share."""
import numpy as np


def topk_ref(scores, k, exclude=None, idx_base=0):
    """``(scores [nq, k] float64, idx [nq, k] int64)`` of a full score matrix
    ``scores`` [nq, n] (int64 or float64): per query the k best rows under
    (higher score, then lower index), a NaN score as -inf, -0.0 equal to +0.0;
    row ``exclude[i] - idx_base`` left out for query i; indices reported as
    ``j + idx_base``; missing entries ``-inf / -1``."""
    s = np.asarray(scores).astype(np.float64)
    s = np.where(np.isnan(s), -np.inf, s) + 0.0  # -0.0 + 0.0 == +0.0
    nq, n = s.shape
    out_s = np.full((nq, k), -np.inf)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    for i in range(nq):
        rows = np.arange(n, dtype=np.int64)
        if exclude is not None:
            rows = rows[rows + idx_base != int(exclude[i])]
        order = np.lexsort((rows, -s[i, rows]))[:k]  # last key first: score, then index
        m = order.shape[0]
        out_s[i, :m] = s[i, rows[order]]
        out_i[i, :m] = rows[order] + idx_base
    return out_s, out_i


def int_case(nq, n, C, seed):
    """Integer operands in [-2, 2] (exact in fp32 and bf16; every dot product
    an integer of magnitude <= 4 C) and their exact int64 score matrix."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-2, 3, size=(nq, C)).astype(np.int64)
    db = rng.integers(-2, 3, size=(n, C)).astype(np.int64)
    return q, db, q @ db.T


def unit_rows(rows, C, seed):
    """Unit-norm Gaussian rows, float32."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, C))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)
