"""F.normalize, BatchNorm statistics and the Adam step, element by element.

Every reference is an fp64 evaluation of the kernel's formula on the SAME fp32
inputs, and every assertion is a per-element bound obtained by counting the
fp32 roundings on the way to that element (u = 2^-24, first order in u).  A
sum of n terms in any order carries at most (n - 1) u Σ|x_i|.  A derived
bound is doubled (SLACK) for the second-order terms and for nothing else.  A
fused multiply-add removes a rounding, so contraction can only help.

An element that fails here is a finding about the kernel: do not widen a bound.
"""
import ctypes

import numpy as np
import pytest
import torch

from molclr_amd import _lib

gpu = pytest.mark.gpu

U = 2.0 ** -24
SLACK = 2.0
F32 = np.float32


def f64(t):
    return t.detach().cpu().double().numpy()


def worst(name, got, ref, bound):
    """max of |got - ref| / bound over the elements (0/0 counts as 0)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    assert np.isfinite(got).all(), name + ": non-finite output"
    ratio = np.where(err == 0.0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    i = np.unravel_index(np.argmax(ratio), ratio.shape) if ratio.size else ()
    return (float(ratio[i]) if ratio.size else 0.0), i


def check(name, got, ref, bound):
    r, i = worst(name, got, ref, bound)
    print("%-14s worst |err| / derived bound = %.3f at %s" % (name, r, i))
    assert r <= SLACK, (name, r, i)


# ===========================================================================
# F.normalize
# ===========================================================================
L2_EPS = 1e-12
L2_EPS32 = float(F32(L2_EPS))          # the kernel rounds eps to fp32 once
ROW_KINDS = 6  # 0 zero, 1 entries 1e-14, 2 entries 1e-20, 3 entries +-1e17, 4 dy || y, 5 ordinary


def l2_fwd_ref(z, eps):
    norm = np.sqrt((z * z).sum(1))
    return z / np.maximum(norm, eps)[:, None], norm


def l2_bwd_ref(dy, y, norm, eps):
    """The backward as the kernel is handed it: dy, the forward's y and norm."""
    dot = (dy * y).sum(1, keepdims=True)
    big = (norm > eps)[:, None]
    return np.where(big, (dy - dot * y) / np.where(big, norm[:, None], 1.0), dy / eps)


def l2_case(rows, D, shift, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((rows, D)).astype(F32)
    sign = np.where(rng.random((rows, D)) < 0.5, -1.0, 1.0).astype(F32)
    kind = (np.arange(rows) + shift) % ROW_KINDS
    z[kind == 0] = 0.0
    z[kind == 1] = (F32(1e-14) * sign)[kind == 1]   # 0 < norm < eps
    z[kind == 2] = (F32(1e-20) * sign)[kind == 2]   # squares underflow; still z / eps
    z[kind == 3] = (F32(1e17) * sign)[kind == 3]    # squares 1e34, their sum < 3.4e38
    dy = rng.standard_normal((rows, D)).astype(F32)
    return z, dy, kind


def test_l2_reference_matches_autograd():
    """The fp64 reference against torch's own F.normalize and its autograd in
    fp64 (CPU): the below-eps rows included (clamp_min passes no gradient to
    the norm there, dz = dy / eps)."""
    z, dy, kind = l2_case(60, 65, 0, 1)
    z = z.astype(np.float64)
    z[kind == 3] *= 1e-17        # fp64 autograd squares these too; keep them ordinary
    dy = dy.astype(np.float64)
    zt = torch.from_numpy(z).requires_grad_(True)
    yt = torch.nn.functional.normalize(zt, dim=1, eps=L2_EPS)
    yt.backward(torch.from_numpy(dy))
    y, norm = l2_fwd_ref(z, L2_EPS)
    np.testing.assert_allclose(y, yt.detach().numpy(), rtol=1e-14, atol=0)
    dz = l2_bwd_ref(dy, y, norm, L2_EPS)
    scale = np.abs(dy).max(1, keepdims=True) / np.maximum(norm, L2_EPS)[:, None]
    assert (np.abs(dz - zt.grad.numpy()) <= 1e-13 * scale).all()
    assert (kind[norm < L2_EPS] <= 2).all() and (norm[kind <= 2] < L2_EPS).all()


@gpu
@pytest.mark.parametrize("D", [1, 2, 63, 64, 65, 256, 300])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 257])
def test_l2norm_elementwise(dev, rows, D):
    """One wave per row, four rows per block: rows on either side of 4, D on
    either side of 64.  A matrix of fewer than six rows cannot hold every kind
    of row, so every rotation of the kinds is run at those sizes.

    Forward.  ss = Σ fl(z_c^2): one rounding per square and D - 1 additions of
    positive terms, relative error D u; a flushed or subnormal square adds at
    most 2^-126 each, D 2^-126 in all.  norm = fl(sqrt(ss)): halves the
    relative error and adds u, and sqrt(a + d) <= sqrt(a) + sqrt(d):
        |norm^ - norm| <= (D/2 + 1) u norm + sqrt(D) 2^-63.
    y = fl(z / max(norm^, eps)): one more rounding,
        |y^ - y| <= ((D/2 + 2) u + sqrt(D) 2^-63 / norm) |y|      (norm > eps)
        |y^ - z / eps| <= u |z / eps|                              (norm < eps).
    Backward, from dy and the forward's own y^, norm^ (S = Σ_k |dy_k y_k|):
    dot carries D u S (D products, D - 1 additions); fl(dot y_c) adds u |dot
    y_c| <= u S |y_c|; the subtraction and the division add u each of
    |dy_c| + S |y_c|:
        |dz^ - dz| <= u (2 |dy_c| + (D + 3) S |y_c|) / norm^      (norm^ > eps)
        |dz^ - dy / eps| <= u |dy / eps|                           (otherwise).
    The row whose dy is parallel to y has dz ~ 0 by cancellation and is held
    to this absolute bound, not to a relative one."""
    lib = _lib.load()
    for shift in range(ROW_KINDS if rows < ROW_KINDS else 1):
        z, dy, kind = l2_case(rows, D, shift, 100 * rows + D)
        zd = torch.from_numpy(z).to(dev)
        yd = torch.full((rows, D), float("nan"), device=dev)
        nd = torch.full((rows,), float("nan"), device=dev)
        assert lib.molclr_l2norm_fwd(zd.data_ptr(), yd.data_ptr(), nd.data_ptr(), rows, D, L2_EPS,
                                     None) == 0
        torch.cuda.synchronize()
        y_ref, n_ref = l2_fwd_ref(z.astype(np.float64), L2_EPS32)
        uf = np.sqrt(D) * 2.0 ** -63
        check("l2 norm", f64(nd), n_ref, (D / 2 + 1) * U * n_ref + uf)
        small = n_ref < L2_EPS32
        assert (small == (kind <= 2)).all()
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(small, U, (D / 2 + 2) * U + uf / n_ref)
        check("l2 y", f64(yd), y_ref, rel[:, None] * np.abs(y_ref))
        assert (f64(yd)[kind == 0] == 0).all()

        # the backward takes the forward's fp32 y and norm; dy of kind 4 is 3 y
        yk, nk = f64(yd), f64(nd)
        dy[kind == 4] = (3.0 * yk[kind == 4]).astype(F32)
        dyd = torch.from_numpy(dy).to(dev)
        dzd = torch.full((rows, D), float("nan"), device=dev)
        assert lib.molclr_l2norm_bwd(dyd.data_ptr(), yd.data_ptr(), nd.data_ptr(), dzd.data_ptr(),
                                     rows, D, L2_EPS, None) == 0
        torch.cuda.synchronize()
        dy64 = dy.astype(np.float64)
        dz_ref = l2_bwd_ref(dy64, yk, nk, L2_EPS32)
        S = np.abs(dy64 * yk).sum(1, keepdims=True)
        big = (nk > L2_EPS32)[:, None]
        assert (big[:, 0] == (kind > 2)).all()
        bound = np.where(big, U * (2 * np.abs(dy64) + (D + 3) * S * np.abs(yk))
                         / np.where(big, nk[:, None], 1.0), U * np.abs(dy64 / L2_EPS32))
        check("l2 dz", f64(dzd), dz_ref, bound)
        if (kind == 4).any() and D > 1:   # cancellation: far below dy / norm
            assert np.abs(dz_ref[kind == 4]).max() < 1e-5 * 3.0 / nk[kind == 4].min()


# ===========================================================================
# BatchNorm statistics conditioning
# ===========================================================================
BN_EPS, BN_MOM = 1e-5, 0.1
BN_EPS32, BN_MOM32 = float(F32(BN_EPS)), float(F32(BN_MOM))
BN_KEEP32 = float(F32(1.0) - F32(BN_MOM))   # the kernel's 1.f - momentum
BN_SEGS = [(2,), (7,), (97,), (400,), (97, 3)]
BN_OFFSET, BN_SIGMA = 100.0, 0.1            # kappa = sqrt(1 + mu^2 / sigma^2) ~ 1e3


def bn_case(rows, D, seed=0):
    """Columns cycle: N(0, 1); +100 + 0.1 N(0, 1); -100 + 0.1 N(0, 1); constant
    (0 in every other constant column, 2.5 in the rest)."""
    rng = np.random.default_rng(1000 * sum(rows) + D + seed)
    N = sum(rows)
    z = rng.standard_normal((N, D))
    j = np.arange(D)
    z[:, j % 4 == 1] = BN_OFFSET + BN_SIGMA * z[:, j % 4 == 1]
    z[:, j % 4 == 2] = -BN_OFFSET + BN_SIGMA * z[:, j % 4 == 2]
    z[:, j % 4 == 3] = np.where((j[j % 4 == 3] // 4) % 2 == 0, 0.0, 2.5)[None, :]
    gamma = rng.uniform(0.5, 1.5, D).astype(F32)
    beta = rng.uniform(-0.5, 0.5, D).astype(F32)
    dy = rng.standard_normal((N, D)).astype(F32)
    return z.astype(F32), dy, gamma, beta


def bn_stats64(x):
    """fp64 mean, biased variance, kappa and max |x| per column."""
    mu = x.mean(0)
    var = ((x - mu) ** 2).mean(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.where(var > 0, np.sqrt(1.0 + mu * mu / np.where(var > 0, var, 1.0)), 0.0)
    return mu, var, kappa, np.abs(x).max(0)


def var_bound(n, kappa):
    """Chan, Golub & LeVeque (1983): an updating algorithm (Welford's steps and
    Chan's pairwise merges are its two forms) computes the sum of squared
    deviations with relative error <= n kappa u."""
    return n * kappa * U


def test_variance_bound_separates_welford_from_cancellation():
    """The bound has teeth only if a cancelling formula breaks it: a condition
    on the INPUTS, checked here on the CPU in numpy fp32 for the very matrices
    of test_batchnorm_conditioning.  Sequential Welford stays inside n kappa u;
    mean(x*x) - mean(x)^2 lies at least 4 x outside what the GPU test allows
    (SLACK n kappa u) in its worst kappa ~ 1e3 column -- the GPU assertion is
    per element, so one column outside fails it."""
    worst_sep = np.inf
    for rows in BN_SEGS:
        for D in (4, 300):
            z = bn_case(rows, D)[0]
            r0 = 0
            for n in rows:
                x = z[r0:r0 + n]
                r0 += n
                _, var, kappa, _ = bn_stats64(x.astype(np.float64))
                cols = np.arange(D) % 4
                hot = (cols == 1) | (cols == 2)
                assert (kappa[hot] > 100).all()
                mean, m2 = np.zeros(D, F32), np.zeros(D, F32)
                for k in range(n):
                    d = x[k] - mean
                    mean = mean + d / F32(k + 1)
                    m2 = m2 + d * (x[k] - mean)
                welford = (m2 / F32(n)).astype(np.float64)
                sos = ((x * x).mean(0, dtype=F32) - x.mean(0, dtype=F32) ** 2).astype(np.float64)
                bound = var_bound(n, kappa[hot]) * var[hot]
                assert (np.abs(welford[hot] - var[hot]) <= bound).all(), (rows, D, n)
                sep = (np.abs(sos[hot] - var[hot]) / (SLACK * bound)).max()
                print("rows %s D %d n %d: sum-of-squares worst column at %.1f x the allowed error"
                      % (rows, D, n, sep))
                worst_sep = min(worst_sep, sep)
                assert sep >= 4.0, (rows, D, n, sep)
    print("smallest separation factor: %.1f" % worst_sep)


def bn_reference(z, dy, gamma, beta, rows, relu, sm_k, si_k, y_k):
    """fp64 values and first-order bounds of everything the two calls write.
    sm_k / si_k / y_k are the KERNEL's save_mean, save_invstd and y: the inputs
    of the backward call (and its ReLU mask, a discrete function of y^)."""
    D = z.shape[1]
    g64, b64 = gamma.astype(np.float64), beta.astype(np.float64)
    out = {k: [] for k in ("mean", "mean_b", "is", "is_b", "y", "y_b", "dz", "dz_b")}
    rm, rm_b = np.zeros(D), np.zeros(D)
    rv, rv_b = np.ones(D), np.zeros(D)
    dg, dg_b, db, db_b = np.zeros(D), np.zeros(D), np.zeros(D), np.zeros(D)
    r0 = 0
    for s, n in enumerate(rows):
        x = z[r0:r0 + n].astype(np.float64)
        g = dy[r0:r0 + n].astype(np.float64)
        mu, var, kappa, M = bn_stats64(x)
        const = var == 0
        e_mu = np.where(const, 0.0, 7 * n * U * M)
        e_var = np.where(const, 0.0, var_bound(n, kappa))              # relative
        istd = 1.0 / np.sqrt(var + BN_EPS32)
        e_is = e_var / 2 + 2.5 * U                                      # relative
        xc = x - mu
        y = xc * istd * g64 + b64
        y_b = (g64 * istd * (np.abs(xc) * (e_is + U) + e_mu)
               + U * (np.abs(b64) + np.abs(mu * g64 * istd)) + U * np.abs(y))
        if relu:
            y = np.maximum(y, 0.0)
        # running statistics, segment after segment
        unb = var * n / (n - 1)
        rm_b = BN_KEEP32 * rm_b + BN_MOM32 * e_mu + 2 * U * (np.abs(BN_KEEP32 * rm) + np.abs(BN_MOM32 * mu))
        rm = BN_KEEP32 * rm + BN_MOM32 * mu
        rv_b = BN_KEEP32 * rv_b + BN_MOM32 * unb * (e_var + U) + 2 * U * (BN_KEEP32 * rv + BN_MOM32 * unb)
        rv = BN_KEEP32 * rv + BN_MOM32 * unb
        # backward from the call's own inputs
        mk, ik = sm_k[s], si_k[s]
        gm = g * (y_k[r0:r0 + n] > 0) if relu else g
        xh = (x - mk) * ik
        a1, a2 = np.abs(gm).mean(0), np.abs(gm * xh).mean(0)
        k1, k2 = gm.mean(0), (gm * xh).mean(0)
        sc = g64 * ik
        dz = (gm - k1 - xh * k2) * sc
        dz_b = np.abs(sc) * U * ((n + 3) * a1 + (n + 8) * np.abs(xh) * a2 + 2 * np.abs(gm)) + 2 * U * np.abs(dz)
        db_s, dg_s = gm.sum(0), (gm * xh).sum(0)
        db_b = db_b + (n - 1) * U * n * a1 + (U * np.abs(db + db_s) if s else 0.0)
        dg_b = dg_b + (n + 2) * U * n * a2 + (U * np.abs(dg + dg_s) if s else 0.0)
        db, dg = db + db_s, dg + dg_s
        for k, v in (("mean", mu), ("mean_b", e_mu), ("is", istd), ("is_b", e_is * istd), ("y", y),
                     ("y_b", y_b), ("dz", dz), ("dz_b", dz_b)):
            out[k].append(v)
        r0 += n
    res = {k: (np.concatenate(v) if k in ("y", "y_b", "dz", "dz_b") else np.stack(v))
           for k, v in out.items()}
    res.update(rm=rm, rm_b=rm_b, rv=rv, rv_b=rv_b, dg=dg, dg_b=dg_b, db=db, db_b=db_b)
    return res


@gpu
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("D", [4, 300])
@pytest.mark.parametrize("rows", BN_SEGS, ids=lambda r: "x".join(map(str, r)))
def test_batchnorm_conditioning(dev, rows, D, relu):
    """molclr_batchnorm_seg_fwd / _bwd, fp32 storage, on columns with
    |mean| / std of 0, +-1e3 and a constant column, per element against fp64.

    n rows in the segment, M = max |x| of the column, kappa = sqrt(1 + mu^2 /
    var), eps and momentum rounded to fp32 once as the kernel does.
    mean: every Welford step or Chan merge forms a + (b - a) w, w <= 1, in four
      roundings (the difference, w, the product, the sum): at most
      3 u |b - a| w + u |new| <= 7 u M, carried on with weight <= 1 through
      fewer than n merges:              |mean^ - mu| <= 7 n u M.
    var: n kappa u relative (var_bound); the division by n is inside SLACK.
    invstd = 1 / sqrt(var + eps): the sum adds u, the root halves and adds u,
      the reciprocal adds u:            e_is = n kappa u / 2 + 2.5 u  (relative).
    A constant column has every difference exactly 0: mean exact, var exactly
      0, invstd = fl(1 / fl(sqrt(eps))) within 2 u.
    y = fma(x, sc, sh), sc = fl(gamma is), sh = fma(-mean, sc, beta):
      (x - mean^) sc differs from (x - mu) gamma is by gamma is (|x - mu|
      (e_is + u) + |dmean|); sh is rounded once, u (|beta| + |mu gamma is|),
      and y once, u |y|.  The shift's rounding is why a constant column of
      value c gives beta + O(u |c| gamma / sqrt(eps)) and beta exactly only for
      c = 0 (every other constant column here); ReLU is 1-Lipschitz.
    running_mean / running_var = fl(fl(keep r) + fl(mom s)): mom times the
      statistic's error plus 2 u (|keep r| + |mom s|), segment after segment;
      the unbiased variance adds one division, u.
    The backward call's inputs are dy, z, gamma, beta and the forward's own
    save_mean, save_invstd (bounded above), so its reference takes those, and
    its ReLU mask is y^ > 0 (an element whose y is within its bound of 0 may
    fall on either side; the backward recomputes the forward's y^ bit for bit).
    With A1 = mean |g|, A2 = mean |g xhat|:
      dbeta = Σ g: (n - 1) u n A1;  dgamma = Σ g xhat: xhat two roundings, the
      product one, n - 1 additions: (n + 2) u n A2;  a second segment's sum is
      added with one more rounding.
      k1 = fl(dbeta fl(1 / n)), k2 likewise: (n + 1) u A1, (n + 4) u A2.
      dz = fl(fl(fl(g - k1) - fl(xhat k2)) sc):
        |dz^ - dz| <= |sc| u ((n + 3) A1 + (n + 8) |xhat| A2 + 2 |g|) + 2 u |dz|.
    """
    lib = _lib.load()
    z, dy, gamma, beta = bn_case(rows, D)
    N, S = sum(rows), len(rows)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    zd, dyd, gd, bd = t(z), t(dy), t(gamma), t(beta)
    seg = (ctypes.c_int64 * S)(*rows)
    wsb = lib.molclr_batchnorm_seg_workspace_bytes(S, seg, D)
    ws = torch.full((wsb + 4096,), 0x5A, dtype=torch.uint8, device=dev)
    rm, rv = torch.zeros(D, device=dev), torch.ones(D, device=dev)
    nbt = torch.zeros(1, dtype=torch.int64, device=dev)
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    y, sm, si = nan(N, D), nan(S, D), nan(S, D)
    assert lib.molclr_batchnorm_seg_fwd(zd.data_ptr(), gd.data_ptr(), bd.data_ptr(), rm.data_ptr(),
                                        rv.data_ptr(), nbt.data_ptr(), y.data_ptr(), sm.data_ptr(),
                                        si.data_ptr(), S, seg, D, 0, BN_MOM, BN_EPS, 1, relu,
                                        ws.data_ptr(), wsb, None) == 0, lib.molclr_last_error()
    dz, dg, db = nan(N, D), nan(D), nan(D)
    assert lib.molclr_batchnorm_seg_bwd(dyd.data_ptr(), zd.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                        sm.data_ptr(), si.data_ptr(), dz.data_ptr(), dg.data_ptr(),
                                        db.data_ptr(), S, seg, D, 0, relu, 0, ws.data_ptr(), wsb,
                                        None) == 0, lib.molclr_last_error()
    torch.cuda.synchronize()
    assert (ws[wsb:] == 0x5A).all() and int(nbt) == S
    ref = bn_reference(z, dy, gamma, beta, rows, relu, f64(sm), f64(si), f64(y))
    check("save_mean", f64(sm), ref["mean"], ref["mean_b"])
    check("save_invstd", f64(si), ref["is"], ref["is_b"])
    check("running_mean", f64(rm), ref["rm"], ref["rm_b"])
    check("running_var", f64(rv), ref["rv"], ref["rv_b"])
    check("y", f64(y), ref["y"], ref["y_b"])
    check("dz", f64(dz), ref["dz"], ref["dz_b"])
    check("dgamma", f64(dg), ref["dg"], ref["dg_b"])
    check("dbeta", f64(db), ref["db"], ref["db_b"])
    # the constant columns: exact mean, invstd within 2 u, y = beta exactly at c = 0
    cc = np.arange(D) % 4 == 3
    zero = cc & ((np.arange(D) // 4) % 2 == 0)
    assert (f64(sm)[:, cc] == z[0, cc].astype(np.float64)).all()
    is0 = 1.0 / np.sqrt(BN_EPS32)
    assert (np.abs(f64(si)[:, cc] - is0) <= 2 * U * is0).all()
    b_ref = np.maximum(beta.astype(np.float64), 0.0) if relu else beta.astype(np.float64)
    assert (f64(y)[:, zero] == b_ref[zero]).all()


# ===========================================================================
# Adam: one step from crafted state
# ===========================================================================
ADAM_LR, ADAM_EPS = 5e-4, 1e-8
ADAM_KINDS = 6  # 0 g=m=v=0  1 g=v=0,m!=0  2 v=1e-30  3 v=1e30  4 ordinary  5 g=m=v=p=0


def adam_state(n, shift, seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(F32)
    g = rng.standard_normal(n).astype(F32)
    m = (0.1 * rng.standard_normal(n)).astype(F32)
    v = (0.01 * rng.random(n) + 1e-4).astype(F32)
    kind = (np.arange(n) + shift) % ADAM_KINDS
    for k in (0, 5):
        g[kind == k] = 0
        m[kind == k] = 0
        v[kind == k] = 0
    p[kind == 5] = 0
    g[kind == 1] = 0
    v[kind == 1] = 0
    m[kind == 1] = (1e-6 * rng.standard_normal(n)).astype(F32)[kind == 1]
    v[kind == 2] = F32(1e-30)
    v[kind == 3] = F32(1e30)
    return p, g, m, v, kind


def adam_reference(p, g, m, v, step, b1, b2, wd):
    """The kernel comment's formula in fp64, its scalars rounded to fp32 once
    (-lr / bc1 and sqrt(bc2) from fp64, as torch's scalar arguments are), with
    the first-order bounds.  e_g: fl(g + fl(wd p)).  m: lerp's branch for
    weight < 0.5 is m + w1 (G - m), else G - (G - m) fl(1 - w1): the
    difference, the product and the sum round once each.  v = fl(fl(v b2) +
    fl(fl(w2 G) G)).  den = fl(fl(sqrt(v)) / s2) + eps).  p = fl(p + fl(nss
    fl(m / den))): ten-odd roundings in all, each propagated below."""
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    lr32 = float(F32(ADAM_LR))
    w1, fb2, w2 = float(F32(1.0 - b1)), float(F32(b2)), float(F32(1.0 - b2))
    omw = float(F32(1.0) - F32(w1))
    nss = float(F32(-(lr32 / (1.0 - b1 ** step))))
    s2 = float(F32(np.sqrt(1.0 - b2 ** step)))
    eps32, wd32 = float(F32(ADAM_EPS)), float(F32(wd))
    G = g + wd32 * p
    e_g = U * (np.abs(wd32 * p) + np.abs(G))
    d = G - m
    if abs(w1) < 0.5:
        M = m + w1 * d
        e_m = w1 * e_g + 2 * U * w1 * np.abs(d) + U * np.abs(M)
    else:
        M = G - d * omw
        e_m = (1 + omw) * e_g + 2 * U * omw * np.abs(d) + U * np.abs(M)
    V = v * fb2 + w2 * G * G
    e_v = U * v * fb2 + 2 * w2 * np.abs(G) * e_g + 2 * U * w2 * G * G + U * V
    rt = np.sqrt(V)
    den = rt / s2 + eps32
    e_den = (np.where(V > 0, e_v / (2 * np.where(V > 0, rt, 1.0)), 0.0) + 2 * U * rt) / s2 + U * den
    q = M / den
    e_q = e_m / den + np.abs(M) * e_den / den ** 2 + U * np.abs(q)
    r = nss * q
    P = p + r
    e_p = abs(nss) * e_q + U * np.abs(r) + U * np.abs(P)
    return (P, e_p), (M, e_m), (V, e_v), G


@gpu
@pytest.mark.parametrize("wd", [0.0, 1e-5])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.999), (0.3, 0.9)], ids=str)
@pytest.mark.parametrize("counter", [0, 1, 999, 99999])
@pytest.mark.parametrize("n", [4, 4 * 1023, 4 * 1024, 4 * 1025])
def test_adam_one_step(dev, n, counter, betas, wd):
    """n on either side of one block's 1024 float4s; the device step counter
    preset; both lerp branches (1 - beta1 below and at or above 0.5).  p must
    stay where G = g + wd p, m and v are all 0 (wd == 0 or p == 0) -- the
    denominator is eps, the step 0 / eps -- and nothing may become NaN."""
    lib = _lib.load()
    shift = (counter + int(10 * betas[0]) + (wd > 0)) % ADAM_KINDS
    p, g, m, v, kind = adam_state(n, shift, n + counter)
    pd, gd, md, vd = (torch.from_numpy(a).to(dev) for a in (p, g, m, v))
    lr = torch.tensor([ADAM_LR], dtype=torch.float32, device=dev)
    step = torch.tensor([counter], dtype=torch.int32, device=dev)
    args = (n, lr.data_ptr(), step.data_ptr(), betas[0], betas[1], ADAM_EPS, wd)
    assert lib.molclr_adam_step_ex(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(),
                                   *args, 0, None) == 0, lib.molclr_last_error()
    torch.cuda.synchronize()
    assert int(step) == counter            # tick = 0 leaves the counter
    (P, e_p), (M, e_m), (V, e_v), G = adam_reference(p, g, m, v, counter + 1, *betas, wd)
    check("adam m", f64(md), M, e_m)
    check("adam v", f64(vd), V, e_v)
    check("adam p", f64(pd), P, e_p)
    still = (G == 0) & (m == 0) & (v == 0)
    assert still[kind == 5].all() and (wd > 0 or still[kind == 0].all())
    assert (f64(pd)[still] == p[still]).all() and (f64(md)[still] == 0).all()
    assert torch.equal(gd.cpu(), torch.from_numpy(g))
    # tick = 1 adds exactly one (the state moves a second step; not compared)
    assert lib.molclr_adam_step_ex(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(),
                                   *args, 1, None) == 0
    torch.cuda.synchronize()
    assert int(step) == counter + 1
    assert torch.isfinite(pd).all() and torch.isfinite(md).all() and torch.isfinite(vd).all()


@gpu
def test_adam_tick_without_elements_and_step_tail(dev):
    lib = _lib.load()
    lr = torch.tensor([ADAM_LR], dtype=torch.float32, device=dev)
    step = torch.tensor([41], dtype=torch.int32, device=dev)
    for tick, want in ((1, 42), (0, 42)):   # n == 0 launches no update and still ticks
        assert lib.molclr_adam_step_ex(None, None, None, None, 0, lr.data_ptr(), step.data_ptr(),
                                       0.9, 0.999, ADAM_EPS, 0.0, tick, None) == 0
        torch.cuda.synchronize()
        assert int(step) == want
    loss_src = torch.tensor([3.25], device=dev)
    loss_dst = torch.tensor([float("nan")], device=dev)
    st_src = torch.tensor([0x14], dtype=torch.int32, device=dev)
    st_acc = torch.tensor([0x41], dtype=torch.int32, device=dev)
    assert lib.molclr_step_tail(step.data_ptr(), loss_src.data_ptr(), loss_dst.data_ptr(),
                                st_src.data_ptr(), st_acc.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert int(step) == 43 and loss_dst.item() == 3.25 and int(st_acc) == 0x55
    assert lib.molclr_step_tail(step.data_ptr(), None, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert int(step) == 44 and loss_dst.item() == 3.25 and int(st_acc) == 0x55
    assert int(st_src) == 0x14 and loss_src.item() == 3.25


@gpu
def test_adam_step_matches_torch_cpu(dev):
    """One ordinary-state step against torch.optim.Adam (single-tensor, CPU,
    fp32) loaded with the same state: within 4 ulp of max(|p|, |dp|)."""
    lib = _lib.load()
    n, counter, wd = 4 * 1025, 999, 1e-5
    rng = np.random.default_rng(5)
    p = rng.standard_normal(n).astype(F32)
    g = rng.standard_normal(n).astype(F32)
    m = (0.1 * rng.standard_normal(n)).astype(F32)
    v = (0.01 * rng.random(n) + 1e-4).astype(F32)
    pr = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.Adam([pr], ADAM_LR, eps=ADAM_EPS, weight_decay=wd, foreach=False)
    pr.grad = torch.from_numpy(g.copy())
    opt.state[pr] = {"step": torch.tensor(float(counter)), "exp_avg": torch.from_numpy(m.copy()),
                     "exp_avg_sq": torch.from_numpy(v.copy())}
    opt.step()
    pd, gd, md, vd = (torch.from_numpy(a).to(dev) for a in (p, g, m, v))
    lr = torch.tensor([ADAM_LR], dtype=torch.float32, device=dev)
    step = torch.tensor([counter], dtype=torch.int32, device=dev)
    assert lib.molclr_adam_step_ex(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n,
                                   lr.data_ptr(), step.data_ptr(), 0.9, 0.999, ADAM_EPS, wd, 1,
                                   None) == 0
    torch.cuda.synchronize()
    assert int(step) == counter + 1 and int(opt.state[pr]["step"]) == counter + 1
    ref = pr.detach().double()
    mag = torch.maximum(torch.from_numpy(p).double().abs(), (ref - torch.from_numpy(p).double()).abs())
    _, e = torch.frexp(mag)                       # mag = f 2^e, f in [0.5, 1): ulp = 2^(e - 24)
    ulp = torch.ldexp(torch.ones_like(mag), e - 24)
    err = (pd.cpu().double() - ref).abs()
    print("adam vs torch CPU: worst %.2f ulp" % (err / ulp).max().item())
    assert (err <= 4 * ulp).all()
