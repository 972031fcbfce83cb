"""The BatchNorm backward through frozen statistics, element by element.

molclr_batchnorm_bwd_frozen / _seg_bwd_frozen / _seg_bwd_frozen_dev /
_seg_bwd_frozen_max against an fp64 evaluation of the same formula on the SAME
inputs: the saved mean and invstd are inputs of the backward, not recomputed.

    g  = dy behind the ReLU mask        (y = (z - mean) invstd gamma + beta > 0)
    dz = gamma invstd g,  dbeta = sum g,  dgamma = sum g (z - mean) invstd

Bounds, counted in roundings as tests/test_gpu_norm_edges.py does (u = 2^-24,
first order, doubled once -- SLACK -- for the second-order terms):

  dz      sc = fl(gamma invstd) and the product fl(sc g): 2 u |dz|; bf16
          storage rounds the stored value once more: + 2^-9 |dz| (dy and z are
          bf16 values, hence exact inputs).
  dbeta   n terms added in some fixed order: n u sum |g|   (n: rows in all,
          plus one addition per segment and one for accumulate).
  dgamma  xhat = fl(fl(z - mean) invstd): 2 u; the product g xhat: u; the sum:
          n u -- (n + 3) u sum |g xhat|.
  accumulate adds the initial value's magnitude to the sum of magnitudes.

The ReLU mask compares a rounded y with 0: the cases keep |y| away from 0 (an
element whose fp64 |y| is below 1e-3 has its z moved onto the mean, where
y = beta and |beta| >= 0.1), so the fp32 and fp64 masks agree.

A row count above 1024 partitions' worth is at least 1024 x 16 x 192 float4s
(12.6 M elements): its fp64 reference alone takes more than a second, so
that size is left out.

The dropout (DropArgs) reaches this kernel through the encoder executors
alone -- no C entry point takes it -- and is checked there
(tests/test_gpu_frozen_models.py) against masks rebuilt by tests/philox.py.
"""
import ctypes

import numpy as np
import pytest
import torch

from molclr_amd import _lib

gpu = pytest.mark.gpu

U = 2.0 ** -24
UB = 2.0 ** -9
SLACK = 2.0
F32 = np.float32
GUARD = 64
SENT = -77.0  # a bf16 value too


def band_unit(D):
    """Rows per partition of the band plan (common.h make_band, norm.hip
    band_parts): band rows per block iteration, 16 iterations."""
    d4 = D // 4
    band = max(256 // d4, 1)
    if band * d4 < 192 and (band + 1) * d4 <= 1024:
        band += 1
    while band * d4 > 1024:
        band -= 1
    return band * 16


def make_case(rows, D, relu, bf16, seed, nseg=1):
    """rows: tuple of segment rows.  Returns fp32 (or bf16-valued) numpy inputs
    and per-segment statistics [S, D]."""
    rng = np.random.default_rng(seed)
    N = sum(rows)
    S = len(rows)
    gamma = rng.uniform(0.5, 1.5, D).astype(F32) * np.where(rng.random(D) < 0.5, -1, 1).astype(F32)
    beta = (rng.uniform(0.1, 0.5, D) * np.where(rng.random(D) < 0.5, -1, 1)).astype(F32)
    mean = rng.normal(0.0, 1.0, (S, D)).astype(F32)
    invstd = rng.uniform(0.5, 2.0, (S, D)).astype(F32)
    z = rng.normal(0.0, 1.5, (N, D)).astype(F32)
    dy = rng.standard_normal((N, D)).astype(F32)
    if bf16:
        z = torch.from_numpy(z).bfloat16().float().numpy()
        dy = torch.from_numpy(dy).bfloat16().float().numpy()
    seg = np.repeat(np.arange(S), rows)
    mu, is_ = mean[seg].astype(np.float64), invstd[seg].astype(np.float64)
    y = (z - mu) * is_ * gamma + beta
    near = np.abs(y) < 1e-3
    if near.any():  # y = beta there; a bf16 z is moved to a bf16 value next to the mean
        zm = mean[seg].astype(F32)
        if bf16:
            zm = torch.from_numpy(zm).bfloat16().float().numpy()
        z = np.where(near, zm, z)
        y = (z - mu) * is_ * gamma + beta
        assert (np.abs(y) >= 1e-3).all()
    return z, dy, gamma, beta, mean, invstd, seg


def reference(z, dy, gamma, beta, mean, invstd, seg, relu):
    mu, is_ = mean[seg].astype(np.float64), invstd[seg].astype(np.float64)
    g64 = gamma.astype(np.float64)
    y = (z.astype(np.float64) - mu) * is_ * g64 + beta
    g = dy.astype(np.float64)
    if relu:
        g = np.where(y > 0, g, 0.0)
    xhat = (z.astype(np.float64) - mu) * is_
    return g64 * is_ * g, g.sum(0), (g * xhat).sum(0), np.abs(g).sum(0), np.abs(g * xhat).sum(0)


def guarded(n, dtype, dev, fill=None):
    t = torch.full((n + GUARD,), SENT, dtype=dtype, device=dev)
    if fill is not None:
        t[:n] = fill
    return t


def guard_ok(t, n):
    return bool((t[n:] == SENT).all().item())


def call_frozen(dev, z, dy, gamma, beta, mean, invstd, rows, relu, accumulate=0, bf16=False,
                init=None, entry="seg", cap=None, rowmax=False):
    """One backward; returns dz [rows or cap, D], dgamma, dbeta (torch, on the
    device) and, for rowmax, the row parts and the slot."""
    lib = _lib.load()
    D = z.shape[1]
    N = cap if cap is not None else sum(rows)
    dt = torch.bfloat16 if bf16 else torch.float32
    zd = torch.from_numpy(z).to(dev).to(dt).contiguous()
    dyd = torch.from_numpy(dy).to(dev).to(dt).contiguous()
    gd, bd = torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev)
    md, sd = torch.from_numpy(mean).to(dev).contiguous(), torch.from_numpy(invstd).to(dev).contiguous()
    dz = guarded(N * D, dt, dev)
    dg = guarded(D, torch.float32, dev, None if init is None else torch.from_numpy(init[0]).to(dev))
    db = guarded(D, torch.float32, dev, None if init is None else torch.from_numpy(init[1]).to(dev))
    S = len(rows)
    c_rows = (ctypes.c_int64 * S)(*rows)
    code = _lib.DTYPE_BF16 if bf16 else _lib.DTYPE_F32
    nparts = int(lib.molclr_bn_row_parts(D))
    rm = guarded(nparts * N, torch.float32, dev) if rowmax else None
    slot = torch.zeros(64 * 32, dtype=torch.float32, device=dev) if rowmax else None
    if entry == "dev":
        wsb = int(lib.molclr_batchnorm_seg_dev_workspace_bytes(S, N, D))
    else:
        wsb = int(lib.molclr_batchnorm_seg_workspace_bytes(S, c_rows, D))
    assert wsb > 0
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    common = (dyd.data_ptr(), zd.data_ptr(), gd.data_ptr(), bd.data_ptr(), md.data_ptr(),
              sd.data_ptr(), dz.data_ptr(), dg.data_ptr(), db.data_ptr())
    if entry == "plain":
        assert S == 1 and not bf16
        rc = lib.molclr_batchnorm_bwd_frozen(*common, rows[0], D, int(relu), accumulate,
                                             ws.data_ptr(), wsb, None)
    elif entry == "seg":
        rc = lib.molclr_batchnorm_seg_bwd_frozen(*common, S, c_rows, D, code, int(relu),
                                                 accumulate, ws.data_ptr(), wsb, None)
    elif entry == "max":
        rc = lib.molclr_batchnorm_seg_bwd_frozen_max(*common, S, c_rows, D, int(relu), accumulate,
                                                     rm.data_ptr(), slot.data_ptr(), ws.data_ptr(),
                                                     wsb, None)
    else:
        rows_dev = torch.tensor(list(rows), dtype=torch.long, device=dev)
        rc = lib.molclr_batchnorm_seg_bwd_frozen_dev(*common, S, rows_dev.data_ptr(), N, D, code,
                                                     int(relu), accumulate, _lib.ptr(rm),
                                                     _lib.ptr(slot), ws.data_ptr(), wsb, None)
    assert rc == 0, lib.molclr_last_error()
    torch.cuda.synchronize()
    assert guard_ok(dz, N * D) and guard_ok(dg, D) and guard_ok(db, D), "guard bytes written"
    if rowmax:
        assert guard_ok(rm, nparts * N), "row-parts guard written"
    out = (dz[:N * D].view(N, D), dg[:D], db[:D])
    return out + ((rm[:nparts * N].view(nparts, N), slot) if rowmax else ())


def f64(t):
    return t.detach().float().cpu().double().numpy()


def check(name, got, ref, bound):
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), name + ": non-finite output"
    err = np.abs(got - ref)
    ratio = np.where(err == 0.0, 0.0, err / np.where(bound > 0, bound, 1e-300))
    r = float(ratio.max()) if ratio.size else 0.0
    print("%-8s worst |err| / derived bound = %.3f" % (name, r))
    assert r <= SLACK, (name, r, np.unravel_index(np.argmax(ratio), ratio.shape))


def check_all(out, z, dy, gamma, beta, mean, invstd, seg, relu, bf16, nseg, init=None):
    dz, dg, db = out[:3]
    n = z.shape[0]
    dz_ref, db_ref, dg_ref, sa, sb = reference(z, dy, gamma, beta, mean, invstd, seg, relu)
    if init is not None:
        dg_ref, db_ref = dg_ref + init[0], db_ref + init[1]
        sb, sa = sb + np.abs(init[0]), sa + np.abs(init[1])
    check("dz", f64(dz), dz_ref, (2 * U + (UB if bf16 else 0.0)) * np.abs(dz_ref))
    check("dbeta", f64(db), db_ref, (n + nseg + 1) * U * sa)
    check("dgamma", f64(dg), dg_ref, (n + nseg + 4) * U * sb)


WIDTHS = [(4, False), (12, False), (300, False), (512, False), (8, True), (304, True), (512, True)]


@gpu
@pytest.mark.parametrize("D,bf16", WIDTHS)
@pytest.mark.parametrize("rows", [1, 3, 257, "edge"])
def test_frozen_one_segment(dev, D, bf16, rows):
    """One segment (a one-row segment included), ReLU on and off, accumulate 0
    and 1 with guard elements after every output; `edge` is one row more than a
    partition of the band plan holds, so two partitions, the second with one
    row.  A second run must repeat the first bit for bit."""
    n = band_unit(D) + 1 if rows == "edge" else rows
    for relu in (0, 1):
        for acc in (0, 1):
            case = make_case((n,), D, relu, bf16, 7 * n + D + relu)
            z, dy, gamma, beta, mean, invstd, seg = case
            rng = np.random.default_rng(n + D)
            init = (rng.standard_normal(D).astype(F32), rng.standard_normal(D).astype(F32)) if acc else None
            out = call_frozen(dev, z, dy, gamma, beta, mean, invstd, (n,), relu, acc, bf16, init)
            check_all(out, z, dy, gamma, beta, mean, invstd, seg, relu, bf16, 1, init)
            again = call_frozen(dev, z, dy, gamma, beta, mean, invstd, (n,), relu, acc, bf16, init)
            assert all(torch.equal(a, b) for a, b in zip(out, again))
            if not bf16 and not acc:
                plain = call_frozen(dev, z, dy, gamma, beta, mean, invstd, (n,), relu, 0, False,
                                    None, entry="plain")
                assert all(torch.equal(a, b) for a, b in zip(out, plain))


@gpu
@pytest.mark.parametrize("D,bf16", WIDTHS)
def test_frozen_two_segments_and_device_plan(dev, D, bf16):
    """Two segments with different saved statistics, host-sized; then the same
    segments device-sized over a capacity with padding rows and spare
    partitions.  The padding's dy and z are NaN: its dz is exactly 0 and the
    sums are the host-sized call's, bit for bit (the same plan per segment)."""
    u = band_unit(D)
    rows = (u + 2, 5)
    for relu in (0, 1):
        z, dy, gamma, beta, mean, invstd, seg = make_case(rows, D, relu, bf16, 31 + D + relu)
        host = call_frozen(dev, z, dy, gamma, beta, mean, invstd, rows, relu, 0, bf16)
        check_all(host, z, dy, gamma, beta, mean, invstd, seg, relu, bf16, 2)
        n = sum(rows)
        cap = n + 2 * u + 3  # padding rows; the bound on the partitions leaves spare ones
        zp = np.full((cap, D), np.nan, dtype=F32)
        dyp = np.full((cap, D), np.nan, dtype=F32)
        zp[:n], dyp[:n] = z, dy
        devp = call_frozen(dev, zp, dyp, gamma, beta, mean, invstd, rows, relu, 0, bf16,
                           entry="dev", cap=cap)
        assert torch.equal(devp[0][:n], host[0])
        assert bool((devp[0][n:] == 0).all().item()), "padding dz must be exactly 0"
        assert torch.equal(devp[1], host[1]) and torch.equal(devp[2], host[2])


@gpu
@pytest.mark.parametrize("D", [4, 12, 300, 512])
def test_frozen_max_variant(dev, D):
    """_max: the row parts fold to the row-wise abs().max() of the dz it
    stored, the slot to its global one, bit for bit; dz, dgamma and dbeta equal
    the plain variant's.  Host-sized (two segments) and device-sized with
    padding rows, whose row parts are 0."""
    u = band_unit(D)
    for rows in ((1,), (3,), (u + 2, 5)):
        z, dy, gamma, beta, mean, invstd, seg = make_case(rows, D, 1, False, 99 + D + sum(rows))
        plain = call_frozen(dev, z, dy, gamma, beta, mean, invstd, rows, 1)
        mx = call_frozen(dev, z, dy, gamma, beta, mean, invstd, rows, 1, entry="max", rowmax=True)
        assert all(torch.equal(a, b) for a, b in zip(plain, mx[:3]))
        assert torch.equal(mx[3].max(0).values, mx[0].abs().max(1).values)
        assert torch.equal(mx[4].max(), mx[0].abs().max())
        n = sum(rows)
        cap = n + u + 3
        zp = np.full((cap, D), np.nan, dtype=F32)
        dyp = np.full((cap, D), np.nan, dtype=F32)
        zp[:n], dyp[:n] = z, dy
        dv = call_frozen(dev, zp, dyp, gamma, beta, mean, invstd, rows, 1, entry="dev", cap=cap,
                         rowmax=True)
        assert torch.equal(dv[0][:n], plain[0]) and bool((dv[0][n:] == 0).all().item())
        assert torch.equal(dv[3].max(0).values, dv[0].abs().max(1).values)
        assert bool((dv[3][:, n:] == 0).all().item())
        assert torch.equal(dv[4].max(), plain[0].abs().max())


@gpu
@pytest.mark.parametrize("D,bf16", [(12, False), (300, False), (8, True), (304, True)])
def test_frozen_exact(dev, D, bf16):
    """dy integers in [-8, 8], gamma and invstd powers of two, mean, beta and z
    integers: every product and every partial sum is an integer multiple of a
    power of two below 2^24, so dz, dbeta and dgamma are exact."""
    rng = np.random.default_rng(D)
    rows = (band_unit(D) + 3, 2)
    n, S = sum(rows), 2
    gamma = (2.0 ** rng.integers(-2, 3, D)).astype(F32) * np.where(rng.random(D) < 0.5, -1, 1).astype(F32)
    beta = rng.integers(1, 4, D).astype(F32)
    mean = rng.integers(-3, 4, (S, D)).astype(F32)
    invstd = (2.0 ** rng.integers(-2, 2, (S, D))).astype(F32)
    z = rng.integers(-6, 7, (n, D)).astype(F32)
    dy = rng.integers(-8, 9, (n, D)).astype(F32)
    seg = np.repeat(np.arange(S), rows)
    for relu in (0, 1):
        dz_ref, db_ref, dg_ref, _, _ = reference(z, dy, gamma, beta, mean, invstd, seg, relu)
        dz, dg, db = call_frozen(dev, z, dy, gamma, beta, mean, invstd, rows, relu, 0, bf16)
        dt = torch.bfloat16 if bf16 else torch.float32
        want = torch.from_numpy(dz_ref).to(dt)
        assert torch.equal(want.double(), torch.from_numpy(dz_ref)), "the case must be exact"
        assert torch.equal(dz.cpu(), want)
        assert torch.equal(db.cpu(), torch.from_numpy(db_ref).float())
        assert torch.equal(dg.cpu(), torch.from_numpy(dg_ref).float())


@gpu
def test_ops_batch_norm_eval_backward(dev):
    """ops.batch_norm in eval mode differentiates (it raised before): the
    gradients of an fp64 torch BatchNorm1d in eval mode, under the bounds above;
    running statistics untouched."""
    from molclr_amd import ops
    torch.manual_seed(0)
    n, D = 70, 12
    bn = torch.nn.BatchNorm1d(D).to(dev)
    with torch.no_grad():
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(0.1, 0.5)
    bn.eval()
    before = [t.clone() for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    z = torch.randn(n, D, device=dev, requires_grad=True)
    dy = torch.randn(n, D, device=dev)
    ops.batch_norm(z, bn, relu=True).backward(dy)
    ref = torch.nn.BatchNorm1d(D).double()
    ref.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.cpu()
                         for k, v in bn.state_dict().items()})
    ref.eval()
    z64 = z.detach().cpu().double().requires_grad_(True)
    torch.relu(ref(z64)).backward(dy.cpu().double())
    assert torch.allclose(z.grad.cpu().double(), z64.grad, rtol=1e-5, atol=1e-6)
    assert torch.allclose(bn.weight.grad.cpu().double(), ref.weight.grad, rtol=1e-5, atol=1e-5)
    assert torch.allclose(bn.bias.grad.cpu().double(), ref.bias.grad, rtol=1e-5, atol=1e-5)
    after = (bn.running_mean, bn.running_var, bn.num_batches_tracked)
    assert all(torch.equal(a, b) for a, b in zip(before, after))


@gpu
def test_workspace_one_byte_short_is_refused(dev):
    """The forward, the backward and the frozen backward, each with real
    tensors and a workspace one byte below the query's answer: every one
    returns MOLCLR_ERR_WORKSPACE and leaves its outputs, prefilled with a
    sentinel, untouched."""
    lib = _lib.load()
    rows, D = (37, 61), 12
    N, S = sum(rows), len(rows)
    z, dy, gamma, beta, mean, invstd, _ = make_case(rows, D, 1, False, 5)
    zd, dyd = torch.from_numpy(z).to(dev), torch.from_numpy(dy).to(dev)
    gd, bd = torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev)
    md, sd = torch.from_numpy(mean).to(dev), torch.from_numpy(invstd).to(dev)
    c_rows = (ctypes.c_int64 * S)(*rows)
    wsb = int(lib.molclr_batchnorm_seg_workspace_bytes(S, c_rows, D))
    assert wsb > 1
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)

    def sent(*shape, dtype=torch.float32):
        return torch.full(shape, int(SENT) if dtype == torch.long else SENT, dtype=dtype,
                          device=dev)

    y, smean, sinv, rmean, rvar = sent(N, D), sent(S, D), sent(S, D), sent(D), sent(D)
    nbt = sent(1, dtype=torch.long)
    rc = lib.molclr_batchnorm_seg_fwd(zd.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                      rmean.data_ptr(), rvar.data_ptr(), nbt.data_ptr(),
                                      y.data_ptr(), smean.data_ptr(), sinv.data_ptr(), S, c_rows,
                                      D, _lib.DTYPE_F32, 0.1, 1e-5, 1, 1, ws.data_ptr(), wsb - 1,
                                      None)
    assert rc == -2, (rc, lib.molclr_last_error())  # MOLCLR_ERR_WORKSPACE
    outs = [y, smean, sinv, rmean, rvar, nbt]
    for entry in ("molclr_batchnorm_seg_bwd", "molclr_batchnorm_seg_bwd_frozen"):
        dz, dg, db = sent(N, D), sent(D), sent(D)
        rc = getattr(lib, entry)(dyd.data_ptr(), zd.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                 md.data_ptr(), sd.data_ptr(), dz.data_ptr(), dg.data_ptr(),
                                 db.data_ptr(), S, c_rows, D, _lib.DTYPE_F32, 1, 0, ws.data_ptr(),
                                 wsb - 1, None)
        assert rc == -2, (entry, rc, lib.molclr_last_error())
        outs += [dz, dg, db]
    torch.cuda.synchronize()
    assert all(bool((t == int(SENT)).all().item()) for t in outs), "a refused call wrote an output"
