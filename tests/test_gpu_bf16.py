"""The bf16 path (BASELINE config c5: GIN 5 x 512, bf16 with fp32 accumulation).

Kernel level, each against float64 on the same bf16-rounded inputs:
* molclr_gemm_bf16 (all epilogues): the fp32-accumulated product, rounded once
  to bf16 -- norm-wise within 2^-8 of the exact result;
* molclr_linear_wgrad_bf16: fp32 outputs within 1e-5 of float64;
* aggregation, atom embedding, pooling: bit-exact against the fp32 kernels run
  on the same (bf16-representable) values and rounded to bf16 (same fp32 adds,
  one rounding);
* segmented BatchNorm in bf16 storage: statistics within 1e-5, outputs within
  bf16 rounding;
* the kernels that do arithmetic and then store bf16 (the products, BatchNorm
  forward and backward) held to CORRECT rounding by tests/rounding.py
  (test_*_rounding): every element in the window of one round-to-nearest-even
  of the fp32-accumulated result, at most 0.5 % of them off RNE_bf16(fp64
  result), no rounding bias -- which truncation, rounding twice or one wrong
  tail path miss, and the norm-wise 2^-8 above does not.
Model level: GINet(precision='bf16') against the fp64 oracle of the reference
(oracle/reference_cpu.py) -- the stated bf16 tolerances (BF16_TOL) below."""
import copy

import numpy as np
import pytest
import torch

from molclr_amd import _lib, ops
from molclr_amd.data import DeviceGraph
from molclr_amd.dataset import SyntheticPairBatches

from . import rounding as R

pytestmark = pytest.mark.gpu
TOL = 1e-5
EPS_BF16 = 2.0 ** -8  # one bf16 rounding, relative
# Model-level tolerances of the bf16 path vs the fp64 reference (norm-wise).
# Forward: node embeddings / projections carry ~5 layers of bf16 activation
# rounding (2^-9 relative each).  Gradients: at random init the step's
# gradients are ill-conditioned (the projections of different molecules are
# nearly parallel, so NT-Xent's gradient is a small difference of large
# terms; the fp32 path already lands 1.5e-3 from fp64 at c2, test_gpu_models)
# and bf16 activations amplify the same way: measured 0.17-0.22 norm-wise on
# the worst parameter (cosine > 0.97).  The bound is a gross-error guard (a
# wrong operand or transposition gives >= 1); the kernels themselves are held
# to exactness above.
BF16_TOL = {"h": 3e-2, "out": 3e-2, "loss": 1e-2, "grad": 0.35}


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return (a - b).norm().item() / max(b.norm().item(), 1e-30)


def bf(t):
    return t.to(torch.bfloat16)


@pytest.mark.parametrize("M,N,K", [(1000, 1024, 512), (1000, 512, 1024), (333, 256, 64),
                                   (4096, 1024, 512), (37, 96, 40), (500, 512, 1000),
                                   # > 256 tiles: persistent blocks (impl 8) walk several,
                                   # with partial row / column tiles among them
                                   (20000, 1024, 512), (17001, 1000, 128)])
def test_gemm_bf16(dev, M, N, K):
    from molclr_amd._lib import EPI_BIAS, EPI_BIAS_RELU, EPI_NONE, EPI_RELU_MASK
    lib = _lib.load()
    torch.manual_seed(M + N + K)
    A = bf(torch.randn(M, K))
    W = torch.randn(N, K)
    b = torch.randn(N)
    aux = bf(torch.randn(M, N))
    Ad, Wd, bd, auxd = A.to(dev), W.to(dev), b.to(dev), aux.to(dev)
    planes = ops.weight_planes(Wd, N, K, K, 0)
    y = A.double() @ bf(W).double().t()  # plane 0 is the RNE bf16 of the weight
    cases = {EPI_NONE: y, EPI_BIAS: y + b.double(), EPI_BIAS_RELU: (y + b.double()).clamp(min=0),
             EPI_RELU_MASK: y * (aux.double() > 0)}
    for epi, ref in cases.items():
        C = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        assert lib.molclr_gemm_bf16(Ad.data_ptr(), planes.data_ptr(), C.data_ptr(), M, N, K, K, N,
                                    epi, bd.data_ptr(), auxd.data_ptr(), N, None) == 0
        assert rel(C, ref) < EPS_BF16, epi
    # transposed weight operand (the data-gradient product dy W)
    Wt = torch.randn(K, N)
    planes_t = ops.weight_planes(Wt.to(dev), N, K, N, 1)
    C = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    assert lib.molclr_gemm_bf16(Ad.data_ptr(), planes_t.data_ptr(), C.data_ptr(), M, N, K, K, N,
                                EPI_NONE, None, None, 0, None) == 0
    assert rel(C, A.double() @ bf(Wt).double()) < EPS_BF16
    # every tile shape: the same result bits (one wave's MFMA chain per output
    # element, in the same k order)
    for epi in (EPI_BIAS_RELU, EPI_RELU_MASK):
        outs = []
        for impl in (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9):
            C = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            assert lib.molclr_gemm_bf16_impl(Ad.data_ptr(), planes.data_ptr(), C.data_ptr(), M, N,
                                             K, K, N, epi, bd.data_ptr(), auxd.data_ptr(), N, None,
                                             impl) == 0
            outs.append(C)
        assert rel(outs[0], cases[epi]) < EPS_BF16
        for impl, C in enumerate(outs[1:]):
            assert torch.equal(C, outs[0]), (epi, impl)


@pytest.mark.parametrize("M,N,K", [(1000, 1024, 512), (20000, 1024, 512), (333, 1000, 64),
                                   (17001, 96, 128), (55342, 1024, 512)])
def test_gemm_bf16_bits(dev, M, N, K):
    """molclr_gemm_bf16_bits: the bias+ReLU product writes the ReLU mask as
    column-block-major bits (bit n % 32 of word [n / 32][m] = C > 0), and the
    ReLU-mask product given those bits equals the aux form bit for bit."""
    from molclr_amd._lib import EPI_BIAS_RELU, EPI_RELU_MASK
    lib = _lib.load()
    torch.manual_seed(M + N)
    A = bf(torch.randn(M, K)).to(dev)
    W = torch.randn(N, K, device=dev)
    b = torch.randn(N, device=dev)
    dz = bf(torch.randn(M, K)).to(dev)
    Wt = torch.randn(K, N, device=dev)
    planes = ops.weight_planes(W, N, K, K, 0)
    planes_t = ops.weight_planes(Wt, N, K, N, 1)
    nw = (N + 31) // 32
    bits = torch.full((nw, M), -1, dtype=torch.int32, device=dev)
    C1 = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    C0 = torch.empty_like(C1)
    assert lib.molclr_gemm_bf16_bits(A.data_ptr(), planes.data_ptr(), C1.data_ptr(), M, N, K, K, N,
                                     EPI_BIAS_RELU, b.data_ptr(), bits.data_ptr(), None, None) == 0
    assert lib.molclr_gemm_bf16_impl(A.data_ptr(), planes.data_ptr(), C0.data_ptr(), M, N, K, K, N,
                                     EPI_BIAS_RELU, b.data_ptr(), None, 0, None, 8) == 0
    torch.cuda.synchronize()
    assert torch.equal(C1, C0)
    pos = torch.zeros(M, nw * 32, dtype=torch.bool, device=dev)
    pos[:, :N] = C1.float() > 0
    w = (pos.view(M, nw, 32).long() << torch.arange(32, device=dev)).sum(2)  # [M, nw]
    want = w.t().contiguous().to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(bits.to(torch.int64) & 0xFFFFFFFF, want)
    D1 = torch.empty_like(C1)
    D0 = torch.empty_like(C1)
    assert lib.molclr_gemm_bf16_bits(dz.data_ptr(), planes_t.data_ptr(), D1.data_ptr(), M, N, K, K,
                                     N, EPI_RELU_MASK, None, None, bits.data_ptr(), None) == 0
    assert lib.molclr_gemm_bf16_impl(dz.data_ptr(), planes_t.data_ptr(), D0.data_ptr(), M, N, K, K,
                                     N, EPI_RELU_MASK, None, C1.data_ptr(), N, None, 8) == 0
    torch.cuda.synchronize()
    assert torch.equal(D1, D0)
    assert rel(D1, (dz.double() @ bf(Wt).double()) * (C1.double() > 0)) < EPS_BF16


@pytest.mark.parametrize("rows,n_out,n_in", [(55000, 1024, 512), (55000, 512, 1024), (777, 64, 128),
                                             (8, 8, 16), (4096, 512, 256), (3001, 264, 520)])
@pytest.mark.parametrize("acc", [0, 1])
def test_linear_wgrad_bf16(dev, rows, n_out, n_in, acc):
    lib = _lib.load()
    torch.manual_seed(rows + n_out)
    dy, x = bf(torch.randn(rows, n_out)), bf(torch.randn(rows, n_in))
    W0, b0 = torch.randn(n_out, n_in), torch.randn(n_out)
    dW, db = W0.clone().to(dev), b0.clone().to(dev)
    ws_bytes = lib.molclr_linear_wgrad_bf16_workspace_bytes(rows, n_out, n_in)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    dyd, xd = dy.to(dev), x.to(dev)
    assert lib.molclr_linear_wgrad_bf16(dyd.data_ptr(), xd.data_ptr(), dW.data_ptr(), db.data_ptr(),
                                        rows, n_out, n_in, n_out, n_in, acc, ws.data_ptr(),
                                        ws_bytes, None) == 0
    refW = dy.double().t() @ x.double() + (W0.double() if acc else 0)
    refb = dy.double().sum(0) + (b0.double() if acc else 0)
    assert rel(dW, refW) < TOL and rel(db, refb) < TOL
    dW2 = torch.empty(n_out, n_in, device=dev)
    assert lib.molclr_linear_wgrad_bf16(dyd.data_ptr(), xd.data_ptr(), dW2.data_ptr(), None, rows,
                                        n_out, n_in, n_out, n_in, 0, ws.data_ptr(), ws_bytes,
                                        None) == 0
    assert rel(dW2, dy.double().t() @ x.double()) < TOL
    for impl in (0, 1, 2, 3):  # every kernel / tile shape and its split-K plan
        dW3, db3 = W0.clone().to(dev), b0.clone().to(dev)
        assert lib.molclr_linear_wgrad_bf16_impl(dyd.data_ptr(), xd.data_ptr(), dW3.data_ptr(),
                                                 db3.data_ptr(), rows, n_out, n_in, n_out, n_in,
                                                 acc, ws.data_ptr(), ws_bytes, None, impl) == 0
        assert rel(dW3, refW) < TOL and rel(db3, refb) < TOL, impl


def test_bf16_aggregation_atom_pool_bit_exact(dev):
    """bf16 storage, fp32 arithmetic: equal to the fp32 kernels on the same
    values, rounded once (same adds in the same order)."""
    lib = _lib.load()
    b = SyntheticPairBatches(200, seed=7, shape="pubchem").next()[0]
    g = DeviceGraph(b.edge_index.to(dev), b.edge_attr.to(dev), b.x.shape[0], b.batch.to(dev),
                    b.num_graphs)
    N, D = b.x.shape[0], 512
    torch.manual_seed(0)
    hb = bf(torch.randn(N, D)).to(dev)
    Ec = torch.randn(15, D).to(dev)
    out_b = torch.empty(N, D, dtype=torch.bfloat16, device=dev)
    out_f = torch.empty(N, D, device=dev)
    hf = hb.float()
    args = (g.rowptr.data_ptr(), g.col.data_ptr(), g.ecode.data_ptr(), g.nbr.data_ptr(),
            Ec.data_ptr())
    assert lib.molclr_gine_aggregate_fwd_bf16(hb.data_ptr(), *args, out_b.data_ptr(), N, D, None) == 0
    assert lib.molclr_gine_aggregate_fwd(hf.data_ptr(), *args, out_f.data_ptr(), N, D, None) == 0
    assert torch.equal(out_b, bf(out_f))
    # backward: transpose gather (bit-exact) and edge-table gradients (fp64 partials)
    gb = bf(torch.randn(N, D)).to(dev)
    dxb = torch.empty(N, D, dtype=torch.bfloat16, device=dev)
    dxf = torch.empty(N, D, device=dev)
    e1b, e2b = torch.empty(5, D, device=dev), torch.empty(3, D, device=dev)
    e1f, e2f = torch.empty(5, D, device=dev), torch.empty(3, D, device=dev)
    wsb = lib.molclr_gine_aggregate_bwd_workspace_bytes(N, D)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    bargs = (g.rowptr_t.data_ptr(), g.col_t.data_ptr(), g.nbr_t.data_ptr(), g.ecount.data_ptr())
    assert lib.molclr_gine_aggregate_bwd_bf16(gb.data_ptr(), *bargs, dxb.data_ptr(), e1b.data_ptr(),
                                              e2b.data_ptr(), N, D, 0, ws.data_ptr(), wsb, None) == 0
    gf = gb.float()
    assert lib.molclr_gine_aggregate_bwd(gf.data_ptr(), *bargs, dxf.data_ptr(), e1f.data_ptr(),
                                         e2f.data_ptr(), N, D, 0, ws.data_ptr(), wsb, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dxb, bf(dxf)) and torch.equal(e1b, e1f) and torch.equal(e2b, e2f)
    # atom embedding (one fp32 add, rounded) and its table gradients
    X1, X2 = torch.randn(119, D).to(dev), torch.randn(3, D).to(dev)
    xi = b.x.to(dev)
    hb2 = torch.empty(N, D, dtype=torch.bfloat16, device=dev)
    assert lib.molclr_atom_embed_fwd_bf16(xi.data_ptr(), X1.data_ptr(), X2.data_ptr(),
                                          hb2.data_ptr(), N, D, 119, 3, None, None) == 0
    assert torch.equal(hb2, bf(X1[xi[:, 0]] + X2[xi[:, 1]]))
    wsa = lib.molclr_atom_embed_bwd_workspace_bytes(N, D, 119, 3)
    wa = torch.empty(wsa, dtype=torch.uint8, device=dev)
    d1b, d2b = torch.empty(119, D, device=dev), torch.empty(3, D, device=dev)
    d1f, d2f = torch.empty(119, D, device=dev), torch.empty(3, D, device=dev)
    assert lib.molclr_atom_embed_bwd_bf16(xi.data_ptr(), gb.data_ptr(), d1b.data_ptr(),
                                          d2b.data_ptr(), N, D, 119, 3, 0, wa.data_ptr(), wsa,
                                          None) == 0
    assert lib.molclr_atom_embed_bwd(xi.data_ptr(), gf.data_ptr(), d1f.data_ptr(), d2f.data_ptr(),
                                     N, D, 119, 3, 0, wa.data_ptr(), wsa, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(d1b, d1f) and torch.equal(d2b, d2f)
    # pooling: bf16 in, fp32 out (== fp32 pooling of the same values); bf16 gradient
    pb, pf = torch.empty(b.num_graphs, D, device=dev), torch.empty(b.num_graphs, D, device=dev)
    for mode in (0, 1):
        assert lib.molclr_segment_pool_fwd_bf16(hb.data_ptr(), g.graph_ptr.data_ptr(), pb.data_ptr(),
                                                b.num_graphs, D, mode, None) == 0
        assert lib.molclr_segment_pool_fwd(hf.data_ptr(), g.graph_ptr.data_ptr(), pf.data_ptr(),
                                           b.num_graphs, D, mode, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(pb, pf)
        dhb = torch.empty(N, D, dtype=torch.bfloat16, device=dev)
        dhf = torch.empty(N, D, device=dev)
        assert lib.molclr_segment_pool_bwd_bf16(pf.data_ptr(), g.graph_ptr.data_ptr(), dhb.data_ptr(),
                                                N, b.num_graphs, D, mode, None) == 0
        assert lib.molclr_segment_pool_bwd(pf.data_ptr(), g.graph_ptr.data_ptr(), dhf.data_ptr(), N,
                                           b.num_graphs, D, mode, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(dhb, bf(dhf))


def test_batchnorm_bf16_segments(dev):
    import ctypes
    lib = _lib.load()
    rows, D = (13000, 14000), 512
    N = sum(rows)
    torch.manual_seed(5)
    z = bf(torch.randn(N, D) * 2 + 1).to(dev)
    gamma, beta = (torch.rand(D) + 0.5).to(dev), torch.randn(D).to(dev)
    seg = (ctypes.c_int64 * 2)(*rows)
    wsb = lib.molclr_batchnorm_seg_workspace_bytes(2, seg, D)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rm, rv = torch.zeros(D, device=dev), torch.ones(D, device=dev)
    y = torch.empty(N, D, dtype=torch.bfloat16, device=dev)
    sm, si = torch.empty(2, D, device=dev), torch.empty(2, D, device=dev)
    assert lib.molclr_batchnorm_seg_fwd(z.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
                                        rv.data_ptr(), None, y.data_ptr(), sm.data_ptr(),
                                        si.data_ptr(), 2, seg, D, 1, 0.1, 1e-5, 1, 1, ws.data_ptr(),
                                        wsb, None) == 0
    zf = z.float().cpu()
    r0 = 0
    rm_ref, rv_ref = torch.zeros(D), torch.ones(D)
    for s, r in enumerate(rows):
        bn = torch.nn.BatchNorm1d(D)
        bn.running_mean.copy_(rm_ref)
        bn.running_var.copy_(rv_ref)
        with torch.no_grad():
            bn.weight.copy_(gamma.cpu())
            bn.bias.copy_(beta.cpu())
            yr = torch.relu(bn(zf[r0:r0 + r].clone()))
        rm_ref, rv_ref = bn.running_mean.clone(), bn.running_var.clone()
        assert rel(y[r0:r0 + r], yr) < EPS_BF16
        assert rel(sm[s], zf[r0:r0 + r].double().mean(0)) < TOL
        r0 += r
    assert rel(rm, rm_ref) < TOL and rel(rv, rv_ref) < TOL


def _figures(what, rep):
    """The figures behind check_bf16_rounded, one line per checked output (pytest -s)."""
    print(f"rounding {what}: share_off={rep['share_off']:.3e} mean_d={rep['mean_d']:+.5f} "
          f"(bound {rep['bias_bound']:.5f}, n={rep['n_bias']}) outside={rep['outside_window']}")


_QB_IMPLS = (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9)  # as test_gemm_bf16


@pytest.mark.parametrize("M,N,K", R.SHAPES)
def test_gemm_bf16_rounding(dev, M, N, K):
    """molclr_gemm_bf16: every epilogue and the K-major weight operand, through
    EVERY tile shape (each impl against the fp64 reference, not against impl
    -1), rounds the fp32-accumulated result once, to nearest even.  Shapes:
    partial row and column tiles, K off the K step, one small tile."""
    from molclr_amd._lib import EPI_BIAS, EPI_BIAS_RELU, EPI_NONE, EPI_RELU_MASK
    lib = _lib.load()
    A, W, Wt, b, aux = R.gemm_case(M, N, K)
    Ad, bd, auxd = bf(A).to(dev), b.to(dev), bf(aux).to(dev)
    planes = ops.weight_planes(W.to(dev), N, K, K, 0)    # plane 0 = W (bf16-valued already)
    planes_t = ops.weight_planes(Wt.to(dev), N, K, N, 1)
    y, mag = R.gemm_ref(A, W)
    yb, magb = R.gemm_ref(A, W, b)
    keep = (aux > 0).double()
    # a ReLU clamps the reference: an element whose window straddles 0 may be 0
    # or the rounded value, both inside [RNE(ref - e), RNE(ref + e)]
    cases = {EPI_NONE: (y, mag), EPI_BIAS: (yb, magb), EPI_BIAS_RELU: (yb.clamp(min=0), magb),
             EPI_RELU_MASK: (y * keep, mag * keep)}
    yt, magt = R.gemm_ref(A, Wt.t())
    for impl in _QB_IMPLS:
        for epi, (ref, m) in cases.items():
            C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
            assert lib.molclr_gemm_bf16_impl(Ad.data_ptr(), planes.data_ptr(), C.data_ptr(), M, N,
                                             K, K, N, epi, bd.data_ptr(), auxd.data_ptr(), N, None,
                                             impl) == 0, lib.molclr_last_error()
            what = f"gemm_bf16 {M}x{N}x{K} impl {impl} epi {epi}"
            _figures(what, R.check_bf16_rounded(C, ref, m, R.GEMM_SLACK, what=what))
        C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
        assert lib.molclr_gemm_bf16_impl(Ad.data_ptr(), planes_t.data_ptr(), C.data_ptr(), M, N, K,
                                         K, N, EPI_NONE, None, None, 0, None, impl) == 0
        what = f"gemm_bf16 {M}x{N}x{K} impl {impl} K-major"
        _figures(what, R.check_bf16_rounded(C, yt, magt, R.GEMM_SLACK, what=what))
    # the plain entry point is the automatic choice
    C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    assert lib.molclr_gemm_bf16(Ad.data_ptr(), planes.data_ptr(), C.data_ptr(), M, N, K, K, N,
                                EPI_BIAS, bd.data_ptr(), None, 0, None) == 0
    R.check_bf16_rounded(C, yb, magb, R.GEMM_SLACK, what="gemm_bf16 plain")


@pytest.mark.parametrize("M,N,K", [s for s in R.SHAPES if s[2] % 64 == 0])  # the entry's K % 64
def test_gemm_bf16_bits_rounding(dev, M, N, K):
    """molclr_gemm_bf16_bits: the bias+ReLU output and the product masked by
    its bits are once-rounded results; the bits equal C > 0."""
    from molclr_amd._lib import EPI_BIAS_RELU, EPI_RELU_MASK
    lib = _lib.load()
    A, W, Wt, b, _ = R.gemm_case(M, N, K)
    dz = R.gemm_case(M, N, K, seed=M + N + K + 1)[0]
    planes = ops.weight_planes(W.to(dev), N, K, K, 0)
    planes_t = ops.weight_planes(Wt.to(dev), N, K, N, 1)
    Ad, dzd, bd = bf(A).to(dev), bf(dz).to(dev), b.to(dev)
    nw = (N + 31) // 32
    bits = torch.full((nw, M), -1, dtype=torch.int32, device=dev)
    C1 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    assert lib.molclr_gemm_bf16_bits(Ad.data_ptr(), planes.data_ptr(), C1.data_ptr(), M, N, K, K, N,
                                     EPI_BIAS_RELU, bd.data_ptr(), bits.data_ptr(), None, None) == 0
    yb, magb = R.gemm_ref(A, W, b)
    what = f"gemm_bf16_bits {M}x{N}x{K} bias+relu"
    _figures(what, R.check_bf16_rounded(C1, yb.clamp(min=0), magb, R.GEMM_SLACK, what=what))
    pos = torch.zeros(M, nw * 32, dtype=torch.bool, device=dev)
    pos[:, :N] = C1.float() > 0
    w = (pos.view(M, nw, 32).long() << torch.arange(32, device=dev)).sum(2)  # [M, nw]
    want = w.t().contiguous().to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(bits.to(torch.int64) & 0xFFFFFFFF, want)
    D1 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
    assert lib.molclr_gemm_bf16_bits(dzd.data_ptr(), planes_t.data_ptr(), D1.data_ptr(), M, N, K, K,
                                     N, EPI_RELU_MASK, None, None, bits.data_ptr(), None) == 0
    keep = (C1.float() > 0).double().cpu()  # the mask the bits hold (checked above)
    yt, magt = R.gemm_ref(dz, Wt.t())
    what = f"gemm_bf16_bits {M}x{N}x{K} mask from bits"
    _figures(what, R.check_bf16_rounded(D1, yt * keep, magt * keep, R.GEMM_SLACK, what=what))


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("rows,D", R.BN_CASES)
def test_batchnorm_bf16_rounding(dev, rows, D, relu):
    """Segmented BatchNorm in bf16 storage against fp64 on the same bf16
    inputs: the forward's y and the backward's dz once-rounded (dz had no fp64
    comparison before), dgamma / dbeta within 1e-5.  Magnitude sums (the
    absolute values of the terms of the fp64 formulas; rounding.bn_fwd_ref /
    bn_bwd_ref):
        y  = gamma (z - mean) invstd + beta
        mag_y  = |gamma| invstd (|z| + |mean|) + |beta|
        dz = gamma invstd (g - mean_rows(g) - xhat mean_rows(g xhat)),  g = dy [y > 0]
        mag_dz = |gamma| invstd (|g| + mean_rows|g| + X mean_rows(|g| X)),
                 X = (|z| + |mean|) invstd.
    The backward's ReLU mask is the kernels' own y > 0 (fp64 autograd through
    BatchNorm times that constant mask); it may differ from the fp64 y > 0
    only where the forward's window straddles 0."""
    import ctypes
    lib = _lib.load()
    n = sum(rows)
    z, dy, gamma, beta = R.bn_case(rows, D)
    zd, dyd, gd, bd = bf(z).to(dev), bf(dy).to(dev), gamma.to(dev), beta.to(dev)
    seg = (ctypes.c_int64 * len(rows))(*rows)
    wsb = lib.molclr_batchnorm_seg_workspace_bytes(len(rows), seg, D)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rm, rv = torch.zeros(D, device=dev), torch.ones(D, device=dev)
    y = torch.full((n, D), float("nan"), dtype=torch.bfloat16, device=dev)
    sm, si = torch.empty(len(rows), D, device=dev), torch.empty(len(rows), D, device=dev)
    assert lib.molclr_batchnorm_seg_fwd(zd.data_ptr(), gd.data_ptr(), bd.data_ptr(), rm.data_ptr(),
                                        rv.data_ptr(), None, y.data_ptr(), sm.data_ptr(),
                                        si.data_ptr(), len(rows), seg, D, _lib.DTYPE_BF16, 0.1, 1e-5,
                                        1, relu, ws.data_ptr(), wsb, None) == 0
    y64, mag, mean64, inv64 = R.bn_fwd_ref(z, gamma, beta, rows)
    assert rel(sm, mean64) < TOL and rel(si, inv64) < TOL
    what = f"batchnorm fwd rows {rows} D {D} relu {relu}"
    _figures(what, R.check_bf16_rounded(y, y64.clamp(min=0) if relu else y64, mag,
                                        R.BN_FWD_SLACK, what=what))
    mask = None
    if relu:
        mask = (y.float() > 0).cpu()
        flipped = mask != (y64 > 0)
        assert bool((y64.abs()[flipped] <= R.BN_FWD_SLACK * R.U32 * mag[flipped]).all())
    dz = torch.full((n, D), float("nan"), dtype=torch.bfloat16, device=dev)
    dg, db = torch.empty(D, device=dev), torch.empty(D, device=dev)
    assert lib.molclr_batchnorm_seg_bwd(dyd.data_ptr(), zd.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                        sm.data_ptr(), si.data_ptr(), dz.data_ptr(), dg.data_ptr(),
                                        db.data_ptr(), len(rows), seg, D, _lib.DTYPE_BF16, relu, 0,
                                        ws.data_ptr(), wsb, None) == 0
    dz64, dg64, db64, bmag = R.bn_bwd_ref(z, dy, gamma, beta, rows, mask)
    what = f"batchnorm bwd rows {rows} D {D} relu {relu}"
    _figures(what, R.check_bf16_rounded(dz, dz64, bmag, R.BN_BWD_SLACK, what=what))
    assert rel(dg, dg64) < TOL and rel(db, db64) < TOL


def _models(L, D, F, seed):
    from molclr_amd.ginet_molclr import GINet
    from oracle.reference_cpu import RefGINet
    torch.manual_seed(seed)
    ref = RefGINet(L, D, F)
    mine = GINet(L, D, F, precision="bf16")
    mine.load_state_dict(ref.state_dict())
    return copy.deepcopy(ref).double(), mine


@pytest.mark.parametrize("L,D,B", [(5, 512, 256), (3, 128, 64)])
def test_ginet_bf16_vs_fp64_reference(dev, L, D, B):
    """GINet(precision='bf16') -- the c5 configuration's arithmetic -- against
    the fp64 reference (both views, paired pass, NT-Xent): within BF16_TOL."""
    from molclr_amd.nt_xent import NTXentLoss
    from molclr_amd.ops import l2_normalize
    from oracle.reference_cpu import RefNTXentLoss
    ref64, mine = _models(L, D, 512, seed=7)
    mine = mine.to(dev)
    xi, xj = SyntheticPairBatches(B, seed=3, shape="pubchem").next()
    hi_r, zi_r = ref64(xi)
    hj_r, zj_r = ref64(xj)
    lr = RefNTXentLoss("cpu", B, 0.1, True)(torch.nn.functional.normalize(zi_r, dim=1),
                                            torch.nn.functional.normalize(zj_r, dim=1))
    lr.backward()
    hp, op = mine.forward_pair(xi.to(dev), xj.to(dev))
    lm = NTXentLoss(dev, B, 0.1, True).forward_pair(l2_normalize(op))
    lm.backward()
    errs = {"h": rel(hp, torch.cat([hi_r, hj_r])), "out": rel(op, torch.cat([zi_r, zj_r])),
            "loss": abs(lm.item() - lr.item()) / abs(lr.item())}
    g64 = dict(ref64.named_parameters())
    gerr = {n: rel(p.grad, g64[n].grad) for n, p in mine.named_parameters()
            if not (n.endswith("mlp.2.bias"))}  # pre-BN bias: exact gradient 0
    errs["grad"] = max(gerr.values())
    for k, v in errs.items():
        assert v < BF16_TOL[k], (k, v, sorted(gerr.items(), key=lambda kv: -kv[1])[:4])
    for name, buf in ref64.named_buffers():
        mb = dict(mine.named_buffers())[name]
        if not name.endswith("num_batches_tracked"):
            assert rel(mb, buf) < BF16_TOL["h"], name


EMU_TOL = 1e-2  # vs the oracle that rounds where the kernels store bf16


def _emu_models(L, D, seed=7):
    from molclr_amd.ginet_molclr import GINet
    from oracle.reference_cpu import RefGINet
    torch.manual_seed(seed)
    emu = RefGINet(L, D, 512, emulate_bf16=True)
    mine = GINet(L, D, 512, precision="bf16")
    mine.load_state_dict(emu.state_dict())
    return emu, mine


@pytest.mark.parametrize("L,D,B", [(5, 512, 256), (3, 128, 64)])
def test_ginet_bf16_encoder_vs_bf16_emulating_oracle(dev, L, D, B):
    """The c5 encoder arithmetic against oracle/reference_cpu.py with
    emulate_bf16: the same rounding points as the HIP bf16 path (node
    features, aggregation outputs, MLP activations, BatchNorm in/outputs and
    the gradients of all of them stored as bf16; bf16 weight operands), fp64
    everywhere else.  What remains is the kernels' fp32 accumulation and the
    elements whose bf16 rounding an fp32 vs fp64 sum flips (one bf16 ulp
    each).  Both views through the paired pass, backward of a fixed random
    functional of the node embeddings.  Node embeddings and BatchNorm running
    statistics within 1e-2 norm-wise.  The parameter gradients are sensitive
    to those one-ulp flips (BatchNorm's backward projects them out of a
    gradient that is largely mean / x_hat-aligned): the SAME emulation run in
    fp32 instead of fp64 moves them by 3-4e-2 at L=3 and ~0.12 at L=5, so
    each gradient is held to 1e-2 or 1.5x that self-noise, whichever is
    larger (measured: 2.4e-2 at L=3, vs 4.1e-2 self-noise)."""
    from oracle.reference_cpu import _StoreBF16
    emu32, mine = _emu_models(L, D)
    emu64 = copy.deepcopy(emu32).double()
    mine = mine.to(dev)
    xi, xj = SyntheticPairBatches(B, seed=3, shape="pubchem").next()
    g = torch.Generator().manual_seed(1)
    refs = []
    for emu in (emu64, emu32):
        hs = []
        for x in (xi, xj):  # the oracle's encoder: ginet_molclr.py:103-111, per view
            h = _StoreBF16.apply(emu.x_embedding1(x.x[:, 0]) + emu.x_embedding2(x.x[:, 1]))
            for layer in range(L):
                h = emu.batch_norms[layer](emu.gnns[layer](h, x.edge_index, x.edge_attr))
                h = _StoreBF16.apply(h if layer == L - 1 else torch.relu(h))
            hs.append(h)
        refs.append(torch.cat(hs))
    w = torch.randn(refs[0].shape, generator=g, dtype=torch.float64)
    (refs[0] * w).sum().backward()
    (refs[1] * w.float()).sum().backward()
    from molclr_amd.data import pair_graph
    xi_d, xj_d = xi.to(dev), xj.to(dev)
    h = mine._run_encoder(torch.cat([xi_d.x, xj_d.x]), pair_graph(xi_d, xj_d))
    (h.float() * w.float().to(dev)).sum().backward()
    assert rel(h, refs[0]) < EMU_TOL
    g64, g32 = dict(emu64.named_parameters()), dict(emu32.named_parameters())
    checked, bad = 0, {}
    for n, p in mine.named_parameters():
        if p.grad is None or n.endswith("mlp.2.bias"):  # pre-BN bias: exact gradient 0
            continue
        checked += 1
        e, e32 = rel(p.grad, g64[n].grad), rel(g32[n].grad, g64[n].grad)
        if e > max(EMU_TOL, 1.5 * e32) or e > BF16_TOL["grad"]:
            bad[n] = (e, e32)
    assert checked == 2 + 7 * L and not bad, bad
    for name, buf in emu64.named_buffers():
        if not name.endswith("num_batches_tracked"):
            assert rel(dict(mine.named_buffers())[name], buf) < EMU_TOL, name


@pytest.mark.parametrize("L,D,B", [(5, 512, 256), (3, 128, 64)])
def test_ginet_bf16_step_vs_bf16_emulating_oracle(dev, L, D, B):
    """The whole c5 step (paired pass, heads, NT-Xent) against the emulating
    oracle: h, out and the loss within 1e-2.  The step's parameter gradients
    at random init are ill-conditioned (the projections are nearly parallel:
    NT-Xent's gradient is a small difference of large terms), so one-ulp bf16
    rounding differences are amplified; each gradient is held to twice what
    the SAME emulation run in fp32 instead of fp64 moves (its own conditioning
    at these rounding points), and to 0.35 as before."""
    from molclr_amd.nt_xent import NTXentLoss
    from molclr_amd.ops import l2_normalize
    from oracle.reference_cpu import RefNTXentLoss
    emu32, mine = _emu_models(L, D)
    emu64 = copy.deepcopy(emu32).double()
    mine = mine.to(dev)
    xi, xj = SyntheticPairBatches(B, seed=3, shape="pubchem").next()
    outs = []
    for m in (emu64, emu32):
        hi, zi = m(xi)
        hj, zj = m(xj)
        loss = RefNTXentLoss("cpu", B, 0.1, True)(torch.nn.functional.normalize(zi, dim=1),
                                                  torch.nn.functional.normalize(zj, dim=1))
        loss.backward()
        outs.append((torch.cat([hi, hj]), torch.cat([zi, zj]), loss))
    hp, op = mine.forward_pair(xi.to(dev), xj.to(dev))
    lm = NTXentLoss(dev, B, 0.1, True).forward_pair(l2_normalize(op))
    lm.backward()
    h64, o64, l64 = outs[0]
    assert rel(hp, h64) < EMU_TOL and rel(op, o64) < EMU_TOL
    assert abs(lm.item() - l64.item()) / abs(l64.item()) < EMU_TOL
    g64, g32 = dict(emu64.named_parameters()), dict(emu32.named_parameters())
    bad = {}
    for n, p in mine.named_parameters():
        if n.endswith("mlp.2.bias"):  # exact gradient 0: rounding noise on every side
            continue
        e, e32 = rel(p.grad, g64[n].grad), rel(g32[n].grad, g64[n].grad)
        if e > max(EMU_TOL, 2 * e32) or e > BF16_TOL["grad"]:
            bad[n] = (e, e32)
    assert not bad, bad


def test_ginet_bf16_training_step_runs_and_is_deterministic(dev):
    from molclr_amd.ginet_molclr import GINet
    from molclr_amd.nt_xent import NTXentLoss
    from molclr_amd.ops import l2_normalize
    from molclr_amd.optim import FusedAdam
    xi, xj = SyntheticPairBatches(128, seed=4, shape="pubchem").next()
    res = []
    for _ in range(2):
        torch.manual_seed(0)
        m = GINet(5, 512, 512, precision="bf16").to(dev)
        opt = FusedAdam(m.parameters(), 5e-4, weight_decay=1e-5)
        crit = NTXentLoss(dev, 128, 0.1, True)
        for _ in range(3):
            opt.zero_grad()
            loss = crit.forward_pair(l2_normalize(m.forward_pair(xi.to(dev), xj.to(dev))[1]))
            loss.backward()
            opt.step()
        assert torch.isfinite(loss)
        res.append(opt.flat.clone())
    assert torch.equal(res[0], res[1])
