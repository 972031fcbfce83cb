"""Correct-rounding check for kernels that compute in fp32 and store bf16.

A kernel that accumulates in fp32 and rounds ONCE, to nearest even, gives for
almost every element exactly RNE_bf16(exact result): the fp32 accumulation
error (a few 2^-24 of the operation's magnitude sum) is far below one bf16 ulp
(2^-8 relative), so it only decides the rounding of elements that sit within
that error of a rounding boundary.  check_bf16_rounded holds a bf16 output to
exactly that statement, against the fp64 result of the same operation on the
same bf16-rounded inputs:

(a) window, every element:  RNE_bf16(ref - e) <= C <= RNE_bf16(ref + e) with
    e = slack * 2^-24 * mag, mag the fp64 sum of the absolute values of the
    operation's terms (|A| |W|^T + |bias| for a product);
(b) share: at most `cap` of the elements differ from RNE_bf16(ref);
(c) no rounding bias: d = (|C| - |ref|) / ulp_bf16(ref) has mean 0 and
    variance 1/12 under round-to-nearest-even, so |mean d| <= 6 / sqrt(12 n)
    (six sigma of the mean of n elements; truncation gives -0.5), over the n
    elements with |ref| above the smallest normal bf16.

A norm-wise 2^-8 bound passes truncation (3.3e-3), rounding twice (2.3e-3) and
a tail path that rounds wrongly; (b) and (c) do not.  A ReLU needs no special
case: with ref the clamped fp64 value, an element whose pre-activation window
straddles 0 may be 0 or the rounded value, and both lie in (a)'s window.

slack is NOT taken from the HIP kernels.  Its basis is the error of a CPU
fp32-accumulated reference on the bf16-valued operands against fp64,
max |y32 - y64| / (2^-24 mag) over the test shapes, and slack is twice that:
the MFMA chain (and the kernels' blocked reductions) sum in another order,
under the same u * sum |a| |w| form of bound.  For the product the reference
is torch's fp32 matmul (+ bias in fp32); for BatchNorm it is _bn32 below, the
formulas in plain fp32 with every sum taken row after row (torch's own fp32
batch norm changes its summation, and its error, with the thread count).
Measured by measure_slack_basis() (`python -m tests.rounding` prints them):

  product, (M, N, K) = (333, 256, 64), (257, 320, 512), (129, 136, 1000),
  (37, 96, 40), without and with bias:      basis 1.942 -> GEMM_SLACK   = 3.89
  BatchNorm forward, segments (700, 900) and (7, 3), D = 512 and 64:
                                            basis 20.49 -> BN_FWD_SLACK = 41.0
  BatchNorm backward, the same, ReLU on and off:
                                            basis 11.62 -> BN_BWD_SLACK = 23.3

(slack = 2 x basis, rounded up to three digits).  Even 41 x 2^-24 is 1/800 of
a bf16 half ulp of a well-conditioned element, so the window still admits no
element one ulp off unless it sits that close to a rounding boundary.  The
share of RNE_bf16(y32) != RNE_bf16(y64) of the CPU product is <= 0.035 % at
every shape (0.023 % at most with this module's seeds); CAP = 0.5 % leaves
> 10x for another summation order, while truncation, double rounding or a
dropped K slice put tens of percent off.
"""
import math

import torch

SHAPES = [(333, 256, 64), (257, 320, 512), (129, 136, 1000), (37, 96, 40)]
BN_CASES = [((700, 900), 512), ((700, 900), 64), ((7, 3), 512), ((7, 3), 64)]
U32 = 2.0 ** -24           # fp32 unit roundoff
CAP = 0.005                # (b): a condition, not a measurement
GEMM_SLACK = 3.89
BN_FWD_SLACK = 41.0
BN_BWD_SLACK = 23.3
BF16_MIN_NORMAL = 2.0 ** -126
_MIN_ULP_EXP = -133        # spacing of the bf16 subnormals


def ulp_bf16(x64):
    """Spacing of the bf16 grid at |x| (8 significant bits), fp64."""
    _, e = torch.frexp(x64.abs().clamp_min(BF16_MIN_NORMAL))  # |x| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x64), (e - 8).clamp_min(_MIN_ULP_EXP))


def rne_bf16(x64):
    """fp64 -> nearest bf16 value (ties to even) in ONE rounding, kept as fp64
    (a .to(bfloat16) of an fp64 tensor rounds to fp32 first)."""
    u = ulp_bf16(x64)
    return torch.round(x64 / u) * u  # x / u is exact; torch.round is half-to-even


def trunc_bf16(x32):
    """fp32 -> bf16 by dropping the low 16 bits (the faulty epilogue of the tests)."""
    return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def rounding_report(C, ref64, mag64, slack, cap=CAP):
    """The figures of (a), (b), (c) and which of them fail."""
    assert C.dtype == torch.bfloat16 and ref64.dtype == torch.float64
    c = C.detach().cpu().double()
    ref64, mag64 = ref64.detach().cpu(), mag64.detach().cpu()
    assert c.shape == ref64.shape == mag64.shape
    e = slack * U32 * mag64
    lo, hi = rne_bf16(ref64 - e), rne_bf16(ref64 + e)
    outside = ~((lo <= c) & (c <= hi))  # a NaN is outside
    off = c != rne_bf16(ref64)
    sel = ref64.abs() > BF16_MIN_NORMAL
    n = int(sel.sum())
    d = (c.abs() - ref64.abs())[sel] / ulp_bf16(ref64)[sel]
    rep = {"elements": c.numel(), "outside_window": int(outside.sum()),
           "share_off": off.double().mean().item() if c.numel() else 0.0, "cap": cap,
           "n_bias": n, "mean_d": d.mean().item() if n else 0.0,
           "bias_bound": 6.0 / math.sqrt(12.0 * n) if n else math.inf}
    if rep["outside_window"]:
        i = int(torch.nonzero(outside.flatten())[0])
        rep["first_outside"] = (i, c.flatten()[i].item(), lo.flatten()[i].item(),
                                hi.flatten()[i].item())
    rep["failed"] = {k for k, bad in (("a", rep["outside_window"] > 0),
                                      ("b", rep["share_off"] > cap),
                                      ("c", not abs(rep["mean_d"]) <= rep["bias_bound"])) if bad}
    return rep


def check_bf16_rounded(C, ref64, mag64, slack, cap=CAP, what=""):
    """Assert (a), (b) and (c) of the module docstring; returns the figures."""
    rep = rounding_report(C, ref64, mag64, slack, cap)
    assert not rep["failed"], (
        f"{what}: not a once-rounded bf16 result, failed {sorted(rep['failed'])}: "
        f"{rep['outside_window']} of {rep['elements']} elements outside the window "
        f"{rep.get('first_outside', '')}; share off RNE_bf16(ref64) {rep['share_off']:.3e} "
        f"(cap {cap:.1e}); mean d {rep['mean_d']:+.4f} ulp (bound {rep['bias_bound']:.4f}, "
        f"n {rep['n_bias']})")
    return rep


def gemm_case(M, N, K, seed=None):
    """bf16-valued randn operands of one product (fp32 tensors): A [M, K], the
    row-major weight W [N, K], its K-major twin Wt [K, N], bias [N] (fp32
    values, as the kernels take it) and the ReLU-mask operand aux [M, N]."""
    g = torch.Generator().manual_seed(M + N + K if seed is None else seed)
    r = lambda *s: torch.randn(*s, generator=g)
    q = lambda t: t.to(torch.bfloat16).float()
    return q(r(M, K)), q(r(N, K)), q(r(K, N)), r(N), q(r(M, N))


def gemm_ref(A, Wnk, bias=None):
    """fp64 A W^T (+ bias) and its magnitude sum |A| |W|^T (+ |bias|)."""
    A64, W64 = A.double(), Wnk.double()
    y, mag = A64 @ W64.t(), A64.abs() @ W64.abs().t()
    if bias is not None:
        y, mag = y + bias.double(), mag + bias.double().abs()
    return y, mag


def bn_case(rows, D, seed=None):
    """bf16-valued z and dy of one segmented BatchNorm, fp32 gamma / beta."""
    g = torch.Generator().manual_seed(sum(rows) + D if seed is None else seed)
    n = sum(rows)
    z = (torch.randn(n, D, generator=g) * 2 + 1).to(torch.bfloat16).float()
    dy = torch.randn(n, D, generator=g).to(torch.bfloat16).float()
    return z, dy, torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)


def bn_fwd_ref(z, gamma, beta, rows, eps=1e-5):
    """fp64 training-mode BatchNorm of every segment, before the ReLU:
        y = gamma (z - mean) invstd + beta,   invstd = (var + eps)^-1/2 (biased var)
    and the sum of the absolute values of its terms
        mag = |gamma| invstd (|z| + |mean|) + |beta|.
    Also mean, invstd [nseg, D]."""
    z64, g64, b64 = z.double(), gamma.double(), beta.double()
    ys, mags, means, invs = [], [], [], []
    r0 = 0
    for r in rows:
        zs = z64[r0:r0 + r]
        mean = zs.mean(0)
        inv = (zs.var(0, unbiased=False) + eps).rsqrt()
        ys.append(g64 * (zs - mean) * inv + b64)
        mags.append(g64.abs() * inv * (zs.abs() + mean.abs()) + b64.abs())
        means.append(mean)
        invs.append(inv)
        r0 += r
    return torch.cat(ys), torch.cat(mags), torch.stack(means), torch.stack(invs)


def bn_bwd_ref(z, dy, gamma, beta, rows, mask=None, eps=1e-5):
    """fp64 autograd of the segmented BatchNorm (times the constant 0/1 `mask`
    of its ReLU when given): dz, dgamma, dbeta (summed over the segments), and
    the magnitude sum of dz.  With g = dy mask, xhat = (z - mean) invstd,
        dz = gamma invstd (g - mean_rows(g) - xhat mean_rows(g xhat))
    so, with X = (|z| + |mean|) invstd >= |xhat| term by term,
        mag = |gamma| invstd (|g| + mean_rows |g| + X mean_rows(|g| X))."""
    z64 = z.double().requires_grad_(True)
    g64 = gamma.double().requires_grad_(True)
    b64 = beta.double().requires_grad_(True)
    m64 = torch.ones_like(z64) if mask is None else mask.double()
    outs, mags = [], []
    r0 = 0
    for r in rows:
        zs = z64[r0:r0 + r]
        mean = zs.mean(0)
        inv = (zs.var(0, unbiased=False) + eps).rsqrt()
        outs.append((g64 * (zs - mean) * inv + b64) * m64[r0:r0 + r])
        with torch.no_grad():
            ga = (dy.double() * m64)[r0:r0 + r].abs()
            X = (zs.abs() + mean.abs()) * inv
            mags.append(g64.abs() * inv * (ga + ga.mean(0) + X * (ga * X).mean(0)))
        r0 += r
    torch.cat(outs).backward(dy.double())
    return z64.grad, g64.grad, b64.grad, torch.cat(mags)


def _bn32(z, dy, gamma, beta, rows, relu, eps=1e-5):
    """The BatchNorm formulas above in plain fp32, every sum taken row after
    row (textbook Welford for the statistics, running sums for the backward's
    two means): the CPU fp32 reference the BatchNorm slacks are measured on.
    Elementwise torch ops only, so it does not depend on a thread count."""
    ys, dzs = [], []
    r0 = 0
    for r in rows:
        zs, gs = z[r0:r0 + r], dy[r0:r0 + r]
        mean, m2 = torch.zeros_like(gamma), torch.zeros_like(gamma)
        for i in range(r):
            d = zs[i] - mean
            mean = mean + d / float(i + 1)
            m2 = m2 + d * (zs[i] - mean)
        inv = 1.0 / torch.sqrt(m2 / float(r) + eps)
        sc = gamma * inv
        y = zs * sc + (beta - mean * sc)
        g = gs * (y > 0) if relu else gs
        xhat = (zs - mean) * inv
        s1, s2 = torch.zeros_like(gamma), torch.zeros_like(gamma)
        for i in range(r):
            s1 = s1 + g[i]
            s2 = s2 + g[i] * xhat[i]
        dzs.append((g - s1 / float(r) - xhat * (s2 / float(r))) * sc)
        ys.append(y)
        r0 += r
    return torch.cat(ys), torch.cat(dzs)


def measure_slack_basis():
    """max |fp32 result - fp64 result| / (2^-24 mag) of the CPU fp32 references
    over the test shapes (the module docstring's figures), and the largest
    share of RNE_bf16(y32) != RNE_bf16(y64) of the product."""
    out = {"gemm": 0.0, "gemm_share": 0.0, "bn_fwd": 0.0, "bn_bwd": 0.0}
    for M, N, K in SHAPES:
        A, W, _, b, _ = gemm_case(M, N, K)
        for bias in (None, b):
            y64, mag = gemm_ref(A, W, bias)
            y32 = A @ W.t() if bias is None else A @ W.t() + bias
            out["gemm"] = max(out["gemm"], ((y32.double() - y64).abs() / (U32 * mag)).max().item())
            share = (rne_bf16(y32.double()) != rne_bf16(y64)).double().mean().item()
            out["gemm_share"] = max(out["gemm_share"], share)
    for rows, D in BN_CASES:
        z, dy, gamma, beta = bn_case(rows, D)
        y64, mag, _, _ = bn_fwd_ref(z, gamma, beta, rows)
        for relu in (False, True):
            y32, dz32 = _bn32(z, dy, gamma, beta, rows, relu)
            out["bn_fwd"] = max(out["bn_fwd"], ((y32.double() - y64).abs() / (U32 * mag)).max().item())
            dz64, _, _, bmag = bn_bwd_ref(z, dy, gamma, beta, rows, (y32 > 0) if relu else None)
            ok = bmag > 0
            out["bn_bwd"] = max(out["bn_bwd"],
                                ((dz32.double() - dz64).abs()[ok] / (U32 * bmag[ok])).max().item())
    return out


if __name__ == "__main__":
    print(measure_slack_basis())
