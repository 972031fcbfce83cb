"""tests/rounding.py has teeth: on the CPU fp32-accumulated product (torch's
fp32 matmul of the bf16-valued operands) at the shapes of the GPU tests, the
once-rounded result passes check_bf16_rounded and each faulty epilogue fails
the condition that is there to catch it."""
import pytest
import torch

from . import rounding as R


@pytest.fixture(scope="module", params=R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def prod(request):
    M, N, K = request.param
    A, W, _, b, _ = R.gemm_case(M, N, K)
    ref, mag = R.gemm_ref(A, W, b)
    return {"A": A, "W": W, "b": b, "ref": ref, "mag": mag, "acc": A @ W.t()}


def _report(C, p):
    return R.rounding_report(C, p["ref"], p["mag"], R.GEMM_SLACK)


def test_cpu_fp32_references_fit_their_slack():
    """The slacks are twice the CPU fp32 references' error as measured when
    they were set (module docstring); whatever BLAS runs here, those references
    stay inside the window, and the product's off-RNE share at 0.035 %."""
    m = R.measure_slack_basis()
    print(m)
    assert m["gemm_share"] <= 3.5e-4
    for key, slack in (("gemm", R.GEMM_SLACK), ("bn_fwd", R.BN_FWD_SLACK), ("bn_bwd", R.BN_BWD_SLACK)):
        assert m[key] < slack, (key, m[key], slack)


def test_rne_bf16_is_one_rounding():
    x = torch.randn(4096, dtype=torch.float64) * torch.pow(2.0, torch.randint(-20, 20, (4096,)))
    x32 = x.float().double()  # fp32-representable: torch's fp32 -> bf16 is the same single RNE
    assert torch.equal(R.rne_bf16(x32), x32.float().to(torch.bfloat16).double())
    # 1 + 2^-8 + 2^-30: above the tie, but fp32 rounds it onto the tie first
    t = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30], dtype=torch.float64)
    assert R.rne_bf16(t).item() == 1.0 + 2.0 ** -7
    assert t.float().to(torch.bfloat16).item() == 1.0
    assert R.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, -3.0], dtype=torch.float64)).tolist() == \
        [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6]


def test_once_rounded_passes(prod):
    C = (prod["acc"] + prod["b"]).to(torch.bfloat16)
    rep = R.check_bf16_rounded(C, prod["ref"], prod["mag"], R.GEMM_SLACK, what="cpu product")
    assert rep["share_off"] <= 3.5e-4
    # and under a ReLU, clamped reference: zeros and window-straddling elements included
    R.check_bf16_rounded(C.clamp(min=0), prod["ref"].clamp(min=0), prod["mag"], R.GEMM_SLACK)


def test_truncation_fails_bias_and_share(prod):
    rep = _report(R.trunc_bf16(prod["acc"] + prod["b"]), prod)
    assert {"b", "c"} <= rep["failed"]
    assert rep["share_off"] > 0.3 and rep["mean_d"] < -0.4
    with pytest.raises(AssertionError, match="share off"):
        R.check_bf16_rounded(R.trunc_bf16(prod["acc"] + prod["b"]), prod["ref"], prod["mag"],
                             R.GEMM_SLACK)


def test_bias_after_rounding_fails_share(prod):
    twice = (prod["acc"].to(torch.bfloat16).float() + prod["b"]).to(torch.bfloat16)
    rep = _report(twice, prod)
    assert "b" in rep["failed"] and rep["share_off"] > 0.1


def test_dropped_k_slice_fails_window(prod):
    K = prod["A"].shape[1]
    short = (prod["A"][:, :K - 8] @ prod["W"][:, :K - 8].t() + prod["b"]).to(torch.bfloat16)
    rep = _report(short, prod)
    assert "a" in rep["failed"] and rep["outside_window"] > 0.1 * rep["elements"]


def test_one_element_two_ulps_off_fails_window(prod):
    C = (prod["acc"] + prod["b"]).to(torch.bfloat16)
    i = int(prod["ref"].abs().flatten().argmax())  # a well-conditioned element
    flat = C.flatten().clone()
    flat[i] = (flat[i].double() + 2 * R.ulp_bf16(prod["ref"].flatten()[i])).to(torch.bfloat16)
    rep = _report(flat.view_as(C), prod)
    assert rep["failed"] == {"a"} and rep["outside_window"] == 1
