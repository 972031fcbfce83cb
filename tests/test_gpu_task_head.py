"""The task-head kernels (task_head.hip, ops.task_head) against an fp64 torch
CPU reference.

Bound: per output (h, pred, loss, dx, every dW_l and db_l) of EVERY case, the
norm-wise relative error against fp64 is at most TWICE that of a CPU fp32
evaluation of the same formulas on the same inputs (ref32: numpy float32,
every dot product accumulated sequentially over k, every row sum row after
row).  Nothing in the bound comes from the kernels.

Floor.  On a single case the fp32 reference's error is one sample: for small
outputs (a scalar loss, a 3 x 3 dW) it often lands far below what an fp32
evaluation is entitled to, down to a few 1e-9 when the roundings happen to
cancel, and a kernel that sums in another order cannot be held to twice a
lucky value.  The reference's error therefore counts as at least
    floor = stages(output) * 2^-24,
one unit roundoff u = 2^-24 per rounded stage on the output's dependency path,
added linearly (first-order worst case).  A stage is one Linear (dot products,
bias, activation), the loss, or one backward product; each consists of
several rounded fp32 operations, so counting ONE rounding of relative size u
per stage is the least any fp32 evaluation can be charged.  With L layers:
h 1, pred L, loss L + 1, dx 2L + 1, dW_l / db_l  L + 1 + (L - 1 - l) + 1 (the
forward, the loss gradient, the backward products down to layer l, and the
row sum).  That is at most 11 u = 6.6e-7 (the 5-layer chain's dx); the
300 -> 512 -> 256 -> 256 -> 2 chain's own reference errors are mostly above it.
"""
import itertools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CHAINS = {"wide": (300, 512, 256, 256, 2), "mid": (44, 40, 20, 1), "tiny": (7, 6, 3, 3, 3, 2)}
BATCHES = (1, 5, 33, 130)
ACTS = ("softplus", "relu")
LOSSES = ("cross_entropy", "mse", "l1", None)
f32 = np.float32


def losses_of(chain):
    return [l for l in LOSSES if l != "cross_entropy" or CHAINS[chain][-1] >= 2]


def make_case(chain, B, act, loss):
    """fp32 CPU tensors of one case.  Layer 0 is feat_lin (no activation), the
    hidden layers use `act`, the output layer none.  Inputs and weights are
    scaled up so the pre-activations spread over tens of units; three units of
    the first hidden layer are pinned (zero weight row) to 25, 19.5 and -60:
    above Softplus's threshold, just below it, and far below zero."""
    dims = CHAINS[chain]
    g = torch.Generator().manual_seed(zlib.crc32(f"{chain}/{B}/{act}/{loss}".encode()))
    L = len(dims) - 1
    x = torch.randn(B, dims[0], generator=g) * 2.0
    Ws, bs = [], []
    for l in range(L):
        K, N = dims[l], dims[l + 1]
        Ws.append((torch.rand(N, K, generator=g) * 2 - 1) * (3.0 / K ** 0.5))
        bs.append(torch.randn(N, generator=g) * 0.5)
    if dims[2] >= 4:
        Ws[1][:3] = 0.0
        bs[1][:3] = torch.tensor([25.0, 19.5, -60.0])
    C = dims[-1]
    target = None
    if loss == "cross_entropy":
        target = torch.randint(0, C, (B,), generator=g)
    elif loss in ("mse", "l1"):
        target = torch.randn(B, C, generator=g)
        if loss == "l1" and C >= 2:  # pred[:, 0] == bias exactly; row 0 ties the target
            Ws[-1][0] = 0.0
            target[0, 0] = bs[-1][0]
    acts = [None] + [act] * (L - 2) + [None]
    gp = torch.randn(B, C, generator=g)   # dpred of the loss-free case
    gh = torch.randn(B, dims[1], generator=g)
    return dict(dims=dims, x=x, Ws=Ws, bs=bs, acts=acts, loss=loss, target=target, gp=gp, gh=gh)


def objective(case, h, pred, loss, extra):
    """What is differentiated: the loss; (pred * gp).sum() without one;
    `extra` adds (h * gh).sum() + (pred * gp).sum() (the dh and dpred inputs)."""
    cast = lambda t: t.to(device=pred.device, dtype=pred.dtype)  # noqa: E731
    tot = loss if loss is not None else (pred * cast(case["gp"])).sum()
    if extra:
        tot = tot + (h * cast(case["gh"])).sum()
        if loss is not None:
            tot = tot + (pred * cast(case["gp"])).sum()
    return tot


def names(L):
    return ["h", "pred", "loss", "dx"] + [f"dW{l}" for l in range(L)] + [f"db{l}" for l in range(L)]


def ref64(case, extra=False):
    x = case["x"].double().requires_grad_(True)
    Ws = [w.double().requires_grad_(True) for w in case["Ws"]]
    bs = [b.double().requires_grad_(True) for b in case["bs"]]
    a, zs, h = x, [], None
    for l, (W, b) in enumerate(zip(Ws, bs)):
        z = a @ W.t() + b
        zs.append(z.detach())
        a = {None: lambda t: t, "relu": torch.relu, "softplus": F.softplus}[case["acts"][l]](z)
        if l == 0:
            h = a
    pred, loss, t = a, None, case["target"]
    if case["loss"] == "cross_entropy":
        loss = F.cross_entropy(pred, t)
    elif case["loss"] == "mse":
        loss = F.mse_loss(pred, t.double())
    elif case["loss"] == "l1":
        loss = F.l1_loss(pred, t.double())
    grads = torch.autograd.grad(objective(case, h, pred, loss, extra), [x] + Ws + bs)
    L = len(Ws)
    out = {"h": h.detach(), "pred": pred.detach(), "dx": grads[0], "zs": zs}
    if loss is not None:
        out["loss"] = loss.detach()
    for l in range(L):
        out[f"dW{l}"], out[f"db{l}"] = grads[1 + l], grads[1 + L + l]
    return out


def _act32(z, act):
    if act == "relu":
        return np.maximum(z, f32(0))
    if act == "softplus":
        return np.where(z > f32(20), z, np.log1p(np.exp(np.minimum(z, f32(20))))).astype(f32)
    return z


def _dact32(a, act):
    if act == "relu":
        return (a > 0).astype(f32)
    if act == "softplus":
        return (-np.expm1(-a)).astype(f32)
    return np.ones_like(a)


def ref32(case, extra=False):
    """The kernels' formulas in numpy float32, every sum sequential."""
    x = case["x"].numpy()
    Ws = [w.numpy() for w in case["Ws"]]
    bs = [b.numpy() for b in case["bs"]]
    L, B = len(Ws), x.shape[0]
    As = [x]
    for l in range(L):
        W, a = Ws[l], As[-1]
        acc = np.zeros((B, W.shape[0]), f32)
        for k in range(W.shape[1]):
            acc += a[:, k:k + 1] * W[:, k][None, :]
        As.append(_act32(acc + bs[l][None, :], case["acts"][l]))
    pred, C = As[-1], Ws[-1].shape[0]
    out = {"h": As[1], "pred": pred}
    d = np.zeros_like(pred)
    if case["loss"] is not None:
        if case["loss"] == "cross_entropy":
            y = case["target"].numpy()
            m = pred.max(1, keepdims=True)
            e = np.exp(pred - m)
            s = np.zeros((B, 1), f32)
            for c in range(C):
                s += e[:, c:c + 1]
            rows = (m + np.log(s))[:, 0] - pred[np.arange(B), y]
            onehot = np.zeros_like(pred)
            onehot[np.arange(B), y] = 1
            d = ((e / s - onehot) / f32(B)).astype(f32)
            cnt = f32(B)
        else:
            diff = pred - case["target"].numpy()
            el = diff * diff if case["loss"] == "mse" else np.abs(diff)
            rows = np.zeros(B, f32)
            for c in range(C):
                rows += el[:, c]
            cnt = f32(B) * f32(C)
            d = (f32(2) * diff / cnt if case["loss"] == "mse" else np.sign(diff) / cnt).astype(f32)
        tot = f32(0)
        for r in range(B):
            tot = f32(tot + rows[r])
        out["loss"] = f32(tot / cnt)
    if case["loss"] is None or extra:
        d = d + case["gp"].numpy()
    if L == 1 and extra:
        d = d + case["gh"].numpy()
    delta = (d * _dact32(pred, case["acts"][-1])).astype(f32)
    for l in range(L - 1, -1, -1):
        W, a_in = Ws[l], As[l]
        dW, db = np.zeros_like(W), np.zeros_like(bs[l])
        for r in range(B):
            dW += delta[r][:, None] * a_in[r][None, :]
            db += delta[r]
        out[f"dW{l}"], out[f"db{l}"] = dW, db
        gin = np.zeros((B, W.shape[1]), f32)
        for n in range(W.shape[0]):
            gin += delta[:, n:n + 1] * W[n][None, :]
        if l == 0:
            out["dx"] = gin
        else:
            if l == 1 and extra:
                gin = gin + case["gh"].numpy()
            delta = (gin * _dact32(As[l], case["acts"][l - 1])).astype(f32)
    return out


U32 = 2.0 ** -24


def stages(name, L):
    """Rounded stages on an output's dependency path (module docstring)."""
    if name == "h":
        return 1
    if name == "pred":
        return L
    if name == "loss":
        return L + 1
    if name == "dx":
        return 2 * L + 1
    return L + 1 + (L - 1 - int(name[2:])) + 1  # dW_l, db_l


def basis_of(r32, r64):
    """Per output of ONE case: the fp32 reference's own error, at least the
    floor."""
    L = sum(1 for n in r64 if n.startswith("dW"))
    return {n: max(relerr(r32[n], r64[n]), stages(n, L) * U32) for n in r64 if n != "zs"}


def relerr(got, want64):
    got = torch.as_tensor(np.asarray(got)).double().reshape(-1)
    want = want64.double().reshape(-1)
    den = want.norm().item()
    num = (got - want).norm().item()
    return num / den if den > 0 else num


_REFS = {}


def refs(chain, act):
    """(case, fp64 reference, the case's own fp32 basis) of every (B, loss) of
    one chain and activation, computed once and shared."""
    key = (chain, act)
    if key not in _REFS:
        cases = {}
        for B, loss in itertools.product(BATCHES, losses_of(chain)):
            case = make_case(chain, B, act, loss)
            r64 = ref64(case)
            cases[(B, loss)] = (case, r64, basis_of(ref32(case), r64))
        _REFS[key] = cases
    return _REFS[key]


def run_gpu(case, dev, extra=False, status=None, params=None):
    from molclr_amd import ops
    x = case["x"].to(dev).requires_grad_(True)
    if params is None:
        Ws = [w.to(dev).requires_grad_(True) for w in case["Ws"]]
        bs = [b.to(dev).requires_grad_(True) for b in case["bs"]]
    else:
        Ws, bs = params
    t = None if case["target"] is None else case["target"].to(dev)
    h, pred, loss = ops.task_head(x, Ws, bs, case["acts"], case["loss"], t, status)
    objective(case, h, pred, loss, extra).backward()
    L = len(Ws)
    out = {"h": h.detach(), "pred": pred.detach(), "dx": x.grad}
    if loss is not None:
        out["loss"] = loss.detach()
    for l in range(L):
        out[f"dW{l}"], out[f"db{l}"] = Ws[l].grad, bs[l].grad
    return out


def check(out, r64, basis, what):
    lines, bad = [], []
    L = sum(1 for n in r64 if n.startswith("dW"))
    for n, ref in r64.items():
        if n == "zs":
            continue
        got = out[n].detach().cpu()
        assert torch.isfinite(got).all(), f"{what}: {n} has inf / NaN"
        e = relerr(got.numpy(), ref)
        lines.append(f"{n} {e:.3e} (fp32 ref {basis[n]:.3e}, floor {stages(n, L) * U32:.1e})")
        if not e <= 2.0 * basis[n]:
            bad.append(lines[-1])
    print(what, "; ".join(lines))
    assert not bad, f"{what}: above twice the fp32 reference's error: {bad}"


ALL = [(c, a, B, l) for c in CHAINS for a in ACTS for B in BATCHES for l in losses_of(c)]


@pytest.mark.parametrize("chain,act,B,loss", ALL)
def test_task_head_matches_fp64(dev, chain, act, B, loss):
    case, r64, basis = refs(chain, act)[(B, loss)]
    check(run_gpu(case, dev), r64, basis, f"{chain} {act} B={B} {loss}")


@pytest.mark.parametrize("chain", ("wide", "mid"))
def test_softplus_inputs_cover_the_threshold(chain):
    """The fp64 pre-activations of the softplus cases straddle the threshold
    and reach far below zero (what the stability claims are tested on)."""
    for (B, loss), (case, r64, _) in refs(chain, "softplus").items():
        z = r64["zs"][1]
        assert (z > 20).any() and ((z > 19) & (z < 20)).any() and (z < -50).any(), (B, loss)


def test_l1_case_has_an_exact_tie():
    case, r64, _ = refs("wide", "relu")[(5, "l1")]
    assert r64["pred"][0, 0].item() == case["target"][0, 0].item()
    assert r64["dW3"][0].abs().max().item() > 0  # other rows of the column still push


@pytest.mark.parametrize("chain,act,B,loss", [("wide", "softplus", 33, "cross_entropy"),
                                              ("mid", "relu", 130, "l1"),
                                              ("tiny", "softplus", 5, "mse")])
def test_bit_identical_from_run_to_run(dev, chain, act, B, loss):
    case = make_case(chain, B, act, loss)
    a, b = run_gpu(case, dev), run_gpu(case, dev)
    for n in a:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("chain,loss", [("wide", "cross_entropy"), ("tiny", "l1")])
def test_extra_gradients_into_h_and_pred(dev, chain, loss):
    """dh and dpred: the gradient of h.sum()-like + pred.sum()-like + loss."""
    case = make_case(chain, 33, "softplus", loss)
    r64 = ref64(case, extra=True)
    basis = basis_of(ref32(case, extra=True), r64)
    check(run_gpu(case, dev, extra=True), r64, basis, f"{chain} extra {loss}")


def test_single_layer_chain(dev):
    """L = 1: h and pred are the same activation; both gradients reach it."""
    g = torch.Generator().manual_seed(11)
    case = dict(dims=(9, 3), x=torch.randn(6, 9, generator=g), Ws=[torch.randn(3, 9, generator=g)],
                bs=[torch.randn(3, generator=g)], acts=["softplus"], loss="mse",
                target=torch.randn(6, 3, generator=g), gp=torch.randn(6, 3, generator=g),
                gh=torch.randn(6, 3, generator=g))
    r64 = ref64(case, extra=True)
    basis = basis_of(ref32(case, extra=True), r64)
    check(run_gpu(case, dev, extra=True), r64, basis, "single layer")


def test_accumulate_into_fused_adam_grads(dev):
    """Parameters owned by a FusedAdam: the kernels add into the flat gradient
    buffer, so two backward passes leave twice the gradient of one (one
    rounding of the addition: g + g is exact, so exactly twice)."""
    from molclr_amd.optim import FusedAdam
    case = make_case("mid", 33, "softplus", "mse")
    Ws = [torch.nn.Parameter(w.to(dev)) for w in case["Ws"]]
    bs = [torch.nn.Parameter(b.to(dev)) for b in case["bs"]]
    opt = FusedAdam(Ws + bs, 1e-3)
    opt.zero_grad()
    run_gpu(case, dev, params=(Ws, bs))
    once = opt.flat_grad.clone()
    assert once.abs().sum().item() > 0
    free = run_gpu(case, dev)  # the same gradients through fresh tensors
    for l in range(len(Ws)):
        assert torch.equal(Ws[l].grad, free[f"dW{l}"]) and torch.equal(bs[l].grad, free[f"db{l}"])
    run_gpu(case, dev, params=(Ws, bs))
    twice = opt.flat_grad
    eps = 2.0 ** -24
    assert ((twice - 2 * once).abs() <= eps * (2 * once).abs()).all()


@pytest.mark.parametrize("label", (2, -1))
def test_label_out_of_range_sets_status(dev, label):
    from molclr_amd import _lib
    from molclr_amd.data import raise_for_status
    case = make_case("wide", 5, "relu", "cross_entropy")
    case["target"][3] = label
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = run_gpu(case, dev, status=status)
    assert int(status.item()) == _lib.STATUS_LABEL_RANGE
    with pytest.raises(ValueError, match="class label"):
        raise_for_status(int(status.item()))
    assert torch.isnan(out["loss"])
    ok = [0, 1, 2, 4]
    assert torch.isfinite(out["dx"][ok]).all() and torch.isfinite(out["pred"]).all()
    # a valid batch leaves the word alone
    status.zero_()
    run_gpu(make_case("wide", 5, "relu", "cross_entropy"), dev, status=status)
    assert int(status.item()) == 0


@pytest.mark.parametrize("chain,act,loss", [("wide", "softplus", "cross_entropy"),
                                            ("wide", "relu", "mse"), ("mid", "softplus", "l1"),
                                            ("tiny", "relu", "cross_entropy"),
                                            ("tiny", "softplus", None)])
def test_composed_path_within_the_same_bound(dev, chain, act, loss, monkeypatch):
    """MOLCLR_TASK_HEAD=0 (the module switch it sets): ops.linear per layer,
    torch activations and loss."""
    from molclr_amd import ops
    monkeypatch.setattr(ops, "TASK_HEAD", False)
    case, r64, basis = refs(chain, act)[(33, loss)]
    check(run_gpu(case, dev), r64, basis, f"composed {chain} {act} {loss}")


def test_softplus_elementwise_at_the_extremes(dev):
    """Softplus and its derivative element by element.  Layer 1 is the identity
    with Softplus, layer 2 sums its three units, so with dpred = 1 the kernel's
    dx[r, k] IS softplus'(x[r, k]) recomputed from the saved activation, and
    h = softplus(x).  Each must be within 4 u of fp64 (log1p, exp / expm1 and
    one rounding of the result: at most a few u); below the smallest normal
    fp32 a result may be flushed, so 2^-126 absolute is allowed.  A cancelling
    derivative such as 1 - exp(-a) gives 0 at z = -60 and fails."""
    from molclr_amd import ops
    z = torch.tensor([[-100.0, -60.0, -20.0], [-1.0, 0.0, 3.0], [19.5, 19.99, 20.0],
                      [20.5, 30.0, -50.5]])
    x = z.to(dev).requires_grad_(True)
    Ws = [torch.eye(3, device=dev), torch.ones(1, 3, device=dev)]
    bs = [torch.zeros(3, device=dev), torch.zeros(1, device=dev)]
    h, pred, _ = ops.task_head(x, Ws, bs, ["softplus", None])
    pred.sum().backward()
    z64 = z.double()
    want_h = F.softplus(z64)
    want_d = torch.where(z64 > 20, torch.ones_like(z64), torch.sigmoid(z64))
    for got, want, what in ((h.detach(), want_h, "softplus"), (x.grad, want_d, "derivative")):
        got = got.cpu().double()
        assert torch.isfinite(got).all(), what
        tol = 4 * U32 * want.abs() + 2.0 ** -126
        assert ((got - want).abs() <= tol).all(), (what, got, want)
    assert x.grad[0, 1].item() > 0 and h[0, 1].item() > 0  # z = -60: no cancellation to 0


def test_widest_layer_and_wider_chains(dev):
    """A layer at the kernels' width limit runs through them; a wider chain is
    routed to the composed path by ops.task_head.  Both within the bound."""
    from molclr_amd import _lib, ops
    for width in (_lib.TASK_HEAD_MAX_DIM, _lib.TASK_HEAD_MAX_DIM + 4):
        g = torch.Generator().manual_seed(width)
        dims = (12, width, 2)
        case = dict(dims=dims, x=torch.randn(5, 12, generator=g),
                    Ws=[torch.randn(width, 12, generator=g) / 12 ** 0.5,
                        torch.randn(2, width, generator=g) / width ** 0.5],
                    bs=[torch.randn(width, generator=g), torch.randn(2, generator=g)],
                    acts=["relu", None], loss="cross_entropy",
                    target=torch.randint(0, 2, (5,), generator=g),
                    gp=torch.randn(5, 2, generator=g), gh=torch.randn(5, width, generator=g))
        r64 = ref64(case)
        assert ops.task_head_fused(dims) == (width <= _lib.TASK_HEAD_MAX_DIM)
        check(run_gpu(case, dev), r64, basis_of(ref32(case), r64), f"width {width}")


def test_argument_errors(dev):
    from molclr_amd import _lib, ops
    x = torch.zeros(2, 4, device=dev)
    W, b = torch.zeros(3, 4, device=dev), torch.zeros(3, device=dev)
    with pytest.raises(ValueError):
        ops.task_head(x, [W] * 11, [b] * 11, [None] * 11)
    with pytest.raises(ValueError):
        ops.task_head(x, [W], [b], [None], loss="mse")  # no target
    # the C entry itself refuses a width above its limit (ops routes such chains)
    n = _lib.TASK_HEAD_MAX_DIM + 1
    big, out = torch.zeros(n, 4, device=dev), torch.zeros(2, n, device=dev)
    c = ops._head_struct(x, [big], [torch.zeros(n, device=dev)], [out], (0,), 0, None, None, None,
                         None)
    import ctypes
    assert _lib.load().molclr_task_head_fwd(ctypes.addressof(c), None, 0, None) == -3
    assert "exceeds" in _lib.last_error()
