"""Backward through running statistics at the executor and model level: the
encoder executors' modes 0 (eval) and 2 (frozen BatchNorm: running statistics,
nothing updated, dropout as in training), the per-op path, the paired pass,
torch.ops.molclr.batch_norm_seg and the captured fine-tuning step.

Oracle parity follows the motif-pool tests' rule: per tensor,
||mine - fp64|| <= max(1e-5 ||fp64||, 2 ||fp32 oracle - fp64||), the oracle's
BatchNorms in eval mode over non-trivial running statistics.  On the parent
commit every backward here raised (NotImplementedError / the executors'
REQUIRE).
"""
import copy

import pytest
import torch

from molclr_amd import ops
from molclr_amd.dataset import SyntheticPairBatches
from molclr_amd.finetune_step import CapturedFinetuneStep
import oracle.reference_cpu as ref_cpu
from oracle.reference_cpu import RefGCN, RefGINet

from . import philox
from .gcn_bf16_ref import emu_gcn
from .test_gpu_dropout import SEED, MaskFeed
from .test_gpu_finetune_step import (Q, batches, compare, eager_step, make, optimizers, sync)

pytestmark = pytest.mark.gpu


def randomize_stats(model, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for bn in model.batch_norms:
            bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=g) * 0.3)
            bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=g) * 1.5 + 0.5)
            bn.weight.copy_(torch.rand(bn.weight.shape, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(bn.bias.shape, generator=g) * 0.2)
            bn.num_batches_tracked.fill_(7)


def stats_of(model):
    return [t.clone() for bn in model.batch_norms
            for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]


def set_mode(model, mode):
    """0: eval; 2: training with frozen BatchNorm."""
    if mode == 0:
        model.eval()
    else:
        model.train()
        model.freeze_bn = True


def frozen_ref(ref):
    ref.train()
    for bn in ref.batch_norms:
        bn.eval()
    return ref


def err(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).norm().item()


def make_models(kind, L, D, p, seed):
    """(oracle fp32, oracle fp64, product) with the same weights and non-trivial
    running statistics; the oracles in training mode with their BatchNorms in
    eval mode.  kind 'gin' / 'gcn': fp32 against oracle/reference_cpu.py;
    'gin-bf16' / 'gcn-bf16': precision='bf16' against the oracle that rounds
    where the kernels store bf16 (emulate_bf16, tests/gcn_bf16_ref.py)."""
    from molclr_amd.gcn_molclr import GCN
    from molclr_amd.ginet_molclr import GINet
    torch.manual_seed(seed)
    gin, bf16 = kind.startswith("gin"), kind.endswith("bf16")
    if gin:
        ref = RefGINet(L, D, 64, drop_ratio=p, emulate_bf16=bf16)
    elif bf16:
        ref = emu_gcn(RefGCN, L, D, 64, drop_ratio=p)
    else:
        ref = RefGCN(L, D, 64, drop_ratio=p)
    randomize_stats(ref, D)
    mine = (GINet if gin else GCN)(L, D, 64, drop_ratio=p, precision="bf16" if bf16 else "fp32")
    mine.load_state_dict(ref.state_dict())
    ref64 = copy.deepcopy(ref).double()
    return frozen_ref(ref), frozen_ref(ref64), mine


def against_oracle(dev, kind, L, D, B, mode, p=0.0, monkeypatch=None, seed=None):
    """The loss and every parameter gradient of one forward / backward against
    the oracle in fp64, per tensor within max(1e-5 ||fp64||, 2 ||fp32 oracle -
    fp64||); running statistics and num_batches_tracked bit-identical before
    and after.  p > 0 (mode 2): the oracle's F.dropout is fed the masks that
    tests/philox.py builds for every layer from the call's key -- not the
    kernels' own -- so a wrong mask or scale anywhere in the forward or the
    backward shows in the gradients."""
    ref, ref64, mine = make_models(kind, L, D, p, L + D if seed is None else seed)
    mine = mine.to(dev)
    set_mode(mine, mode)
    bi, _ = SyntheticPairBatches(B, seed=B).next()
    N = bi.x.shape[0]
    feed = None
    if p > 0:
        assert mode == 2 and mine._dim_pad() == 0
        mine.dropout_state = torch.tensor([SEED, 5], dtype=torch.long, device=dev)
        masks = [torch.from_numpy(philox.dropout_mask(SEED, 5, l, p, N, D)) for l in range(L)]
        feed = MaskFeed(masks, p)
        monkeypatch.setattr(ref_cpu.F, "dropout", feed)
    else:
        for r in (ref, ref64):
            r.eval()  # the oracle of mode 0, and of mode 2 without dropout
    torch.manual_seed(3)
    h_r, out_r = ref(bi)
    w1, w2 = torch.randn_like(h_r), torch.randn_like(out_r)
    loss_r = (h_r * w1).sum() + (out_r * w2).sum()
    if feed:
        feed.view(slice(None))
    h_6, out_6 = ref64(bi)
    loss_6 = (h_6 * w1.double()).sum() + (out_6 * w2.double()).sum()
    before = stats_of(mine)
    assert mine._executor_ok()
    h_m, out_m = mine(bi.to(dev))
    loss_m = (h_m * w1.to(dev)).sum() + (out_m * w2.to(dev)).sum()
    for l in (loss_r, loss_6, loss_m):
        l.backward()
    torch.cuda.synchronize()
    if p > 0:
        assert mine.dropout_state.tolist() == [SEED, 6]
    assert all(torch.equal(a, b) for a, b in zip(before, stats_of(mine)))
    bound = max(1e-5 * abs(loss_6.item()), 2 * abs(loss_r.item() - loss_6.item()))
    print(f"{kind} L={L} D={D} mode {mode} p={p}: loss {loss_m.item():.9g} fp64 "
          f"{loss_6.item():.9g} |err| {abs(loss_m.item() - loss_6.item()):.3g} bound {bound:.3g}")
    g32, g64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    bad, worst = {}, (0.0, None)
    for n, q in mine.named_parameters():
        b = max(1e-5 * g64[n].grad.norm().item(), 2 * err(g32[n].grad, g64[n].grad))
        e = err(q.grad, g64[n].grad)
        worst = max(worst, (e / b if b > 0 else float(e > 0), n))
        if e > b:
            bad[n] = (e, b, g64[n].grad.norm().item())
    print(f"  worst gradient |err| / bound = {worst[0]:.3f} ({worst[1]})")
    assert abs(loss_m.item() - loss_6.item()) <= bound
    assert not bad, bad
    return N


# (kind, L, D, B, the fp32 GIN's product mode).  GIN in fp32 takes the h3
# products (the BatchNorm backward with dz's row maxima) wherever ops.h3_ok
# holds, which under the default MOLCLR_FP32_GEMM is every width here; the x6
# cases set ops.FP32_GEMM to reach the executor's call without row maxima.
# The GCN executor never asks for row maxima.  D = 62 and 30 run padded to 64
# and 32 (_PaddedBatchNorm: the statistics are copied back unchanged).
FP32_CASES = [("gin", 2, 12, 5, "x6"), ("gin", 2, 12, 5, "h3"), ("gcn", 2, 12, 7, "h3"),
              ("gin", 5, 128, 40, "h3"), ("gcn", 5, 128, 40, "h3"), ("gin", 2, 300, 33, "h3"),
              ("gin", 5, 64, 9, "x6"), ("gin", 2, 62, 6, "h3"), ("gcn", 2, 30, 6, "h3")]


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("kind,L,D,B,gemm", FP32_CASES)
def test_modes_against_oracle(dev, monkeypatch, kind, L, D, B, gemm, mode):
    monkeypatch.setattr(ops, "FP32_GEMM", gemm)
    N = against_oracle(dev, kind, L, D, B, mode)
    Dp = D + (-D) % 4
    assert (ops.h3_ok(N, Dp) if kind == "gin" else ops.gcn_h3_ok(N, Dp)) == (gemm == "h3")


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("kind,L,D,B", [("gin-bf16", 2, 64, 9), ("gcn-bf16", 2, 64, 9),
                                        ("gin-bf16", 5, 64, 20), ("gcn-bf16", 5, 64, 20)])
def test_bf16_modes_against_emulating_oracle(dev, kind, L, D, B, mode):
    """emb_dim 64 in bf16 storage, both executors, against the bf16-emulating
    oracle under the same rule."""
    against_oracle(dev, kind, L, D, B, mode)


@pytest.mark.parametrize("kind,L,D,B,gemm", [("gin", 2, 64, 9, "h3"), ("gin", 3, 64, 9, "x6"),
                                             ("gcn", 3, 64, 9, "h3"), ("gin-bf16", 2, 64, 9, "h3"),
                                             ("gcn-bf16", 2, 64, 9, "h3")])
def test_frozen_dropout_against_oracle(dev, monkeypatch, kind, L, D, B, gemm):
    """Mode 2 with drop_ratio 0.3, fp32 and bf16: every layer's mask rebuilt by
    tests/philox.py and fed to the oracle."""
    monkeypatch.setattr(ops, "FP32_GEMM", gemm)
    against_oracle(dev, kind, L, D, B, 2, p=0.3, monkeypatch=monkeypatch)


@pytest.mark.parametrize("kind,L,D,B", [("gin", 2, 16, 4), ("gin", 3, 128, 33), ("gcn", 2, 32, 5),
                                        ("gcn", 3, 128, 33)])
def test_executor_matches_per_op_path_frozen(dev, kind, L, D, B):
    """As tests/test_gpu_models.py holds the training-mode pair: node
    embeddings and every parameter gradient bit-identical, buffers untouched."""
    from molclr_amd.gcn_molclr import GCN
    from molclr_amd.ginet_molclr import GINet
    torch.manual_seed(1)
    a = (GINet if kind == "gin" else GCN)(L, D, 64)
    randomize_stats(a, 5)
    a = a.to(dev)
    b = copy.deepcopy(a)
    b.use_executor = False
    xi, _ = SyntheticPairBatches(B, seed=L + D).next()
    xi = xi.to(dev)
    g = torch.randn(xi.x.shape[0], D, device=dev)
    for mode in (2, 0):
        outs = []
        for m in (a, b):
            set_mode(m, mode)
            m.zero_grad(set_to_none=True)
            before = stats_of(m)
            h, _ = m.encode(xi)
            (h * g).sum().backward()
            outs.append(h.detach())
            assert all(torch.equal(s, t) for s, t in zip(before, stats_of(m)))
        assert a._executor_ok() and not b._executor_ok()
        assert torch.equal(outs[0], outs[1])
        pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
        for n in pa:
            assert (pa[n].grad is None) == (pb[n].grad is None), n
            assert pa[n].grad is None or torch.equal(pa[n].grad, pb[n].grad), (mode, n)


@pytest.mark.parametrize("kind", ["gin", "gcn", "bf16"])
def test_frozen_dropout(dev, kind):
    """Mode 2 with drop_ratio 0.3: the output is dropped (it differs from mode
    0, and the last layer's zeros are the mask tests/philox.py rebuilds from
    the call's key); the backward sees the forward's mask (a dropped element
    of the last layer passes no gradient back: the gradient of sum(h) with
    respect to the last BatchNorm's bias counts the kept elements times
    1 / (1 - p)); resetting dropout_state repeats the gradient bit for bit."""
    from molclr_amd.gcn_molclr import GCN
    from molclr_amd.ginet_molclr import GINet
    torch.manual_seed(2)
    L, D, p = 2, 64, 0.3
    if kind == "gcn":
        m = GCN(L, D, 64, drop_ratio=p)
    else:
        m = GINet(L, D, 64, drop_ratio=p, precision="bf16" if kind == "bf16" else "fp32")
    randomize_stats(m, 9)
    m = m.to(dev)
    xi, _ = SyntheticPairBatches(9, seed=4).next()
    xi = xi.to(dev)
    set_mode(m, 0)
    with torch.no_grad():
        h0 = m.encode(xi)[0].float()
    set_mode(m, 2)
    before = stats_of(m)
    grads = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        if m.dropout_state is not None:
            m.dropout_state[1] = 0
        h, _ = m.encode(xi)
        key = m.dropout_state.clone()
        key[1] = 0  # the call this forward drew (the counter has moved on)
        h.float().sum().backward()
        grads.append([q.grad.clone() for q in m.parameters() if q.grad is not None])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    assert all(torch.equal(a, b) for a, b in zip(before, stats_of(m)))
    h = h.detach().float()
    N = h.shape[0]
    keep = torch.from_numpy(philox.dropout_mask(int(key[0]), 0, L - 1, p, N, D)).to(dev)
    assert not torch.equal(h, h0)
    assert bool((h[~keep.bool()] == 0).all().item())
    live = keep.bool() & (h0 != 0)
    assert bool((h[live] != 0).all().item())
    # the last layer has no ReLU: dbeta = sum over rows of keep / (1 - p)
    want = keep.float().sum(0) / (1 - p)
    got = m.batch_norms[L - 1].bias.grad.float()
    assert torch.allclose(got, want, rtol=1e-2 if kind == "bf16" else 1e-5, atol=0), (got, want)


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("kind", ["gin", "gcn", "gin-bf16", "gcn-bf16"])
def test_paired_and_staged_pass_frozen(dev, kind, p):
    """forward_pair and forward_staged (device-sized segments over padded
    buffers: 37 padding rows, 500 padding edges) in mode 2 equal the eager
    result -- two calls of forward, whose dropout rows are the views' own, so
    with dropout the eager side is forward_pair: loss 1e-6, gradient 1e-5,
    bf16 1e-4.  Running statistics stay bit-identical."""
    from molclr_amd.data import pair_graph
    from molclr_amd.graph_step import StagedPairGraph
    _, _, a = make_models(kind, 3, 64, p, 4)
    a = a.to(dev)
    b, c = copy.deepcopy(a), copy.deepcopy(a)
    xi, xj = SyntheticPairBatches(12, seed=8).next()
    xi, xj = xi.to(dev), xj.to(dev)
    ref = pair_graph(xi, xj)
    staged = StagedPairGraph(dev, ref.num_nodes + 37, ref.num_edges + 500, [12, 12])
    staged.stage([xi, xj])
    staged.build()
    w = torch.randn(24, 32, device=dev)
    losses, flats = [], []
    for m, fwd in ((a, lambda: a.forward_pair(xi, xj)[1]),
                   (b, lambda: b.forward_staged(staged)[1]),
                   (c, lambda: torch.cat([c(xi)[1], c(xj)[1]], 0) if p == 0
                    else c.forward_pair(xi, xj)[1])):
        set_mode(m, 2)
        if p > 0:
            m.dropout_state = torch.tensor([SEED, 2], dtype=torch.long, device=dev)
        before = stats_of(m)
        loss = (fwd() * w).sum()
        loss.backward()
        torch.cuda.synchronize()
        assert all(torch.equal(s, t) for s, t in zip(before, stats_of(m)))
        losses.append(loss.item())
        flats.append(torch.cat([q.grad.flatten() for q in m.parameters()]))
    tol = 1e-4 if kind.endswith("bf16") else 1e-5
    for k in (0, 1):
        print(f"{kind} p={p} {('pair', 'staged')[k]}: loss rel "
              f"{abs(losses[k] - losses[2]) / abs(losses[2]):.3g} grad rel "
              f"{err(flats[k], flats[2]) / flats[2].norm().item():.3g}")
    for k in (0, 1):
        assert abs(losses[k] - losses[2]) <= 1e-6 * abs(losses[2])
        assert err(flats[k], flats[2]) <= tol * flats[2].norm().item()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batch_norm_seg_eval_backward(dev, relu, dtype):
    """torch.ops.molclr.batch_norm_seg in eval mode differentiates; one segment
    equals ops.batch_norm's eval backward bit for bit (fp32); opcheck passes
    for the new op."""
    import molclr_amd.torch_ops as tops
    torch.manual_seed(0)
    n, D = 70, 24
    bn = torch.nn.BatchNorm1d(D).to(dev)
    with torch.no_grad():
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    bn.eval()
    z = torch.randn(n, D, device=dev).to(dtype).requires_grad_(True)
    dy = torch.randn(n, D, device=dev).to(dtype)
    y = tops.batch_norm_seg_module(z, bn, [n], relu)
    y.backward(dy)
    got = (z.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone())
    if dtype == torch.float32:
        bn.zero_grad(set_to_none=True)
        z2 = z.detach().clone().requires_grad_(True)
        y2 = ops.batch_norm(z2, bn, relu=relu)
        y2.backward(dy)
        assert torch.equal(y, y2)
        assert torch.equal(got[0], z2.grad) and torch.equal(got[1], bn.weight.grad)
        assert torch.equal(got[2], bn.bias.grad)
    # two segments: the same statistics for both, so the same dz
    bn.zero_grad(set_to_none=True)
    z3 = z.detach().clone().requires_grad_(True)
    tops.batch_norm_seg_module(z3, bn, [n - 9, 9], relu).backward(dy)
    assert torch.equal(z3.grad, got[0])
    mean = bn.running_mean.detach().clone().repeat(2, 1)
    invstd = (bn.running_var.detach() + bn.eps).rsqrt().repeat(2, 1)
    torch.library.opcheck(torch.ops.molclr.batch_norm_seg_bwd_frozen.default,
                          (dy, z.detach(), bn.weight.detach(), bn.bias.detach(), mean, invstd,
                           [n - 9, 9], relu))


@pytest.mark.parametrize("kind", ["gin", "gcn", "bf16"])
def test_captured_finetune_step_frozen(dev, kind):
    """CapturedFinetuneStep on a frozen model (drop_ratio 0, two buckets):
    replays follow eager from the same state at the captured steps' bounds; the
    running statistics never move; flipping freeze_bn after capture is caught."""
    crit = "cross_entropy"
    data = batches(crit, dev)
    ref = make(kind, crit, 5)
    randomize_stats(ref, 1)
    ref = ref.to(dev)
    cap = copy.deepcopy(ref)
    for m in (ref, cap):
        m.train()
        m.freeze_bn = True
    before = stats_of(cap)
    opts_r, opts_c = optimizers(ref), optimizers(cap)
    step = CapturedFinetuneStep(cap, opts_c, crit, None, **Q)
    use = [data[0], data[6], data[0], data[6]]
    for i, d in enumerate(use):
        sync(ref, opts_r, cap, opts_c)
        loss_r = eager_step(ref, opts_r, d, crit, None)
        loss_c = step.step(d).clone()
        compare(i, kind, step, ref, opts_r, cap, opts_c, loss_r, loss_c)
    assert step.captures == 2 and step.replays == 4
    assert all(torch.equal(a, b) for a, b in zip(before, stats_of(cap)))
    assert all(torch.equal(a, b) for a, b in zip(before, stats_of(ref)))
    step.check()
    cap.freeze_bn = False
    with pytest.raises(RuntimeError, match="BatchNorm"):
        step.step(data[0])
    cap.freeze_bn = True
    step.step(data[0])  # the captured mode again: replays
    step.close()
