"""The GCN encoder's bf16 storage path (precision='bf16'): the aggregation
kernels bit for bit against the fp32 ones, the executor against the oracle that
rounds where the kernels store bf16 (tests/gcn_bf16_ref.py) and against the
plain fp64 oracle, dropout under the kernels' own masks, determinism, isolation
of the fp32 path, the captured steps and the trainers' ``gcn_bf16`` key.

Bounds: tests/test_gpu_bf16.py's (EMU_TOL with the 1.5x self-noise margin of
test_ginet_bf16_encoder_vs_bf16_emulating_oracle; BF16_TOL against fp64) and
the captured steps' bf16 bounds of tests/test_gpu_graph_step.py /
test_gpu_finetune_step.py (loss 1e-6, flat gradient 1e-4, statistics 1e-6).
"""
import copy
import warnings

import numpy as np
import pytest
import torch

import oracle.reference_cpu as ref_cpu
from molclr_amd import _lib
from molclr_amd.data import DeviceGraph
from molclr_amd.dataset import SyntheticPairBatches, collate_views, random_molecule
from oracle.reference_cpu import RefGCN

from .gcn_bf16_ref import emu_gcn
from .test_gpu_bf16 import BF16_TOL, EMU_TOL, bf, rel
from .test_gpu_models import pre_bn_bias

pytestmark = pytest.mark.gpu
FEAT = 64


# ---------------------------------------------------------------------------
# 1. the aggregation kernels, bit for bit
# ---------------------------------------------------------------------------
def _hand_graph():
    """8 atoms, symmetric bonds: in- (= out-) degrees 0, 6, 4, 3, 3, 2, 1, 1 --
    an isolated atom, every slot count 1..4 and one row that walks the CSR (and
    the CSC in the backward)."""
    bonds = [(1, k) for k in range(2, 8)] + [(2, 3), (2, 4), (2, 5), (3, 4)]
    ei = torch.tensor([e for a, b in bonds for e in ((a, b), (b, a))], dtype=torch.long).t()
    g = torch.Generator().manual_seed(3)
    attr = torch.stack([torch.randint(0, 4, (len(bonds),), generator=g),
                        torch.randint(0, 3, (len(bonds),), generator=g)], 1)
    deg = torch.bincount(ei[1], minlength=8).tolist()
    assert deg == [0, 6, 4, 3, 3, 2, 1, 1]
    return ei.contiguous(), attr.repeat_interleave(2, 0).contiguous(), 8


def _graphs(dev):
    b = SyntheticPairBatches(20, seed=7, shape="pubchem").next()[0]
    out = {"hand": _hand_graph(),
           "single": (torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, 2, dtype=torch.long), 1),
           "batch20": (b.edge_index, b.edge_attr, int(b.x.shape[0]))}
    return {k: (DeviceGraph(ei.to(dev), ea.to(dev), n), n) for k, (ei, ea, n) in out.items()}


@pytest.fixture(scope="module")
def agg_graphs(dev):
    return _graphs(dev)


@pytest.mark.parametrize("D", [8, 12, 304, 512])  # 12: the 8-byte (4-element) units
def test_gcn_aggregation_bf16_bit_exact(dev, agg_graphs, D):
    """On bf16-representable inputs the bf16 kernels equal the fp32 kernels on
    the widened values: out and dxw rounded once, dE1 / dE2 / dbias bit for
    bit (accumulate 0 and 1)."""
    lib = _lib.load()
    for name, (g, N) in agg_graphs.items():
        gen = torch.Generator().manual_seed(D + N)
        rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        xw = bf(rnd(N, D)).to(dev)
        E1, E2, bias = rnd(5, 1).to(dev), rnd(3, 1).to(dev), rnd(D).to(dev)
        out_b = torch.empty(N, D, dtype=torch.bfloat16, device=dev)
        out_f = torch.empty(N, D, device=dev)
        xf = xw.float()
        args = (g.rowptr.data_ptr(), g.col.data_ptr(), g.ecode.data_ptr(), g.nbr.data_ptr(),
                E1.data_ptr(), E2.data_ptr(), bias.data_ptr())
        assert lib.molclr_gcn_aggregate_fwd_bf16(xw.data_ptr(), *args, out_b.data_ptr(), N, D,
                                                 None) == 0
        assert lib.molclr_gcn_aggregate_fwd(xf.data_ptr(), *args, out_f.data_ptr(), N, D, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(out_b, bf(out_f)), (name, D)
        assert out_f.abs().sum() > 0

        gb = bf(rnd(N, D)).to(dev)
        gf = gb.float()
        wsb = lib.molclr_gcn_aggregate_bwd_workspace_bytes(N, D)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        bargs = (g.rowptr_t.data_ptr(), g.col_t.data_ptr(), g.nbr_t.data_ptr(), g.ecount.data_ptr())
        init = [rnd(5, 1).to(dev), rnd(3, 1).to(dev), rnd(D).to(dev)]
        for acc in (0, 1):
            dxb = torch.empty(N, D, dtype=torch.bfloat16, device=dev)
            dxf = torch.empty(N, D, device=dev)
            tb, tf = [t.clone() for t in init], [t.clone() for t in init]
            assert lib.molclr_gcn_aggregate_bwd_bf16(
                gb.data_ptr(), *bargs, dxb.data_ptr(), *[t.data_ptr() for t in tb], N, D, acc,
                ws.data_ptr(), wsb, None) == 0
            assert lib.molclr_gcn_aggregate_bwd(
                gf.data_ptr(), *bargs, dxf.data_ptr(), *[t.data_ptr() for t in tf], N, D, acc,
                ws.data_ptr(), wsb, None) == 0
            torch.cuda.synchronize()
            assert torch.equal(dxb, bf(dxf)), (name, D, acc)
            for what, a, b_, i in zip(("dE1", "dE2", "dbias"), tb, tf, init):
                assert torch.equal(a, b_), (name, D, acc, what)
                assert not torch.equal(a, i), (name, D, acc, what)  # written


# ---------------------------------------------------------------------------
# 2. / 3. the executor against the emulating oracle (and the fp64 oracle)
# ---------------------------------------------------------------------------
def batch6(seed=5):
    rng = np.random.default_rng(seed)
    mols = [random_molecule(rng) for _ in range(6)]
    return collate_views([(m.x, m.edge_index, m.edge_attr) for m in mols])


def _trio(L, D, drop=0.0, seed=7):
    """(emulation fp32, emulation fp64, plain fp64 oracle, the bf16 model), one
    set of parameters."""
    from molclr_amd.gcn_molclr import GCN
    torch.manual_seed(seed)
    emu32 = emu_gcn(RefGCN, L, D, FEAT, drop_ratio=drop)
    ref64 = RefGCN(L, D, FEAT, drop_ratio=drop)
    ref64.load_state_dict(emu32.state_dict())
    mine = GCN(L, D, FEAT, drop_ratio=drop, precision="bf16")
    mine.load_state_dict(emu32.state_dict())
    return emu32, copy.deepcopy(emu32).double(), ref64.double(), mine


def _loss(h, out):
    return h.square().mean() + out.square().mean()


def _run(model, views, feed=None):
    """(h, out, loss) of ``model`` over the views one after the other (the
    reference's two calls), the loss backpropagated."""
    hs, outs, row = [], [], 0
    for v in views:
        if feed is not None:
            feed.view(slice(row, row + v.x.shape[0]))
        row += v.x.shape[0]
        h, out = model(v)
        hs.append(h)
        outs.append(out)
    h, out = torch.cat(hs), torch.cat(outs)
    loss = _loss(h, out)
    loss.backward()
    return h, out, loss


def _check(tag, L, mine, got, emu32, emu64, ref64, feed=None, views=None):
    """got = (h, out, loss) of the bf16 model, its gradients in place."""
    e32, e64, r64 = (_run(m, views, feed) for m in (emu32, emu64, ref64))
    hm, om, lm = got
    # the emulation: 1e-2, or 1.5x what the same emulation moves between fp32
    # and fp64 evaluation where that is larger; gradients also under the gross
    # bound
    g64, g32 = dict(emu64.named_parameters()), dict(emu32.named_parameters())
    figs, bad = {}, {}
    for what, a, b32, b64 in (("h", hm, e32[0], e64[0]), ("out", om, e32[1], e64[1])):
        figs[what] = (rel(a, b64), rel(b32, b64))
    checked = 0
    for n, p in mine.named_parameters():
        if pre_bn_bias(n):  # the bias in front of a BatchNorm: exact gradient 0
            continue
        checked += 1
        figs[n] = (rel(p.grad, g64[n].grad), rel(g32[n].grad, g64[n].grad))
    for what, (e, self_noise) in figs.items():
        print(f"{tag} emulation {what}: {e:.3e} (fp32 emulation {self_noise:.3e})")
        if e > max(EMU_TOL, 1.5 * self_noise) or (what not in ("h", "out") and e > BF16_TOL["grad"]):
            bad[what] = (e, self_noise)
    assert checked == 2 + 5 * L + 6
    for name, buf in emu64.named_buffers():
        if not name.endswith("num_batches_tracked"):
            e = rel(dict(mine.named_buffers())[name], buf)
            print(f"{tag} emulation {name}: {e:.3e}")
            if e > EMU_TOL:
                bad[name] = e
    # the plain fp64 oracle: the gross-error guard the GIN model has
    gr = dict(ref64.named_parameters())
    gerr = {n: rel(p.grad, gr[n].grad) for n, p in mine.named_parameters() if not pre_bn_bias(n)}
    errs = {"h": rel(hm, r64[0]), "out": rel(om, r64[1]),
            "loss": abs(lm.item() - r64[2].item()) / abs(r64[2].item()), "grad": max(gerr.values())}
    print(f"{tag} fp64 oracle:", {k: f"{v:.3e}" for k, v in errs.items()})
    for k, v in errs.items():
        if v >= BF16_TOL[k]:
            bad["fp64 " + k] = (v, sorted(gerr.items(), key=lambda kv: -kv[1])[:4])
    assert not bad, bad


@pytest.mark.parametrize("L,D", [(2, 40), (2, 44), (3, 40), (3, 44)])  # 44 runs padded to 48
def test_gcn_bf16_executor_vs_emulating_oracle(dev, L, D):
    emu32, emu64, ref64, mine = _trio(L, D)
    mine = mine.to(dev)
    data = batch6()
    assert mine._executor_ok() and mine._dim_pad() == (-D) % 8
    h, out = mine(data.to(dev))
    loss = _loss(h, out)
    loss.backward()
    _check(f"L={L} D={D}", L, mine, (h, out, loss), emu32, emu64, ref64, views=[data])


def test_gcn_bf16_paired_pass_keeps_per_view_statistics(dev):
    """forward_pair against the oracle's two calls: every BatchNorm normalises
    each view with its own statistics and updates the running statistics for
    view i, then view j (checked by _check's buffer comparison)."""
    L, D = 3, 40
    emu32, emu64, ref64, mine = _trio(L, D)
    mine = mine.to(dev)
    xi, xj = batch6(5), batch6(6)
    h, out = mine.forward_pair(xi.to(dev), xj.to(dev))
    loss = _loss(h, out)
    loss.backward()
    assert int(mine.batch_norms[0].num_batches_tracked) == 2
    _check("paired", L, mine, (h, out, loss), emu32, emu64, ref64, views=[xi, xj])


def test_gcn_bf16_dropout_under_the_kernels_masks(dev, monkeypatch):
    from .test_gpu_dropout import MaskFeed, export_masks, state
    L, D, P = 2, 40, 0.3
    emu32, emu64, ref64, mine = _trio(L, D, drop=P)
    mine = mine.to(dev).train()
    data = batch6()
    mine.dropout_state = state(dev, call=1)
    feed = MaskFeed(export_masks(mine, P, data.x.shape[0]), P)
    monkeypatch.setattr(ref_cpu.F, "dropout", feed)
    h, out = mine(data.to(dev))
    loss = _loss(h, out)
    loss.backward()
    assert mine.dropout_state.tolist()[1] == 2
    _check("dropout", L, mine, (h, out, loss), emu32, emu64, ref64, feed=feed, views=[data])


# ---------------------------------------------------------------------------
# 4. determinism, and the fp32 path left alone
# ---------------------------------------------------------------------------
def test_gcn_bf16_training_steps_are_deterministic(dev):
    from molclr_amd.gcn_molclr import GCN
    from molclr_amd.nt_xent import NTXentLoss
    from molclr_amd.ops import l2_normalize
    from molclr_amd.optim import FusedAdam
    xi, xj = SyntheticPairBatches(32, seed=4, shape="pubchem").next()
    res = []
    for _ in range(2):
        torch.manual_seed(0)
        m = GCN(3, 64, FEAT, precision="bf16").to(dev)
        opt = FusedAdam(m.parameters(), 5e-4, weight_decay=1e-5)
        crit = NTXentLoss(dev, 32, 0.1, True)
        for _ in range(2):
            opt.zero_grad()
            loss = crit.forward_pair(l2_normalize(m.forward_pair(xi.to(dev), xj.to(dev))[1]))
            loss.backward()
            opt.step()
        assert torch.isfinite(loss)
        res.append((opt.flat.clone(), opt.flat_grad.clone(), loss.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_fp32_gcn_is_untouched_by_a_bf16_one(dev):
    """An fp32 GCN before and after a bf16 one -- a separate model, and the
    SAME parameters run as bf16 in between (the bf16 products read plane 0 of
    the very images the fp32 products read): h, out and gradients bit for bit."""
    from molclr_amd.gcn_molclr import GCN
    data = batch6().to(dev)

    def run(m):
        m.zero_grad()
        h, out = m(data)
        _loss(h, out).backward()
        return [h.detach().clone(), out.detach().clone()] + [p.grad.clone() for p in m.parameters()]

    def make(precision):
        torch.manual_seed(0)
        return GCN(3, 64, FEAT, precision=precision).to(dev)

    before_model = make("fp32")
    before = run(before_model)
    run(make("bf16"))
    before_model.precision = "bf16"  # the same weights, hence the same cached images
    as_bf16 = run(before_model)
    assert as_bf16[0].dtype == torch.float32 and not torch.equal(as_bf16[0], before[0])
    before_model.precision = "fp32"
    again = run(before_model)
    after = run(make("fp32"))
    for a, b, c in zip(before, again, after):
        assert torch.equal(a, b) and torch.equal(a, c)


# ---------------------------------------------------------------------------
# 5. the captured steps
# ---------------------------------------------------------------------------
def test_captured_train_step_takes_a_bf16_gcn(dev):
    from molclr_amd.gcn_molclr import GCN
    from molclr_amd.graph_step import CapturedTrainStep
    from molclr_amd.nt_xent import NTXentLoss
    from molclr_amd.optim import FusedAdam

    from .test_gpu_graph_step import _eager_step, _sync, _to
    B = 32
    batches = [_to(p, dev) for p in SyntheticPairBatches(B, seed=11).take(6)]
    torch.manual_seed(5)
    ref = GCN(num_layer=3, emb_dim=64, feat_dim=64, precision="bf16").to(dev)
    cap = copy.deepcopy(ref)
    opt_r = FusedAdam(ref.parameters(), 5e-4, weight_decay=1e-5)
    opt_c = FusedAdam(cap.parameters(), 5e-4, weight_decay=1e-5)
    crit = NTXentLoss(dev, B, 0.1, True)
    step = CapturedTrainStep(cap, opt_c, crit, node_quantum=128, edge_quantum=512, node_slack=0)
    for i, (xi, xj) in enumerate(batches + batches[:2]):
        _sync(ref, opt_r, cap, opt_c)
        lr_ = _eager_step(ref, opt_r, crit, xi, xj)
        lc = step(xi, xj).clone()
        torch.cuda.synchronize()
        r = rel(opt_c.flat_grad, opt_r.flat_grad)
        print(f"step {i}: loss eager {lr_.item():.9g} replay {lc.item():.9g} flat gradient {r:.3g}")
        assert abs(lc.item() - lr_.item()) <= 1e-6 * abs(lr_.item()), (i, lc.item(), lr_.item())
        assert r < 1e-4, (i, r)
        for bc, br in zip(cap.batch_norms, ref.batch_norms):
            assert rel(bc.running_mean, br.running_mean) < 1e-6, i
            assert rel(bc.running_var, br.running_var) < 1e-6, i
            assert int(bc.num_batches_tracked) == int(br.num_batches_tracked), i
    assert step.captures >= 2 and step.replays == len(batches) + 2
    step.last_graph.check()
    step.close()


def test_captured_finetune_step_takes_a_bf16_gcn(dev):
    from molclr_amd.finetune_step import CapturedFinetuneStep, unsupported_reason
    from molclr_amd.gcn_finetune import GCN

    from .test_gpu_finetune_step import Q, batches, compare, eager_step, optimizers, sync
    crit = "mse"
    data = batches(crit, dev)[0]
    torch.manual_seed(5)
    ref = GCN("regression", 2, 64, 128, precision="bf16").to(dev)
    assert unsupported_reason(ref) is None
    cap = copy.deepcopy(ref)
    opts_r, opts_c = optimizers(ref), optimizers(cap)
    step = CapturedFinetuneStep(cap, opts_c, crit, None, **Q)
    for i in range(3):
        sync(ref, opts_r, cap, opts_c)
        loss_r = eager_step(ref, opts_r, data, crit, None)
        loss_c = step.step(data).clone()
        compare(i, "bf16", step, ref, opts_r, cap, opts_c, loss_r, loss_c)
    assert step.captures == 1 and step.replays == 3 and len(step.buckets) == 1
    step.check()
    step.close()


# ---------------------------------------------------------------------------
# 6. the trainers' gcn_bf16 key
# ---------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.train_loss = []

    def add_scalar(self, tag, value, global_step=None):
        if tag == "train_loss":
            self.train_loss.append(float(torch.as_tensor(value).detach()))

    def close(self):
        pass


def _first_loss(trainer, precision):
    """Train with a recording writer; the model must be built in ``precision``
    without a warning.  Returns the logged training losses."""
    built = []
    build = trainer.build_model

    def build_model():
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            built.append(build())
        assert not [str(w.message) for w in caught if issubclass(w.category, RuntimeWarning)]
        return built[-1]

    trainer.build_model = build_model
    trainer.writer = rec = _Recorder()
    trainer.train()
    assert built and all(m.precision == precision for m in built)
    assert all(p.dtype == torch.float32 for p in built[0].parameters())  # fp32 master weights
    assert len(rec.train_loss) == 2 and all(np.isfinite(rec.train_loss)), rec.train_loss
    return rec.train_loss


def test_pretraining_trainer_gcn_bf16_key(dev, tmp_path, monkeypatch):
    from molclr_amd.molclr import MolCLR

    from .test_gpu_trainer import _config, _wrapper
    monkeypatch.chdir(tmp_path)
    first = {}
    for prec in ("bf16", "fp32"):
        # 40 molecules, a fifth for validation: two training steps of 16
        config = _config("node", "synthetic:40", tmp_path / prec, model_type="gcn",
                         fp16=prec == "bf16")
        config["gcn_bf16"] = prec == "bf16"
        torch.manual_seed(0)
        first[prec] = _first_loss(MolCLR(_wrapper(config), config), prec)[0]
    print("first losses", first)
    assert abs(first["bf16"] - first["fp32"]) <= BF16_TOL["loss"] * abs(first["fp32"])


def test_finetune_trainer_gcn_bf16_key(dev, tmp_path):
    from molclr_amd.dataset_test import MolTestDatasetWrapper
    from molclr_amd.finetune import FineTune

    from .test_gpu_finetune import config_of, write_csv
    write_csv(tmp_path / "data.csv", "regression", n=80)
    first = {}
    for prec in ("bf16", "fp32"):
        # 80 molecules, a tenth each for validation and test: two steps of 32
        cfg = config_of(tmp_path, "regression", "gcn", epochs=1, log_every_n_steps=1,
                        fp16_precision=prec == "bf16", gcn_bf16=prec == "bf16")
        ft = FineTune(MolTestDatasetWrapper(cfg["batch_size"], **cfg["dataset"]), cfg)
        first[prec] = _first_loss(ft, prec)[0]
    print("first losses", first)
    assert abs(first["bf16"] - first["fp32"]) <= BF16_TOL["loss"] * abs(first["fp32"])
