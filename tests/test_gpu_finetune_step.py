"""The captured fine-tuning step and evaluation pass (molclr_amd.finetune_step)
against the eager loop of molclr_amd.finetune, at the bounds
tests/test_gpu_graph_step.py holds the captured pre-training step to: loss
1e-6 relative, flat gradient 1e-5 norm-wise (bf16 storage 1e-4), running
statistics 1e-6, counters equal.

Shapes: the models of tests/test_gpu_finetune.py (L = 2, D = 64, FEAT = 128),
batches of 32 random molecules and one partial batch of 5, node_quantum 128 /
edge_quantum 512 / node_slack 0, so several buckets are captured and replayed
with about a quarter of the rows padding.
"""
import copy
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from molclr_amd import _lib, ops
from molclr_amd.dataset import collate_views, random_molecule
from molclr_amd.finetune import Normalizer, mae_score, rmse_score, roc_auc_score
from molclr_amd.finetune_step import CapturedEval, CapturedFinetuneStep
from molclr_amd.optim import FusedAdam

from .test_gpu_finetune import FEAT, L, config_of, write_csv
from .test_gpu_graph_step import _Poison

pytestmark = pytest.mark.gpu
Q = dict(node_quantum=128, edge_quantum=512, node_slack=0)
KINDS = ["gin", "bf16", "gcn"]
CRITS = ["cross_entropy", "mse", "l1"]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).norm().item() / max(b.norm().item(), 1e-30)


def make(kind, crit, seed, drop=0.0):
    from molclr_amd.gcn_finetune import GCN
    from molclr_amd.ginet_finetune import GINet
    task = "classification" if crit == "cross_entropy" else "regression"
    torch.manual_seed(seed)
    if kind == "gcn":
        return GCN(task, L, 64, FEAT, drop)
    return GINet(task, L, 64, FEAT, drop, precision="bf16" if kind == "bf16" else "fp32")


def optimizers(model):
    """FineTune.build_optimizers: 'pred_lin' parameters (GCN's head) in a group
    of their own with another learning rate."""
    head = [p for n, p in model.named_parameters() if "pred_lin" in n]
    base = [p for n, p in model.named_parameters() if "pred_lin" not in n]
    opts = [FusedAdam(base, 5e-4, weight_decay=1e-5)]
    if head:
        opts.append(FusedAdam(head, 2e-3, weight_decay=1e-5))
    return opts


def labelled(B, crit, rng, dev, shape="uniform"):
    mols = [random_molecule(rng, shape) for _ in range(B)]
    b = collate_views([(m.x, m.edge_index, m.edge_attr) for m in mols])
    if crit == "cross_entropy":
        b.y = torch.from_numpy(rng.integers(0, 2, (B, 1)))
    else:  # a learnable-sized target with an offset, so the normaliser matters
        b.y = torch.from_numpy((rng.normal(size=(B, 1)) * 3 + 7).astype(np.float32))
    return b.to(dev)


_BATCHES = {}


def batches(crit, dev):
    """Six batches of 32 -- two size distributions alternating, so that they
    spread over several node buckets -- and a partial one of 5, made once per
    criterion and never modified."""
    if crit not in _BATCHES:
        rng = np.random.default_rng(17)
        _BATCHES[crit] = [labelled(32, crit, rng, dev, ("uniform", "pubchem")[k % 2])
                          for k in range(6)] + [labelled(5, crit, rng, dev)]
    return _BATCHES[crit]


def normalizer_of(crit, dev):
    """qm7 / qm9 style: L1 regression on normalised labels."""
    if crit != "l1":
        return None
    return Normalizer(torch.cat([b.y for b in batches(crit, dev)]))


def target_of(data, crit, norm):
    if crit == "cross_entropy":
        return data.y.flatten()
    return norm.norm(data.y) if norm else data.y


def eager_step(model, opts, data, crit, norm):
    """FineTune.train_step."""
    for o in opts:
        o.zero_grad()
    _, _, loss = model.loss(data, target_of(data, crit, norm), crit)
    loss.backward()
    for o in opts:
        o.step()
    return loss.detach().clone()


def sync(ref, opts_r, cap, opts_c):
    """ref's optimizer and BatchNorm state := cap's (tests/test_gpu_graph_step.py
    _sync, for every optimizer)."""
    with torch.no_grad():
        for o_r, o_c in zip(opts_r, opts_c):
            for a, b in ((o_r.flat, o_c.flat), (o_r.exp_avg, o_c.exp_avg),
                         (o_r.exp_avg_sq, o_c.exp_avg_sq), (o_r._step_dev, o_c._step_dev)):
                a.copy_(b)
        for br, bc in zip(ref.batch_norms, cap.batch_norms):
            br.running_mean.copy_(bc.running_mean)
            br.running_var.copy_(bc.running_var)
            br.num_batches_tracked.copy_(bc.num_batches_tracked)
    ops.bump_param_generation()


def compare(i, kind, step, ref, opts_r, cap, opts_c, loss_r, loss_c):
    torch.cuda.synchronize()
    print(f"step {i}: loss eager {loss_r.item():.9g} replay {loss_c.item():.9g}")
    assert abs(loss_c.item() - loss_r.item()) <= 1e-6 * abs(loss_r.item()), \
        (i, loss_c.item(), loss_r.item())
    tol = 1e-4 if kind == "bf16" else 1e-5
    for k, (o_c, o_r) in enumerate(zip(opts_c, opts_r)):
        r = rel(o_c.flat_grad, o_r.flat_grad)
        print(f"  optimizer {k}: flat gradient rel {r:.3g}")
        if r >= tol:
            per = sorted(((rel(pc.grad, pr.grad), n, pc.grad.norm().item(), pr.grad.norm().item())
                          for (n, pc), pr in zip(cap.named_parameters(), ref.parameters())),
                         reverse=True)[:8]
            raise AssertionError(f"step {i}, optimizer {k}: rel {r:.3g}, captures {step.captures}, "
                                 f"replays {step.replays}; worst (rel, name, |cap|, |eager|): {per}")
        assert o_c.steps_taken == o_r.steps_taken
    for bc, br in zip(cap.batch_norms, ref.batch_norms):
        assert rel(bc.running_mean, br.running_mean) < 1e-6, i
        assert rel(bc.running_var, br.running_var) < 1e-6, i
        assert int(bc.num_batches_tracked) == int(br.num_batches_tracked), i


@pytest.mark.parametrize("crit", CRITS)
@pytest.mark.parametrize("kind", KINDS)
def test_replay_follows_eager(dev, kind, crit):
    """Every replay (first captures of several buckets, the partial batch's own
    bucket, later replays) against the eager step from the same state."""
    data = batches(crit, dev)
    norm = normalizer_of(crit, dev)
    ref = make(kind, crit, 5).to(dev)
    cap = copy.deepcopy(ref)
    opts_r, opts_c = optimizers(ref), optimizers(cap)
    assert len(opts_c) == (2 if kind == "gcn" else 1)
    step = CapturedFinetuneStep(cap, opts_c, crit, norm, **Q)
    for i, d in enumerate(data + data[:3]):
        sync(ref, opts_r, cap, opts_c)
        loss_r = eager_step(ref, opts_r, d, crit, norm)
        loss_c = step.step(d).clone()
        compare(i, kind, step, ref, opts_r, cap, opts_c, loss_r, loss_c)
    print("buckets", step.buckets)
    # several buckets of 32 and the partial batch's own; the last three replays
    # captured nothing
    assert 3 <= step.captures <= len(data) and step.replays == len(data) + 3
    assert step.bucket(data[6]) in step.buckets and step.bucket(data[6])[2] == 5
    step.check()
    # eager use after replays sees the replayed weights (planes refreshed)
    sync(ref, opts_r, cap, opts_c)
    cap.eval()
    ref.eval()
    with torch.no_grad():
        assert torch.equal(cap(data[0])[1], ref(data[0])[1])
    step.close()


def test_two_optimizers_follow_their_schedulers(dev):
    """GCN's pred_lin group has its own learning rate; a scheduler-style change
    of one group's lr between replays is what the next replay uses."""
    data = batches("mse", dev)
    model = make("gcn", "mse", 1).to(dev)
    base, head = optimizers(model)
    step = CapturedFinetuneStep(model, [base, head], "mse", **Q)
    step.step(data[0])
    base_before, head_before = base.flat.clone(), head.flat.clone()
    head.param_groups[0]["lr"] = 0.0
    step.step(data[0])
    torch.cuda.synchronize()
    assert torch.equal(head.flat, head_before) and not torch.equal(base.flat, base_before)
    base_before = base.flat.clone()
    base.param_groups[0]["lr"] = 0.0
    head.param_groups[0]["lr"] = 2e-3
    step.step(data[0])
    torch.cuda.synchronize()
    assert torch.equal(base.flat, base_before) and not torch.equal(head.flat, head_before)
    assert base.steps_taken == 3 and head.steps_taken == 3
    assert step.captures == 1 and step.replays == 3


@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_dropout_replays(dev, kind):
    """drop_ratio 0.3: the masks come from the model's device counter, so a
    replay from a restored dropout_state is the eager step from that state,
    and consecutive replays draw fresh masks."""
    crit = "cross_entropy"
    data = batches(crit, dev)
    ref = make(kind, crit, 8, drop=0.3).to(dev)
    cap = copy.deepcopy(ref)
    opts_r, opts_c = optimizers(ref), optimizers(cap)
    step = CapturedFinetuneStep(cap, opts_c, crit, **Q)
    step.step(data[0])  # captures; the model's dropout_state exists from here on
    for i, d in enumerate([data[1], data[0], data[1]]):
        state = cap.dropout_state.clone()
        sync(ref, opts_r, cap, opts_c)
        ref.dropout_state = state.clone()
        loss_r = eager_step(ref, opts_r, d, crit, None)
        cap.dropout_state.copy_(state)  # in place: the graph holds its address
        loss_c = step.step(d).clone()
        compare(i, kind, step, ref, opts_r, cap, opts_c, loss_r, loss_c)
        assert torch.equal(cap.dropout_state, ref.dropout_state)
        assert int(cap.dropout_state[1]) == int(state[1]) + 1
    for o in opts_c:  # parameters fixed: only the masks differ between replays
        o.param_groups[0]["lr"] = 0.0
    a = step.step(data[0]).clone()
    b = step.step(data[0]).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(a) and torch.isfinite(b) and a.item() != b.item()


def test_labels_status_is_sticky_and_targets_are_staged(dev):
    crit = "cross_entropy"
    data = batches(crit, dev)
    ref = make("gin", crit, 3).to(dev)
    cap = copy.deepcopy(ref)
    opts_r, opts_c = optimizers(ref), optimizers(cap)
    step = CapturedFinetuneStep(cap, opts_c, crit, **Q)
    # the same graph with other targets: the loss is the eager one for them
    other = copy.copy(data[0])
    other.y = 1 - data[0].y
    losses = []
    for i, d in enumerate([data[0], other, data[0]]):
        sync(ref, opts_r, cap, opts_c)
        loss_r = eager_step(ref, opts_r, d, crit, None)
        loss_c = step.step(d).clone()
        compare(i, "gin", step, ref, opts_r, cap, opts_c, loss_r, loss_c)
        losses.append(loss_c.item())
    assert step.captures == 1 and losses[0] != losses[1]
    step.check()
    # a class label outside [0, 2) at step k, no check until step k + 3
    bad = copy.copy(data[1])
    bad.y = data[1].y.clone()
    bad.y[3, 0] = 5
    step.step(bad)
    for d in data[2:5]:
        step.step(d)
    with pytest.raises(ValueError, match="class label"):
        step.check()


def _poisoned(dev, kind, value, order, evals):
    crit = "cross_entropy"
    with _Poison(value):
        model = make(kind, crit, 9).to(dev)
        opts = optimizers(model)
        step = CapturedFinetuneStep(model, opts, crit, **Q)
        losses = [step.step(d).clone() for d in order]
        grads = [o.flat_grad.clone() for o in opts]
        flats = [o.flat.clone() for o in opts]
        ev = CapturedEval(model, crit, **Q)
        out = ev.run(evals)
        step.close()
        ev.close()
        torch.cuda.synchronize()
        bn = [(b.running_mean.clone(), b.running_var.clone()) for b in model.batch_norms]
        return torch.stack(losses), grads, flats, bn, out


@pytest.mark.parametrize("kind", KINDS)
def test_no_uninitialised_reads(dev, kind):
    """tests/test_gpu_graph_step.py test_no_uninitialised_reads for the new
    step and evaluation pass: every fresh floating-point buffer pre-filled
    with 0, 3e38 or NaN, bit-identical results across the fills."""
    data = batches("cross_entropy", dev)
    order = data[:4] + [data[6], data[0], data[2], data[1]]
    runs = {v: _poisoned(dev, kind, v, order, [data[4], data[6], data[5]])
            for v in (0.0, 3e38, float("nan"))}
    base = runs[0.0]
    assert torch.isfinite(base[0]).all()
    for v, r in runs.items():
        assert torch.equal(r[0], base[0]), (v, r[0], base[0])
        for a, b in zip(r[1] + r[2], base[1] + base[2]):
            assert torch.equal(a, b), (v, rel(a, b))
        for (m, s), (m0, s0) in zip(r[3], base[3]):
            assert torch.equal(m, m0) and torch.equal(s, s0), v
        assert r[4][0] == base[4][0], v
        assert np.array_equal(r[4][1], base[4][1]) and np.array_equal(r[4][2], base[4][2]), v


def eager_evaluate(model, loader, crit, norm):
    """The body of FineTune._evaluate."""
    predictions, labels = [], []
    total, num_data = 0.0, 0
    with torch.no_grad():
        model.eval()
        for data in loader:
            _, pred, loss = model.loss(data, target_of(data, crit, norm), crit)
            total += loss.item() * data.y.size(0)
            num_data += data.y.size(0)
            if norm:
                pred = norm.denorm(pred)
            predictions.append(pred.cpu().numpy())
            labels.append(data.y.cpu().flatten().numpy())
    model.train()
    return total / max(num_data, 1), np.concatenate(predictions), np.concatenate(labels)


def metric_of(crit, labels, predictions):
    if crit == "cross_entropy":
        return roc_auc_score(labels, predictions[:, 1])
    return mae_score(labels, predictions) if crit == "l1" else rmse_score(labels, predictions)


@pytest.mark.parametrize("kind,crit", [("gin", "cross_entropy"), ("gcn", "mse"), ("bf16", "l1")])
def test_evaluation_pass_matches_eager(dev, kind, crit):
    """CapturedEval.run over five batches (the partial one in the middle)
    against the eager pass: predictions 1e-6 norm-wise, labels equal, mean
    loss 1e-6 relative, the metric to 1e-6.

    Measured on an MI355X: the predictions came out bit-identical in all
    three cases (the padding rows lie outside every molecule and eval-mode
    BatchNorm uses the running statistics, so no arithmetic sees them); the
    test prints whether they did."""
    data = batches(crit, dev)
    loader = [data[0], data[1], data[6], data[2], data[3]]
    norm = normalizer_of(crit, dev)
    model = make(kind, crit, 12).to(dev)
    with torch.no_grad():  # running statistics other than the initial 0 / 1
        for bn in model.batch_norms:
            bn.running_mean.uniform_(-0.5, 0.5)
            bn.running_var.uniform_(0.5, 1.5)
    ev = CapturedEval(model, crit, norm, **Q)
    loss_e, pred_e, lab_e = eager_evaluate(model, loader, crit, norm)
    loss_c, pred_c, lab_c = ev.run(loader)
    assert model.training
    assert pred_c.shape == pred_e.shape and pred_c.dtype == pred_e.dtype
    assert lab_c.dtype == lab_e.dtype and np.array_equal(lab_c, lab_e)
    print("bit-identical predictions:", np.array_equal(pred_c, pred_e),
          "loss eager", loss_e, "captured", loss_c)
    assert rel(torch.from_numpy(pred_c), torch.from_numpy(pred_e)) <= 1e-6
    assert abs(loss_c - loss_e) <= 1e-6 * abs(loss_e)
    assert abs(metric_of(crit, lab_c, pred_c) - metric_of(crit, lab_e, pred_e)) <= 1e-6
    # a second pass replays (nothing new captured) and starts from an empty gather
    n = ev.captures
    loss_2, pred_2, lab_2 = ev.run(loader[:3])
    assert ev.captures == n and len(pred_2) == 69
    assert np.array_equal(pred_2, pred_c[:69]) and np.array_equal(lab_2, lab_c[:69])
    ev.check()
    # a capacity one row too small: refused by the status bit
    small = CapturedEval(model, crit, norm, capacity=len(pred_e) - 1, **Q)
    with pytest.raises(ValueError, match="capacity"):
        small.run(loader)
    assert int(small.cursor.item()) == len(pred_e) - 32  # the last batch was not taken
    ev.close()
    small.close()


@pytest.mark.parametrize("labels", [True, False], ids=["int64", "fp32"])
def test_eval_tail_refuses_rows_past_the_capacity(dev, labels):
    """molclr_eval_tail with a capacity one row too small: the status bit, no
    store (gather buffers and the guard region behind them unchanged), cursor
    and loss sum kept; with the row it lacked, the batch lands behind the
    cursor."""
    B, C, n0, guard = 7, 1 if labels else 3, 10, 64
    st = _lib.stream_of(dev)
    pred = torch.randn(B, C, device=dev)
    if labels:
        target, tw = torch.arange(B, device=dev) + 100, 2
        target_all = torch.full((n0 + B + guard,), -7, dtype=torch.long, device=dev)
    else:
        target, tw = torch.randn(B, C, device=dev), C
        target_all = torch.full((n0 + B + guard, C), -7.0, device=dev)
    pred_all = torch.full((n0 + B + guard, C), -7.0, device=dev)
    loss = torch.tensor(0.3, device=dev)
    batch_status = torch.tensor([8], dtype=torch.int32, device=dev)

    def call(capacity):
        cursor = torch.tensor([n0], device=dev)
        acc = torch.tensor([1.5], dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.call("molclr_eval_tail", pred.data_ptr(), target.data_ptr(), B, C, tw,
                  loss.data_ptr(), pred_all.data_ptr(), target_all.data_ptr(), capacity,
                  cursor.data_ptr(), acc.data_ptr(), batch_status.data_ptr(), status.data_ptr(),
                  st)
        torch.cuda.synchronize()
        return int(cursor), float(acc), int(status)

    cursor, acc, status = call(n0 + B - 1)
    assert status == _lib.STATUS_EVAL_OVERFLOW | 8 and cursor == n0 and acc == 1.5
    assert bool((pred_all == -7).all()) and bool((target_all == -7).all())
    cursor, acc, status = call(n0 + B)
    assert status == 8 and cursor == n0 + B
    assert acc == 1.5 + float(np.float32(0.3)) * B
    assert torch.equal(pred_all[n0:n0 + B], pred) and bool((pred_all[:n0] == -7).all())
    assert bool((pred_all[n0 + B:] == -7).all()) and bool((target_all[n0 + B:] == -7).all())
    assert torch.equal(target_all[n0:n0 + B].reshape(target.shape), target)


def test_stage_task_refusals(dev):
    """molclr_stage_task refuses what molclr_stage_segments refuses, and a
    target count that is not the graph's."""
    from molclr_amd.finetune_step import StagedTaskGraph
    d = batches("mse", dev)[6]
    n, e = d.x.shape[0], d.edge_index.shape[1]
    with pytest.raises(_lib.MolclrError, match="nodes"):
        StagedTaskGraph(dev, n - 1, e, 5, False, 1).stage_task(d)
    with pytest.raises(_lib.MolclrError, match="edges"):
        StagedTaskGraph(dev, n, e - 1, 5, False, 1).stage_task(d)
    with pytest.raises(ValueError, match="molecules"):
        StagedTaskGraph(dev, n, e, 6, False, 1).stage_task(d)
    g = StagedTaskGraph(dev, n + 9, e + 5, 5, False, 1)
    g.stage_task(d)
    torch.cuda.synchronize()
    assert torch.equal(g.target, d.y) and torch.equal(g.x[:n], d.x)
    assert int(g.x[n:].abs().sum()) == 0 and g.counts.tolist() == [n, e]
    src = _lib.StageSourceC(d.x.data_ptr(), d.edge_index.data_ptr(), d.edge_attr.data_ptr(),
                            d.batch.data_ptr(), n, e)
    rc = _lib.load().molclr_stage_task(
        ctypes.addressof(src), ctypes.addressof(g._dst), g.x.data_ptr(), g.num_nodes, g.num_edges,
        g.counts.data_ptr(), d.y.data_ptr(), g.target.data_ptr(), 4, 1, 1, _lib.stream_of(dev))
    assert rc == -1 and b"target rows" in _lib.load().molclr_last_error()


@pytest.mark.parametrize("task,kind", [("classification", "gin"), ("regression", "gcn")])
def test_trainer_with_hip_graph(dev, tmp_path, task, kind):
    """FineTune with hip_graph: True learns, and its final metric is the one
    an eager evaluation of the saved checkpoint gives."""
    from molclr_amd.dataset_test import MolTestDatasetWrapper
    from molclr_amd.finetune import FineTune
    write_csv(tmp_path / "data.csv", task)
    cfg = config_of(tmp_path, task, kind, hip_graph=True)
    dataset = MolTestDatasetWrapper(cfg["batch_size"], **cfg["dataset"])
    loaders = dataset.get_data_loaders()  # one split for the run and the check below
    dataset.get_data_loaders = lambda: loaders
    ft = FineTune(dataset, cfg)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        model = ft.train()
    assert not [w for w in caught if "hip_graph" in str(w.message)]  # no fallback
    step, ev = ft._captured[2], ft._captured[3]
    assert step.replays == 3 * len(loaders[1]) and ev.replays > 0
    print("epoch losses", ft.epoch_train_loss, "captures", step.captures, ev.captures)
    assert len(ft.epoch_train_loss) == 3 and np.isfinite(ft.epoch_train_loss).all()
    # "decreasing" as tests/test_gpu_finetune.py reads it for the eager trainer
    assert ft.epoch_train_loss[-1] < ft.epoch_train_loss[0]
    assert os.path.exists(os.path.join(ft.log_dir, "checkpoints", "model.pth"))
    captured = ft.roc_auc if task == "classification" else ft.rmse
    ft.hip_graph = False  # the same checkpoint through the eager pass
    eager = ft._test(model, loaders[3])
    print("metric captured", captured, "eager", eager)
    assert np.isfinite(captured) and abs(captured - eager) <= 1e-6
    if task == "classification":
        assert captured > 0.5


def test_trainer_motif_model_falls_back_with_one_warning(dev, tmp_path):
    from molclr_amd.dataset_test import MolTestDatasetWrapper
    from molclr_amd.finetune import FineTune
    write_csv(tmp_path / "data.csv", "classification", n=120)
    cfg = config_of(tmp_path, "classification", "gin_motif", epochs=1, hip_graph=True)
    ft = FineTune(MolTestDatasetWrapper(cfg["batch_size"], **cfg["dataset"]), cfg)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        ft.train()
    mine = [w for w in caught if issubclass(w.category, RuntimeWarning)
            and "hip_graph" in str(w.message)]
    assert len(mine) == 1 and "motif" in str(mine[0].message)
    assert ft._captured is None and len(ft.epoch_train_loss) == 1
    assert np.isfinite(ft.epoch_train_loss[0]) and np.isfinite(ft.roc_auc)
