"""The motif model (ginet_finetune_mp) through the captured fine-tuning step
and evaluation pass (molclr_amd.finetune_step) against the eager loop, at the
bounds of tests/test_gpu_finetune_step.py: loss 1e-6 relative, flat gradient
1e-5 norm-wise (bf16 storage 1e-4), running statistics 1e-6, counters equal.

Shapes: that file's batches (six of 32 molecules, a partial one of 5; L = 2,
D = 64, FEAT = 128) with items from a vocabulary of 50 motifs -- about one
item per molecule in the even batches and about five in the odd ones, so that
with item_quantum 64 the buckets differ in their item capacity too.
"""
import copy
import warnings

import numpy as np
import pytest
import torch

from molclr_amd.finetune_step import CapturedEval, CapturedFinetuneStep

from .test_gpu_finetune import FEAT, L, config_of, write_csv
from .test_gpu_finetune_step import (CRITS, Q, batches, compare, metric_of, normalizer_of,
                                     optimizers, rel, sync, target_of)

pytestmark = pytest.mark.gpu
VOCAB = 50
QM = dict(Q, item_quantum=64)
_ITEMS = {}


def items(dev):
    """(mol_idx, clique_idx) of each of the seven batches, made once: molecules
    without items, repeated ids across molecules, distinct ids within one."""
    if not _ITEMS:
        rng = np.random.default_rng(23)
        for k, B in enumerate([32] * 6 + [5]):
            counts = rng.integers(0, 3, B) if k % 2 == 0 else rng.integers(2, 9, B)
            clique = np.concatenate([rng.choice(VOCAB, n, replace=False) for n in counts] +
                                    [np.zeros(0, np.int64)]).astype(np.int64)
            mol = np.concatenate([np.repeat(np.arange(B), counts), np.arange(B)])
            _ITEMS[k] = (torch.from_numpy(mol).to(dev), torch.from_numpy(clique).to(dev))
    return [_ITEMS[k] for k in range(7)]


def make(kind, crit, seed, drop=0.0):
    from molclr_amd.ginet_finetune_mp import GINet
    task = "classification" if crit == "cross_entropy" else "regression"
    torch.manual_seed(seed)
    return GINet(VOCAB, task, L, 64, FEAT, drop, precision="bf16" if kind == "bf16" else "fp32")


def eager_step(model, opts, data, motif, crit, norm):
    for o in opts:
        o.zero_grad()
    _, _, loss = model.loss(data, *motif, target_of(data, crit, norm), crit)
    loss.backward()
    for o in opts:
        o.step()
    return loss.detach().clone()


@pytest.mark.parametrize("crit", CRITS)
@pytest.mark.parametrize("kind", ["gin", "bf16"])
def test_replay_follows_eager(dev, kind, crit):
    """Every replay -- first captures, the partial batch's bucket, later
    replays on buckets of two item capacities -- against the eager step from
    the same state."""
    data, its = batches(crit, dev), items(dev)
    norm = normalizer_of(crit, dev)
    ref = make(kind, crit, 5).to(dev)
    cap = copy.deepcopy(ref)
    opts_r, opts_c = optimizers(ref), optimizers(cap)
    step = CapturedFinetuneStep(cap, opts_c, crit, norm, **QM)
    order = list(range(7)) + [0, 1, 2]
    for i, k in enumerate(order):
        sync(ref, opts_r, cap, opts_c)
        loss_r = eager_step(ref, opts_r, data[k], its[k], crit, norm)
        loss_c = step.step(data[k], *its[k]).clone()
        compare(i, kind, step, ref, opts_r, cap, opts_c, loss_r, loss_c)
    print("buckets", step.buckets)
    assert 3 <= step.captures <= 7 and step.replays == len(order)
    assert all(len(k) == 4 for k in step.buckets)
    assert len({k[3] for k in step.buckets if k[2] == 32}) >= 2  # two item capacities
    assert step.bucket(data[6], its[6]) in step.buckets and step.bucket(data[6], its[6])[2] == 5
    step.check()
    sync(ref, opts_r, cap, opts_c)
    cap.eval()
    ref.eval()
    with torch.no_grad():
        assert torch.equal(cap(data[0], *its[0])[1], ref(data[0], *its[0])[1])
    step.close()


def test_more_items_than_the_capacity_take_a_larger_bucket(dev):
    """The same graph with more items than its bucket's item capacity is
    captured again on a larger one; nothing is staged past a buffer's end."""
    crit = "cross_entropy"
    data, its = batches(crit, dev), items(dev)
    model = make("gin", crit, 2).to(dev)
    step = CapturedFinetuneStep(model, optimizers(model), crit, **QM)
    step.step(data[0], *its[0])
    small = step.buckets[0]
    assert its[1][1].shape[0] > small[3]
    mol = torch.cat([torch.sort(torch.arange(its[1][1].shape[0], device=dev) % 32)[0],
                     torch.arange(32, device=dev)])
    loss = step.step(data[0], mol, its[1][1]).clone()
    assert step.captures == 2 and torch.isfinite(loss)
    big = [k for k in step.buckets if k != small][0]
    assert big[:3] == small[:3] and big[3] >= its[1][1].shape[0]
    with pytest.raises(ValueError, match="built for"):
        step._graphs[small].graph.stage_items(mol, its[1][1])
    with pytest.raises(TypeError, match="mol_idx"):
        step.step(data[0])
    step.check()
    step.close()


def test_bad_items_are_sticky(dev):
    crit = "cross_entropy"
    data, its = batches(crit, dev), items(dev)
    model = make("gin", crit, 2).to(dev)
    step = CapturedFinetuneStep(model, optimizers(model), crit, **QM)
    step.step(data[1], *its[1])
    step.check()
    bad = its[1][1].clone()
    bad[7] = VOCAB  # outside the table
    step.step(data[1], its[1][0], bad)
    step.step(data[1], *its[1])
    with pytest.raises(ValueError, match="motif index"):
        step.check()
    step.close()


def test_dropout_replays(dev):
    """drop_ratio 0.3: two replays of one batch draw different masks, and a
    replay from a restored dropout_state repeats one."""
    crit = "cross_entropy"
    data, its = batches(crit, dev), items(dev)
    model = make("gin", crit, 8, drop=0.3).to(dev)
    opts = optimizers(model)
    step = CapturedFinetuneStep(model, opts, crit, **QM)
    step.step(data[1], *its[1])  # captures; the model's dropout_state exists from here on
    for o in opts:  # parameters fixed: only the masks differ between replays
        o.param_groups[0]["lr"] = 0.0
    state = model.dropout_state.clone()
    a = step.step(data[1], *its[1]).clone()
    b = step.step(data[1], *its[1]).clone()
    model.dropout_state.copy_(state)  # in place: the graph holds its address
    c = step.step(data[1], *its[1]).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(a) and torch.isfinite(b)
    assert a.item() != b.item() and a.item() == c.item()
    assert int(model.dropout_state[1]) == int(state[1]) + 1
    assert step.captures == 1
    step.close()


def eager_evaluate(model, loader, motifs, crit, norm):
    """The body of FineTune._evaluate."""
    predictions, labels = [], []
    total, num_data = 0.0, 0
    with torch.no_grad():
        model.eval()
        for data, motif in zip(loader, motifs):
            _, pred, loss = model.loss(data, *motif, target_of(data, crit, norm), crit)
            total += loss.item() * data.y.size(0)
            num_data += data.y.size(0)
            if norm:
                pred = norm.denorm(pred)
            predictions.append(pred.cpu().numpy())
            labels.append(data.y.cpu().flatten().numpy())
    model.train()
    return total / max(num_data, 1), np.concatenate(predictions), np.concatenate(labels)


class _SyncCount:
    """Counts what makes the host wait for the device: Tensor.cpu / .item /
    .tolist of a device tensor and torch.cuda.synchronize."""

    def __enter__(self):
        self.n = 0
        self._saved = [(torch.Tensor, name, getattr(torch.Tensor, name))
                       for name in ("cpu", "item", "tolist")]
        self._saved.append((torch.cuda, "synchronize", torch.cuda.synchronize))
        for owner, name, fn in self._saved:
            setattr(owner, name, self._wrap(fn, owner is torch.Tensor))
        return self

    def _wrap(self, fn, method):
        def counted(*a, **kw):
            if not method or a[0].is_cuda:
                self.n += 1
            return fn(*a, **kw)
        return counted

    def __exit__(self, *exc):
        for owner, name, fn in self._saved:
            setattr(owner, name, fn)


@pytest.mark.parametrize("kind,crit", [("gin", "cross_entropy"), ("gin", "mse"), ("bf16", "l1")])
def test_evaluation_pass_matches_eager(dev, kind, crit):
    """CapturedEval.run over five batches (the partial one in the middle)
    against the eager pass: predictions 1e-6 norm-wise, labels equal, mean
    loss 1e-6 relative, the metric to 1e-6; a pass of replays waits for the
    device once.

    Measured on an MI355X: the predictions and the mean loss came out
    bit-identical in all three cases; the test prints whether they did and
    does not assert it."""
    data, its = batches(crit, dev), items(dev)
    pick = [0, 1, 6, 2, 3]
    loader, motifs = [data[k] for k in pick], [its[k] for k in pick]
    lookup = {id(d): m for d, m in zip(loader, motifs)}
    norm = normalizer_of(crit, dev)
    model = make(kind, crit, 12).to(dev)
    with torch.no_grad():  # running statistics other than the initial 0 / 1
        for bn in model.batch_norms:
            bn.running_mean.uniform_(-0.5, 0.5)
            bn.running_var.uniform_(0.5, 1.5)
    ev = CapturedEval(model, crit, norm, **QM)
    loss_e, pred_e, lab_e = eager_evaluate(model, loader, motifs, crit, norm)
    loss_c, pred_c, lab_c = ev.run(loader, motif=lambda d: lookup[id(d)])
    assert model.training
    assert pred_c.shape == pred_e.shape and pred_c.dtype == pred_e.dtype
    assert lab_c.dtype == lab_e.dtype and np.array_equal(lab_c, lab_e)
    print("bit-identical predictions:", np.array_equal(pred_c, pred_e),
          "loss eager", loss_e, "captured", loss_c)
    assert rel(torch.from_numpy(pred_c), torch.from_numpy(pred_e)) <= 1e-6
    assert abs(loss_c - loss_e) <= 1e-6 * abs(loss_e)
    assert abs(metric_of(crit, lab_c, pred_c) - metric_of(crit, lab_e, pred_e)) <= 1e-6
    # a second pass replays (nothing new captured) with one wait for the device
    n = ev.captures
    with _SyncCount() as waits:
        loss_2, pred_2, lab_2 = ev.run(loader, motif=lambda d: lookup[id(d)])
    assert ev.captures == n and waits.n == 1
    assert loss_2 == loss_c and np.array_equal(pred_2, pred_c) and np.array_equal(lab_2, lab_c)
    with pytest.raises(TypeError, match="motif"):
        ev.run(loader)
    ev.check()
    ev.close()


def test_trainer_motif_model_runs_from_graphs(dev, tmp_path):
    """FineTune with model_type gin_motif, hip_graph True and hip_graph_motif
    True: no fallback, the step and the evaluation replay, and the run's metric
    is that of the eager run from the same seed."""
    from molclr_amd.dataset_test import MolTestDatasetWrapper
    from molclr_amd.finetune import FineTune
    write_csv(tmp_path / "data.csv", "classification", n=120)
    runs = {}
    for hip_graph in (True, False):
        cfg = config_of(tmp_path, "classification", "gin_motif", epochs=2, hip_graph=hip_graph,
                        hip_graph_motif=True,
                        log_root=str(tmp_path / f"runs{int(hip_graph)}"))
        ft = FineTune(MolTestDatasetWrapper(cfg["batch_size"], **cfg["dataset"]), cfg)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            ft.train()
        assert not [w for w in caught if issubclass(w.category, RuntimeWarning)
                    and "hip_graph" in str(w.message)]  # no fallback
        runs[hip_graph] = ft
    cap, eager = runs[True], runs[False]
    step, ev = cap._captured[2], cap._captured[3]
    assert eager._captured is None
    assert step.captures > 0 and ev.captures > 0 and step.replays > 0 and ev.replays > 0
    assert all(len(k) == 4 for k in step.buckets + ev.buckets)
    print("epoch losses captured", cap.epoch_train_loss, "eager", eager.epoch_train_loss,
          "roc_auc", cap.roc_auc, eager.roc_auc)
    assert len(cap.epoch_train_loss) == 2 and np.isfinite(cap.epoch_train_loss).all()
    assert np.isfinite(cap.roc_auc) and abs(cap.roc_auc - eager.roc_auc) <= 1e-6 * eager.roc_auc
