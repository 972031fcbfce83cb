"""Fine-tuning step and task-head timings: the fused head (task_head.hip)
against the composed one (MOLCLR_TASK_HEAD=0: ops.linear per layer, torch
activations and loss).

GIN 5 x 300, feat_dim 512, pred_n_layer 2, softplus, classification, synthetic
molecules; batches of 32 and 256, drop_ratio 0 and 0.3.  Each configuration
times the whole step (zero_grad, model.loss, backward, FusedAdam) and the head
alone (forward + backward on pooled features, gradients accumulating into
FusedAdam's buffer, nothing else launched), the two head paths alternating
round by round in one process so drift hits both alike.  Per round: `iters`
back-to-back iterations between two device syncs, wall-clock per iteration;
reported are the median over rounds and the spread (min .. max).  Kernel
launches per iteration are counted with the torch profiler.

The captured column (molclr_amd.finetune_step) alternates with the eager one
in the same rounds: ``step_captured`` is CapturedFinetuneStep.step on the same
model and optimizer after ``prepare`` (``captures_in_timed_region`` counts what was
captured while timing: 0 when prepare covered every batch), and
``eval_eager`` / ``eval_captured`` are one evaluation pass over the batches --
the eager loop of FineTune._evaluate (loss.item() and two .cpu() per batch)
against CapturedEval.run -- in microseconds per batch.

``--motif`` times the motif model (ginet_finetune_mp: 1000 motifs, 4 to 14
items per molecule) instead, drop_ratio 0, batches of 32 and 256: the eager
step and evaluation pass against the captured ones, alternating round by round,
with the launches per iteration of each (a replay's are the graph's kernel
nodes plus the two staging launches).

``--freeze-bn`` adds rows after the others: the eager step with batch
statistics against the step with frozen BatchNorm (``model.freeze_bn``: running
statistics, one backward pass over dy and z), GIN 5 x 300 and GCN 5 x 300,
fp32, alternating round by round on one model, with the launches of each.

``--loader`` adds rows after the others: the step's wall-clock with the loader
in it (run_loader: a whole epoch of 64 batches of real SMILES per round) -- the
trainer's host DataLoader (num_workers 0 and 8) against the device-resident
task store (molclr_amd.task_store), each with the eager and the captured step.

    python tools/bench_finetune.py [--rounds 9] [--iters 50] [--motif] [--freeze-bn] [--loader]
                                   [--loader-rounds 5] [--out FILE]
prints one JSON line per configuration.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from molclr_amd import ops  # noqa: E402
from molclr_amd.dataset import collate_views, random_molecule  # noqa: E402
from molclr_amd.finetune_step import CapturedEval, CapturedFinetuneStep  # noqa: E402
from molclr_amd.ginet_finetune import GINet  # noqa: E402
from molclr_amd.optim import FusedAdam  # noqa: E402


def batches(B, n, dev, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        mols = [random_molecule(rng, "pubchem") for _ in range(B)]
        b = collate_views([(m.x, m.edge_index, m.edge_attr) for m in mols])
        b.y = torch.from_numpy(rng.integers(0, 2, (B, 1)))
        b = b.to(dev)
        out.append((b, b.y.flatten()))
    return out


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn(0)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(0)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def summary(xs):
    return {"median_us": round(statistics.median(xs), 1), "min_us": round(min(xs), 1),
            "max_us": round(max(xs), 1)}


def run(B, drop, rounds, iters, dev):
    torch.manual_seed(0)
    model = GINet("classification", 5, 300, 512, drop, "mean", 2, "softplus").to(dev)
    model.train()
    opt = FusedAdam(model.parameters(), 1e-4, weight_decay=1e-6)
    data = batches(B, 8, dev)

    def step(i):
        b, y = data[i % len(data)]
        opt.zero_grad()
        model.loss(b, y)[2].backward()
        opt.step()

    lins, acts = model._head_layers()
    Ws = [model.feat_lin.weight] + [m.weight for m in lins]
    bs = [model.feat_lin.bias] + [m.bias for m in lins]
    pooled = torch.randn(B, 300, device=dev, requires_grad=True)
    y0 = data[0][1]

    def head(i):  # the head's launches alone: no zero_grad, no input-gradient accumulation
        pooled.grad = None
        ops.task_head(pooled, Ws, bs, [None] + acts, "cross_entropy", y0)[2].backward()

    # the captured column: the same model and optimizer (a second model's
    # weight images would be regenerated with this one's after every step)
    cstep = CapturedFinetuneStep(model, opt, "cross_entropy")
    ceval = CapturedEval(model, "cross_entropy")
    loader = [b for b, _ in data]
    cstep.prepare(loader)
    ceval.prepare(loader)

    def step_captured(i):
        cstep.step(loader[i % len(loader)])

    def eval_eager(i):  # the body of FineTune._evaluate
        total, preds, labels = 0.0, [], []
        with torch.no_grad():
            model.eval()
            for b, y in data:
                _, pred, loss = model.loss(b, y)
                total += loss.item() * b.y.size(0)
                preds.append(pred.cpu().numpy())
                labels.append(b.y.cpu().flatten().numpy())
        model.train()
        return total, np.concatenate(preds), np.concatenate(labels)

    def eval_captured(i):
        return ceval.run(loader)

    passes = max(1, iters // len(loader))
    res = {"batch": B, "drop_ratio": drop, "rounds": rounds, "iters": iters,
           "eval_batches": len(loader), "eval_passes_per_round": passes}
    times = {(w, f): [] for w in ("step", "head") for f in (1, 0)}
    times.update({k: [] for k in (("step", "captured"), ("eval", "eager"), ("eval", "captured"))})
    timed(step_captured, 10)
    eval_eager(0)
    eval_captured(0)
    res["launches_step_captured"] = launches(step_captured)
    res["buckets_step"] = cstep.buckets
    captures_before = cstep.captures + ceval.captures
    for fused in (1, 0):
        ops.TASK_HEAD = bool(fused)
        timed(step, 10)
        timed(head, 10)
        res[f"launches_step_fused{fused}"] = launches(step)
        res[f"launches_head_fused{fused}"] = launches(head)
    for _ in range(rounds):
        for fused in (1, 0):  # alternate the two paths round by round
            ops.TASK_HEAD = bool(fused)
            times[("step", fused)].append(timed(step, iters))
            times[("head", fused)].append(timed(head, iters))
            if fused:  # the captured step and the evaluation passes, same rounds
                times[("step", "captured")].append(timed(step_captured, iters))
                times[("eval", "eager")].append(timed(eval_eager, passes) / len(loader))
                times[("eval", "captured")].append(timed(eval_captured, passes) / len(loader))
    ops.TASK_HEAD = True
    res["captures_in_timed_region"] = cstep.captures + ceval.captures - captures_before
    for (w, f), xs in times.items():
        res[f"{w}_fused{f}" if f in (0, 1) else f"{w}_{f}"] = summary(xs)
    cstep.close()
    ceval.close()
    return res


def motif_items(loader, num_motifs, dev, seed=1):
    """(mol_idx, clique_idx) per batch: 4 to 14 distinct motifs per molecule."""
    rng = np.random.default_rng(seed)
    out = []
    for b in loader:
        B = int(b.y.shape[0])
        counts = rng.integers(4, 15, B)
        clique = np.concatenate([rng.choice(num_motifs, n, replace=False) for n in counts])
        mol = np.concatenate([np.repeat(np.arange(B), counts), np.arange(B)])
        out.append((torch.from_numpy(mol).to(dev), torch.from_numpy(clique.astype(np.int64)).to(dev)))
    return out


def run_motif(B, rounds, iters, dev, num_motifs=1000):
    from molclr_amd.ginet_finetune_mp import GINet as MotifGINet
    torch.manual_seed(0)
    model = MotifGINet(num_motifs, "classification", 5, 300, 512, 0.0, "mean", 2,
                       "softplus").to(dev)
    model.train()
    opt = FusedAdam(model.parameters(), 1e-4, weight_decay=1e-6)
    data = batches(B, 8, dev)
    loader = [b for b, _ in data]
    items = motif_items(loader, num_motifs, dev)
    of = {id(b): it for b, it in zip(loader, items)}

    def step_eager(i):
        k = i % len(data)
        opt.zero_grad()
        model.loss(data[k][0], *items[k], data[k][1])[2].backward()
        opt.step()

    cstep = CapturedFinetuneStep(model, opt, "cross_entropy")
    ceval = CapturedEval(model, "cross_entropy")
    cstep.prepare(loader, lambda b: of[id(b)])
    ceval.prepare(loader, lambda b: of[id(b)])

    def step_captured(i):
        k = i % len(loader)
        cstep.step(loader[k], *items[k])

    def eval_eager(i):  # the body of FineTune._evaluate
        total, preds, labels = 0.0, [], []
        with torch.no_grad():
            model.eval()
            for (b, y), it in zip(data, items):
                _, pred, loss = model.loss(b, *it, y)
                total += loss.item() * b.y.size(0)
                preds.append(pred.cpu().numpy())
                labels.append(b.y.cpu().flatten().numpy())
        model.train()
        return total, np.concatenate(preds), np.concatenate(labels)

    def eval_captured(i):
        return ceval.run(loader, lambda b: of[id(b)])

    passes = max(1, iters // len(loader))
    res = {"model": "gin_motif", "batch": B, "num_motifs": num_motifs,
           "items_per_batch": [int(it[1].shape[0]) for it in items], "rounds": rounds,
           "iters": iters, "eval_batches": len(loader), "eval_passes_per_round": passes}
    fns = {"step_eager": (step_eager, iters, 1), "step_captured": (step_captured, iters, 1),
           "eval_eager": (eval_eager, passes, len(loader)),
           "eval_captured": (eval_captured, passes, len(loader))}
    for name, (fn, n, per) in fns.items():
        timed(fn, min(n, 10))
        res[f"launches_{name}"] = round(launches(fn) / per, 1)
    # a replay: two staging launches, then the graph's kernel nodes
    res["graph_nodes_step"] = res["launches_step_captured"] - 2
    res["graph_nodes_eval"] = res["launches_eval_captured"] - 2
    res["buckets_step"], res["buckets_eval"] = cstep.buckets, ceval.buckets
    captures_before = cstep.captures + ceval.captures
    times = {name: [] for name in fns}
    for _ in range(rounds):  # eager and captured alternate round by round
        for name, (fn, n, per) in fns.items():
            times[name].append(timed(fn, n) / per)
    res["captures_in_timed_region"] = cstep.captures + ceval.captures - captures_before
    for name, xs in times.items():
        res[name] = summary(xs)
    cstep.close()
    ceval.close()
    return res


def run_freeze(kind, B, rounds, iters, dev):
    """The eager training step with batch statistics against the step with
    frozen BatchNorm (model.freeze_bn) on ONE model, alternating round by round:
    GIN 5 x 300 or GCN 5 x 300, fp32, drop_ratio 0; launches per step of each."""
    from molclr_amd.gcn_finetune import GCN
    torch.manual_seed(0)
    if kind == "gcn":
        model = GCN("classification", 5, 300, 512, 0.0, "mean").to(dev)
    else:
        model = GINet("classification", 5, 300, 512, 0.0, "mean", 2, "softplus").to(dev)
    model.train()
    opt = FusedAdam(model.parameters(), 1e-4, weight_decay=1e-6)
    data = batches(B, 8, dev)

    def step(i):
        b, y = data[i % len(data)]
        opt.zero_grad()
        model.loss(b, y)[2].backward()
        opt.step()

    res = {"model": kind, "batch": B, "rounds": rounds, "iters": iters}
    times = {0: [], 1: []}
    for frozen in (0, 1):
        model.freeze_bn = bool(frozen)
        timed(step, 10)
        res[f"launches_step_frozen{frozen}"] = launches(step)
    for _ in range(rounds):
        for frozen in (0, 1):
            model.freeze_bn = bool(frozen)
            times[frozen].append(timed(step, iters))
    model.freeze_bn = False
    for frozen, xs in times.items():
        res[f"step_frozen{frozen}"] = summary(xs)
    return res


def run_loader(B, rounds, dev, nbatches=64):
    """Wall-clock per training step INCLUDING the loader, a whole epoch of
    ``nbatches`` batches per round over real SMILES (the lines of
    tests/data/smiles_small.txt, repeated), GIN 5 x 300, drop_ratio 0:
      host_w0 / host_w8        the trainer's DataLoader (num_workers 0 / 8:
                               featurise, collate, copy) + the eager step
      device_eager             DeviceTaskLoader (device collate) + the eager step
      host_w0_captured / _w8_  the DataLoader + CapturedFinetuneStep.step
      device_captured          DeviceTaskLoader.ids() + step_ids
    The arms alternate round by round in one process; one untimed epoch of
    each comes first (worker start-up, the first captures)."""
    import tempfile

    from molclr_amd.dataset_test import MolTestDatasetWrapper
    from molclr_amd.task_store import device_loaders
    root = Path(__file__).resolve().parent.parent
    smiles = [l.strip() for l in (root / "tests" / "data" / "smiles_small.txt").read_text()
              .splitlines() if l.strip()]
    torch.manual_seed(0)
    np.random.seed(0)
    model = GINet("classification", 5, 300, 512, 0.0, "mean", 2, "softplus").to(dev)
    model.train()
    opt = FusedAdam(model.parameters(), 1e-4, weight_decay=1e-6)
    cstep = CapturedFinetuneStep(model, opt, "cross_entropy")
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "data.csv"
        with open(path, "w") as f:
            f.write("smiles,label\nC,0\n")  # the first data row is skipped
            for i in range(nbatches * B):
                f.write(f"{smiles[i % len(smiles)]},{i % 2}\n")

        def wrapper(workers):
            return MolTestDatasetWrapper(B, workers, 0.0, 0.0, "classification", str(path),
                                         "label", "random")

        t0 = time.perf_counter()
        _, store, dev_loader, _, _ = device_loaders(wrapper(0), dev)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        host = {w: wrapper(w).get_data_loaders()[1] for w in (0, 8)}
        assert len(dev_loader) == nbatches and all(len(l) == nbatches for l in host.values())

        def eager(data):
            opt.zero_grad()
            model.loss(data, data.y.flatten())[2].backward()
            opt.step()

        def host_epoch(workers, captured):
            for data in host[workers]:
                data = data.to(dev)  # FineTune._to_device
                cstep.step(data) if captured else eager(data)

        def device_epoch(captured):
            if captured:
                for ids_d, ids_h in dev_loader.ids():
                    cstep.step_ids(store, ids_d, ids_h)
            else:
                for data in dev_loader:
                    eager(data)

        arms = {"host_w0": lambda: host_epoch(0, False), "host_w8": lambda: host_epoch(8, False),
                "device_eager": lambda: device_epoch(False),
                "host_w0_captured": lambda: host_epoch(0, True),
                "host_w8_captured": lambda: host_epoch(8, True),
                "device_captured": lambda: device_epoch(True)}
        res = {"loader": True, "batch": B, "batches_per_epoch": nbatches, "rounds": rounds,
               "molecules": store.num_molecules, "store_build_s": round(build_s, 3)}
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
        captures_before = cstep.captures
        times = {name: [] for name in arms}
        for _ in range(rounds):
            for name, fn in arms.items():
                times[name].append(timed(lambda i: fn(), 1) / nbatches)
        res["captures_in_timed_region"] = cstep.captures - captures_before
        res["buckets_step"] = cstep.buckets
        cstep.check()
    for name, xs in times.items():
        res[name] = summary(xs)

    def below(a, *bs):  # a's slowest round under the fastest round of the better of bs
        best = min(bs, key=lambda b: res[b]["median_us"])
        return res[a]["max_us"] < res[best]["min_us"]

    res["device_eager_below_host"] = below("device_eager", "host_w0", "host_w8")
    res["device_captured_below_host_captured"] = below("device_captured", "host_w0_captured",
                                                       "host_w8_captured")
    cstep.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--motif", action="store_true",
                    help="time the motif model, eager against captured, instead")
    ap.add_argument("--freeze-bn", action="store_true",
                    help="add rows: batch statistics against frozen BatchNorm (GIN and GCN)")
    ap.add_argument("--loader", action="store_true",
                    help="add rows: wall-clock per step with the loader in it, the host "
                         "DataLoader against the device-resident task store")
    ap.add_argument("--loader-rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for B in (32, 256):
        for drop in (0.0, 0.3) if not a.motif else ():
            lines.append(json.dumps(run(B, drop, a.rounds, a.iters, dev)))
            print(lines[-1], flush=True)
        if a.motif:
            lines.append(json.dumps(run_motif(B, a.rounds, a.iters, dev)))
            print(lines[-1], flush=True)
    if a.freeze_bn:
        for kind in ("gin", "gcn"):
            for B in (32, 256):
                lines.append(json.dumps(run_freeze(kind, B, a.rounds, a.iters, dev)))
                print(lines[-1], flush=True)
    if a.loader:
        for B in (32, 256):
            lines.append(json.dumps(run_loader(B, a.loader_rounds, dev)))
            print(lines[-1], flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
