"""The GCN pre-training step in fp32 against bf16 storage (precision='bf16').

Two shapes: GCN 5 x 512 at batch 1024, and the c3 shape 5 x 300 at batch 512 run
at emb_dim 304 -- the width the bf16 path pads 300 to (the captured step takes
unpadded widths only, so both precisions run at 304).  Per shape one fp32 and
one bf16 model, each with its own FusedAdam and CapturedTrainStep over the same
synthetic batches; the two alternate round by round in ONE process, so drift
hits both alike.  A round is `iters` back-to-back replays between two HIP
events; reported per precision: the median over rounds and the spread
(min .. max), in microseconds per step, and the ratio of the medians.

    python tools/bench_gcn_bf16.py [--rounds 9] [--iters 40] [--shapes 512,304] [--out FILE]
prints one JSON line per shape.  Per-kernel times: run it once under
``rocprofv3 --kernel-trace --stats`` with ``--rounds 2`` (a run of its own).
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from molclr_amd.dataset import SyntheticPairBatches  # noqa: E402
from molclr_amd.gcn_molclr import GCN  # noqa: E402
from molclr_amd.graph_step import CapturedTrainStep  # noqa: E402
from molclr_amd.nt_xent import NTXentLoss  # noqa: E402
from molclr_amd.optim import FusedAdam  # noqa: E402

SHAPES = {512: (5, 512, 1024), 304: (5, 304, 512)}  # emb_dim: (layers, emb_dim, batch)


def summary(xs):
    return {"median_us": round(statistics.median(xs), 1), "min_us": round(min(xs), 1),
            "max_us": round(max(xs), 1)}


def run(L, D, B, rounds, iters, dev):
    data = [(xi.to(dev), xj.to(dev))
            for xi, xj in SyntheticPairBatches(B, seed=0, shape="pubchem").take(4)]
    crit = NTXentLoss(dev, B, 0.1, True)
    steps = {}
    for prec in ("fp32", "bf16"):
        torch.manual_seed(0)
        model = GCN(L, D, 256, precision=prec).to(dev).train()
        opt = FusedAdam(model.parameters(), 5e-4, weight_decay=1e-5)
        step = CapturedTrainStep(model, opt, crit)
        for xi, xj in data + data:  # every bucket captured and replayed before timing
            step(xi, xj)
        steps[prec] = step
    torch.cuda.synchronize()
    times = {p: [] for p in steps}
    nodes = sum(int(xi.x.shape[0] + xj.x.shape[0]) for xi, xj in data) / len(data)
    for _ in range(rounds):
        for prec, step in steps.items():
            captures = step.captures
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                step(*data[i % len(data)])
            e1.record()
            e1.synchronize()
            assert step.captures == captures, "a capture inside the timed region"
            times[prec].append(e0.elapsed_time(e1) * 1e3 / iters)
    out = {"model": f"gcn {L}x{D}", "batch": B, "mean_nodes_per_step": round(nodes),
           "rounds": rounds, "iters": iters, **{p: summary(t) for p, t in times.items()}}
    out["bf16_over_fp32"] = round(out["bf16"]["median_us"] / out["fp32"]["median_us"], 3)
    for step in steps.values():
        step.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--shapes", default="512,304")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gcn_bf16: needs a GPU")
    dev = torch.device("cuda", 0)
    lines = [json.dumps(run(*SHAPES[int(s)], a.rounds, a.iters, dev)) for s in a.shapes.split(",")]
    for ln in lines:
        print(ln, flush=True)
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
