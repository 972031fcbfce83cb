"""Exact top-k search: the fused kernel against matmul + topk.

One process on one GPU per row.  Database of unit-norm random rows, n x C
(default 1,000,000 x 512: 2 GB in fp32, 1 GB in bf16, far beyond the 256 MB
Infinity Cache), k = 10, nq in {1, 16, 64, 1024}.  The two arms alternate
round by round and are timed with device events:

  fused     ops.topk_dot(q, db, k)
  composed  torch.topk(torch.matmul(q, db32.T), k) -- for a bf16 database
            db32 is the database widened to fp32 ONCE, outside the timed
            region (the composed arm then reads 4 bytes per value)

Per row: median (min .. max) microseconds over the rounds after warm-up; for
the fused arm the bytes it must read, ceil(nq / 32) * n * C * s, and their
rate as a fraction of the 8 TB/s HBM peak.  A row is "ok" when the fused
median is not above the composed median by more than the larger of the two
arms' own round-to-round spread (max - min) in this run.

    python tools/bench_retrieval.py [--n 1000000] [--dim 512] [-k 10]
        [--nq 1 16 64 1024] [--rounds 9] [--warmup 3] [--timeout 240]

Every row runs in a child process of its own under ``timeout``; a row that
fails or runs out of time is reported as such and the others still run.
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HBM_PEAK = 8.0e12  # bytes / s


def run_row(args) -> dict:
    """One (dtype, nq) row in this process."""
    sys.path.insert(0, str(ROOT))
    import torch

    from molclr_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_retrieval: no GPU visible (no CPU path)")
    dev = torch.device("cuda", 0)
    n, C, k, nq = args.n, args.dim, args.k, args.row_nq
    g = torch.Generator(device=dev).manual_seed(1)
    db32 = torch.empty((n, C), device=dev)
    step = 1 << 18
    for r in range(0, n, step):  # in pieces: no second full-size temporary
        x = torch.randn((min(step, n - r), C), generator=g, device=dev)
        db32[r:r + x.shape[0]] = x / x.norm(dim=1, keepdim=True)
    q = torch.randn((nq, C), generator=g, device=dev)
    q = q / q.norm(dim=1, keepdim=True)
    bf16 = args.row_dtype == "bf16"
    db = db32.to(torch.bfloat16) if bf16 else db32
    if bf16:  # the composed arm's widened copy holds the same values
        db32 = db.float()

    def fused():
        return ops.topk_dot(q, db, k)

    def composed():
        return torch.topk(torch.matmul(q, db32.t()), k, dim=1)

    arms = {"fused": fused, "composed": composed}
    for _ in range(args.warmup):
        for fn in arms.values():
            out = fn()
    torch.cuda.synchronize()
    fs, fi = fused()
    cs, ci = composed()
    agree = (fi == ci).float().mean().item()
    close = (fs - cs).abs().max().item()
    del fs, fi, cs, ci, out
    times = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    nbytes = -(-nq // 32) * n * C * (2 if bf16 else 4)
    row = {"dtype": args.row_dtype, "nq": nq, "n": n, "C": C, "k": k, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "index_agreement": agree,
           "max_score_diff": close, "fused_bytes": nbytes}
    for name, t in times.items():
        row[name] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
    row["fused_hbm_fraction"] = nbytes / (row["fused"]["median_us"] * 1e-6) / HBM_PEAK
    spread = max(row[a]["max_us"] - row[a]["min_us"] for a in arms)
    row["ok"] = row["fused"]["median_us"] <= row["composed"]["median_us"] + spread
    return row


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 16, 64, 1024])
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"], choices=["fp32", "bf16"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per row")
    ap.add_argument("--row-dtype", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--row-nq", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7")
    if args.row_dtype is not None:
        print("ROW " + json.dumps(run_row(args)), flush=True)
        return 0
    rows, failed = [], []
    for dtype in args.dtypes:
        for nq in args.nq:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, __file__,
                   "--n", str(args.n), "--dim", str(args.dim), "-k", str(args.k),
                   "--rounds", str(args.rounds), "--warmup", str(args.warmup),
                   "--row-dtype", dtype, "--row-nq", str(nq)]
            r = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("ROW ")]
            if r.returncode != 0 or len(line) != 1:
                failed.append((dtype, nq, r.returncode))
                print(f"{dtype} nq {nq}: FAILED (exit {r.returncode})\n{r.stderr[-1500:]}",
                      flush=True)
                if r.returncode in (124, 134, 137, 139, -6, -11):
                    print("a row hung or faulted: the remaining rows are not run", flush=True)
                    break
                continue
            row = json.loads(line[0][4:])
            rows.append(row)
            f, c = row["fused"], row["composed"]
            print(f"{dtype:4s} nq {nq:5d}  fused {f['median_us']:10.1f} us "
                  f"({f['min_us']:.1f} .. {f['max_us']:.1f})  "
                  f"{row['fused_bytes'] / 1e9:7.2f} GB  {100 * row['fused_hbm_fraction']:5.1f} % of "
                  f"8 TB/s   composed {c['median_us']:10.1f} us ({c['min_us']:.1f} .. "
                  f"{c['max_us']:.1f})"
                  f"{' (database widened to fp32 outside the timed region)' if dtype == 'bf16' else ''}"
                  f"   {'ok' if row['ok'] else 'SLOWER'}   same indices "
                  f"{100 * row['index_agreement']:.2f} %", flush=True)
        else:
            continue
        break
    print("RESULT " + json.dumps({"rows": rows, "failed": failed}), flush=True)
    return 0 if rows and not failed and all(r["ok"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
