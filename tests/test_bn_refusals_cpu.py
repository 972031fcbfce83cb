"""What the BatchNorm entry points refuse before any HIP call: the status and
the message of every call in a table, all made with NULL data pointers so
nothing can launch (the forward stops at its null-pointer check, the backward
at "bad args", at the latest).  The expected pairs were recorded from the
library as it was before the host path was folded into molclr::bn_forward /
bn_backward; where two faults coincide the table pins which one is reported.
Workspace refusals need real pointers: tests/test_gpu_bn_frozen.py."""
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

_CHILD = r"""
import ctypes
import json
from molclr_amd import _lib
lib = _lib.load()
_fake = ctypes.create_string_buffer(64)   # stands for a device pointer: never read
FAKE = ctypes.addressof(_fake)

# entry point -> (kind, segments, takes a dtype, takes rowmax / slot)
ENTRIES = {
    "molclr_batchnorm_fwd": ("fwd", "one", False, False),
    "molclr_batchnorm_seg_fwd": ("fwd", "host", True, False),
    "molclr_batchnorm_seg_fwd_dev": ("fwd", "dev", True, False),
    "molclr_batchnorm_seg_coeffs": ("coeffs", "host", True, False),
    "molclr_batchnorm_seg_coeffs_dev": ("coeffs", "dev", True, False),
    "molclr_batchnorm_bwd": ("bwd", "one", False, False),
    "molclr_batchnorm_seg_bwd": ("bwd", "host", True, False),
    "molclr_batchnorm_seg_bwd_max": ("bwd", "host", False, True),
    "molclr_batchnorm_seg_bwd_dev": ("bwd", "dev", True, True),
    "molclr_batchnorm_bwd_frozen": ("bwd", "one", False, False),
    "molclr_batchnorm_seg_bwd_frozen": ("bwd", "host", True, False),
    "molclr_batchnorm_seg_bwd_frozen_max": ("bwd", "host", False, True),
    "molclr_batchnorm_seg_bwd_frozen_dev": ("bwd", "dev", True, True),
}
DEFAULT = dict(nseg=2, seg=[5, 7], cap=12, D=8, dtype=0, training=1, segdev=True, rowmax=True,
               coeffs=True)

def cases(kind, segs, has_dtype, has_max):
    c = {"null_save_mean": {}, "dim2": dict(D=2), "dim4100": dict(D=4100),
         "dim2_null_pointers": dict(D=2, segdev=False, rowmax=False, coeffs=False)}
    if segs != "one":
        c["nseg0"] = dict(nseg=0)
        c["nseg9"] = dict(nseg=9)
    if segs == "dev":
        c["negative_cap"] = dict(cap=-1)
        c["null_seg_rows_dev"] = dict(segdev=False)
    else:
        c["negative_segment"] = dict(seg=[5, -1] if segs == "host" else [-1])
    if has_dtype:
        c["dtype7"] = dict(dtype=7, rowmax=False)
        c["dtype7_nseg0"] = dict(dtype=7, rowmax=False, nseg=0)
    if kind != "bwd":
        c["eval_no_running_stats"] = dict(training=0)
        if segs != "dev":
            c["train_one_row"] = dict(seg=[7, 1] if segs == "host" else [1])
    if kind == "coeffs":
        c["null_coeffs"] = dict(coeffs=False)
    if has_max and segs == "host":
        c["null_rowmax"] = dict(rowmax=False)
    if has_max and has_dtype:
        c["rowmax_bf16"] = dict(dtype=1)
        c["rowmax_dtype7"] = dict(dtype=7)
    return c

def args(kind, segs, has_dtype, has_max, o):
    o = dict(DEFAULT, **o)
    seg = (ctypes.c_int64 * 9)(*(o["seg"] + [3] * (9 - len(o["seg"]))))
    if segs == "one":
        where = [o["seg"][0]]
    elif segs == "host":
        where = [o["nseg"], seg]
    else:
        where = [o["nseg"], FAKE if o["segdev"] else None, o["cap"]]
    where += [o["D"]] + ([o["dtype"]] if has_dtype else [])
    ws = [None, 0, None]
    if kind == "bwd":
        mx = [FAKE if o["rowmax"] else None, None] if has_max else []
        return [None] * 9 + where + [0, 0] + mx + ws, seg
    ptrs = [None] * 9 if kind == "fwd" else [None] * 8 + [FAKE if o["coeffs"] else None]
    return ptrs + where + [0.1, 1e-5, o["training"]] + ([0] if kind == "fwd" else []) + ws, seg

out = {}
for name, e in ENTRIES.items():
    for case, o in cases(*e).items():
        a, keep = args(*e, o)
        rc = getattr(lib, name)(*a)
        out[name[len("molclr_batchnorm_"):] + "/" + case] = [rc, lib.molclr_last_error().decode()]
nine = (ctypes.c_int64 * 9)(*([5] * 9))
neg = (ctypes.c_int64 * 2)(5, -1)
q = lib.molclr_batchnorm_seg_workspace_bytes
out["seg_workspace_bytes"] = [int(q(0, nine, 8)), int(q(9, nine, 8)), int(q(2, nine, 2)),
                              int(q(2, nine, 4100)), int(q(2, neg, 8)), int(q(2, None, 8))]
q = lib.molclr_batchnorm_seg_dev_workspace_bytes
out["seg_dev_workspace_bytes"] = [int(q(0, 12, 8)), int(q(9, 12, 8)), int(q(2, 12, 2)),
                                  int(q(2, 12, 4100))]
q = lib.molclr_batchnorm_workspace_bytes
out["workspace_bytes"] = [int(q(12, 2)), int(q(12, 4100)), int(q(-1, 8))]
print("REFUSALS " + json.dumps(out))
"""

ARG = -1  # MOLCLR_ERR_ARG: the status of every call in the table
N0 = "batchnorm: 0 segments (1..8)"
N9 = "batchnorm: 9 segments (1..8)"
D2 = "batchnorm: dim 2 must be a multiple of 4 in [4, 4096]"
D4100 = "batchnorm: dim 4100 must be a multiple of 4 in [4, 4096]"
NEG = "batchnorm: negative segment rows"
NEGCAP = "batchnorm: negative row capacity"
ONE_ROW = "batchnorm_fwd: need more than 1 row per segment when training"
EVAL = "batchnorm_fwd: eval needs running stats"
FWD_NULL = "batchnorm_fwd: null pointer"
BWD_BAD = "batchnorm_bwd: bad args"
FROZEN_BAD = "batchnorm_bwd_frozen: bad args"

# entry point (after "molclr_batchnorm_") -> case -> message, as recorded
MESSAGES = {
    "fwd": {
        "dim2": D2, "dim2_null_pointers": D2, "dim4100": D4100, "negative_segment": NEG,
        "train_one_row": ONE_ROW, "eval_no_running_stats": EVAL, "null_save_mean": FWD_NULL},
    "seg_fwd": {
        "nseg0": N0, "nseg9": N9, "dim2": D2, "dim2_null_pointers": D2, "dim4100": D4100,
        "dtype7": "batchnorm_seg_fwd: dtype 7", "dtype7_nseg0": "batchnorm_seg_fwd: dtype 7",
        "negative_segment": NEG, "train_one_row": ONE_ROW, "eval_no_running_stats": EVAL,
        "null_save_mean": FWD_NULL},
    "seg_fwd_dev": {
        "nseg0": N0, "nseg9": N9, "dim2": D2,
        "dim2_null_pointers": "batchnorm_seg_fwd_dev: null seg_rows_dev", "dim4100": D4100,
        "dtype7": "batchnorm_seg_fwd_dev: dtype 7",
        "dtype7_nseg0": "batchnorm_seg_fwd_dev: dtype 7", "negative_cap": NEGCAP,
        "null_seg_rows_dev": "batchnorm_seg_fwd_dev: null seg_rows_dev",
        "eval_no_running_stats": EVAL, "null_save_mean": FWD_NULL},
    "seg_coeffs": {
        "nseg0": N0, "nseg9": N9, "dim2": D2,
        "dim2_null_pointers": "batchnorm_seg_coeffs: null coeffs", "dim4100": D4100,
        "dtype7": "batchnorm_seg_coeffs: dtype 7", "dtype7_nseg0": "batchnorm_seg_coeffs: dtype 7",
        "negative_segment": NEG, "train_one_row": ONE_ROW, "eval_no_running_stats": EVAL,
        "null_coeffs": "batchnorm_seg_coeffs: null coeffs", "null_save_mean": FWD_NULL},
    "seg_coeffs_dev": {
        "nseg0": N0, "nseg9": N9, "dim2": D2,
        "dim2_null_pointers": "batchnorm_seg_coeffs_dev: null coeffs / seg_rows_dev",
        "dim4100": D4100, "dtype7": "batchnorm_seg_coeffs_dev: dtype 7",
        "dtype7_nseg0": "batchnorm_seg_coeffs_dev: dtype 7", "negative_cap": NEGCAP,
        "null_seg_rows_dev": "batchnorm_seg_coeffs_dev: null coeffs / seg_rows_dev",
        "null_coeffs": "batchnorm_seg_coeffs_dev: null coeffs / seg_rows_dev",
        "eval_no_running_stats": EVAL, "null_save_mean": FWD_NULL},
    "bwd": {
        "dim2": D2, "dim2_null_pointers": D2, "dim4100": D4100, "negative_segment": NEG,
        "null_save_mean": BWD_BAD},
    "seg_bwd": {
        "nseg0": N0, "nseg9": N9, "dim2": D2, "dim2_null_pointers": D2, "dim4100": D4100,
        "dtype7": "batchnorm_seg_bwd: dtype 7", "dtype7_nseg0": "batchnorm_seg_bwd: dtype 7",
        "negative_segment": NEG, "null_save_mean": BWD_BAD},
    "seg_bwd_max": {
        "nseg0": N0, "nseg9": N9, "dim2": D2,
        "dim2_null_pointers": "batchnorm_seg_bwd_max: null rowmax", "dim4100": D4100,
        "negative_segment": NEG, "null_rowmax": "batchnorm_seg_bwd_max: null rowmax",
        "null_save_mean": BWD_BAD},
    "seg_bwd_dev": {
        "nseg0": N0, "nseg9": N9, "dim2": D2,
        "dim2_null_pointers": "batchnorm_seg_bwd_dev: null seg_rows_dev", "dim4100": D4100,
        "dtype7": "batchnorm_seg_bwd_dev: dtype 7",
        "dtype7_nseg0": "batchnorm_seg_bwd_dev: dtype 7", "negative_cap": NEGCAP,
        "null_seg_rows_dev": "batchnorm_seg_bwd_dev: null seg_rows_dev",
        "rowmax_bf16": "batchnorm_seg_bwd_dev: row maxima are fp32 only",
        "rowmax_dtype7": "batchnorm_seg_bwd_dev: row maxima are fp32 only",
        "null_save_mean": BWD_BAD},
    "bwd_frozen": {
        "dim2": D2, "dim2_null_pointers": D2, "dim4100": D4100, "negative_segment": NEG,
        "null_save_mean": FROZEN_BAD},
    "seg_bwd_frozen": {
        "nseg0": N0, "nseg9": N9, "dim2": D2, "dim2_null_pointers": D2, "dim4100": D4100,
        "dtype7": "batchnorm_seg_bwd_frozen: dtype 7",
        "dtype7_nseg0": "batchnorm_seg_bwd_frozen: dtype 7", "negative_segment": NEG,
        "null_save_mean": FROZEN_BAD},
    "seg_bwd_frozen_max": {
        "nseg0": N0, "nseg9": N9, "dim2": D2,
        "dim2_null_pointers": "batchnorm_seg_bwd_frozen_max: null rowmax", "dim4100": D4100,
        "negative_segment": NEG, "null_rowmax": "batchnorm_seg_bwd_frozen_max: null rowmax",
        "null_save_mean": FROZEN_BAD},
    "seg_bwd_frozen_dev": {
        "nseg0": N0, "nseg9": N9, "dim2": D2,
        "dim2_null_pointers": "batchnorm_seg_bwd_frozen_dev: null seg_rows_dev", "dim4100": D4100,
        "dtype7": "batchnorm_seg_bwd_frozen_dev: dtype 7",
        "dtype7_nseg0": "batchnorm_seg_bwd_frozen_dev: dtype 7", "negative_cap": NEGCAP,
        "null_seg_rows_dev": "batchnorm_seg_bwd_frozen_dev: null seg_rows_dev",
        "rowmax_bf16": "batchnorm_seg_bwd_frozen_dev: row maxima are fp32 only",
        "rowmax_dtype7": "batchnorm_seg_bwd_frozen_dev: row maxima are fp32 only",
        "null_save_mean": FROZEN_BAD},
}
EXPECTED = {e + "/" + c: (ARG, m) for e, cs in MESSAGES.items() for c, m in cs.items()}
# the workspace queries answer 0 to a plan they cannot make
EXPECTED["seg_workspace_bytes"] = [0, 0, 0, 0, 0, 0]
EXPECTED["seg_dev_workspace_bytes"] = [0, 0, 0, 0]
EXPECTED["workspace_bytes"] = [0, 0, 0]


def test_refusals_before_any_hip_call():
    from molclr_amd.build import build
    build()
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=str(ROOT), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("REFUSALS ")]
    assert len(lines) == 1, r.stdout[-2000:]
    got = {k: tuple(v) if k.count("/") else v for k, v in json.loads(lines[0][9:]).items()}
    assert sorted(got) == sorted(EXPECTED)
    wrong = {k: (got[k], EXPECTED[k]) for k in EXPECTED if got[k] != EXPECTED[k]}
    assert not wrong, wrong
