"""The C-ABI library builds, loads and exports every symbol include/molclr.h
declares (no compute calls: argument validation returns before any HIP call)."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "molclr.h"


def declared_symbols():
    text = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(molclr_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from molclr_amd import _lib
    from molclr_amd.build import build
    build()
    return _lib.load()


def test_header_declares_the_path():
    syms = declared_symbols()
    for s in ("molclr_graph_build", "molclr_gine_aggregate_fwd", "molclr_gine_aggregate_bwd",
              "molclr_gemm_f32", "molclr_ntxent_fwd", "molclr_ntxent_bwd", "molclr_adam_step"):
        assert s in syms


def test_library_exports_every_declared_symbol(lib):
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, missing


def test_ctypes_signatures_cover_header():
    from molclr_amd._lib import SIGNATURES
    assert sorted(SIGNATURES) == declared_symbols()


def test_version_and_error_plumbing(lib):
    assert b"gfx950" in lib.molclr_version()
    # bad epilogue -> MOLCLR_ERR_ARG before any device work
    rc = lib.molclr_gemm_f32(None, None, None, 4, 4, 4, 4, 4, 4, 0, 0, 99, None, None, 0, None, 0, None)
    assert rc == -1
    assert b"epilogue" in lib.molclr_last_error()
    rc = lib.molclr_gine_aggregate_fwd(None, None, None, None, None, None, None, 10, 301, None)
    assert rc == -1 and b"multiple of 4" in lib.molclr_last_error()
    rc = lib.molclr_edge_tables_combine(17, None, None, None, 300, None)
    assert rc == -1 and b"layers" in lib.molclr_last_error()
    rc = lib.molclr_graph_build(None, None, None, (1 << 24) + 1, 0, 1, None, None, None, None, None,
                                None, None, None, None, None, None, 0, None)
    assert rc == -1 and b"neighbour-slot" in lib.molclr_last_error()


def test_workspace_queries(lib):
    assert lib.molclr_graph_build_workspace_bytes(100, 300) >= 300 * 4 * 4
    assert lib.molclr_gemm_f32_workspace_bytes(300, 600, 15000) > 0   # split-K weight gradient
    assert lib.molclr_gemm_f32_workspace_bytes(15000, 600, 300) == 0  # no split needed
    assert lib.molclr_ntxent_workspace_bytes(1024, 1024, 256) > 0


def test_product_path_has_no_cpu_fallback():
    """The product package never imports the oracle."""
    for p in (ROOT / "molclr_amd").rglob("*.py"):
        assert "oracle" not in re.sub(r'""".*?"""', "", p.read_text(), flags=re.S).replace(
            "# oracle", ""), p


def test_torch_ops_registered():
    """import molclr_amd.torch_ops registers the operator seam
    in the torch.ops.molclr namespace (no device needed to register)."""
    import torch

    import molclr_amd.torch_ops as tops
    for name in tops.OPS:
        assert hasattr(torch.ops.molclr, name), name
    schema = str(torch.ops.molclr.gine_aggregate.default._schema)
    assert schema.startswith("molclr::gine_aggregate(Tensor h, Tensor E1, Tensor E2")


_BAND_CHILD = r"""
import json
from molclr_amd import _lib
lib = _lib.load()
out = {}
def err():
    return lib.molclr_last_error().decode()
for w in (0, 2, 4100):
    out["colsum_ws_%d" % w] = int(lib.molclr_colsum_f32_workspace_bytes(100, w))
    rc = lib.molclr_colsum_f32(None, None, 100, w, w, 0, None, 0, None)
    out["colsum_%d" % w] = [rc, err()]
for w in (2, 4100):
    out["bn_ws_%d" % w] = int(lib.molclr_batchnorm_workspace_bytes(100, w))
    rc = lib.molclr_batchnorm_fwd(None, None, None, None, None, None, None, None, None, 100, w,
                                  0.1, 1e-5, 1, 0, None, 0, None)
    out["bn_%d" % w] = [rc, err()]
    out["agg_ws_%d" % w] = int(lib.molclr_gine_aggregate_bwd_workspace_bytes(100, w))
    rc = lib.molclr_gine_aggregate_bwd(None, None, None, None, None, None, None, None, 100, w, 0,
                                       None, 0, None)
    out["agg_%d" % w] = [rc, err()]
# the supported range is unchanged at its ends
out["colsum_ws_4"] = int(lib.molclr_colsum_f32_workspace_bytes(100, 4))
out["colsum_ws_4096"] = int(lib.molclr_colsum_f32_workspace_bytes(100, 4096))
print("BAND " + json.dumps(out))
"""


def test_band_width_is_refused_not_divided_by(lib):
    """A width make_band() cannot plan (dim < 4: d4 == 0; dim > 4096: band == 0)
    divided by zero on the host.  Every entry point that plans a band now
    refuses it with MOLCLR_ERR_ARG and its workspace query returns 0.  Run in a
    child process: a SIGFPE must not take the test process with it."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", _BAND_CHILD], cwd=str(ROOT), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("BAND ")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0][5:])
    for w in (0, 2, 4100):
        assert out["colsum_ws_%d" % w] == 0
        rc, msg = out["colsum_%d" % w]
        assert rc == -1 and "cols %d " % w in msg, (w, rc, msg)
    for w in (2, 4100):
        assert out["bn_ws_%d" % w] == 0 and out["agg_ws_%d" % w] == 0
        for key in ("bn_%d", "agg_%d"):
            rc, msg = out[key % w]
            assert rc == -1 and "dim %d " % w in msg, (key, w, rc, msg)
    # P * cols floats + 256: 100 rows are one partition at band 256 (cols 4)
    # and ceil(100 / 16) = 7 at band 1 (cols 4096)
    assert out["colsum_ws_4"] == 1 * 4 * 4 + 256
    assert out["colsum_ws_4096"] == 7 * 4096 * 4 + 256
