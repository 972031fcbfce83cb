"""The GCN's bf16 storage path, the parts that need no GPU: constructor
validation, the pad multiple, unchanged state_dict / seeded initialisation, the
ctypes mirror of struct molclr_gcn_encoder and the new symbols' bindings."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def _classes():
    from molclr_amd import gcn_finetune, gcn_molclr
    return (lambda **kw: gcn_molclr.GCN(2, 44, 32, **kw),
            lambda **kw: gcn_finetune.GCN("regression", 2, 44, 32, **kw))


def test_precision_is_validated():
    for make in _classes():
        assert make().precision == "fp32"
        assert make(precision="bf16").precision == "bf16"
        with pytest.raises(ValueError, match="precision"):
            make(precision="fp16")


def test_pad_multiple_is_8_for_bf16():
    for make in _classes():
        m32, m16 = make(), make(precision="bf16")
        assert m32._pad_multiple() == 4 and m32._dim_pad() == 0
        assert m16._pad_multiple() == 8 and m16._dim_pad() == 4  # 44 -> 48
    from molclr_amd.gcn_molclr import GCN
    assert GCN(2, 300, 32, precision="bf16")._dim_pad() == 4  # the c3 width runs at 304
    # the padded parameter list: zero columns / rows up to the multiple
    m = GCN(2, 44, 32, precision="bf16")
    shapes = [tuple(p.shape) for p in m._encoder_params()]
    assert shapes == [(119, 48), (3, 48)] + [(48, 48), (48,), (5, 1), (3, 1), (48,), (48,)] * 2
    W = m._encoder_params()[2]
    assert torch.equal(W[:44, :44], m.gnns[0].weight) and not W[44:].any() and not W[:, 44:].any()


def test_state_dict_and_seeded_parameters_are_the_fp32_models():
    for make in _classes():
        torch.manual_seed(3)
        a = make()
        torch.manual_seed(3)
        b = make(precision="bf16")
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]), k
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]


def test_bf16_runs_through_the_executor_only():
    from molclr_amd.gcn_molclr import GCN
    m = GCN(2, 48, 32, precision="bf16")
    m.use_executor = False
    with pytest.raises(NotImplementedError, match="bf16 runs through the encoder executor only"):
        m.encode(type("D", (), {"x": torch.zeros(1, 2, dtype=torch.long)})(), graph=object())


def test_struct_has_dtype_in_the_padding_after_fp32_gemm():
    """dtype sits in what was padding between fp32_gemm and status: a
    zero-initialised struct is the fp32 path, the struct keeps its size and
    every other field its offset (callers built against the struct without the
    field stay binary-compatible); header and ctypes mirror agree."""
    from molclr_amd._lib import DTYPE_BF16, DTYPE_F32, GcnEncoder
    names = [f[0] for f in GcnEncoder._fields_]
    assert names[names.index("fp32_gemm") + 1] == "dtype" and names[-4:] == [
        "dtype", "status", "drop_ratio", "drop_state"]
    assert GcnEncoder.dtype.size == 4 and GcnEncoder.dtype.offset == GcnEncoder.fp32_gemm.offset + 4

    class Without(ctypes.Structure):
        _fields_ = [f for f in GcnEncoder._fields_ if f[0] != "dtype"]

    assert ctypes.sizeof(Without) == ctypes.sizeof(GcnEncoder)
    for name in names:
        if name != "dtype":
            assert getattr(Without, name).offset == getattr(GcnEncoder, name).offset, name
    assert GcnEncoder().dtype == DTYPE_F32 == 0 and DTYPE_BF16 == 1
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "molclr.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct molclr_gcn_encoder \{(.*?)\} molclr_gcn_encoder;", header,
                     flags=re.S).group(1)
    fields = [" ".join(ln.split()) for ln in body.split(";") if ln.strip()]
    assert fields[-5:] == ["int32_t fp32_gemm", "int32_t dtype", "int32_t* status",
                           "double drop_ratio", "int64_t* drop_state"]


def test_new_symbols_declared_and_bound():
    from molclr_amd import ops
    from molclr_amd._lib import SIGNATURES
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "molclr.h").read_text(), flags=re.S)
    for sym, nargs in (("molclr_gcn_aggregate_fwd_bf16", 12), ("molclr_gcn_aggregate_bwd_bf16", 15),
                       ("molclr_gcn_encoder_arena_bytes_dtype", 4),
                       ("molclr_gcn_encoder_workspace_bytes_dtype", 4)):
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % sym, header, flags=re.S)
        assert decl, sym
        assert sym in SIGNATURES and len(SIGNATURES[sym][1]) == nargs == decl.group(1).count(",") + 1
    # the executor takes h_out / dh_out in either storage type
    assert re.search(r"molclr_gcn_encoder_fwd\([^;]*\bvoid\* h_out", header)
    assert re.search(r"molclr_gcn_encoder_bwd\([^;]*\bconst void\* dh_out", header)
    assert ops._GCN.sized_by_dtype and ops._GCN.size_suffix == "_dtype"
    from molclr_amd import _lib
    lib = _lib.load()  # binds every signature: a missing export raises here
    # the three-argument queries keep their fp32 meaning; bf16 halves the node features
    L, N, D = 3, 1000, 64
    assert lib.molclr_gcn_encoder_arena_bytes_dtype(L, N, D, 0) == \
        lib.molclr_gcn_encoder_arena_bytes(L, N, D)
    assert lib.molclr_gcn_encoder_workspace_bytes_dtype(L, N, D, 0) == \
        lib.molclr_gcn_encoder_workspace_bytes(L, N, D)
    feat = (2 * L + 1) * N * D  # z_l, h_l, h0
    assert lib.molclr_gcn_encoder_arena_bytes(L, N, D) - \
        lib.molclr_gcn_encoder_arena_bytes_dtype(L, N, D, 1) == 2 * feat
    assert lib.molclr_gcn_encoder_arena_bytes_dtype(L, N, D, 7) == 0
