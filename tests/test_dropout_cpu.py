"""Dropout inside the encoder executors, the parts that need no GPU: the
stream's definition, the models' routing, what stays out of state_dict, the
seed derivation and the C ABI's new symbols."""
import re
from pathlib import Path

import numpy as np
import torch

from . import philox

ROOT = Path(__file__).resolve().parent.parent


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    zero = philox.philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(w) for w in zero] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xFFFFFFFF
    ones = philox.philox4x32_10((f, f, f, f), (f, f))
    assert [int(w) for w in ones] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    # arrays: element by element the scalar function
    ctr = np.arange(5, dtype=np.uint64)
    many = philox.philox4x32_10((ctr, 7, 1, 2), (3, 4))
    for i in range(5):
        one = philox.philox4x32_10((i, 7, 1, 2), (3, 4))
        assert [int(w[i]) for w in many] == [int(w) for w in one]


def test_mask_layout():
    m = philox.dropout_mask(seed=-5, call=(1 << 32) + 3, layer=2, p=0.3, N=3, D=8)
    assert m.shape == (3, 8) and m.dtype == np.uint8
    seed = -5 & 0xFFFFFFFFFFFFFFFF
    w = philox.philox4x32_10((2, 1, 2, 3), (seed & 0xFFFFFFFF, (seed >> 32) ^ 1))
    assert [int(x) for x in m[2, 4:8]] == [int(int(x) >= philox.threshold(0.3)) for x in w]
    assert philox.dropout_mask(0, 0, 0, 0.0, 4, 8).all()  # p = 0 keeps everything


def _models(drop):
    from molclr_amd import gcn_finetune, gcn_molclr, ginet_finetune, ginet_molclr
    return [ginet_molclr.GINet(2, 16, 32, drop_ratio=drop), gcn_molclr.GCN(2, 16, 32, drop_ratio=drop),
            ginet_finetune.GINet("classification", 2, 16, 32, drop),
            gcn_finetune.GCN("regression", 2, 16, 32, drop)]


def test_executor_takes_dropout():
    for m in _models(0.3):
        m.train()
        assert m._executor_ok(), type(m)
        m.eval()
        assert m._executor_ok(), type(m)
    for m in _models(1.0):  # F.dropout's all-zero output stays on the per-op path
        m.train()
        assert not m._executor_ok(), type(m)
    m = _models(0.3)[0]
    m.use_executor = False
    assert not m.train()._executor_ok()


def test_dropout_state_is_no_part_of_the_state_dict():
    for a, b in zip(_models(0.3), _models(0.0)):
        assert a.dropout_state is None
        assert list(a.state_dict()) == list(b.state_dict())
        assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
        a.dropout_state = torch.tensor([7, 0])  # as the first training forward sets it
        assert list(a.state_dict()) == list(b.state_dict())
        assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]


def test_seed_function():
    from molclr_amd.encoder import dropout_seed
    g = torch.Generator().manual_seed(3)
    s0 = dropout_seed(g, rank=0)
    g.manual_seed(3)
    assert dropout_seed(g, rank=0) == s0
    g.manual_seed(3)
    s1 = dropout_seed(g, rank=1)
    assert s1 != s0
    assert (s0 ^ s1) & 0xFFFFFFFFFFFFFFFF == 0x9E3779B97F4A7C15
    assert dropout_seed(g, rank=0) != s0  # the next draw of the same generator
    for s in (s0, s1):
        assert -2 ** 63 <= s < 2 ** 63
    torch.manual_seed(11)
    a = dropout_seed()
    torch.manual_seed(11)
    assert dropout_seed() == a  # the default generator: torch.manual_seed repeats a run


def test_new_symbols_declared_and_typed():
    from molclr_amd._lib import SIGNATURES, GcnEncoder, GinEncoder
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "molclr.h").read_text(), flags=re.S)
    for sym in ("molclr_dropout_next_key", "molclr_dropout_mask"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in SIGNATURES, sym
    for struct in (GinEncoder, GcnEncoder):  # the two fields, at the end
        assert [f[0] for f in struct._fields_][-2:] == ["drop_ratio", "drop_state"]
    for name in ("molclr_gin_encoder", "molclr_gcn_encoder"):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
        fields = [ln.strip() for ln in body.split(";") if ln.strip()]
        assert fields[-2:] == ["double drop_ratio", "int64_t* drop_state"], fields[-2:]
