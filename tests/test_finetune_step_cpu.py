"""The captured fine-tuning step without a GPU: its C ABI is declared and
typed, the bucket / lookup arithmetic, and the trainer's ``hip_graph`` key."""
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
NEW = ("molclr_stage_task", "molclr_task_step_tail", "molclr_eval_tail")


def test_new_symbols_declared_and_typed():
    from molclr_amd._lib import SIGNATURES
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "molclr.h").read_text(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, name
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        res, args = SIGNATURES[name]
        assert len(args) == nargs, (name, len(args), nargs)
    assert "hipMemsetAsync" not in (ROOT / "molclr_amd/csrc/finetune_step.hip").read_text()
    assert "hipMemcpyAsync" not in (ROOT / "molclr_amd/csrc/finetune_step.hip").read_text()


def _objects(node_slack):
    """A CapturedEval (its constructor needs no GPU) and a CapturedFinetuneStep
    made without its optimizers (FusedAdam is GPU-only): the arithmetic under
    test is the shared base's."""
    from molclr_amd.finetune_step import CapturedEval, CapturedFinetuneStep, _CapturedTask
    from molclr_amd.ginet_finetune import GINet
    model = GINet("regression", 2, 64, 128)
    ev = CapturedEval(model, "mse", node_quantum=128, edge_quantum=512, node_slack=node_slack)
    step = CapturedFinetuneStep.__new__(CapturedFinetuneStep)
    _CapturedTask.__init__(step, model, "mse", None, 128, 512, 16, node_slack, 0.04)
    return step, ev


@pytest.mark.parametrize("which", [0, 1], ids=["step", "eval"])
def test_bucket_and_lookup_arithmetic(which):
    obj = _objects(0)[which]
    # nodes up to the node quantum, edges (+4 % headroom, + 1) up to the edge quantum
    assert obj.bucket((700, 1500, 32)) == (768, 2048, 32)
    assert obj.bucket((768, 1500, 32)) == (768, 2048, 32)
    assert obj.bucket((769, 1500, 32)) == (896, 2048, 32)
    assert obj.bucket((1, 0, 1)) == (128, 512, 1)
    assert obj.bucket((100, 492, 5)) == (128, 512, 5)
    assert obj.bucket((100, 493, 5)) == (128, 1024, 5)  # int(493 * 1.04) + 1 = 513
    keys = [(768, 2048, 32), (896, 2048, 32), (128, 512, 5)]
    # the smallest graph that holds the batch
    assert obj.pick(keys, (760, 2000, 32)) == (768, 2048, 32)
    assert obj.pick(keys, (770, 2000, 32)) == (896, 2048, 32)
    assert obj.pick(keys, (770, 2049, 32)) is None  # edges do not fit
    assert obj.pick(keys, (900, 100, 32)) is None   # nodes do not fit
    # slack 0: a smaller batch does not ride on a larger graph's padding rows
    assert obj.pick(keys, (600, 1000, 32)) is None
    # a partial last batch is a bucket of its own, whatever fits by size
    assert obj.pick(keys, (100, 200, 5)) == (128, 512, 5)
    assert obj.pick(keys, (100, 200, 6)) is None
    assert obj.pick([(768, 2048, 32)], (100, 200, 5)) is None
    assert obj.lookup((100, 200, 5)) is None  # nothing captured yet


def test_node_slack_is_honoured():
    step, ev = _objects(256)
    keys = [(1024, 4096, 32)]
    for obj in (step, ev):
        assert obj.node_slack == 256
        # 700 -> 768 rounded; 768 + 256 = 1024 is still within the slack
        assert obj.pick(keys, (700, 1500, 32)) == (1024, 4096, 32)
        # 600 -> 640 rounded; 640 + 256 < 1024
        assert obj.pick(keys, (600, 1500, 32)) is None
        # of two that fit, the smaller
        assert obj.pick(keys + [(896, 2048, 32)], (700, 1500, 32)) == (896, 2048, 32)
    from molclr_amd.finetune_step import CapturedEval
    assert CapturedEval(step.model, node_quantum=64).node_slack == 128  # default: two quanta


def test_step_needs_fused_adam_and_a_task_model():
    from molclr_amd.finetune_step import CapturedEval, CapturedFinetuneStep
    from molclr_amd.ginet_finetune import GINet
    from molclr_amd.ginet_molclr import GINet as PreGINet
    model = GINet("classification", 2, 64, 128)
    with pytest.raises(TypeError, match="FusedAdam"):
        CapturedFinetuneStep(model, [torch.optim.Adam(model.parameters())])
    with pytest.raises(TypeError, match="loss_staged"):
        CapturedEval(PreGINet(2, 64, 128))
    with pytest.raises(ValueError, match="criterion"):
        CapturedEval(model, "hinge")
    assert CapturedEval(model).criterion == "cross_entropy"


def test_unsupported_reason_names_the_cause():
    from molclr_amd import _lib
    from molclr_amd.finetune_step import unsupported_reason
    from molclr_amd.gcn_finetune import GCN
    from molclr_amd.ginet_finetune import GINet
    from molclr_amd.ginet_finetune_mp import GINet as MotifGINet
    assert unsupported_reason(GINet("classification", 2, 64, 128)) is None
    assert unsupported_reason(GCN("regression", 2, 64, 128)) is None
    assert "motif" in unsupported_reason(MotifGINet(10, "classification", 2, 64, 128))
    assert "padding" in unsupported_reason(GINet("classification", 2, 62, 128))
    off = GINet("classification", 2, 64, 128)
    off.use_executor = False
    assert "executor" in unsupported_reason(off)
    wide = GINet("classification", 2, 64, _lib.TASK_HEAD_MAX_DIM + 4)
    assert "composed" in unsupported_reason(wide)
    with pytest.raises(NotImplementedError):
        off.loss_staged(None, None)
    with pytest.raises(NotImplementedError):
        MotifGINet(10, "classification", 2, 64, 128).loss_staged(None, None)


def test_trainer_accepts_hip_graph_and_defaults_to_false(tmp_path, monkeypatch):
    from molclr_amd.finetune import FineTune
    monkeypatch.setattr(FineTune, "_get_device", lambda self: torch.device("cpu"))
    cfg = {"task_name": "BBBP", "dataset": {"task": "classification", "target": "label"},
           "log_root": str(tmp_path)}
    assert FineTune(None, dict(cfg)).hip_graph is False
    assert FineTune(None, dict(cfg, hip_graph=False)).hip_graph is False
    ft = FineTune(None, dict(cfg, hip_graph=True))
    assert ft.hip_graph is True and ft._captured is None
