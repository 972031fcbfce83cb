"""The captured fine-tuning step's host side for the motif model (no GPU): the
fourth term of the bucket key -- the item capacity -- and what
unsupported_reason says about the motif model."""
import pytest
import torch

from molclr_amd import _lib


def _eval(motif, **kw):
    from molclr_amd.finetune_step import CapturedEval
    from molclr_amd.ginet_finetune import GINet
    from molclr_amd.ginet_finetune_mp import GINet as MotifGINet
    model = MotifGINet(50, "regression", 2, 64, 128) if motif else GINet("regression", 2, 64, 128)
    return CapturedEval(model, "mse", node_quantum=128, edge_quantum=512, node_slack=0, **kw)


def test_fourth_key_term_is_the_item_capacity():
    ev = _eval(True, item_quantum=64)
    assert ev.motif and ev.item_quantum == 64
    assert ev.bucket((700, 1500, 32, 0)) == (768, 2048, 32, 64)
    assert ev.bucket((700, 1500, 32, 64)) == (768, 2048, 32, 64)
    assert ev.bucket((700, 1500, 32, 65)) == (768, 2048, 32, 128)
    assert ev.bucket((700, 1500, 32), 130) == (768, 2048, 32, 192)  # the count on its own
    items = (torch.zeros(7 + 32, dtype=torch.long), torch.zeros(7, dtype=torch.long))
    assert ev.bucket((700, 1500, 32), items) == (768, 2048, 32, 64)  # (mol_idx, clique_idx)
    assert _eval(True).bucket((700, 1500, 32, 1)) == (768, 2048, 32, 256)  # default quantum
    with pytest.raises(TypeError, match="items"):
        ev.bucket((700, 1500, 32))
    keys = [(768, 2048, 32, 64), (768, 2048, 32, 192), (896, 2048, 32, 64), (128, 512, 5, 64)]
    # the smallest graph that holds the batch and its items
    assert ev.pick(keys, (760, 2000, 32, 60)) == (768, 2048, 32, 64)
    assert ev.pick(keys, (760, 2000, 32, 64)) == (768, 2048, 32, 64)
    # more items than the capacity: the larger bucket, or none -- then a new one
    assert ev.pick(keys, (760, 2000, 32, 65)) == (768, 2048, 32, 192)
    assert ev.pick(keys, (760, 2000, 32, 193)) is None
    assert ev.bucket((760, 2000, 32, 193)) == (768, 2560, 32, 256)
    assert ev.pick(keys, (770, 2000, 32, 65)) is None  # the node bucket that fits has 64
    assert ev.pick(keys, (770, 2000, 32, 10)) == (896, 2048, 32, 64)
    # molecule count, nodes and edges as for the plain models
    assert ev.pick(keys, (100, 200, 5, 3)) == (128, 512, 5, 64)
    assert ev.pick(keys, (100, 200, 6, 3)) is None
    assert ev.pick(keys, (600, 1000, 32, 3)) is None  # node_slack 0
    assert ev.lookup((100, 200, 5, 3)) is None  # nothing captured yet


def test_plain_models_keep_three_term_keys():
    ev = _eval(False, item_quantum=64)
    assert not ev.motif
    assert ev.bucket((700, 1500, 32)) == (768, 2048, 32)
    assert ev.bucket((100, 493, 5)) == (128, 1024, 5)
    keys = [(768, 2048, 32), (896, 2048, 32), (128, 512, 5)]
    assert ev.pick(keys, (760, 2000, 32)) == (768, 2048, 32)
    assert ev.pick(keys, (770, 2000, 32)) == (896, 2048, 32)
    assert ev.pick(keys, (770, 2049, 32)) is None
    assert ev.pick(keys, (100, 200, 5)) == (128, 512, 5)
    assert ev.lookup((100, 200, 5)) is None


def test_unsupported_reason_for_the_motif_model(monkeypatch):
    """With the batch's items handed over (motif_items=True) the motif model is
    taken at FEAT 128; asked without, the answer names the items."""
    from molclr_amd import ops
    from molclr_amd.finetune_step import unsupported_reason
    from molclr_amd.ginet_finetune_mp import GINet as MotifGINet

    def reason(model):
        return unsupported_reason(model, motif_items=True)

    assert reason(MotifGINet(50, "classification", 2, 64, 128)) is None
    assert reason(MotifGINet(50, "regression", 2, 64, 128)) is None
    assert "motif" in unsupported_reason(MotifGINet(50, "classification", 2, 64, 128))
    # the first pred_head layer is 2 * feat_dim wide: the fused head refuses it first
    half = _lib.TASK_HEAD_MAX_DIM // 2 + 2
    why = reason(MotifGINet(5, "classification", 2, 64, half))
    assert "composed" in why and str(2 * half) in why
    assert "padding" in reason(MotifGINet(5, "classification", 2, 62, 128))
    off = MotifGINet(5, "classification", 2, 64, 128)
    off.use_executor = False
    assert "executor" in reason(off)
    monkeypatch.setattr(ops, "MOTIF_POOL", False)
    assert "MOLCLR_MOTIF_POOL" in reason(MotifGINet(50, "classification", 2, 64, 128))


def test_trainer_reads_the_motif_key(tmp_path, monkeypatch):
    from molclr_amd.finetune import FineTune
    monkeypatch.setattr(FineTune, "_get_device", lambda self: torch.device("cpu"))
    cfg = {"task_name": "BBBP", "dataset": {"task": "classification", "target": "label"},
           "log_root": str(tmp_path), "hip_graph": True}
    assert FineTune(None, dict(cfg)).hip_graph_motif is False
    assert FineTune(None, dict(cfg, hip_graph_motif=True)).hip_graph_motif is True


def test_loss_staged_needs_the_items():
    from molclr_amd.ginet_finetune_mp import GINet as MotifGINet
    with pytest.raises(NotImplementedError, match="items"):
        MotifGINet(5, "classification", 2, 64, 128).loss_staged(None, None)


def test_signatures_of_the_new_entry_points():
    from molclr_amd._lib import SIGNATURES
    for name in ("molclr_motif_pool_fwd", "molclr_motif_pool_bwd"):
        assert SIGNATURES[name + "_cap"] == SIGNATURES[name]
    assert SIGNATURES["molclr_motif_pool_cap_workspace_bytes"] == \
        SIGNATURES["molclr_motif_pool_workspace_bytes"]
    assert len(SIGNATURES["molclr_stage_motif"][1]) == 11
    bits = (_lib.STATUS_ITEM_OVERFLOW, _lib.STATUS_ITEM_ORDER, _lib.STATUS_ITEM_MOL)
    assert bits == (128, 256, 512) and _lib.MOTIF_PAD == 2 ** 63 - 1
