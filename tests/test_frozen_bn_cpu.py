"""Frozen BatchNorm without a GPU: the header's declarations, the struct
layout, the models' train() and the trainer's config key."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "molclr.h").read_text()


def test_header_declares_the_frozen_backward():
    for name in ("molclr_batchnorm_bwd_frozen", "molclr_batchnorm_seg_bwd_frozen",
                 "molclr_batchnorm_seg_bwd_frozen_dev", "molclr_batchnorm_seg_bwd_frozen_max"):
        assert re.search(r"\bint\s+%s\s*\(" % name, HEADER), name
    for name, value in (("MOLCLR_MODE_EVAL", 0), ("MOLCLR_MODE_TRAIN", 1),
                        ("MOLCLR_MODE_FROZEN_BN", 2)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), HEADER), name


def test_ctypes_names_and_signatures():
    from molclr_amd import _lib
    assert (_lib.MODE_EVAL, _lib.MODE_TRAIN, _lib.MODE_FROZEN_BN) == (0, 1, 2)
    sig = _lib.SIGNATURES
    # the frozen entry points take their training-mode counterparts' arguments
    for a, b in (("molclr_batchnorm_bwd_frozen", "molclr_batchnorm_bwd"),
                 ("molclr_batchnorm_seg_bwd_frozen", "molclr_batchnorm_seg_bwd"),
                 ("molclr_batchnorm_seg_bwd_frozen_dev", "molclr_batchnorm_seg_bwd_dev"),
                 ("molclr_batchnorm_seg_bwd_frozen_max", "molclr_batchnorm_seg_bwd_max")):
        assert sig[a][0] is sig[b][0] and list(sig[a][1]) == list(sig[b][1]), a


# sizeof and the offsets of the last two fields (drop_ratio, drop_state) as they
# were before `training` gained its third value
PINNED = {"GinEncoder": (2016, 2000, 2008), "GcnEncoder": (1504, 1488, 1496)}


def test_encoder_struct_layout_unchanged():
    """`training` stays an int32 at offset 4 between num_layer and dim; the
    size and the last two fields of both encoder structs stay where they were."""
    from molclr_amd import _lib
    for S in (_lib.GinEncoder, _lib.GcnEncoder):
        size, ratio, state = PINNED[S.__name__]
        assert ctypes.sizeof(S) == size
        assert [n for n, *_ in S._fields_][-2:] == ["drop_ratio", "drop_state"]
        assert S.drop_ratio.offset == ratio and S.drop_state.offset == state
        assert S.training.offset == 4 and S.training.size == 4
        assert S.num_layer.offset == 0 and S.dim.offset == 8
    for struct in ("molclr_gin_encoder", "molclr_gcn_encoder"):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, re.S).group(1)
        assert re.search(r"int32_t\s+training\s*;", body)
        fields = re.findall(r"(\w+)\s*(?:\[[^\]]*\])?\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert fields[:3] == ["num_layer", "training", "dim"]
        assert fields[-2:] == ["drop_ratio", "drop_state"]


def _models():
    from molclr_amd.gcn_finetune import GCN as FtGCN
    from molclr_amd.gcn_molclr import GCN
    from molclr_amd.ginet_finetune import GINet as FtGIN
    from molclr_amd.ginet_finetune_mp import GINet as MotifGIN
    from molclr_amd.ginet_molclr import GINet
    yield GINet(num_layer=2, emb_dim=12, feat_dim=16)
    yield GCN(num_layer=2, emb_dim=12, feat_dim=16)
    yield FtGIN("classification", num_layer=2, emb_dim=12, feat_dim=16)
    yield FtGCN("regression", num_layer=2, emb_dim=12, feat_dim=16)
    yield MotifGIN(7, "classification", num_layer=2, emb_dim=12, feat_dim=16)


def test_train_with_freeze_bn_leaves_batchnorms_in_eval():
    for model in _models():
        assert model.freeze_bn is False
        model.train()
        assert all(bn.training for bn in model.batch_norms) and not model.bn_frozen()
        model.freeze_bn = True  # takes effect at once
        assert model.training and not any(bn.training for bn in model.batch_norms)
        assert model.bn_frozen()
        model.eval()
        model.train()  # a trainer's per-epoch call does not undo it
        assert model.training and not any(bn.training for bn in model.batch_norms)
        others = [m for m in model.modules()
                  if not isinstance(m, torch.nn.BatchNorm1d) and m is not model]
        assert all(m.training for m in others)
        assert model._executor_ok()
        model.freeze_bn = False
        assert all(bn.training for bn in model.batch_norms)
        # by hand: the same mode until the next train()
        for bn in model.batch_norms:
            bn.eval()
        assert model.bn_frozen() and model._executor_ok()
        assert "freeze_bn" not in model.state_dict() and "_freeze_bn" not in model.state_dict()


def _config(**extra):
    cfg = {"batch_size": 4, "epochs": 1, "eval_every_n_epochs": 1, "fine_tune_from": "none",
           "log_every_n_steps": 50, "fp16_precision": False, "init_lr": 5e-4,
           "init_base_lr": 1e-4, "weight_decay": "1e-6", "gpu": "cpu", "task_name": "BBBP",
           "model_type": "gin",
           "model": {"num_layer": 2, "emb_dim": 12, "feat_dim": 16, "drop_ratio": 0.3,
                     "pool": "mean"},
           "dataset": {"task": "classification", "target": "p_np"}}
    cfg.update(extra)
    return cfg


@pytest.mark.parametrize("model_type", ["gin", "gcn"])
def test_config_key_parses(model_type, tmp_path):
    from molclr_amd.finetune import FineTune
    built = {}
    for key in (None, False, True):
        extra = {} if key is None else {"freeze_bn": key}
        # the trainer's constructor insists on a GPU; build_model needs its
        # config, task and device alone
        ft = object.__new__(FineTune)
        ft.config = _config(model_type=model_type, ckpt_root=str(tmp_path), **extra)
        ft.task, ft.device = ft.config["dataset"]["task"], torch.device("cpu")
        torch.manual_seed(0)
        model = ft.build_model()
        built[key] = model
        assert model.freeze_bn is bool(key)
        model.train()
        assert all(bn.training != bool(key) for bn in model.batch_norms)
    # default off: the model is built as before, parameter for parameter
    a, b = built[None].state_dict(), built[False].state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
