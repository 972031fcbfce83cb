"""molclr_amd.task_store without a GPU: the loader's partition arithmetic on a
stub store, the trainer's ``device_data`` key, the store's refusal of a CPU
device, and the new entry points' declarations."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from molclr_amd.task_store import DeviceTaskLoader, DeviceTaskStore

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("molclr_collate_task", "molclr_stage_task_ids", "molclr_stage_motif_ids",
                "molclr_motif_items")


class StubStore:
    """What DeviceTaskLoader reads of a store: the device, and collate."""
    device = torch.device("cpu")

    def collate(self, ids, host_ids=None):
        assert torch.equal(ids.cpu(), torch.from_numpy(np.asarray(host_ids)))
        return ("batch", np.asarray(host_ids).copy())


@pytest.mark.parametrize("n,bs", [(1, 4), (8, 4), (19, 8), (33, 32), (40, 1)])
@pytest.mark.parametrize("shuffle", [False, True])
def test_loader_partitions_the_indices(n, bs, shuffle):
    indices = np.random.default_rng(n).permutation(100)[:n] + 7
    loader = DeviceTaskLoader(StubStore(), indices.tolist(), bs, shuffle=shuffle,
                              generator=torch.Generator().manual_seed(3))
    assert len(loader) == -(-n // bs) and len(loader.sampler) == n
    epochs = []
    for _ in range(2):
        pairs = list(loader.ids())
        assert len(pairs) == len(loader)
        for k, (d, h) in enumerate(pairs):
            assert d.dtype == torch.long and torch.equal(d, torch.from_numpy(np.asarray(h)))
            want = bs if k < len(pairs) - 1 else n - bs * (len(pairs) - 1)  # the partial last batch
            assert len(h) == want
        seen = np.concatenate([h for _, h in pairs])
        assert sorted(seen.tolist()) == sorted(indices.tolist())  # every index exactly once
        if not shuffle:
            assert seen.tolist() == indices.tolist()
        epochs.append(seen.tolist())
    if shuffle and n >= 19:
        assert epochs[0] != epochs[1]  # one permutation per epoch
    got = [b for _, b in loader]  # __iter__ collates each (dev_ids, host_ids)
    assert len(got) == len(loader) and sum(len(b) for b in got) == n


def test_loader_refuses_an_empty_batch_size():
    with pytest.raises(ValueError):
        DeviceTaskLoader(StubStore(), [0, 1], 0)


def test_store_needs_a_gpu():
    z = np.zeros((0, 2), np.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        DeviceTaskStore(z, [0], np.zeros((2, 0), np.int64), z, [0], "cpu", np.zeros(0, np.int64))

    class DS:
        smiles_data, labels, task, conversion = ["C"], [1], "classification", 1
    with pytest.raises(RuntimeError, match="GPU"):
        DeviceTaskStore.from_dataset(DS(), "cpu")


def test_package_exports_the_store():
    import molclr_amd
    assert molclr_amd.DeviceTaskStore is DeviceTaskStore
    assert molclr_amd.DeviceTaskLoader is DeviceTaskLoader


class _Asked(Exception):
    pass


class StubDataset:
    def get_data_loaders(self):
        raise _Asked("host")


def test_device_data_is_opt_in(tmp_path, monkeypatch):
    """Without the key the trainer asks the dataset for its host loaders, as
    it always did; ``device_data: True`` asks task_store.device_loaders."""
    from molclr_amd import task_store
    from molclr_amd.finetune import FineTune
    monkeypatch.setattr(FineTune, "_get_device", lambda self: torch.device("cpu"))

    def asked(wrapper, device):
        raise _Asked("device")

    monkeypatch.setattr(task_store, "device_loaders", asked)
    cfg = {"task_name": "BBBP", "dataset": {"task": "classification", "target": "label"},
           "log_root": str(tmp_path), "model_type": "gin"}
    assert "device_data" not in cfg
    off = FineTune(StubDataset(), dict(cfg))
    assert off.device_data is False
    with pytest.raises(_Asked, match="host"):
        off.train()
    assert FineTune(StubDataset(), dict(cfg, device_data=False)).device_data is False
    on = FineTune(StubDataset(), dict(cfg, device_data=True))
    assert on.device_data is True
    with pytest.raises(_Asked, match="device"):
        on.train()


def test_entry_points_are_declared_and_bound():
    """As tests/test_capi.py checks every symbol: declared in include/molclr.h
    outside comments, bound in _lib.SIGNATURES, exported by the library."""
    from molclr_amd import _lib
    from molclr_amd.build import build
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "molclr.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(molclr_[a-z0-9_]+)\s*\(", text))
    build()
    lib = _lib.load()
    for name in ENTRY_POINTS + ("molclr_collate_task_workspace_bytes",):
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # argument validation returns before any HIP call
    rc = lib.molclr_collate_task(None, None, None, None, None, 0, 0, None, -1, None, 1, 0, None,
                                 None, None, None, None, None, 0, 0, None, None, 0, None)
    assert rc == -1 and b"collate_task" in lib.molclr_last_error()
    rc = lib.molclr_motif_items(None, None, 0, None, 0, 0, None, None, None, None, 0, None)
    assert rc == -1 and b"motif_items" in lib.molclr_last_error()
    assert lib.molclr_collate_task_workspace_bytes(32) >= 2 * 33 * 8
