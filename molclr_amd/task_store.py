"""Labelled molecules resident in HBM and their on-device collate.

The fine-tuning counterpart of :class:`~molclr_amd.augment.DeviceMoleculeStore`.
The reference's fine-tuning loader (dataset/dataset_test.py:114-169) parses
every SMILES again for every batch of every epoch and collates on the host;
:class:`DeviceTaskStore` featurises a ``MolTestDataset`` once, keeps the
molecules, their targets and (for the motif model) their motif assignments on
the device, and builds a batch from its molecule ids with
``molclr_collate_task`` (molclr_amd/csrc/task_collate.hip).  The batch is what
``collate_labelled([dataset[i] for i in ids]).to(device)`` gives, field for
field.  :class:`DeviceTaskLoader` iterates such batches like the trainer's
DataLoader (one ``torch.randperm`` per epoch, uploaded once); its ``ids()``
yields the ids alone for the captured steps, which gather straight into their
fixed buffers (``StagedTaskGraph.stage_task_ids``).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import smiles as msmiles
from .augment import DeviceMoleculeStore
from .data import Batch

# molclr_collate_task / molclr_motif_items status bits
STATUS_ID_RANGE, STATUS_SIZE_MISMATCH, STATUS_EDGE_CLAMPED = 1, 2, 4


def raise_for_collate_status(st: int) -> None:
    """ValueError naming every bit of a device collate's status word."""
    if st:
        what = []
        if st & STATUS_ID_RANGE:
            what.append("molecule id outside the store")
        if st & STATUS_SIZE_MISMATCH:
            what.append("the host's batch sizes are not the device's sums")
        if st & STATUS_EDGE_CLAMPED:
            what.append("a stored edge index outside its molecule (clamped)")
        raise ValueError("invalid device collate: " + ", ".join(what))


class DeviceTaskStore(DeviceMoleculeStore):
    """A DeviceMoleculeStore with targets ``y`` -- int64 [G] class labels or
    float32 [G, C] -- and optionally the motif assignments as a CSR
    (``set_motifs``).  Host copies of the per-molecule counts size every batch
    without a device round trip (``sizes``)."""

    def __init__(self, x, atom_ptr, edge_index, edge_attr, bond_ptr, device, y):
        super().__init__(x, atom_ptr, edge_index, edge_attr, bond_ptr, device)
        y = torch.as_tensor(y)
        if y.dtype in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
            y = y.to(torch.int64).reshape(-1)
        else:
            y = y.to(torch.float32)
            y = y.reshape(-1, 1) if y.dim() < 2 else y.reshape(y.shape[0], -1)
        if y.shape[0] != self.num_molecules:
            raise ValueError(f"y holds {y.shape[0]} rows, the store {self.num_molecules} molecules")
        self.y = y.to(self.device).contiguous()
        self.labels = self.y.dtype == torch.int64
        self.cols = 1 if self.labels else int(self.y.shape[1])
        self.motif_ptr = self.motif_ids = self.num_motif_items = None

    # -- construction ----------------------------------------------------------
    @classmethod
    def from_molecules(cls, mols, y, device) -> "DeviceTaskStore":
        """From objects with ``x`` / ``edge_index`` / ``edge_attr`` (as the
        parent's) and their targets."""
        xs = [np.asarray(m.x, dtype=np.int64).reshape(-1, 2) for m in mols]
        eis = [np.asarray(m.edge_index, dtype=np.int64).reshape(2, -1) for m in mols]
        eas = [np.asarray(m.edge_attr, dtype=np.int64).reshape(-1, 2) for m in mols]
        atom_ptr = np.concatenate([[0], np.cumsum([x.shape[0] for x in xs])]).astype(np.int64)
        bond_ptr = np.concatenate([[0], np.cumsum([e.shape[1] // 2 for e in eis])]).astype(np.int64)
        return cls(np.concatenate(xs, 0), atom_ptr, np.concatenate(eis, 1),
                   np.concatenate(eas, 0), bond_ptr, device, y)

    @classmethod
    def from_dataset(cls, dataset, device) -> "DeviceTaskStore":
        """Every molecule of a ``MolTestDataset`` featurised exactly once, with
        the dataset's own label rule (dataset_test.py:136-141: long labels, or
        float32 of ``label * conversion``).  Molecule id = dataset index."""
        if torch.device(device).type != "cuda":
            raise RuntimeError("DeviceTaskStore needs a GPU device (no CPU path)")
        mols = [msmiles.featurise(s, add_hs=True) for s in dataset.smiles_data]
        if dataset.task == 'classification':
            y = torch.tensor([int(v) for v in dataset.labels], dtype=torch.long)
        else:
            y = torch.tensor([v * dataset.conversion for v in dataset.labels],
                             dtype=torch.float).view(-1, 1)
        return cls.from_molecules(mols, y, device)

    def set_motifs(self, assignments) -> None:
        """The motif indices of every molecule (``assignments[i]``: a sequence,
        as molclr_amd.motifs.load_motifs returns) as a CSR on the device."""
        if len(assignments) != self.num_molecules:
            raise ValueError(f"{len(assignments)} assignments, {self.num_molecules} molecules")
        counts = np.array([len(a) for a in assignments], dtype=np.int64)
        ids = np.array([m for a in assignments for m in a], dtype=np.int64)
        ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.num_motif_items = counts
        self.motif_ptr = torch.from_numpy(ptr).to(self.device)
        # one spare entry: the table's pointer is never NULL
        self.motif_ids = torch.from_numpy(np.concatenate([ids, [0]]).astype(np.int64)).to(self.device)

    # -- sizes -----------------------------------------------------------------
    def _host_ids(self, ids, host_ids) -> np.ndarray:
        if host_ids is None:
            host_ids = torch.as_tensor(ids).cpu()
        ids_h = np.asarray(host_ids, dtype=np.int64).reshape(-1)
        if ids_h.size and (ids_h.min() < 0 or ids_h.max() >= self.num_molecules):
            raise IndexError("molecule id out of range")
        return ids_h

    def _dev_ids(self, ids, ids_h) -> torch.Tensor:
        if isinstance(ids, torch.Tensor) and ids.device == self.device:
            return ids.to(torch.int64).contiguous()
        return torch.as_tensor(ids_h).to(self.device, non_blocking=True)

    def sizes(self, host_ids) -> tuple:
        """(nodes, directed edges) of the batch of the host ids -- with motifs
        set, (nodes, edges, motif items) -- from the host count arrays."""
        ids_h = np.asarray(host_ids, dtype=np.int64).reshape(-1)
        n = int(self.num_atoms[ids_h].sum())
        e = int(2 * self.num_bonds[ids_h].sum())
        if self.num_motif_items is None:
            return n, e
        return n, e, int(self.num_motif_items[ids_h].sum())

    # -- collate ---------------------------------------------------------------
    def collate_into(self, ids, N: int, E: int, x, edge_index, edge_attr, batch, ptr, y,
                     status) -> None:
        """``molclr_collate_task`` of the device ids into caller-made buffers
        sized for ``N`` nodes and ``E`` edges (the launch itself: no checks)."""
        B = int(ids.shape[0])
        ws_bytes = _lib.query("molclr_collate_task_workspace_bytes", B)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        _lib.call("molclr_collate_task", self.x.data_ptr(), self.atom_ptr.data_ptr(),
                  self.edge_index.data_ptr(), self.edge_attr.data_ptr(), self.bond_ptr.data_ptr(),
                  self.num_molecules, int(self.edge_index.shape[1]), ids.data_ptr(), B,
                  self.y.data_ptr(), self.cols, int(not self.labels), x.data_ptr(),
                  edge_index.data_ptr(), edge_attr.data_ptr(), batch.data_ptr(), ptr.data_ptr(),
                  y.data_ptr(), int(N), int(E), status.data_ptr(), ws.data_ptr(), ws_bytes,
                  _lib.stream_of(self.device))

    def collate(self, ids, host_ids=None, check: bool = False) -> Batch:
        """The collated batch of the molecules ``ids``: the fields of
        ``collate_labelled`` on the device -- ``x``, ``edge_index``,
        ``edge_attr``, ``batch``, ``ptr``, ``y`` [B, 1] (float targets: [B, C]),
        ``mol_index`` -- and ``status``, the launch's validity word.

        ``ids`` may already be an int64 device tensor; give its host copy as
        ``host_ids`` to size the outputs without a device round trip."""
        ids_h = self._host_ids(ids, host_ids)
        ids_d = self._dev_ids(ids, ids_h)
        B = int(ids_h.shape[0])
        N, E = self.sizes(ids_h)[:2]
        i64 = dict(dtype=torch.int64, device=self.device)
        x = torch.empty(N, 2, **i64)
        ei = torch.empty(2, E, **i64)
        ea = torch.empty(E, 2, **i64)
        batch = torch.empty(N, **i64)
        ptr = torch.empty(B + 1, **i64)
        y = torch.empty((B, 1) if self.labels else (B, self.cols), dtype=self.y.dtype,
                        device=self.device)
        status = torch.empty(1, dtype=torch.int32, device=self.device)
        self.collate_into(ids_d, N, E, x, ei, ea, batch, ptr, y, status)
        if check:
            raise_for_collate_status(int(status.item()))
        b = Batch(x=x, edge_index=ei, edge_attr=ea, batch=batch)
        b.ptr = ptr
        b.y = y
        b.mol_index = ids_d
        b._num_graphs = B
        b.status = status
        b._molclr_host_ids = ids_h  # sizes the motif items without a round trip
        return b

    def motif_items(self, ids, host_ids=None, check: bool = False) -> tuple:
        """``(mol_idx [T + B], clique_idx [T])`` of the batch, as
        molclr_amd.motifs.motif_batch builds them on the host."""
        if self.motif_ptr is None:
            raise RuntimeError("DeviceTaskStore: no motifs set (set_motifs)")
        ids_h = self._host_ids(ids, host_ids)
        ids_d = self._dev_ids(ids, ids_h)
        B = int(ids_h.shape[0])
        T = int(self.num_motif_items[ids_h].sum())
        i64 = dict(dtype=torch.int64, device=self.device)
        mol_idx = torch.empty(T + B, **i64)
        clique_idx = torch.empty(T, **i64)
        if B == 0:
            return mol_idx, clique_idx
        status = torch.empty(1, dtype=torch.int32, device=self.device)
        ws_bytes = _lib.query("molclr_motif_items_workspace_bytes", B)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        _lib.call("molclr_motif_items", self.motif_ptr.data_ptr(), self.motif_ids.data_ptr(),
                  self.num_molecules, ids_d.data_ptr(), B, T, mol_idx.data_ptr(),
                  clique_idx.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes,
                  _lib.stream_of(self.device))
        if check:
            raise_for_collate_status(int(status.item()))
        return mol_idx, clique_idx


class _IndexSampler:
    """What ``loader.sampler`` must offer: the number of molecules per epoch
    (finetune_step.CapturedEval sizes its gather buffers by it)."""

    def __init__(self, indices):
        self.indices = indices

    def __len__(self) -> int:
        return len(self.indices)

    def __iter__(self):
        return iter(self.indices)


class DeviceTaskLoader:
    """Batches of a :class:`DeviceTaskStore` over the molecule ids
    ``indices``, like ``DataLoader(dataset, batch_size,
    sampler=SubsetRandomSampler(indices), drop_last=False)``.

    With ``shuffle`` every epoch draws one ``torch.randperm`` (from
    ``generator``, else torch's global one), gathers the epoch's ids on the
    host and uploads them once; a batch's device ids are a slice of that
    tensor and its host ids -- which size the batch -- the same slice of the
    host array.  Iterating yields collated device batches; ``ids()`` yields
    ``(dev_ids, host_ids)`` alone."""

    def __init__(self, store, indices, batch_size: int, shuffle: bool = True, generator=None):
        self.store = store
        self.indices = np.asarray(list(indices), dtype=np.int64).reshape(-1)
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        self.shuffle = bool(shuffle)
        self.generator = generator
        self.sampler = _IndexSampler(self.indices)

    def __len__(self) -> int:
        return (len(self.indices) + self.batch_size - 1) // self.batch_size

    def epoch_ids(self) -> np.ndarray:
        """The epoch's molecule ids on the host, in batch order."""
        if not self.shuffle:
            return self.indices
        perm = torch.randperm(len(self.indices), generator=self.generator).numpy()
        return self.indices[perm]

    def ids(self):
        ids_h = self.epoch_ids()
        ids_d = torch.from_numpy(np.ascontiguousarray(ids_h)).to(self.store.device,
                                                                 non_blocking=True)
        for k in range(0, len(ids_h), self.batch_size):
            yield ids_d[k:k + self.batch_size], ids_h[k:k + self.batch_size]

    def __iter__(self):
        for ids_d, ids_h in self.ids():
            yield self.store.collate(ids_d, ids_h)


def device_loaders(wrapper, device) -> tuple:
    """``(smiles_data, store, train, valid, test)`` for a
    dataset_test.MolTestDatasetWrapper (read only: its ``data_path``,
    ``target``, ``task``, ``batch_size`` and ``split_indices``): the dataset
    featurised once into a :class:`DeviceTaskStore` on ``device`` and three
    DeviceTaskLoaders over the same split as the wrapper's host loaders.  What
    the trainer calls with the config key ``device_data``."""
    from .dataset_test import MolTestDataset
    dataset = MolTestDataset(data_path=wrapper.data_path, target=wrapper.target, task=wrapper.task)
    store = DeviceTaskStore.from_dataset(dataset, device)
    train_idx, valid_idx, test_idx = wrapper.split_indices(len(dataset))
    train, valid, test = (DeviceTaskLoader(store, idx, wrapper.batch_size, shuffle=True)
                          for idx in (train_idx, valid_idx, test_idx))
    return dataset.smiles_data, store, train, valid, test


__all__ = ["DeviceTaskLoader", "DeviceTaskStore", "device_loaders", "raise_for_collate_status"]
