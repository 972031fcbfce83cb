"""Labelled molecules for fine-tuning — drop-in for dataset/dataset_test.py.

``read_smiles`` / ``MolTestDataset`` / ``MolTestDatasetWrapper`` with the
reference's arguments (dataset_test.py:94-226).  Molecules are featurised by
molclr_amd.smiles (no RDKit) with explicit hydrogens, as the reference's
``Chem.AddHs`` does (dataset_test.py:126-127); a SMILES our parser rejects is
skipped where the reference skips one RDKit rejects.

Differences: the random split's test indices are the slice AFTER the
validation indices (the reference's ``indices[:split+split2]`` also contains
the validation molecules, dataset_test.py:203); ``splitting: scaffold`` needs
RDKit's Murcko scaffolds and raises NotImplementedError; an optional ``seed``
makes the split independent of numpy's global state.
"""
from __future__ import annotations

import csv

import numpy as np
import torch
from torch.utils.data.sampler import SubsetRandomSampler

from . import smiles as msmiles
from .data import Batch, Data

HARTREE_TO_EV = 27.211386246


def _parses(smiles: str) -> bool:
    try:
        msmiles.featurise(smiles, add_hs=True)
    except (ValueError, KeyError, IndexError):
        return False
    return True


def read_smiles(data_path, target, task):
    """CSV columns ``smiles`` and ``target`` -> (smiles list, label list).
    Rows with an empty label or an unparsable SMILES are skipped, and so is
    the first data row, as in the reference (its ``if i != 0`` after
    DictReader has already consumed the header, dataset_test.py:98-99)."""
    if task not in ('classification', 'regression'):
        raise ValueError('task must be either regression or classification')
    smiles_data, labels = [], []
    with open(data_path) as csv_file:
        for i, row in enumerate(csv.DictReader(csv_file, delimiter=',')):
            if i == 0:
                continue
            smiles, label = row['smiles'], row[target]
            if label == '' or label is None or not _parses(smiles):
                continue
            smiles_data.append(smiles)
            labels.append(int(label) if task == 'classification' else float(label))
    return smiles_data, labels


class MolTestDataset(torch.utils.data.Dataset):
    """dataset_test.py:114-169: ``Data(x, y [1, 1], edge_index, edge_attr)``
    with ``mol_index``; y long (classification) or float (regression, times
    the qm9 Hartree -> eV conversion for its energy targets)."""

    def __init__(self, data_path, target, task):
        super().__init__()
        self.smiles_data, self.labels = read_smiles(data_path, target, task)
        self.task = task
        self.conversion = 1
        if 'qm9' in data_path and target in ['homo', 'lumo', 'gap', 'zpve', 'u0']:
            self.conversion = HARTREE_TO_EV

    def __getitem__(self, index):
        mol = msmiles.featurise(self.smiles_data[index], add_hs=True)
        if self.task == 'classification':
            y = torch.tensor(self.labels[index], dtype=torch.long).view(1, -1)
        else:
            y = torch.tensor(self.labels[index] * self.conversion, dtype=torch.float).view(1, -1)
        data = Data(x=torch.from_numpy(mol.x), y=y, edge_index=torch.from_numpy(mol.edge_index),
                    edge_attr=torch.from_numpy(mol.edge_attr))
        data.mol_index = index
        return data

    def __len__(self):
        return len(self.smiles_data)


def collate_labelled(data_list) -> Batch:
    """Batch.from_data_list plus the labels: ``y`` [B, 1] and ``mol_index`` [B]
    (PyG's collate concatenates every tensor attribute)."""
    data_list = list(data_list)
    b = Batch.from_data_list(data_list)
    b.y = torch.cat([d.y for d in data_list], 0)
    b.mol_index = torch.tensor([int(getattr(d, 'mol_index', -1)) for d in data_list],
                               dtype=torch.long)
    return b


class MolTestDatasetWrapper(object):
    """dataset_test.py:172-226."""

    def __init__(self, batch_size, num_workers, valid_size, test_size, task, data_path, target,
                 splitting, seed=None):
        self.data_path = data_path
        self.batch_size = batch_size
        self.num_workers = num_workers
        self.valid_size = valid_size
        self.test_size = test_size
        self.target = target
        self.task = task
        self.splitting = splitting
        self.seed = seed
        assert splitting in ['random', 'scaffold']

    def get_data_loaders(self):
        dataset = MolTestDataset(data_path=self.data_path, target=self.target, task=self.task)
        train_loader, valid_loader, test_loader = self.get_train_validation_data_loaders(dataset)
        return dataset.smiles_data, train_loader, valid_loader, test_loader

    def split_indices(self, num):
        """(train, valid, test) index lists: disjoint, together range(num)."""
        if self.splitting == 'scaffold':
            raise NotImplementedError(
                "splitting: scaffold needs RDKit's Murcko scaffolds (MurckoScaffoldSmiles), which "
                "molclr_amd does not reimplement; use splitting: random")
        indices = list(range(num))
        rng = np.random if self.seed is None else np.random.RandomState(self.seed)
        rng.shuffle(indices)
        split = int(np.floor(self.valid_size * num))
        split2 = int(np.floor(self.test_size * num))
        return indices[split + split2:], indices[:split], indices[split:split + split2]

    def get_train_validation_data_loaders(self, dataset):
        train_idx, valid_idx, test_idx = self.split_indices(len(dataset))

        def loader(idx):
            return torch.utils.data.DataLoader(
                dataset, batch_size=self.batch_size, sampler=SubsetRandomSampler(idx),
                num_workers=self.num_workers, drop_last=False, collate_fn=collate_labelled)

        return loader(train_idx), loader(valid_idx), loader(test_idx)
