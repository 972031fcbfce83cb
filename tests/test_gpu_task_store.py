"""Labelled molecules resident in HBM (molclr_amd.task_store) against the
host path they replace.  Every integer field is compared with ``torch.equal``
to the project's own host code: ``collate_labelled`` for the eager collate,
``StagedTaskGraph.stage_task`` for the captured steps' buffers,
``motifs.motif_batch`` + ``stage_items`` for the motif model's items; the
captured step and evaluation pass by ids are compared bit for bit with the
same objects fed host-collated batches.

Shapes: the 50 molecules of tests/data/smiles_small.txt (with hydrogens, 16
to about 60 atoms) for batches up to 33; for 257 and 1025 molecules a
synthetic store of 1-3 atom molecules, lone atoms, one chain of 300 atoms and
one ring of 600 (larger than any block).  Models: 2 layers, emb_dim 64,
feat_dim 128, batches of 8.
"""
import copy
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from molclr_amd import _lib, smiles
from molclr_amd.data import Data
from molclr_amd.dataset_test import MolTestDataset, collate_labelled
from molclr_amd.finetune_step import (CapturedEval, CapturedFinetuneStep, StagedMotifGraph,
                                      StagedTaskGraph)
from molclr_amd.motifs import motif_batch
from molclr_amd.optim import FusedAdam
from molclr_amd.task_store import DeviceTaskLoader, DeviceTaskStore

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SMILES = [l.strip() for l in (ROOT / "tests" / "data" / "smiles_small.txt").read_text().splitlines()
          if l.strip()]
CANARY = -0x5A5A5A5A5A5A5A5B
TAIL = 64
VOCAB = 50


# ---------------------------------------------------------------------------
# molecules, labels and the host reference
# ---------------------------------------------------------------------------
def mol_of(x, bonds):
    """A molecule of atoms ``x`` [n, 2] and bonds [(s, e, type, dir)]: every
    bond as the directed pair (s, e), (e, s), as dataset_test.py builds them."""
    row, col, attr = [], [], []
    for s, e, t, d in bonds:
        row += [s, e]
        col += [e, s]
        attr += [[t, d], [t, d]]
    return SimpleNamespace(x=np.asarray(x, np.int64).reshape(-1, 2),
                           edge_index=np.asarray([row, col], np.int64).reshape(2, -1),
                           edge_attr=np.asarray(attr, np.int64).reshape(-1, 2))


def chain(n, rng, ring=False):
    x = np.stack([rng.integers(0, 119, n), rng.integers(0, 3, n)], 1)
    bonds = [(i, i + 1, int(rng.integers(0, 4)), int(rng.integers(0, 3))) for i in range(n - 1)]
    if ring:
        bonds.append((n - 1, 0, 1, 0))
    return mol_of(x, bonds)


def labels_of(kind, G, rng):
    if kind == "int64":
        return torch.from_numpy(rng.integers(0, 2, G))
    C = 1 if kind == "fp32x1" else 3
    return torch.from_numpy(rng.normal(size=(G, C)).astype(np.float32))


class HostSet:
    """MolTestDataset.__getitem__ over molecules already featurised: the Data
    ``collate_labelled`` takes (y [1, C], mol_index)."""

    def __init__(self, mols, y):
        self.mols, self.y = mols, y

    def __getitem__(self, i):
        m = self.mols[i]
        d = Data(x=torch.from_numpy(m.x), y=self.y[i].view(1, -1),
                 edge_index=torch.from_numpy(m.edge_index), edge_attr=torch.from_numpy(m.edge_attr))
        d.mol_index = int(i)
        return d


_CACHE = {}


def smiles_mols():
    if "smiles" not in _CACHE:
        _CACHE["smiles"] = [smiles.featurise(s, add_hs=True) for s in SMILES]
    return _CACHE["smiles"]


def synthetic_mols():
    """Ids 0-39: 1-3 atom chains; 40-43: lone atoms; 44: a chain of 300 atoms
    and 299 bonds; 45: a ring of 600 atoms."""
    if "synthetic" not in _CACHE:
        rng = np.random.default_rng(11)
        mols = [chain(int(rng.integers(1, 4)), rng) for _ in range(40)]
        mols += [chain(1, rng) for _ in range(4)]
        mols += [chain(300, rng), chain(600, rng, ring=True)]
        assert mols[44].edge_index.shape[1] == 2 * 299 and mols[45].edge_index.shape[1] == 1200
        _CACHE["synthetic"] = mols
    return _CACHE["synthetic"]


def pair(name, kind, dev):
    """(host set, device store) of one molecule pool and label kind, made once."""
    key = (name, kind)
    if key not in _CACHE:
        mols = smiles_mols() if name == "smiles" else synthetic_mols()
        y = labels_of(kind, len(mols), np.random.default_rng(5))
        _CACHE[key] = (HostSet(mols, y), DeviceTaskStore.from_molecules(mols, y, dev))
    return _CACHE[key]


def reference(host, ids, dev):
    return collate_labelled([host[int(i)] for i in ids]).to(dev)


def assert_same_batch(got, ref):
    for f in ("x", "edge_index", "edge_attr", "batch", "ptr", "y", "mol_index"):
        a, b = getattr(got, f), getattr(ref, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (f, a.dtype, b.dtype, a.shape, b.shape)
        assert torch.equal(a, b), f
    assert got.num_graphs == ref.num_graphs
    assert int(got.status.item()) == 0


# ---------------------------------------------------------------------------
# collate against the host collate
# ---------------------------------------------------------------------------
def ids_cases():
    rng = np.random.default_rng(3)
    cases = {
        "one": ("smiles", [7]),
        "two": ("smiles", [49, 0]),
        "descending": ("smiles", list(range(32, -1, -1))),          # 33 molecules
        "repeated": ("smiles", [4, 4, 9, 4, 31, 9, 9]),
        "lone_first_middle_last": ("synthetic", [40, 3, 7, 41, 12, 42]),
        "no_edges": ("synthetic", [40, 41, 42, 43, 40]),            # E = 0
        "one_lone_atom": ("synthetic", [43]),
        "large": ("synthetic", [2, 44, 40, 45, 5]),                 # 300-chain, 600-ring
        "b257": ("synthetic", rng.integers(0, 44, 257).tolist()),
        "b1025": ("synthetic", rng.integers(0, 44, 1025).tolist()),
        "b1025_large_last": ("synthetic", rng.integers(0, 44, 1023).tolist() + [45, 44]),
    }
    return cases


CASES = ids_cases()


@pytest.mark.parametrize("kind", ["int64", "fp32x1", "fp32x3"])
@pytest.mark.parametrize("case", list(CASES))
def test_collate_is_the_host_collate(dev, case, kind):
    name, ids = CASES[case]
    host, store = pair(name, kind, dev)
    ref = reference(host, ids, dev)
    got = store.collate(ids)
    assert_same_batch(got, ref)
    # ids already on the device, sized by their host copy
    ids_h = np.asarray(ids, np.int64)
    got = store.collate(torch.from_numpy(ids_h).to(dev), ids_h, check=True)
    assert_same_batch(got, ref)
    assert store.sizes(ids_h) == (int(ref.x.shape[0]), int(ref.edge_index.shape[1]))
    if case == "no_edges":
        assert ref.edge_index.shape[1] == 0


def test_from_dataset_follows_the_dataset(dev, tmp_path, monkeypatch):
    """The store of a MolTestDataset: its own label conversion and dtype rule,
    every molecule featurised once; batches equal the dataset's collate."""
    for task, sub in (("classification", "plain"), ("regression", "qm9")):
        d = tmp_path / sub
        d.mkdir()
        with open(d / "data.csv", "w") as f:
            f.write("smiles,homo\nC,0\n")
            for i, s in enumerate(SMILES[:20]):
                f.write(f"{s},{i % 2 if task == 'classification' else -0.25 + 0.01 * i}\n")
        ds = MolTestDataset(str(d / "data.csv"), "homo", task)
        assert len(ds) == 20 and (ds.conversion != 1) == (sub == "qm9")
        calls = []
        real = smiles.featurise
        monkeypatch.setattr(smiles, "featurise", lambda *a, **k: calls.append(a[0]) or real(*a, **k))
        store = DeviceTaskStore.from_dataset(ds, dev)
        assert len(calls) == 20
        ids = [19, 3, 3, 0, 11]
        got = store.collate(ids)
        assert len(calls) == 20
        monkeypatch.setattr(smiles, "featurise", real)
        assert_same_batch(got, reference(ds, ids, dev))


# ---------------------------------------------------------------------------
# the status word; nothing is stored outside the outputs
# ---------------------------------------------------------------------------
def guarded(n, dev, dtype=torch.int64):
    """A buffer of n elements followed by a canary tail."""
    fill = CANARY if dtype == torch.int64 else -12345
    return torch.full((n + TAIL,), fill, dtype=dtype, device=dev)


def raw_collate(store, ids, N, E, dev):
    """collate_into with canary tails behind every output: (fields, status)."""
    B = len(ids)
    buf = dict(x=guarded(2 * N, dev), ei=guarded(2 * E, dev), ea=guarded(2 * E, dev),
               batch=guarded(N, dev), ptr=guarded(B + 1, dev), y=guarded(B, dev),
               status=guarded(1, dev, torch.int32))
    ids_d = torch.tensor(ids, dtype=torch.long, device=dev)
    store.collate_into(ids_d, N, E, buf["x"][:2 * N].view(N, 2), buf["ei"][:2 * E].view(2, E),
                       buf["ea"][:2 * E].view(E, 2), buf["batch"][:N], buf["ptr"][:B + 1],
                       buf["y"][:B], buf["status"][:1])
    torch.cuda.synchronize()
    sizes = dict(x=2 * N, ei=2 * E, ea=2 * E, batch=N, ptr=B + 1, y=B, status=1)
    for k, t in buf.items():
        want = CANARY if t.dtype == torch.int64 else -12345
        assert bool((t[sizes[k]:] == want).all()), f"canary behind {k} overwritten"
    out = SimpleNamespace(x=buf["x"][:2 * N].view(N, 2), edge_index=buf["ei"][:2 * E].view(2, E),
                          edge_attr=buf["ea"][:2 * E].view(E, 2), batch=buf["batch"][:N],
                          ptr=buf["ptr"][:B + 1], y=buf["y"][:B])
    return out, int(buf["status"][0].item())


def test_status_molecule_id_out_of_range(dev):
    host, store = pair("smiles", "int64", dev)
    G = store.num_molecules
    ids, valid = [5, -1, 9, G, 2], [5, 9, 2]
    ref = reference(host, valid, dev)
    N, E = int(ref.x.shape[0]), int(ref.edge_index.shape[1])
    out, st = raw_collate(store, ids, N, E, dev)
    assert st == 1
    # the refused molecules contribute nothing: the valid ones' rows, in order
    assert torch.equal(out.x, ref.x) and torch.equal(out.edge_index, ref.edge_index)
    assert torch.equal(out.edge_attr, ref.edge_attr)
    n = [int(v) for v in ref.ptr]
    assert out.ptr.tolist() == [0, n[1], n[1], n[2], n[2], n[3]]
    assert torch.equal(out.batch, torch.tensor([0, 2, 4], device=dev)[ref.batch])
    assert out.y.tolist() == [int(ref.y[0]), 0, int(ref.y[1]), 0, int(ref.y[2])]
    with pytest.raises(IndexError):
        store.collate(ids)


@pytest.mark.parametrize("dn,de", [(1, 0), (-1, 0), (0, 2), (0, -2), (-5, -4)])
def test_status_host_sizes_disagree(dev, dn, de):
    host, store = pair("smiles", "int64", dev)
    ids = [1, 8, 20]
    N, E = store.sizes(ids)
    out, st = raw_collate(store, ids, N + dn, E + de, dev)
    assert st == 2
    assert out.ptr.tolist() == reference(host, ids, dev).ptr.tolist()  # the device's own sums


def test_status_edge_index_outside_its_molecule(dev):
    rng = np.random.default_rng(2)
    mols = [chain(3, rng), chain(4, rng), chain(2, rng)]
    bad = copy.deepcopy(mols)
    bad[1].edge_index[1, 2] = 4   # one past the molecule's atoms
    bad[1].edge_index[0, 5] = -1
    y = torch.zeros(3, dtype=torch.long)
    store = DeviceTaskStore.from_molecules(bad, y, dev)
    clamped = copy.deepcopy(mols)
    clamped[1].edge_index[1, 2] = 3
    clamped[1].edge_index[0, 5] = 0
    ref = reference(HostSet(clamped, y), [2, 1, 0], dev)
    out, st = raw_collate(store, [2, 1, 0], 9, int(ref.edge_index.shape[1]), dev)
    assert st == 4
    assert torch.equal(out.edge_index, ref.edge_index) and torch.equal(out.x, ref.x)
    with pytest.raises(ValueError, match="edge index"):
        store.collate([2, 1, 0], check=True)


# ---------------------------------------------------------------------------
# staging against stage_task
# ---------------------------------------------------------------------------
def staged_fields(g, N, E):
    return dict(counts=g.counts, target=g.target, x=g.x[:N], ei=g.st_ei[0][:, :E],
                ea=g.st_ea[0][:E], batch=g.st_batch[0][:N])


def assert_same_staging(a, b, N, E):
    torch.cuda.synchronize()
    assert a.counts.tolist() == [N, E]
    fa, fb = staged_fields(a, N, E), staged_fields(b, N, E)
    for k in fa:
        assert torch.equal(fa[k], fb[k]), k
    assert int(a.x[N:].abs().sum()) == 0 and int(b.x[N:].abs().sum()) == 0
    assert int(a.ids_status.item()) == 0


@pytest.mark.parametrize("kind", ["int64", "fp32x1", "fp32x3"])
def test_staging_is_stage_task(dev, kind):
    host, store = pair("smiles", kind, dev)
    labels, cols = kind == "int64", 3 if kind == "fp32x3" else 1
    big, small = [8, 2, 30, 12, 8], [7, 3, 5, 3, 45]
    N, E = store.sizes(big)
    Ns, Es = store.sizes(small)
    assert Ns < N and Es < E
    # capacity exactly N / E
    a, b = (StagedTaskGraph(dev, N, E, 5, labels, cols) for _ in range(2))
    ids_h = np.asarray(big, np.int64)
    a.stage_task_ids(store, torch.from_numpy(ids_h).to(dev), ids_h)
    b.stage_task(reference(host, big, dev))
    assert_same_staging(a, b, N, E)
    # capacity with padding: a large batch, then a smaller one into the same graphs
    a, b = (StagedTaskGraph(dev, N + 37, E + 101, 5, labels, cols) for _ in range(2))
    for ids in (big, small):
        ids_h = np.asarray(ids, np.int64)
        a.stage_task_ids(store, torch.from_numpy(ids_h).to(dev), ids_h)
        b.stage_task(reference(host, ids, dev))
        assert_same_staging(a, b, *store.sizes(ids))


def test_staging_refuses_what_the_capacities_do_not_hold(dev):
    host, store = pair("smiles", "int64", dev)
    ids = [8, 2, 30]
    ids_h = np.asarray(ids, np.int64)
    ids_d = torch.from_numpy(ids_h).to(dev)
    N, E = store.sizes(ids)
    for ncap, ecap, what in ((N - 1, E, "nodes"), (N, E - 2, "edges")):
        a, b = (StagedTaskGraph(dev, ncap, ecap, 3, True, 1) for _ in range(2))
        with pytest.raises(_lib.MolclrError, match=f"status -1.*{what}") as by_ids:
            a.stage_task_ids(store, ids_d, ids_h)
        with pytest.raises(_lib.MolclrError, match=f"status -1.*{what}") as by_batch:
            b.stage_task(reference(host, ids, dev))
        # the same refusal, word for word after the entry point's name
        assert str(by_ids.value).split(":", 2)[2] == str(by_batch.value).split(":", 2)[2]
        torch.cuda.synchronize()
        for t in (a.x, a.counts, a.target, a.st_ei[0], a.st_ea[0], a.st_batch[0]):
            assert int(t.abs().sum()) == 0  # no launch happened
    g = StagedTaskGraph(dev, N, E, 4, True, 1)
    with pytest.raises(ValueError, match="built for 4"):
        g.stage_task_ids(store, ids_d, ids_h)
    _, floats = pair("smiles", "fp32x3", dev)
    with pytest.raises(ValueError, match="targets"):
        StagedTaskGraph(dev, N, E, 3, True, 1).stage_task_ids(floats, ids_d, ids_h)


def test_staging_flags_sizes_the_device_does_not_confirm(dev):
    _, store = pair("smiles", "int64", dev)
    ids_h = np.asarray([8, 2, 30], np.int64)
    N, E = store.sizes(ids_h)
    g = StagedTaskGraph(dev, N + 8, E + 8, 3, True, 1)
    g.stage_task_ids(store, torch.from_numpy(ids_h).to(dev), ids_h, sizes=(N - 3, E))
    torch.cuda.synchronize()
    assert int(g.ids_status.item()) == 2 and g.counts.tolist() == [0, 0]


# ---------------------------------------------------------------------------
# motif items
# ---------------------------------------------------------------------------
def assignments_of(G):
    """Molecules without motifs (every fifth), ids repeated across molecules
    (a vocabulary of 6 over up to 5 items each), distinct within one."""
    rng = np.random.default_rng(9)
    return [[] if i % 5 == 0 else rng.choice(6, int(rng.integers(1, 6)), replace=False).tolist()
            for i in range(G)]


def motif_store(dev):
    if "motif" not in _CACHE:
        mols = smiles_mols()
        store = DeviceTaskStore.from_molecules(mols, torch.zeros(len(mols), dtype=torch.long), dev)
        assign = assignments_of(len(mols))
        store.set_motifs(assign)
        _CACHE["motif"] = (store, assign)
    return _CACHE["motif"]


MOTIF_IDS = {
    "mixed": [3, 0, 7, 7, 12, 5, 44],       # molecules 0 and 5 have no motifs
    "none_at_all": [0, 5, 10, 45],          # T = 0
    "one_molecule": [13],
    "zero_first_and_last": [10, 1, 2, 3, 20],
    "b33": list(range(33)),
}


@pytest.mark.parametrize("case", list(MOTIF_IDS))
def test_motif_items_are_motif_batch(dev, case):
    store, assign = motif_store(dev)
    ids = MOTIF_IDS[case]
    mol_ref, clique_ref = motif_batch(np.asarray(ids), assign, dev)
    mol, clique = store.motif_items(ids, check=True)
    assert torch.equal(mol, mol_ref) and torch.equal(clique, clique_ref)
    ids_h = np.asarray(ids, np.int64)
    mol, clique = store.motif_items(torch.from_numpy(ids_h).to(dev), ids_h)
    assert torch.equal(mol, mol_ref) and torch.equal(clique, clique_ref)
    assert store.sizes(ids_h)[2] == clique_ref.shape[0]
    if case == "none_at_all":
        assert clique_ref.shape[0] == 0


def motif_graph_fields(g):
    return dict(clique=g.clique, mol_ptr=g.mol_ptr, sorted_idx=g.sorted_idx, order=g.order,
                item_status=g.item_status)


@pytest.mark.parametrize("case,slack", [("mixed", 9), ("mixed", 0), ("mixed", -1),
                                        ("none_at_all", 4), ("zero_first_and_last", 300),
                                        ("b33", 0), ("b33", 200)])
def test_staged_items_are_stage_items(dev, case, slack):
    """slack 0: T == item_cap; slack -1: T = item_cap + 1, the overflow bit."""
    store, assign = motif_store(dev)
    ids = MOTIF_IDS[case]
    ids_h = np.asarray(ids, np.int64)
    B, T = len(ids), store.sizes(ids_h)[2]
    cap = T + slack
    a, b = (StagedMotifGraph(dev, 64, 64, B, True, 1, cap) for _ in range(2))
    a.stage_items_ids(store, torch.from_numpy(ids_h).to(dev), ids_h)
    mol, clique = motif_batch(ids_h, assign, dev)
    if slack >= 0:
        b.stage_items(mol, clique)
    else:  # stage_items refuses on the host; the launch it would make refuses on the device
        _lib.call("molclr_stage_motif", mol.data_ptr(), clique.data_ptr(), T, B, cap,
                  b.clique.data_ptr(), b.mol_ptr.data_ptr(), b.sorted_idx.data_ptr(),
                  b.order.data_ptr(), b.item_status.data_ptr(), _lib.stream_of(dev))
    torch.cuda.synchronize()
    fa, fb = motif_graph_fields(a), motif_graph_fields(b)
    for k in fa:
        assert torch.equal(fa[k], fb[k]), k
    want = _lib.STATUS_ITEM_OVERFLOW if slack < 0 else 0
    assert int(a.item_status.item()) == want
    if slack >= 0:
        assert int(a.mol_ptr[B]) == T


# ---------------------------------------------------------------------------
# the captured step and evaluation pass by ids
# ---------------------------------------------------------------------------
def model_of(kind, seed):
    from molclr_amd.gcn_finetune import GCN
    from molclr_amd.ginet_finetune import GINet
    from molclr_amd.ginet_finetune_mp import GINet as MotifGINet
    torch.manual_seed(seed)
    if kind == "gcn":
        return GCN("regression", 2, 64, 128, 0.0), "mse", "fp32x1"
    if kind == "motif":
        return MotifGINet(VOCAB, "classification", 2, 64, 128, 0.0), "cross_entropy", "int64"
    precision = "bf16" if kind == "bf16" else "fp32"
    return GINet("classification", 2, 64, 128, 0.0, precision=precision), "cross_entropy", "int64"


def optimizers_of(model):
    head = [p for n, p in model.named_parameters() if "pred_lin" in n]
    base = [p for n, p in model.named_parameters() if "pred_lin" not in n]
    opts = [FusedAdam(base, 5e-4, weight_decay=1e-5)]
    if head:
        opts.append(FusedAdam(head, 2e-3, weight_decay=1e-5))
    return opts


def step_store(kind, label_kind, dev):
    """(host set, store, assignments or None): the SMILES pool; the motif
    model's store carries assignments over its vocabulary."""
    host, store = pair("smiles", label_kind, dev)
    if kind != "motif":
        return host, store, None
    if "motif_step" not in _CACHE:
        rng = np.random.default_rng(4)
        assign = [rng.choice(VOCAB, int(rng.integers(0, 7)), replace=False).tolist()
                  for _ in range(store.num_molecules)]
        mstore = DeviceTaskStore.from_molecules(host.mols, host.y, dev)
        mstore.set_motifs(assign)
        _CACHE["motif_step"] = (mstore, assign)
    return (host,) + _CACHE["motif_step"]


@pytest.mark.parametrize("kind", ["gin", "gcn", "motif", "bf16"])
def test_step_ids_is_step(dev, kind):
    """Two identically seeded models and optimizers, three steps of batch 8:
    ``step(host-collated batch)`` and ``step_ids`` on the same ids give equal
    losses and parameters."""
    model_a, crit, label_kind = model_of(kind, 6)
    host, store, assign = step_store(kind, label_kind, dev)
    model_a = model_a.to(dev)
    model_b = copy.deepcopy(model_a)
    opts_a, opts_b = optimizers_of(model_a), optimizers_of(model_b)
    q = dict(node_quantum=128, edge_quantum=512, item_quantum=64)
    step_a = CapturedFinetuneStep(model_a, opts_a, crit, **q)
    step_b = CapturedFinetuneStep(model_b, opts_b, crit, **q)
    rng = np.random.default_rng(21)
    for i in range(3):
        ids_h = rng.integers(0, store.num_molecules, 8).astype(np.int64)
        data = reference(host, ids_h, dev)
        items = motif_batch(ids_h, assign, dev) if kind == "motif" else ()
        loss_a = step_a.step(data, *items).clone()
        loss_b = step_b.step_ids(store, torch.from_numpy(ids_h).to(dev), ids_h).clone()
        torch.cuda.synchronize()
        print(f"{kind} step {i}: loss {loss_a.item():.9g} by ids {loss_b.item():.9g}")
        assert torch.isfinite(loss_a) and torch.equal(loss_a, loss_b), i
        assert step_a.buckets == step_b.buckets
        for (n, pa), pb in zip(model_a.named_parameters(), model_b.parameters()):
            assert torch.equal(pa, pb), (i, n)
    step_a.check()
    step_b.check()
    assert step_b.replays == 3
    step_a.close()
    step_b.close()


@pytest.mark.parametrize("kind", ["gin", "motif"])
def test_eval_by_ids_is_eval(dev, kind):
    """CapturedEval over a DeviceTaskLoader against the same pass over the
    host-collated batches in the same order, a partial last batch included."""
    model, crit, label_kind = model_of(kind, 2)
    host, store, assign = step_store(kind, label_kind, dev)
    model = model.to(dev)
    idx = [int(i) for i in np.random.default_rng(8).permutation(store.num_molecules)[:19]]
    loader = DeviceTaskLoader(store, idx, 8, shuffle=False)
    assert len(loader) == 3
    batches = [collate_labelled([host[i] for i in idx[k:k + 8]]) for k in range(0, 19, 8)]
    assert batches[-1].num_graphs == 3
    q = dict(node_quantum=128, edge_quantum=512, item_quantum=64)
    ev_a, ev_b = CapturedEval(model, crit, **q), CapturedEval(model, crit, **q)
    motif = (lambda d: motif_batch(d.mol_index, assign, dev)) if kind == "motif" else None
    loss_a, pred_a, lab_a = ev_a.run(batches, motif)
    loss_b, pred_b, lab_b = ev_b.run(loader)
    print(f"{kind}: mean loss {loss_a!r} by ids {loss_b!r}")
    assert pred_a.shape == (19, 2) and np.isfinite(loss_a)
    assert loss_a == loss_b and np.array_equal(pred_a, pred_b) and np.array_equal(lab_a, lab_b)
    assert lab_b.tolist() == [int(host.y[i]) for i in idx]
    assert ev_a.buckets == ev_b.buckets
    ev_b.check()
    ev_a.close()
    ev_b.close()


# ---------------------------------------------------------------------------
# the trainer: featurise once
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("hip_graph", [False, True])
def test_trainer_featurises_once(dev, tmp_path, monkeypatch, hip_graph):
    from molclr_amd.dataset_test import MolTestDatasetWrapper
    from molclr_amd.finetune import FineTune

    from .test_gpu_finetune import config_of
    with open(tmp_path / "data.csv", "w") as f:
        f.write("smiles,label\nC,0\n")
        for i, s in enumerate(SMILES[:40]):
            f.write(f"{s},{i % 2}\n")
    cfg = config_of(tmp_path, "classification", "gin", device_data=True, hip_graph=hip_graph,
                    batch_size=8, epochs=2)
    cfg["dataset"].update(valid_size=0.25, test_size=0.25)
    calls, built = [0], []
    real = smiles.featurise

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    monkeypatch.setattr(smiles, "featurise", counted)
    wrapper = MolTestDatasetWrapper(cfg["batch_size"], **cfg["dataset"])
    from molclr_amd import task_store
    loaders = task_store.device_loaders

    def device_loaders(w, device):
        out = loaders(w, device)
        built.append(calls[0])
        return out

    monkeypatch.setattr(task_store, "device_loaders", device_loaders)
    ft = FineTune(wrapper, cfg)
    ft.train()
    # read_smiles' parse check and the store's one pass; nothing after
    assert built == [2 * 40] and calls[0] == built[0]
    assert len(ft.epoch_train_loss) == 2 and all(np.isfinite(v) for v in ft.epoch_train_loss)
    assert np.isfinite(ft.roc_auc)
    ft.check_inputs()
    assert ft.hip_graph is hip_graph
    if hip_graph:
        step, ev = ft._captured[2], ft._captured[3]
        assert step.replays == 2 * 3 and ev.replays >= 2 * 2  # 20 / 8 and 10 / 8 batches
