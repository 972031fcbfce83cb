"""molclr_amd.retrieval on the device: embed_store against the fp64 oracle's
eval-mode embedding of every molecule ALONE, the index built from it end to
end, and the command line."""
import copy
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from molclr_amd import smiles
from molclr_amd.data import Batch, Data
from oracle.reference_cpu import RefGCN, RefGINet

from .test_gpu_models import TOL, rel

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SMILES_FILE = ROOT / "tests" / "data" / "smiles_small.txt"
SMILES = [l.strip() for l in SMILES_FILE.read_text().splitlines() if l.strip()]
DUP = (3, 40)  # molecule 40 of the store is molecule 3 again
ARGS = dict(num_layer=2, emb_dim=44, feat_dim=40)
_CACHE = {}


def mols():
    if "mols" not in _CACHE:
        m = [smiles.featurise(s) for s in SMILES[:40]]
        _CACHE["mols"] = m + [m[DUP[0]]]
    return _CACHE["mols"]


def seeded_ref(cls):
    """The oracle with seeded weights and non-trivial running statistics."""
    torch.manual_seed(7)
    ref = cls(**ARGS)
    g = torch.Generator().manual_seed(11)
    for bn in ref.batch_norms:
        bn.running_mean.copy_(torch.randn(bn.num_features, generator=g) * 0.5)
        bn.running_var.copy_(torch.rand(bn.num_features, generator=g) * 1.5 + 0.5)
    return ref


def oracle_rows(ref):
    """(h, out) [G, .] fp64 of every molecule alone, eval mode; computed once
    per oracle class."""
    key = type(ref).__name__
    if key not in _CACHE:
        ref64 = copy.deepcopy(ref).double().eval()
        hs, outs = [], []
        with torch.no_grad():
            for m in mols():
                b = Batch.from_data_list([Data(x=torch.from_numpy(m.x),
                                               edge_index=torch.from_numpy(m.edge_index),
                                               edge_attr=torch.from_numpy(m.edge_attr))])
                h, out = ref64(b)
                hs.append(h)
                outs.append(out)
        _CACHE[key] = (torch.cat(hs), torch.cat(outs))
    return _CACHE[key]


def store_of(dev):
    from molclr_amd.augment import DeviceMoleculeStore
    return DeviceMoleculeStore.from_molecules(mols(), dev)


def models(kind):
    from molclr_amd import gcn_molclr, ginet_molclr
    ref = seeded_ref({"gin": RefGINet, "gcn": RefGCN}[kind])
    mine = {"gin": ginet_molclr.GINet, "gcn": gcn_molclr.GCN}[kind](**ARGS)
    mine.load_state_dict(ref.state_dict())
    return ref, mine


@pytest.mark.parametrize("kind", ["gin", "gcn"])
def test_embed_store_against_the_oracle(dev, kind):
    from molclr_amd.retrieval import embed_store
    ref, mine = models(kind)
    mine = mine.to(dev)
    h64, out64 = oracle_rows(ref)
    store = store_of(dev)
    for training in (True, False):
        mine.train(training)
        for bs in (7, 64):
            h = embed_store(mine, store, batch_size=bs, normalize=False)
            assert h.shape == h64.shape and h.dtype == torch.float32
            print(f"{kind} batch_size {bs}: rel {rel(h, h64):.3e}")
            assert rel(h, h64) <= TOL
            assert mine.training == training and all(bn.training == training
                                                     for bn in mine.batch_norms)
    out = embed_store(mine, store, batch_size=7, which='out', normalize=False)
    assert rel(out, out64) <= TOL
    # the statistics the oracle was given are still there: nothing trained
    for bn, rbn in zip(mine.batch_norms, ref.batch_norms):
        assert torch.equal(bn.running_mean.cpu(), rbn.running_mean)
    hn = embed_store(mine, store, batch_size=64)
    assert (hn.double().norm(dim=1) - 1).abs().max().item() <= 1e-6
    assert rel(hn, h64 / h64.norm(dim=1, keepdim=True)) <= TOL
    # bf16: the fp32 result rounded once, to nearest even
    for norm in (False, True):
        e32 = embed_store(mine, store, batch_size=64, normalize=norm)
        e16 = embed_store(mine, store, batch_size=64, normalize=norm, dtype=torch.bfloat16)
        assert e16.dtype == torch.bfloat16 and torch.equal(e16, e32.to(torch.bfloat16))
    # the model's mode comes back when a batch raises, too
    mine.train(True)
    with pytest.raises(ValueError):
        embed_store(mine, store, which='nope')
    with pytest.raises(TypeError):
        embed_store(mine, object())
    assert mine.training


def test_embed_store_finetune_models(dev):
    """The fine-tuning GIN's h against the plain oracle that shares its encoder
    and feat_lin (strict=False: the oracle keeps its own out_lin); the motif
    model is refused."""
    from molclr_amd import ginet_finetune, ginet_finetune_mp
    from molclr_amd.retrieval import embed_store
    from molclr_amd.task_store import DeviceTaskStore
    ref = seeded_ref(RefGINet)
    torch.manual_seed(3)
    mine = ginet_finetune.GINet('classification', **ARGS)
    mine.load_my_state_dict(ref.state_dict())
    mine = mine.to(dev)
    store = DeviceTaskStore.from_molecules(mols(), torch.zeros(len(mols()), dtype=torch.long), dev)
    h = embed_store(mine, store, batch_size=7, normalize=False)
    assert rel(h, oracle_rows(ref)[0]) <= TOL
    pred = embed_store(mine, store, batch_size=64, which='out', normalize=False)
    assert pred.shape == (len(mols()), 2)
    motif = ginet_finetune_mp.GINet(5, 'classification', **ARGS)
    with pytest.raises(NotImplementedError, match="motif"):
        embed_store(motif, store)


def test_index_end_to_end(dev):
    from molclr_amd.retrieval import MoleculeIndex, embed_store
    ref, mine = models("gin")
    emb = embed_store(mine.to(dev), store_of(dev), batch_size=64)
    G, C = emb.shape
    index = MoleculeIndex(emb)
    ids = torch.arange(G)
    s, i = index.search_ids(ids, k=5, exclude_self=False)
    s, i = s.cpu(), i.cpu()
    # every molecule is its own best hit; of the two copies the lower id wins
    want = ids.clone()
    want[DUP[1]] = DUP[0]
    assert torch.equal(i[:, 0], want)
    assert (s[:, 0] - 1).abs().max().item() <= 1e-6
    assert i[DUP[0], 1] == DUP[1] and i[DUP[1], 1] == DUP[1]
    assert (s[[DUP[0], DUP[1]], 1] - 1).abs().max().item() <= 1e-6
    # exclude_self: no row holds its own id
    s, i = index.search_ids(ids, k=5, exclude_self=True)
    s, i = s.cpu().double(), i.cpu()
    assert not (i == ids[:, None]).any() and ((i >= 0) & (i < G)).all()
    # completeness against the fp64 cosine similarities of the oracle embeddings
    h64 = oracle_rows(ref)[0]
    u = h64 / h64.norm(dim=1, keepdim=True)
    s64 = u @ u.t()
    tol = 2 * C * 2.0 ** -24 + 2e-5
    for r in range(G):
        rest = torch.ones(G, dtype=torch.bool)
        rest[i[r]] = False
        rest[r] = False
        assert (s[r] - s64[r, i[r]]).abs().max().item() <= tol
        assert s64[r, rest].max().item() <= s64[r, i[r, -1]].item() + 2 * tol, r
    # queries from outside, cosine by default: a scaled row finds its own molecule
    s, i = index.search(emb[:4].float() * 3.0, k=1)
    assert i.cpu().flatten().tolist() == [0, 1, 2, 3] and (s.cpu() - 1).abs().max() <= 1e-6
    s, i = index.search(emb[:4].float() * 3.0, k=1, metric='dot')
    assert (s.cpu() - 3).abs().max() <= 1e-5
    # a bf16 library: the best row by the fp64 scores of the rounded rows (its
    # rows are no longer unit vectors, so a molecule need not be its own hit)
    e16 = emb.to(torch.bfloat16)
    s16, i16 = MoleculeIndex(e16).search(emb, k=1, metric='dot')
    t64 = emb.double().cpu() @ e16.double().cpu().t()
    best = t64.max(dim=1).values
    tol = 2 * C * 2.0 ** -24
    assert (s16.cpu().double()[:, 0] - t64.gather(1, i16.cpu())[:, 0]).abs().max().item() <= tol
    assert (best - t64.gather(1, i16.cpu())[:, 0]).max().item() <= 2 * tol


def test_command_line(dev, tmp_path):
    """Three queries (one of them refused by the featuriser is a fourth line)
    against the small library: 3 k well-formed lines."""
    import yaml
    k = 4
    config = {"model_type": "gin", "model": dict(ARGS, drop_ratio=0, pool="mean")}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(config))
    from molclr_amd import ginet_molclr
    torch.manual_seed(0)
    torch.save(ginet_molclr.GINet(**config["model"]).state_dict(), tmp_path / "model.pth")
    (tmp_path / "query.txt").write_text("\n".join([SMILES[5], "not a molecule", SMILES[0],
                                                   SMILES[17]]) + "\n")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m",
                        "molclr_amd.retrieval", "--config", str(tmp_path / "config.yaml"),
                        "--checkpoint", str(tmp_path / "model.pth"), "--library",
                        str(SMILES_FILE), "--query", str(tmp_path / "query.txt"), "-k", str(k)],
                       cwd=str(ROOT), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "skipped 'not a molecule'" in r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3 * k, r.stdout
    rows = [l.split() for l in lines]
    assert [int(a) for a, _, _ in rows] == [0] * k + [1] * k + [2] * k
    assert all(0 <= int(b) < len(SMILES) for _, b, _ in rows)
    sc = np.array([float(c) for _, _, c in rows]).reshape(3, k)
    assert (np.diff(sc, axis=1) <= 0).all() and np.abs(sc[:, 0] - 1).max() <= 1e-5
    # each query is a library molecule: it is its own first hit
    assert [int(rows[j * k][1]) for j in range(3)] == [5, 0, 17]
