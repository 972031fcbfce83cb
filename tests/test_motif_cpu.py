"""The motif model's pieces that need no GPU: parameter layout and seeded
initialisation against the reference's creation order (tests/motif_ref.py),
load_my_state_dict, the built-in fragmenter on hand-derived cases, the JSON
source and the batch index tensors."""
import itertools
import json

import pytest
import torch

from molclr_amd import ginet_finetune_mp, ginet_molclr, motifs

from .motif_ref import MotifGINetLayout, reference_motif_batch


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("task,n_layer,act", list(itertools.product(
    ("classification", "regression"), (1, 2, 3), ("softplus", "relu"))))
def test_state_dict_matches_reference_layout(task, n_layer, act):
    kw = dict(num_layer=2, emb_dim=12, feat_dim=10, pred_n_layer=n_layer, pred_act=act)
    ours = ginet_finetune_mp.GINet(7, task, drop_ratio=0.1, pool='add', **kw)
    ref = MotifGINetLayout(7, task, **kw)
    assert list(ours.state_dict()) == list(ref.state_dict())
    assert _shapes(ours) == _shapes(ref)
    keys = list(ours.state_dict())
    assert keys.index("x_embedding2.weight") + 1 == keys.index("motif_embedding.weight")
    assert keys.index("feat_lin.bias") + 1 == keys.index("motif_lin.weight")
    assert keys.index("motif_lin.bias") + 1 == keys.index("motif_pool.gate_nn.0.weight")
    assert ours.state_dict()["pred_head.0.weight"].shape == (5, 20)
    assert not any(k.startswith("out_lin") for k in keys)


@pytest.mark.parametrize("task", ("classification", "regression"))
def test_seeded_build_equals_the_reference_order(task):
    """Tensor for tensor, the gate Linear's second draw included."""
    kw = dict(num_layer=2, emb_dim=12, feat_dim=10, pred_n_layer=2, pred_act="softplus")
    torch.manual_seed(3)
    ours = ginet_finetune_mp.GINet(9, task, **kw).state_dict()
    torch.manual_seed(3)
    ref = MotifGINetLayout(9, task, **kw).state_dict()
    for k in ref:
        assert torch.equal(ours[k], ref[k]), k
    assert ours["motif_pool.gate_nn.0.weight"].shape == (1, 10)
    # the second draw matters: undoing it in the product gives other parameters
    torch.manual_seed(3)
    from unittest import mock
    with mock.patch.object(ginet_finetune_mp.GlobalAttention, "reset_parameters", lambda self: None):
        once = ginet_finetune_mp.GINet(9, task, **kw).state_dict()
    assert not torch.equal(once["motif_pool.gate_nn.0.weight"], ref["motif_pool.gate_nn.0.weight"])
    assert not torch.equal(once["pred_head.0.weight"], ref["pred_head.0.weight"])


def test_constructor_errors():
    with pytest.raises(ValueError):
        ginet_finetune_mp.GINet(3, pred_act='gelu', num_layer=1, emb_dim=8, feat_dim=8)
    with pytest.raises(ValueError):
        ginet_finetune_mp.GINet(3, 'ranking', num_layer=1, emb_dim=8, feat_dim=8)


def test_load_my_state_dict_and_init_motif_emb():
    torch.manual_seed(1)
    pre = ginet_molclr.GINet(num_layer=2, emb_dim=12, feat_dim=10)
    model = ginet_finetune_mp.GINet(6, 'classification', num_layer=2, emb_dim=12, feat_dim=10)
    for bn in pre.batch_norms:
        bn.running_mean.uniform_(-1, 1)
        bn.num_batches_tracked.fill_(7)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    sd = pre.state_dict()
    model.load_my_state_dict(sd)
    after = model.state_dict()
    for k, v in after.items():
        if k.startswith(("motif_", "pred_head.")):
            assert torch.equal(v, before[k]), k  # untouched
        else:
            assert torch.equal(v, sd[k]), k
    assert not any(k.startswith("out_lin.") for k in after)
    init = torch.arange(60, dtype=torch.float32).reshape(6, 10)
    weight = model.motif_embedding.weight
    model.init_motif_emb(init)
    assert model.motif_embedding.weight is weight and torch.equal(weight.data, init)
    with pytest.raises(RuntimeError):
        model.init_motif_emb(torch.zeros(5, 10))


def test_segment_pointers_from_the_reference_layout():
    # mol_idx [T + B]: molecules 0, 0, 2 of the three items, then 0 1 2; molecule 1 has none
    model = ginet_finetune_mp.GINet(6, num_layer=1, emb_dim=8, feat_dim=8)
    assert model._mol_ptr(torch.tensor([0, 0, 2, 0, 1, 2]), 3, 3).tolist() == [0, 2, 2, 3]


# -- the built-in fragmenter -------------------------------------------------------
def test_fragmenter_hand_derived_cases():
    # toluene: the methyl carbon is cut from the ring
    assert motifs.fragment("Cc1ccccc1") == [[0], [1, 2, 3, 4, 5, 6]]
    # isobutane: the branch atom and its three neighbours, each alone
    assert motifs.fragment("CC(C)C") == [[0], [1], [2], [3]]
    assert motifs.fragment("C") == [[0]]
    # a chain on which no rule fires stays whole
    assert motifs.fragment("CCOC") == [[0, 1, 2, 3]]
    # biphenyl: the chain bond between the rings is cut
    assert motifs.fragment("c1ccccc1-c1ccccc1") == [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11]]
    # fused rings share a ring bond: one clique
    assert motifs.fragment("c1ccc2ccccc2c1") == [list(range(10))]
    # ring substituent that branches: ring | branch atom | its two other neighbours
    assert motifs.fragment("c1ccccc1C(C)O") == [[0, 1, 2, 3, 4, 5], [6], [7], [8]]


def test_motif_identity_and_vocabulary_order():
    data = ["c1ccccc1-c1ccccc1", "Cc1ccccc1", "CC(C)C", "OCC", "CCO", "NCC"]
    vocab, assign = motifs.builtin_motifs(data)
    # biphenyl: two rings, one motif id; toluene: the methyl atom first, then that ring
    assert assign[0] == [0] and assign[1] == [1, 0]
    # isobutane: branch carbon and methyl carbon are both a lone C -- the toluene methyl
    assert assign[2] == [1]
    # ethanol written from either end is one motif; the amine is another
    assert assign[3] == assign[4] == [2] and assign[5] == [3]
    assert len(vocab) == 4
    # every motif's SMILES parses back to a graph of the motif's size
    sizes = [6, 1, 3, 3]
    assert [m.graph.x.shape[0] for m in vocab] == sizes
    ring = vocab[0].graph
    assert ring.edge_index.shape == (2, 12) and (ring.edge_attr[:, 0] == 3).all()
    # deterministic: the same list gives the same names and indices
    again = motifs.builtin_motifs(data)
    assert [m.smiles for m in again[0]] == [m.smiles for m in vocab] and again[1] == assign
    # atom types and bond types tell motifs apart
    v2, a2 = motifs.builtin_motifs(["CC", "C=C", "CN", "CC"])
    assert a2 == [[0], [1], [2], [0]] and len(v2) == 3


def test_motif_smiles_keeps_chirality_and_ring_bonds():
    vocab, _ = motifs.builtin_motifs(["C[C@H](N)C(=O)O", "C1CC1=O"])
    for m in vocab:
        assert m.graph is not None, m.smiles
    # the alanine centre is a branch atom of its own and keeps its tag ('@': 2)
    assert any(m.graph.x.tolist() == [[5, 2]] for m in vocab)
    # the carboxyl carbon (three neighbours) is cut from its double-bonded oxygen too
    assert any(m.graph.x.tolist() == [[7, 0]] for m in vocab)
    # cyclopropanone: the ring closure survives the round trip, the exocyclic O is cut
    ring = [m for m in vocab if m.graph.x.shape[0] == 3]
    assert len(ring) == 1 and ring[0].graph.edge_index.shape == (2, 6)
    assert (ring[0].graph.edge_attr == 0).all()


def test_json_source_round_trips_and_missing_molecule_raises(tmp_path):
    data = ["Cc1ccccc1", "CC(C)C", "OCC", "c1ccccc1-c1ccccc1"]
    vocab, assign = motifs.builtin_motifs(data)
    path = tmp_path / "motifs.json"
    motifs.write_json(path, data, vocab, assign)
    doc = json.loads(path.read_text())
    assert set(doc) == {"clique_list", "mol_to_clique"} and set(doc["mol_to_clique"]) == set(data)
    v2, a2 = motifs.load_motifs(str(path), data)
    assert a2 == assign and [m.smiles for m in v2] == [m.smiles for m in vocab]
    for m, n in zip(vocab, v2):
        assert (m.graph.x == n.graph.x).all() and (m.graph.edge_index == n.graph.edge_index).all()
    with pytest.raises(ValueError, match="no motif assignment"):
        motifs.json_motifs(str(path), data + ["CCCl"])
    # a clique SMILES the parser rejects has no graph; one warning gives the count
    doc["clique_list"].append("C1CC")
    path.write_text(json.dumps(doc))
    with pytest.warns(RuntimeWarning, match="1 of"):
        v3, _ = motifs.json_motifs(str(path), data)
    assert v3[-1].graph is None
    assert motifs.load_motifs("builtin", data)[1] == assign


def test_motif_batch_equals_the_reference_loop():
    clique_list = ["a", "b", "c", "d"]
    mol_to_clique = {0: {"a": 1, "c": 2}, 1: {"b": 1}, 2: {"d": 1, "a": 1, "b": 3}, 3: {"c": 1}}
    assignments = [[clique_list.index(c) for c in mol_to_clique[i]] for i in range(4)]
    batch = [2, 0, 3, 1]
    mol_idx, clique_idx = motifs.motif_batch(torch.tensor(batch), assignments)
    ref_mol, ref_clique = reference_motif_batch(batch, mol_to_clique, clique_list)
    assert mol_idx.dtype == clique_idx.dtype == torch.long
    assert torch.equal(mol_idx, ref_mol) and torch.equal(clique_idx, ref_clique)
    assert mol_idx.tolist() == [0, 0, 0, 1, 1, 2, 3, 0, 1, 2, 3]
