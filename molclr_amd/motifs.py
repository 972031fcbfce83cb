"""Motif (clique) assignments for the motif fine-tuning model, without RDKit.

The reference fragments every molecule with RDKit's BRICS rules plus three
rules of its own (utils/clique.py:11-90), names a fragment by its RDKit
SMILES and trains one embedding per distinct name (finetune.py:104-119).
RDKit is not installed here, so there are two sources of assignments; both
give ``(vocabulary, assignments)``: a list of :class:`Motif` and, per
molecule, the list of its distinct motif indices.

``builtin_motifs`` (**parity unpinned**, like molclr_amd.smiles): the
reference's non-BRICS rules applied to every molecule, over
``smiles.featurise(s, add_hs=False)`` and ``smiles._ring_bonds``:

* one clique per bond; a single atom is one clique;
* a bond that is on no ring and touches a ring atom is broken, a non-ring end
  becoming a clique of its own (clique.py:35-45; a chain bond between two
  rings, which the reference leaves to BRICS, is broken too);
* a non-ring atom with more than two neighbours becomes a clique of its own,
  its bonds broken (clique.py:47-58);
* overlapping cliques are merged (clique.py:60-71).

There is no BRICS bond table and no kekulisation.  A motif's identity is a
canonical key of the induced subgraph: colour refinement from (atom type,
chirality) over the bond types, the key the sorted colours plus the sorted
bond tuples; two different subgraphs with the same key (a refinement
collision) become one motif.  The vocabulary is ordered by first appearance
and a motif keeps its first occurrence as its graph, written as a SMILES
(``motif_smiles``) and read back by the featuriser, so both sources hand the
trainer graphs made the same way.

``json_motifs``: a file ``{"clique_list": [smiles, ...], "mol_to_clique":
{"<molecule smiles>": ["<clique smiles>", ...]}}``, what the reference's
``_gen_cliques`` produces keyed by SMILES, for users who export it where
RDKit exists.  A molecule missing from the file raises ValueError; a clique
SMILES the parser rejects has no graph (the trainer keeps that row's
nn.Embedding initialisation).

``motif_batch`` builds a batch's ``(mol_idx, clique_idx)`` in the reference's
layout (finetune.py:202-210).
"""
from __future__ import annotations

import hashlib
import json
import warnings
from typing import NamedTuple

import numpy as np
import torch

from . import smiles as msmiles


class Motif(NamedTuple):
    smiles: str
    graph: object  # dataset.Molecule, or None when the parser rejects the SMILES


def _bonds_of(mol):
    """(a, b, type, dir) per bond of a featurised molecule (each bond is the
    directed pair at columns 2k, 2k + 1)."""
    ei, ea = mol.edge_index, mol.edge_attr
    return [(int(ei[0, k]), int(ei[1, k]), int(ea[k, 0]), int(ea[k, 1]))
            for k in range(0, ei.shape[1], 2)]


def fragment_bonds(n_atoms: int, bonds) -> list:
    """The cliques (sorted atom lists, ordered by their first atom) of a
    molecule of ``n_atoms`` atoms and ``bonds`` (a, b, ...)."""
    if n_atoms == 1:
        return [[0]]
    on_ring = msmiles._ring_bonds(n_atoms, [(b[0], b[1], None, 0) for b in bonds])
    ring_atom = np.zeros(n_atoms, dtype=bool)
    degree = np.zeros(n_atoms, dtype=np.int64)
    for k, b in enumerate(bonds):
        degree[b[0]] += 1
        degree[b[1]] += 1
        if on_ring[k]:
            ring_atom[b[0]] = ring_atom[b[1]] = True
    branch = (degree > 2) & ~ring_atom
    parent = list(range(n_atoms))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for k, (a, b, *_) in enumerate(bonds):
        broken = (not on_ring[k] and (ring_atom[a] or ring_atom[b])) or branch[a] or branch[b]
        if not broken:  # the bond's clique joins the cliques of both ends
            parent[find(a)] = find(b)
    groups = {}
    for v in range(n_atoms):
        groups.setdefault(find(v), []).append(v)
    return sorted(groups.values(), key=lambda c: c[0])


def fragment(smiles: str) -> list:
    """The cliques of a SMILES (heavy atoms in SMILES order)."""
    mol = msmiles.featurise(smiles, add_hs=False)
    return fragment_bonds(mol.x.shape[0], _bonds_of(mol))


def _h(obj) -> int:
    return int.from_bytes(hashlib.blake2b(repr(obj).encode(), digest_size=8).digest(), "big")


def motif_key(x, bonds, atoms) -> tuple:
    """Canonical key of the subgraph induced by ``atoms``: colour refinement
    (as many rounds as atoms) from (atom type, chirality) over bond types."""
    inside = set(atoms)
    sub = [(a, b, t) for a, b, t, _ in bonds if a in inside and b in inside]
    colour = {v: _h((int(x[v, 0]), int(x[v, 1]))) for v in atoms}
    for _ in range(len(atoms)):
        nbrs = {v: [] for v in atoms}
        for a, b, t in sub:
            nbrs[a].append((t, colour[b]))
            nbrs[b].append((t, colour[a]))
        colour = {v: _h((colour[v], sorted(nbrs[v]))) for v in atoms}
    return (tuple(sorted(colour.values())),
            tuple(sorted((min(colour[a], colour[b]), max(colour[a], colour[b]), t)
                         for a, b, t in sub)))


_BOND_CHAR = {(msmiles.SINGLE, msmiles.DIR_NONE): "-", (msmiles.SINGLE, msmiles.DIR_UP): "/",
              (msmiles.SINGLE, msmiles.DIR_DOWN): "\\", (msmiles.DOUBLE, msmiles.DIR_NONE): "=",
              (msmiles.TRIPLE, msmiles.DIR_NONE): "#", (msmiles.AROMATIC, msmiles.DIR_NONE): ":"}
_CHI_TAG = {msmiles.CHI_NONE: "", msmiles.CHI_CCW: "@", msmiles.CHI_CW: "@@",
            msmiles.CHI_OTHER: "@SP1"}


def motif_smiles(x, bonds, atoms) -> str:
    """A SMILES of the connected subgraph induced by ``atoms``, depth first
    from its first atom: every atom in brackets (no hydrogens; the featuriser
    reads none without add_hs) and every bond written out, so the parser
    infers nothing."""
    inside = set(atoms)
    adj = {v: [] for v in atoms}
    for k, (a, b, t, d) in enumerate(bonds):
        if a in inside and b in inside:
            adj[a].append((b, k))
            adj[b].append((a, k))
    sym = lambda k: _BOND_CHAR.get((bonds[k][2], bonds[k][3]), "-")  # noqa: E731
    tree, seen_bond = {v: [] for v in atoms}, set()
    closures = {v: [] for v in atoms}  # (ring number, bond) at each end
    # iterative depth-first search: tree children per atom, the other bonds close rings
    visited = {atoms[0]}
    ring = 0
    it = [(atoms[0], iter(adj[atoms[0]]))]
    while it:
        v, nbrs = it[-1]
        for u, k in nbrs:
            if k in seen_bond:
                continue
            seen_bond.add(k)
            if u in visited:
                ring += 1
                closures[u].append((ring, k, True))   # u was written first: it opens
                closures[v].append((ring, k, False))
            else:
                visited.add(u)
                tree[v].append((u, k))
                it.append((u, iter(adj[u])))
            break
        else:
            it.pop()

    def number(n):
        return str(n) if n < 10 else f"%{n}" if n < 100 else f"%({n})"

    def emit(v):
        s = "[" + msmiles._ELEMENTS[int(x[v, 0])] + _CHI_TAG.get(int(x[v, 1]), "") + "]"
        for n, k, opens in closures[v]:
            s += (sym(k) if opens else "") + number(n)
        kids = tree[v]
        for i, (u, k) in enumerate(kids):
            t = sym(k) + emit(u)
            s += t if i == len(kids) - 1 else "(" + t + ")"
        return s

    return emit(atoms[0])


def _graph_of(smiles: str):
    try:
        return msmiles.featurise(smiles, add_hs=False)
    except (ValueError, KeyError, IndexError):
        return None


def builtin_motifs(smiles_data):
    """(vocabulary, assignments) of the built-in fragmenter over a list of
    SMILES: the vocabulary in order of first appearance, each molecule's
    distinct motif indices in order of their first clique."""
    index, vocabulary, assignments = {}, [], []
    for s in smiles_data:
        mol = msmiles.featurise(s, add_hs=False)
        bonds = _bonds_of(mol)
        mine = []
        for atoms in fragment_bonds(mol.x.shape[0], bonds):
            key = motif_key(mol.x, bonds, atoms)
            m = index.get(key)
            if m is None:
                m = index[key] = len(vocabulary)
                name = motif_smiles(mol.x, bonds, atoms)
                vocabulary.append(Motif(name, _graph_of(name)))
            if m not in mine:
                mine.append(m)
        assignments.append(mine)
    return vocabulary, assignments


def json_motifs(path, smiles_data):
    """(vocabulary, assignments) from a JSON file of the reference's
    ``_gen_cliques`` output keyed by SMILES (module docstring)."""
    with open(path) as f:
        doc = json.load(f)
    clique_list, mol_to_clique = list(doc["clique_list"]), doc["mol_to_clique"]
    index = {c: i for i, c in enumerate(clique_list)}
    vocabulary = [Motif(c, _graph_of(c)) for c in clique_list]
    rejected = sum(m.graph is None for m in vocabulary)
    if rejected:
        warnings.warn(f"{path}: {rejected} of {len(vocabulary)} clique SMILES are not parsed; their "
                      "motif embeddings keep the random initialisation", RuntimeWarning,
                      stacklevel=2)
    assignments = []
    for s in smiles_data:
        if s not in mol_to_clique:
            raise ValueError(f"{path}: no motif assignment for training molecule {s!r}")
        mine = []
        for c in mol_to_clique[s]:
            if c not in index:
                raise ValueError(f"{path}: clique {c!r} of molecule {s!r} is not in clique_list")
            if index[c] not in mine:
                mine.append(index[c])
        assignments.append(mine)
    return vocabulary, assignments


def write_json(path, smiles_data, vocabulary, assignments) -> None:
    """Write assignments in the JSON source's format."""
    doc = {"clique_list": [m.smiles for m in vocabulary],
           "mol_to_clique": {s: [vocabulary[m].smiles for m in mine]
                             for s, mine in zip(smiles_data, assignments)}}
    with open(path, "w") as f:
        json.dump(doc, f)


def load_motifs(source, smiles_data):
    """``builtin`` or the path of a JSON file."""
    if source in (None, "builtin"):
        return builtin_motifs(smiles_data)
    return json_motifs(source, smiles_data)


def motif_batch(mol_index, assignments, device=None):
    """``(mol_idx [T + B], clique_idx [T])`` int64 of a batch whose molecules
    are ``mol_index`` (dataset indices): the motifs of molecule 0, of molecule
    1, ..., each with its position in the batch, then ``0 .. B - 1`` for the
    molecules' own rows (finetune.py:202-210)."""
    if isinstance(mol_index, torch.Tensor):
        mol_index = mol_index.cpu().numpy()
    mol_index = np.asarray(mol_index, dtype=np.int64).reshape(-1)
    B = len(mol_index)
    counts = np.array([len(assignments[i]) for i in mol_index], dtype=np.int64)
    clique_idx = np.array([m for i in mol_index for m in assignments[i]], dtype=np.int64)
    mol_idx = np.concatenate([np.repeat(np.arange(B, dtype=np.int64), counts),
                              np.arange(B, dtype=np.int64)])
    return (torch.from_numpy(mol_idx).to(device, non_blocking=True),
            torch.from_numpy(clique_idx).to(device, non_blocking=True))
