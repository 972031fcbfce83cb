"""Molecule retrieval with a trained encoder (the nearest-neighbour analysis
of the MolCLR paper; no reference module).

:func:`embed_store` turns molecules resident in HBM (a
:class:`~molclr_amd.task_store.DeviceTaskStore`, or a
:class:`~molclr_amd.augment.DeviceMoleculeStore`) into an embedding matrix:
un-augmented batches collated on the device, the model in eval mode, every
row written straight into the result.  :class:`MoleculeIndex` searches such a
matrix with the exact fused top-k kernel (``ops.topk_dot``): no
``[queries, library]`` score matrix is ever written.  :func:`merge_topk`
combines the results of the pieces of a sharded library under the kernel's
total order -- exactly, because the kernel's summation order of a (query,
row) pair does not depend on where the row sits.

``python -m molclr_amd.retrieval --config config.yaml --checkpoint model.pth
--library smiles.txt|shard --query smiles.txt -k 10`` prints one line per
query and neighbour: query index, library index, score.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

from . import ops
from .augment import DeviceMoleculeStore
from .task_store import DeviceTaskStore, raise_for_collate_status


def _as_task_store(store) -> DeviceTaskStore:
    if isinstance(store, DeviceTaskStore):
        return store
    if isinstance(store, DeviceMoleculeStore):  # a dummy target per molecule
        return DeviceTaskStore(store.x, store.atom_ptr, store.edge_index, store.edge_attr,
                               store.bond_ptr, store.device,
                               torch.zeros(store.num_molecules, dtype=torch.int64))
    raise TypeError(f"embed_store: a DeviceTaskStore or DeviceMoleculeStore, got {type(store)}")


def embed_store(model, store, batch_size: int = 1024, which: str = 'h', normalize: bool = True,
                dtype=torch.float32) -> torch.Tensor:
    """``[G, F]`` embeddings of the store's molecules in id order.

    ``model`` is any of the encoders that return ``(h, out)`` / ``(h, pred)``
    from ``forward(batch)``; ``which`` picks ``'h'`` (the representation) or
    ``'out'`` (the projection / prediction).  Runs without autograd in eval
    mode (running BatchNorm statistics, no dropout) and puts the model back
    into the mode it was in.  Batches are sized from the store's host count
    arrays, so none waits for the device; the collate and graph status words
    are read once at the end.  ``normalize`` stores unit rows;
    ``dtype=torch.bfloat16`` rounds once (to nearest even) at the store."""
    from .data import device_graph, raise_for_status
    from .ginet_finetune_mp import GINet as MotifGINet
    if isinstance(model, MotifGINet):
        raise NotImplementedError("embed_store: the motif model needs the molecules' motif items, "
                                  "which a store walk does not make; embed with the plain GIN")
    if which not in ('h', 'out'):
        raise ValueError("embed_store: which must be 'h' or 'out'")
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("embed_store: dtype must be torch.float32 or torch.bfloat16")
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("embed_store: batch_size must be at least 1")
    store = _as_task_store(store)
    G = store.num_molecules
    ids_h = np.arange(G, dtype=np.int64)
    ids_d = torch.from_numpy(ids_h).to(store.device)
    status = torch.zeros(1, dtype=torch.int32, device=store.device)
    cstatus = torch.zeros(1, dtype=torch.int32, device=store.device)
    out = None
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for k in range(0, G, batch_size):
                batch = store.collate(ids_d[k:k + batch_size], ids_h[k:k + batch_size])
                z = model(batch)[0 if which == 'h' else 1]
                if normalize:
                    z = ops.l2_normalize(z)
                if out is None:
                    out = torch.empty((G, z.shape[1]), dtype=dtype, device=store.device)
                out[k:k + z.shape[0]].copy_(z)  # fp32 -> bf16: round to nearest even
                torch.bitwise_or(cstatus, batch.status, out=cstatus)
                torch.bitwise_or(status, device_graph(batch).status, out=status)
    finally:
        model.train(was_training)
    if out is None:
        raise ValueError("embed_store: the store holds no molecules")
    raise_for_collate_status(int(cstatus.item()))
    raise_for_status(int(status.item()))
    return out


def merge_topk(parts, k: int | None = None):
    """``(scores, idx)`` of the union of per-shard results ``[(scores, idx),
    ...]`` (each ``[nq, k_i]``, as ``ops.topk_dot`` returns them with the
    shard's ``idx_base``) under the kernel's total order: higher score first,
    equal scores by lower index, ``idx == -1`` padding last.  Torch ops on
    whatever device the parts live on (CPU tensors too)."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_topk: no parts")
    s = torch.cat([p[0] for p in parts], 1)
    i = torch.cat([p[1] for p in parts], 1)
    k = int(parts[0][0].shape[1] if k is None else k)
    big = torch.iinfo(torch.int64).max
    key = torch.where(i < 0, torch.full_like(i, big), i)
    o = torch.argsort(key, dim=1, stable=True)            # by index ...
    s, i = torch.gather(s, 1, o), torch.gather(i, 1, o)
    o = torch.argsort(s, dim=1, descending=True, stable=True)  # ... then, stably, by score
    s, i = torch.gather(s, 1, o), torch.gather(i, 1, o)
    if s.shape[1] < k:
        pad = k - s.shape[1]
        s = torch.cat([s, s.new_full((s.shape[0], pad), float('-inf'))], 1)
        i = torch.cat([i, i.new_full((i.shape[0], pad), -1)], 1)
    return s[:, :k].contiguous(), i[:, :k].contiguous()


def _to_numpy(emb: torch.Tensor) -> np.ndarray:
    """fp32 as it is, bf16 as its uint16 bit patterns."""
    emb = emb.detach().cpu().contiguous()
    if emb.dtype == torch.bfloat16:
        return emb.view(torch.int16).numpy().view(np.uint16)
    return emb.numpy()


def _from_numpy(arr: np.ndarray, dtype: str) -> torch.Tensor:
    if dtype == 'bfloat16':
        if arr.dtype != np.uint16:
            raise ValueError("a bfloat16 index file holds uint16 bit patterns")
        return torch.from_numpy(arr.view(np.int16).copy()).view(torch.bfloat16)
    if dtype != 'float32' or arr.dtype != np.float32:
        raise ValueError(f"index file: dtype {dtype!r} with {arr.dtype} data")
    return torch.from_numpy(arr.copy())


def _sidecar(path) -> Path:
    path = Path(path)
    return path.with_name(path.name + '.json')


class MoleculeIndex:
    """An embedding matrix ``[G, F]`` (fp32 or bf16) and its exact search.

    ``normalized`` says that the rows are unit vectors (``embed_store``'s
    default), which makes cosine similarity the default metric; ``which``
    records what was embedded.  On a GPU the matrix is laid out once the way
    the kernel reads it."""

    def __init__(self, embeddings: torch.Tensor, normalized: bool = True, which: str = 'h'):
        if embeddings.dim() != 2 or embeddings.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("MoleculeIndex: a [G, F] float32 or bfloat16 matrix")
        self.embeddings = embeddings.detach()
        self.normalized = bool(normalized)
        self.which = which
        self._rows = None  # the kernel's layout of the matrix, made by the first search

    def __len__(self) -> int:
        return int(self.embeddings.shape[0])

    @property
    def dim(self) -> int:
        return int(self.embeddings.shape[1])

    def _db(self) -> torch.Tensor:
        if self._rows is None:
            self._rows = ops.topk_rows(self.embeddings)
        return self._rows

    def search(self, queries: torch.Tensor, k: int = 10, exclude=None, metric: str | None = None):
        """``(scores [nq, k], ids [nq, k])`` of fp32 ``queries`` [nq, F]:
        ``metric='cosine'`` (the default for unit rows) normalises the queries
        first, ``'dot'`` takes them as they are.  ``exclude`` [nq] names one
        library id per query to leave out."""
        metric = metric or ('cosine' if self.normalized else 'dot')
        if metric not in ('cosine', 'dot'):
            raise ValueError("search: metric must be 'cosine' or 'dot'")
        if queries.dim() != 2 or queries.shape[1] != self.dim:
            raise ValueError(f"search: queries must be [nq, {self.dim}]")
        q = queries.detach()
        if q.dtype != torch.float32:
            raise TypeError("search: queries must be float32")
        if metric == 'cosine' and q.shape[0]:
            q = ops.l2_normalize(q)
        if exclude is not None:
            exclude = torch.as_tensor(exclude, dtype=torch.int64).to(q.device)
        db = self._db()
        return ops.topk_dot(q if db.shape[1] == q.shape[1] else ops.topk_rows(q), db, k, exclude)

    def search_ids(self, mol_ids, k: int = 10, exclude_self: bool = True):
        """The neighbours of library molecules: the query rows are the index's
        own rows ``mol_ids``; ``exclude_self`` leaves each one's own id out."""
        ids = torch.as_tensor(mol_ids, dtype=torch.int64).to(self.embeddings.device).reshape(-1)
        q = self.embeddings.index_select(0, ids).float()
        return self.search(q, k, ids if exclude_self else None,
                           'dot' if self.normalized else None)

    # -- files -------------------------------------------------------------
    def save(self, path) -> None:
        """``path`` (.npy: the matrix, bf16 as uint16 bit patterns) and
        ``path + '.json'`` (dtype, normalized, which, count, dim)."""
        path = Path(path)
        with open(path, 'wb') as f:
            np.save(f, _to_numpy(self.embeddings))
        meta = {"dtype": str(self.embeddings.dtype).replace('torch.', ''),
                "normalized": self.normalized, "which": self.which, "count": len(self),
                "dim": self.dim}
        _sidecar(path).write_text(json.dumps(meta, indent=1) + "\n")

    @classmethod
    def load(cls, path, device='cpu') -> "MoleculeIndex":
        meta = json.loads(_sidecar(path).read_text())
        with open(path, 'rb') as f:
            arr = np.load(f, allow_pickle=False)
        emb = _from_numpy(arr, meta["dtype"])
        if emb.dim() != 2 or emb.shape[0] != meta["count"]:
            raise ValueError(f"{path}: {tuple(emb.shape)} does not match the sidecar's count "
                             f"{meta['count']}")
        return cls(emb.to(device), meta["normalized"], meta["which"])


# -- command line ---------------------------------------------------------------
def _model_from_config(config: dict, device):
    """The encoder a pre-training or fine-tuning config describes (the
    trainers' model_type / model keys; a fine-tuning config has ``dataset.task``)."""
    kind = config['model_type']
    mcfg = dict(config['model'])
    task = (config.get('dataset') or {}).get('task')
    if kind == 'gin':
        if task:
            from .ginet_finetune import GINet
            return GINet(task, **mcfg).to(device)
        from .ginet_molclr import GINet
        return GINet(**mcfg).to(device)
    if kind == 'gcn':
        if task:
            from .gcn_finetune import GCN
            return GCN(task, **mcfg).to(device)
        from .gcn_molclr import GCN
        return GCN(**mcfg).to(device)
    raise ValueError(f"model_type {kind!r}: retrieval embeds with 'gin' or 'gcn'")


def _molecules(path, what: str, add_hs: bool = False) -> list:
    """The molecules of a shard, or of a SMILES file (one the featuriser
    refuses is reported on stderr and skipped).  ``add_hs``: explicit
    hydrogens, as the fine-tuning datasets featurise."""
    from . import shards, smiles
    if shards.is_shard(path):
        shard = shards.GraphShard(path)
        return shards.molecules_of(shard, range(len(shard)))
    mols = []
    for n, s in enumerate(shards.read_smiles(path)):
        s = s.strip()
        if not s:
            continue
        try:
            m = smiles.featurise(s, add_hs=add_hs)
            if m.x.size and int(m.x[:, 1].max()) >= shards.NUM_CHIRALITY_TAG:
                raise ValueError("chirality tag without an embedding row")
        except ValueError as e:
            print(f"{what} line {n}: skipped {s!r}: {e}", file=sys.stderr)
            continue
        mols.append(m)
    return mols


def main(argv=None) -> int:
    import argparse

    import yaml
    ap = argparse.ArgumentParser(prog="python -m molclr_amd.retrieval", description=__doc__)
    ap.add_argument("--config", required=True, help="pre-training or fine-tuning yaml")
    ap.add_argument("--checkpoint", default=None, help="model.pth (state_dict); none: as initialised")
    ap.add_argument("--library", required=True, help="SMILES file or featurised shard")
    ap.add_argument("--query", required=True, help="SMILES file or featurised shard")
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--which", default='h', choices=('h', 'out'))
    ap.add_argument("--bf16", action="store_true", help="keep the library in bf16")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    with open(args.config) as f:
        config = yaml.safe_load(f)
    device = torch.device(args.device)
    model = _model_from_config(config, device)
    if args.checkpoint:
        state = torch.load(args.checkpoint, map_location=device, weights_only=True)
        if hasattr(model, 'load_my_state_dict'):
            with torch.no_grad():
                model.load_my_state_dict(state)
        else:
            model.load_state_dict(state)
    add_hs = bool((config.get('dataset') or {}).get('task'))  # a fine-tuning config
    lib = _molecules(args.library, "library", add_hs)
    qry = _molecules(args.query, "query", add_hs)
    if not lib or not qry:
        print("nothing to search: empty library or query", file=sys.stderr)
        return 1
    emb = embed_store(model, DeviceMoleculeStore.from_molecules(lib, device), args.batch_size,
                      args.which, True, torch.bfloat16 if args.bf16 else torch.float32)
    q = embed_store(model, DeviceMoleculeStore.from_molecules(qry, device), args.batch_size,
                    args.which, True)
    scores, ids = MoleculeIndex(emb, True, args.which).search(q, args.k)
    scores, ids = scores.cpu().numpy(), ids.cpu().numpy()
    for i in range(ids.shape[0]):
        for s, j in zip(scores[i], ids[i]):
            print(f"{i} {int(j)} {float(s):.6f}")
    return 0


__all__ = ["MoleculeIndex", "embed_store", "merge_topk"]

if __name__ == "__main__":
    sys.exit(main())
