"""Supervised fine-tuning driver — drop-in for the reference's finetune.py.

Same ``FineTune(dataset, config).train()`` loop and ``config_finetune.yaml``
keys as finetune.py:61-380: the criterion by task (cross-entropy; L1 for
qm7 / qm8 / qm9; MSE for the other regressions), a label ``Normalizer`` for
qm7 / qm9, ``fine_tune_from`` loaded through ``load_my_state_dict``, Adam in
two learning-rate groups, ``train_loss`` logged every ``log_every_n_steps``,
validation every ``eval_every_n_epochs`` with the best weights (highest
ROC-AUC, lowest RMSE / MAE) saved to ``<log_dir>/checkpoints/model.pth``, and a
final test on the reloaded checkpoint that leaves ``self.roc_auc``,
``self.rmse`` or ``self.mae``.

Differences: the criterion is computed inside the task head's launch
(``model.loss``: ops.task_head); one :class:`FusedAdam` per learning-rate group;
the metrics are numpy (no scikit-learn); ``model_type: gin`` trains
ginet_finetune.GINet, and the motif model the reference goes on to there
(ginet_finetune_mp.py) is ``model_type: gin_motif``: as finetune.py:144-161,
the plain model embeds the motif vocabulary, then ginet_finetune_mp.GINet is
built, loaded and given those rows as its motif table.  The motifs come from
the optional key ``motifs``: ``builtin`` (molclr_amd.motifs' fragmenter, no
RDKit, parity unpinned; the default) or the path of a JSON export of the
reference's BRICS cliques.  Optional keys ``log_root``, ``ckpt_root``,
``seed``, ``device_data`` and ``hip_graph`` (default False): with ``hip_graph: True`` the
training step and the evaluation passes are replayed from HIP graphs
(molclr_amd.finetune_step); a model those cannot take trains eagerly after
one RuntimeWarning.  The motif model is taken with ``hip_graph_motif: True``
(default False) next to ``hip_graph: True``: the batch's items from
molclr_amd.motifs.motif_batch are then staged next to the batch; without that
key it warns and trains eagerly.  ``model_type: gcn`` with ``fp16_precision:
True`` trains in fp32 after a RuntimeWarning unless ``gcn_bf16: True`` (default
False) is set too, which builds the GCN with ``precision='bf16'``.  ``freeze_bn:
True`` (default False) keeps every BatchNorm of the encoder on its running
statistics for the whole run (``model.freeze_bn``).  ``device_data:
True`` (default False) featurises the dataset once into HBM and collates every
batch on the device (molclr_amd.task_store: DeviceTaskStore / DeviceTaskLoader);
with ``hip_graph: True`` the captured steps gather each batch by its molecule
ids straight into their buffers, the motif model's items included.  Invalid inputs (graph indices, atom features, class
labels, motif indices) raise at the next log step (``check_inputs``), as in
molclr_amd.molclr.
"""
from __future__ import annotations

import os
import sys
import warnings
from datetime import datetime

import numpy as np
import torch
import yaml

from .molclr import _summary_writer

# task_name -> (task, data_path, target columns) of the MoleculeNet benchmarks
# the reference lists (finetune.py:401-491)
BENCHMARKS = {
    'BBBP': ('classification', 'data/bbbp/BBBP.csv', ["p_np"]),
    'Tox21': ('classification', 'data/tox21/tox21.csv',
              ["NR-AR", "NR-AR-LBD", "NR-AhR", "NR-Aromatase", "NR-ER", "NR-ER-LBD",
               "NR-PPAR-gamma", "SR-ARE", "SR-ATAD5", "SR-HSE", "SR-MMP", "SR-p53"]),
    'ClinTox': ('classification', 'data/clintox/clintox.csv', ['CT_TOX', 'FDA_APPROVED']),
    'HIV': ('classification', 'data/hiv/HIV.csv', ["HIV_active"]),
    'BACE': ('classification', 'data/bace/bace.csv', ["Class"]),
    'FreeSolv': ('regression', 'data/freesolv/freesolv.csv', ["expt"]),
    'ESOL': ('regression', 'data/esol/esol.csv', ["measured log solubility in mols per litre"]),
    'Lipo': ('regression', 'data/lipophilicity/Lipophilicity.csv', ["exp"]),
    'qm7': ('regression', 'data/qm7/qm7.csv', ["u0_atom"]),
    'qm8': ('regression', 'data/qm8/qm8.csv',
            ["E1-CC2", "E2-CC2", "f1-CC2", "f2-CC2", "E1-PBE0", "E2-PBE0", "f1-PBE0", "f2-PBE0",
             "E1-CAM", "E2-CAM", "f1-CAM", "f2-CAM"]),
    'qm9': ('regression', 'data/qm9/qm9.csv',
            ['mu', 'alpha', 'homo', 'lumo', 'gap', 'r2', 'zpve', 'cv']),
}
MAE_TASKS = ('qm7', 'qm8', 'qm9')


# ---------------------------------------------------------------------------
# Metrics (numpy; sklearn.metrics' roc_auc_score / mean_squared_error /
# mean_absolute_error of finetune.py:15)
# ---------------------------------------------------------------------------
def roc_auc_score(labels, scores) -> float:
    """Area under the ROC curve of binary ``labels`` by ``scores``: the
    Mann-Whitney statistic with tied scores given their average rank."""
    y = np.asarray(labels).reshape(-1)
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    pos = y == 1
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in labels. ROC AUC score is not defined")
    order = np.argsort(s, kind="mergesort")
    ranks = np.empty(len(s), dtype=np.float64)
    sorted_s = s[order]
    i = 0
    while i < len(s):
        j = i
        while j + 1 < len(s) and sorted_s[j + 1] == sorted_s[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return float((ranks[pos].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def rmse_score(labels, predictions) -> float:
    d = np.asarray(labels, dtype=np.float64).reshape(-1) - \
        np.asarray(predictions, dtype=np.float64).reshape(-1)
    return float(np.sqrt(np.mean(d * d)))


def mae_score(labels, predictions) -> float:
    d = np.asarray(labels, dtype=np.float64).reshape(-1) - \
        np.asarray(predictions, dtype=np.float64).reshape(-1)
    return float(np.mean(np.abs(d)))


class Normalizer(object):
    """Normalize a tensor by the mean and std of a sample, and restore it
    (finetune.py:38-58)."""

    def __init__(self, tensor):
        self.mean = torch.mean(tensor)
        self.std = torch.std(tensor)

    def norm(self, tensor):
        return (tensor - self.mean) / self.std

    def denorm(self, normed_tensor):
        return normed_tensor * self.std + self.mean

    def state_dict(self):
        return {'mean': self.mean, 'std': self.std}

    def load_state_dict(self, state_dict):
        self.mean = state_dict['mean']
        self.std = state_dict['std']


class FineTune(object):
    def __init__(self, dataset, config):
        self.config = config
        self.device = self._get_device()
        dir_name = (datetime.now().strftime('%b%d_%H-%M-%S') + '_' + config['task_name'] + '_' +
                    str(config['dataset']['target']))
        self.log_dir = os.path.join(config.get('log_root', 'finetune'), dir_name)
        self.writer = _summary_writer(self.log_dir)
        self.dataset = dataset
        self.task = config['dataset']['task']
        if self.task == 'classification':
            self.criterion = 'cross_entropy'
        elif self.task == 'regression':
            self.criterion = 'l1' if config['task_name'] in MAE_TASKS else 'mse'
        else:
            raise ValueError("dataset.task must be 'classification' or 'regression'")
        self.normalizer = None
        self.vocabulary = self.assignments = None  # model_type: gin_motif (load_motifs)
        # sticky OR of every step's graph + head status word (check_inputs)
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        # hip_graph: the captured step objects of the model being trained
        # (_captured_for); None while the loop runs eagerly
        self.hip_graph = bool(config.get('hip_graph', False))
        self.hip_graph_motif = bool(config.get('hip_graph_motif', False))
        self._captured = None
        # device_data: True -- the dataset featurised once into HBM and every
        # batch collated on the device (molclr_amd.task_store); off: the host
        # DataLoader, exactly as before
        self.device_data = bool(config.get('device_data', False))
        self._store = None
        self._collate_status = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _get_device(self):
        if not torch.cuda.is_available() or self.config.get('gpu', 'cuda:0') == 'cpu':
            raise RuntimeError("molclr_amd fine-tuning runs on MI355X GPUs only")
        device = torch.device(self.config.get('gpu', 'cuda:0'))
        torch.cuda.set_device(device)
        return device

    # -- model and optimizer --------------------------------------------------
    def build_model(self):
        model = self._build_model()
        # freeze_bn: True (default off) -- every BatchNorm of the encoder on its
        # running statistics for the whole run (model.freeze_bn: model.train()
        # leaves them in eval mode); dropout and every other layer train on
        if self.config.get('freeze_bn', False):
            model.freeze_bn = True
        return model

    def _build_model(self):
        task, mcfg = self.task, dict(self.config['model'])
        if self.config['model_type'] == 'gin':
            from .ginet_finetune import GINet
            if self.config.get('fp16_precision', False):
                mcfg['precision'] = 'bf16'
            model = GINet(task, **mcfg).to(self.device)
        elif self.config['model_type'] == 'gcn':
            from .gcn_finetune import GCN
            if self.config.get('fp16_precision', False) and self.config.get('gcn_bf16', False):
                mcfg['precision'] = 'bf16'  # opt-in: the GCN's bf16 storage path
            elif self.config.get('fp16_precision', False):
                warnings.warn("fp16_precision: True with model_type: gcn -- the GCN encoder has "
                              "no reduced-precision path; training in fp32", RuntimeWarning,
                              stacklevel=2)
            model = GCN(task, **mcfg).to(self.device)
        elif self.config['model_type'] == 'gin_motif':
            return self._build_motif_model(task, mcfg)
        else:
            raise ValueError('Undefined GNN model.')
        return self._load_pre_trained_weights(model)

    # -- the motif model (model_type: gin_motif) ------------------------------------
    def load_motifs(self, smiles_data):
        """The motif vocabulary and every molecule's motif indices, from the
        config's ``motifs`` source (molclr_amd.motifs)."""
        from .motifs import load_motifs
        self.vocabulary, self.assignments = load_motifs(self.config.get('motifs', 'builtin'),
                                                        smiles_data)

    def embed_vocabulary(self, model):
        """``(rows, h)``: the plain model's ``h`` of the vocabulary's graphs in
        batches of ``batch_size``, in vocabulary order and in training mode as
        finetune.py:149-156 (batch statistics, dropout active), under no_grad;
        ``rows`` are the motifs that have a graph."""
        from .data import Batch, Data
        rows = [i for i, m in enumerate(self.vocabulary) if m.graph is not None]
        feats = []
        with torch.no_grad():
            for k in range(0, len(rows), self.config['batch_size']):
                graphs = [self.vocabulary[i].graph for i in rows[k:k + self.config['batch_size']]]
                batch = Batch.from_data_list([
                    Data(x=torch.from_numpy(g.x), edge_index=torch.from_numpy(g.edge_index),
                         edge_attr=torch.from_numpy(g.edge_attr)) for g in graphs])
                feats.append(model(batch.to(self.device))[0])
        h = torch.cat(feats) if feats else torch.zeros(0, model.feat_dim, device=self.device)
        return torch.tensor(rows, dtype=torch.long, device=self.device), h

    def _build_motif_model(self, task, mcfg):
        """finetune.py:144-161: the plain model embeds the vocabulary, the motif
        model starts from those rows."""
        from .ginet_finetune import GINet as PlainGINet
        from .ginet_finetune_mp import GINet
        if self.vocabulary is None:
            self.load_motifs(self.dataset.get_data_loaders()[0])
        if self.config.get('fp16_precision', False):
            mcfg['precision'] = 'bf16'
        plain = self._load_pre_trained_weights(PlainGINet(task, **mcfg).to(self.device))
        rows, feats = self.embed_vocabulary(plain)
        model = GINet(len(self.vocabulary), task, **mcfg).to(self.device)
        model = self._load_pre_trained_weights(model)
        init = model.motif_embedding.weight.detach().clone()
        init[rows] = feats
        model.init_motif_emb(init)
        return model

    def build_optimizers(self, model):
        """finetune.py:167-178: parameters whose name contains 'pred_lin' at
        init_lr, everything else at init_base_lr.  For GIN the head is called
        pred_head, so every parameter lands in the base group -- the
        reference's behaviour, kept.  One FusedAdam per non-empty group."""
        from .optim import FusedAdam
        wd = float(eval(str(self.config['weight_decay'])))
        head = [p for n, p in model.named_parameters() if 'pred_lin' in n]
        base = [p for n, p in model.named_parameters() if 'pred_lin' not in n]
        opts = []
        if base:
            opts.append(FusedAdam(base, self.config['init_base_lr'], weight_decay=wd))
        if head:
            opts.append(FusedAdam(head, self.config['init_lr'], weight_decay=wd))
        return opts

    def _load_pre_trained_weights(self, model):
        try:
            folder = os.path.join(self.config.get('ckpt_root', './ckpt'),
                                  str(self.config['fine_tune_from']), 'checkpoints')
            state_dict = torch.load(os.path.join(folder, 'model.pth'), map_location=self.device,
                                    weights_only=True)
            model.load_my_state_dict(state_dict)
            print("Loaded pre-trained model with success.")
        except FileNotFoundError:
            print("Pre-trained weights not found. Training from scratch.")
        return model

    # -- one batch ----------------------------------------------------------------
    def _motif_of(self, data):
        """The motif model's (mol_idx, clique_idx) of a host batch, on the
        device; the index tensors are built from the host copy of mol_index."""
        from .motifs import motif_batch
        return motif_batch(data.mol_index, self.assignments, self.device)

    def _to_device(self, data):
        """(data on the device, the motif model's (mol_idx, clique_idx) or
        None)."""
        motif = None
        if self.device_data:  # a task_store batch: on the device already
            if self.config['model_type'] == 'gin_motif':
                motif = self._store.motif_items(data.mol_index,
                                                getattr(data, "_molclr_host_ids", None))
            torch.bitwise_or(self._collate_status, data.status, out=self._collate_status)
            return data, motif
        if self.config['model_type'] == 'gin_motif':
            motif = self._motif_of(data)
        return data.to(self.device), motif

    def _step(self, model, data, motif=None):
        """(pred, loss) of a batch (finetune.py:89-102); the graph's status
        word -- which the head adds its label bit to -- joins the sticky word."""
        if self.task == 'classification':
            target = data.y.flatten()
        else:
            target = self.normalizer.norm(data.y) if self.normalizer else data.y
        if motif is not None:
            _, pred, loss = model.loss(data, *motif, target, self.criterion)
        else:
            _, pred, loss = model.loss(data, target, self.criterion)
        g = getattr(data, "_molclr_graph", None)
        if g is not None:
            torch.bitwise_or(self._status, g.status, out=self._status)
        return pred, loss

    def check_inputs(self) -> None:
        """Raise if any batch so far had invalid inputs (a sync: called at the
        log steps and once per evaluation)."""
        from .data import raise_for_status
        st = int(self._status.item())
        if self._captured is not None:  # the step objects' sticky words
            step, ev = self._captured[2], self._captured[3]
            if step is not None and step._made:
                st |= int(step.status.item())
            st |= ev._sticky
        raise_for_status(st)
        if self.device_data:  # the device collates' own words
            from .task_store import raise_for_collate_status
            cst = int(self._collate_status.item())
            if self._captured is not None:
                step, ev = self._captured[2], self._captured[3]
                if step is not None and step._made:
                    cst |= int(step.collate_status.item())
                cst |= ev._collate_sticky
            raise_for_collate_status(cst)

    # -- hip_graph: True ----------------------------------------------------------
    def _captured_for(self, model, optimizers=None):
        """(step, eval) objects replaying ``model``'s train step and evaluation
        from HIP graphs, or None: hip_graph is off, or the captured steps
        cannot take the model (one RuntimeWarning naming the reason)."""
        if not self.hip_graph:
            return None
        c = self._captured
        if c is None or c[0] is not model:
            from .finetune_step import CapturedEval, unsupported_reason
            reason = unsupported_reason(model, motif_items=self.hip_graph_motif)
            if reason is not None:
                warnings.warn(f"hip_graph: True -- {reason}; fine-tuning runs eagerly",
                              RuntimeWarning, stacklevel=3)
                self.hip_graph = False
                return None
            c = self._captured = [model, None, None,
                                  CapturedEval(model, self.criterion, self.normalizer)]
        if optimizers is not None and (c[2] is None or c[1] is not optimizers):
            from .finetune_step import CapturedFinetuneStep
            c[1] = optimizers
            c[2] = CapturedFinetuneStep(model, optimizers, self.criterion, self.normalizer)
        return c[2], c[3]

    def train_step(self, model, optimizers, data):
        captured = self._captured_for(model, optimizers)
        if captured is not None and self.device_data:
            # data: (dev_ids, host_ids) of DeviceTaskLoader.ids(); the batch and
            # the motif model's items are gathered into the graph's buffers
            return captured[0].step_ids(self._store, *data).clone()
        if captured is not None:
            # the step's loss is its own buffer, overwritten by the next replay
            data, motif = self._to_device(data)
            return captured[0].step(data, *(motif or ())).clone()
        data, motif = self._to_device(data)
        for opt in optimizers:
            opt.zero_grad()
        _, loss = self._step(model, data, motif)
        loss.backward()
        for opt in optimizers:
            opt.step()
        return loss

    # -- the loop -----------------------------------------------------------------
    def train(self):
        if self.config.get('seed') is not None:
            torch.manual_seed(int(self.config['seed']))
            np.random.seed(int(self.config['seed']))
        if self.device_data:
            from . import task_store
            smiles_data, self._store, train_loader, valid_loader, test_loader = \
                task_store.device_loaders(self.dataset, self.device)
        else:
            smiles_data, train_loader, valid_loader, test_loader = self.dataset.get_data_loaders()
        if self.config['model_type'] == 'gin_motif':
            self.load_motifs(smiles_data)
            if self.device_data:
                self._store.set_motifs(self.assignments)

        self.normalizer = None
        if self.config['task_name'] in ['qm7', 'qm9']:
            if self.device_data:
                train_ids = torch.from_numpy(train_loader.indices).to(self.device)
                labels = self._store.y[train_ids]
            else:
                labels = torch.cat([d.y for d in train_loader])
            self.normalizer = Normalizer(labels.to(self.device))

        model = self.build_model()
        optimizers = self.build_optimizers(model)

        folder = os.path.join(self.log_dir, 'checkpoints')
        os.makedirs(folder, exist_ok=True)
        with open(os.path.join(folder, 'config_finetune.yaml'), 'w') as f:
            yaml.safe_dump(self.config, f)

        n_iter = valid_n_iter = 0
        best_valid_rgr, best_valid_cls = np.inf, 0
        self.epoch_train_loss = []
        for epoch_counter in range(self.config['epochs']):
            losses = []
            batches = train_loader
            if self.device_data and self._captured_for(model, optimizers) is not None:
                batches = train_loader.ids()  # the captured step gathers by ids
            for bn, data in enumerate(batches):
                loss = self.train_step(model, optimizers, data)
                losses.append(loss.detach())
                if n_iter % self.config['log_every_n_steps'] == 0:
                    self.check_inputs()
                    self.writer.add_scalar('train_loss', loss, global_step=n_iter)
                    print(epoch_counter, bn, loss.item())
                n_iter += 1
            if losses:  # one sync per epoch
                self.epoch_train_loss.append(float(torch.stack(losses).mean().item()))

            if epoch_counter % self.config['eval_every_n_epochs'] == 0:
                valid_loss, metric = self._evaluate(model, valid_loader, 'Validation')
                better = metric > best_valid_cls if self.task == 'classification' \
                    else metric < best_valid_rgr
                if better:
                    if self.task == 'classification':
                        best_valid_cls = metric
                    else:
                        best_valid_rgr = metric
                    torch.save(model.state_dict(), os.path.join(folder, 'model.pth'))
                self.writer.add_scalar('validation_loss', valid_loss, global_step=valid_n_iter)
                valid_n_iter += 1

        self._test(model, test_loader)
        return model

    def _evaluate(self, model, loader, what):
        """(mean loss, metric) over a loader under no_grad / eval()
        (finetune.py:259-317): ROC-AUC of the class-1 logit, or MAE / RMSE of
        the de-normalised prediction."""
        captured = self._captured_for(model)
        if captured is not None:
            motif = self._motif_of if self.config['model_type'] == 'gin_motif' else None
            total, predictions, labels = captured[1].run(loader, motif)
            model.train()
            self.check_inputs()
        else:
            total, predictions, labels = self._evaluate_eager(model, loader)
        if self.task == 'classification':
            metric, name = roc_auc_score(labels, predictions[:, 1]), 'ROC AUC'
        elif self.config['task_name'] in MAE_TASKS:
            metric, name = mae_score(labels, predictions), 'MAE'
        else:
            metric, name = rmse_score(labels, predictions), 'RMSE'
        print(f'{what} loss:', total, f'{name}:', metric)
        return total, metric

    def _evaluate_eager(self, model, loader):
        """(mean loss, predictions, labels) of the launch-by-launch pass."""
        predictions, labels = [], []
        total, num_data = 0.0, 0
        with torch.no_grad():
            model.eval()
            for data in loader:
                data, motif = self._to_device(data)
                pred, loss = self._step(model, data, motif)
                total += loss.item() * data.y.size(0)
                num_data += data.y.size(0)
                if self.normalizer:
                    pred = self.normalizer.denorm(pred)
                predictions.append(pred.cpu().numpy())
                labels.append(data.y.cpu().flatten().numpy())
            self.check_inputs()
        model.train()
        total /= max(num_data, 1)
        return total, np.concatenate(predictions), np.concatenate(labels)

    def _test(self, model, test_loader):
        model_path = os.path.join(self.log_dir, 'checkpoints', 'model.pth')
        state_dict = torch.load(model_path, map_location=self.device, weights_only=True)
        with torch.no_grad():  # in place: the parameters stay FusedAdam's views
            model.load_state_dict(state_dict)
        print("Loaded trained model with success.")
        _, metric = self._evaluate(model, test_loader, 'Test')
        if self.task == 'classification':
            self.roc_auc = metric
        elif self.config['task_name'] in MAE_TASKS:
            self.mae = metric
        else:
            self.rmse = metric
        return metric


def run(config):
    from .dataset_test import MolTestDatasetWrapper
    dataset = MolTestDatasetWrapper(config['batch_size'], **config['dataset'])
    fine_tune = FineTune(dataset, config)
    fine_tune.train()
    if config['dataset']['task'] == 'classification':
        return fine_tune.roc_auc
    return fine_tune.mae if config['task_name'] in MAE_TASKS else fine_tune.rmse


def main(config_path: str = "config_finetune.yaml"):
    """finetune.py:398-506: one run per target column of ``task_name``.  A
    config whose ``dataset`` already names ``task``, ``data_path`` and
    ``target`` (any CSV with a ``smiles`` column) runs that alone."""
    with open(config_path, "r") as f:
        config = yaml.safe_load(f)
    ds = config['dataset']
    if all(k in ds for k in ('task', 'data_path', 'target')):
        targets = [ds['target']]
    elif config['task_name'] in BENCHMARKS:
        ds['task'], ds['data_path'], targets = BENCHMARKS[config['task_name']]
    else:
        raise ValueError('Undefined downstream task!')
    print(config)
    results = []
    for target in targets:
        ds['target'] = target
        results.append([target, run(config)])
    os.makedirs('experiments', exist_ok=True)
    out = 'experiments/{}_{}_finetune.csv'.format(config['fine_tune_from'], config['task_name'])
    with open(out, 'a') as f:
        for target, result in results:
            f.write(f'{target},{result}\n')
    return results


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "config_finetune.yaml")
