"""Fine-tuning models and trainer on the GPU against the oracle's encoders with
a torch head (fp64 on the CPU, same weights), at the bounds
tests/test_gpu_models.py holds the pre-training models to."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from molclr_amd.dataset import collate_views, random_molecule
from oracle.reference_cpu import RefGCN, RefGINet

from .test_gpu_models import TOL, check_grads, pre_bn_bias, rel

pytestmark = pytest.mark.gpu
L, FEAT = 2, 128


def ref_model(kind, task, D, pred_n_layer=2, act="softplus"):
    """The oracle's encoder + feat_lin with the reference's task head, under
    the product's parameter names."""
    base = RefGINet if kind == "gin" else RefGCN
    out_dim = 2 if task == "classification" else 1
    a = {"softplus": nn.Softplus, "relu": nn.ReLU}[act]

    class Ref(base):
        def __init__(self):
            super().__init__(L, D, FEAT)
            del self.out_lin
            head = [nn.Linear(FEAT, FEAT // 2), a()]
            for _ in range((pred_n_layer if kind == "gin" else 1) - 1):
                head += [nn.Linear(FEAT // 2, FEAT // 2), a()]
            head.append(nn.Linear(FEAT // 2, out_dim))
            setattr(self, "pred_head" if kind == "gin" else "pred_lin", nn.Sequential(*head))

        def forward(self, data):
            h = self.x_embedding1(data.x[:, 0]) + self.x_embedding2(data.x[:, 1])
            for l in range(self.num_layer):
                h = self.batch_norms[l](self.gnns[l](h, data.edge_index, data.edge_attr))
                if l != self.num_layer - 1:
                    h = F.relu(h)
            h = self.feat_lin(self.pool(h, data.batch))
            return h, (self.pred_head if kind == "gin" else self.pred_lin)(h)

    return Ref()


def mine_model(kind, task, D, drop=0.0, **kw):
    from molclr_amd.gcn_finetune import GCN
    from molclr_amd.ginet_finetune import GINet
    if kind == "gin":
        return GINet(task, L, D, FEAT, drop, **kw)
    return GCN(task, L, D, FEAT, drop)


def batch6(seed=5):
    rng = np.random.default_rng(seed)
    mols = [random_molecule(rng) for _ in range(6)]
    return collate_views([(m.x, m.edge_index, m.edge_attr) for m in mols])


def target_of(task, seed=2):
    g = torch.Generator().manual_seed(seed)
    if task == "classification":
        return torch.randint(0, 2, (6,), generator=g)
    return torch.randn(6, 1, generator=g)


def criterion(task, pred, t):
    return F.cross_entropy(pred, t) if task == "classification" else F.mse_loss(pred, t.to(pred.dtype))


CASES = [("gin", "classification", 64), ("gin", "regression", 64), ("gcn", "classification", 64),
         ("gcn", "regression", 64), ("gin", "classification", 62), ("gcn", "regression", 62)]


@pytest.mark.parametrize("kind,task,D", CASES)
def test_model_matches_oracle(dev, kind, task, D):
    torch.manual_seed(0)
    ref = ref_model(kind, task, D)
    ref64 = copy.deepcopy(ref).double()
    mine = mine_model(kind, task, D)
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(dev)
    data, t = batch6(), target_of(task)

    # eval mode: (h, pred)
    for m in (ref, ref64, mine):
        m.eval()
    with torch.no_grad():
        h6, p6 = ref64(data)
        hm, pm = mine(data.to(dev))
    assert hm.shape == (6, FEAT) and pm.shape == (6, 2 if task == "classification" else 1)
    assert rel(hm, h6) < TOL and rel(pm, p6) < TOL

    # training mode, dropout 0: loss and every parameter gradient
    for m in (ref, ref64, mine):
        m.train()
    _, pr = ref(data)
    criterion(task, pr, t).backward()
    _, p6 = ref64(data)
    l6 = criterion(task, p6, t)
    l6.backward()
    hm, pm, lm = mine.loss(data.to(dev), t.to(dev))
    lm.backward()
    assert rel(lm, l6) < TOL and rel(pm, p6) < TOL
    g64 = dict(ref64.named_parameters())
    err32 = {}
    for n, p in ref.named_parameters():  # the reference's own fp32 error
        e = (p.grad.double() - g64[n].grad).norm().item()
        err32[n] = {"err32": e, "err32_identity": e}
    check_grads(mine, ref64, err32, record=f"finetune_{kind}")
    for name, buf in ref.named_buffers():
        assert rel(dict(mine.named_buffers())[name].float(), buf.float()) < TOL, name


def test_pred_stays_differentiable_for_a_user_criterion(dev):
    """criterion(pred, y) in user code gives the gradients of model.loss."""
    torch.manual_seed(1)
    a = mine_model("gin", "classification", 64).to(dev)
    b = copy.deepcopy(a)
    data, t = batch6().to(dev), target_of("classification").to(dev)
    a.loss(data, t)[2].backward()
    F.cross_entropy(b(data)[1], t).backward()
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    for n in ga:
        assert gb[n].grad is not None, n
        if pre_bn_bias(n):  # exact gradient 0: rounding noise on both sides
            continue
        assert (ga[n].grad - gb[n].grad).norm() <= 1e-5 * ga[n].grad.norm() + 1e-9, n


@pytest.mark.parametrize("kind", ("gin", "gcn"))
def test_dropout_training_and_eval(dev, kind):
    torch.manual_seed(4)
    m = mine_model(kind, "classification", 64, drop=0.3).to(dev)
    data, t = batch6().to(dev), target_of("classification").to(dev)
    m.train()
    h, pred, loss = m.loss(data, t)
    loss.backward()
    assert torch.isfinite(h).all() and torch.isfinite(pred).all() and torch.isfinite(loss)
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    m.eval()
    with torch.no_grad():
        h1, p1 = m(data)
        h2, p2 = m(data)
    assert torch.equal(h1, h2) and torch.equal(p1, p2)


def test_bf16_precision_accepted(dev):
    from molclr_amd.ginet_finetune import GINet
    torch.manual_seed(6)
    m = GINet("regression", L, 64, FEAT, precision="bf16").to(dev)
    h, pred, loss = m.loss(batch6().to(dev), target_of("regression").to(dev))
    loss.backward()
    assert h.dtype == torch.float32 and pred.dtype == torch.float32 and torch.isfinite(loss)


FRAGS = ["C", "CC", "N", "O", "C(C)", "C(=O)", "c1ccccc1", "C(N)", "C(O)"]


def write_csv(path, task, n=260, seed=0):
    """Synthetic labelled SMILES: 1 if the molecule contains nitrogen, or the
    heavy-atom count."""
    from molclr_amd.smiles import featurise
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        f.write("smiles,label\n")
        f.write("C,0\n")  # the first data row is skipped, as in the reference
        for _ in range(n):
            s = "".join(FRAGS[i] for i in rng.integers(0, len(FRAGS), rng.integers(2, 7)))
            y = int("N" in s) if task == "classification" else featurise(s).x.shape[0]
            f.write(f"{s},{y}\n")
    return str(path)


def config_of(tmp_path, task, kind="gin", **over):
    cfg = {
        "batch_size": 32, "epochs": 3, "eval_every_n_epochs": 1, "fine_tune_from": "none",
        "log_every_n_steps": 4, "fp16_precision": False, "init_lr": 3e-3, "init_base_lr": 3e-3,
        "weight_decay": "1e-6", "gpu": "cuda:0", "seed": 0,
        "task_name": "BBBP" if task == "classification" else "ESOL", "model_type": kind,
        "model": {"num_layer": 2, "emb_dim": 64, "feat_dim": 128, "drop_ratio": 0,
                  "pool": "mean" if task == "classification" else "add"},
        "dataset": {"num_workers": 0, "valid_size": 0.1, "test_size": 0.1, "splitting": "random",
                    "task": task, "data_path": str(tmp_path / "data.csv"), "target": "label"},
        "log_root": str(tmp_path / "runs"), "ckpt_root": str(tmp_path / "ckpt"),
    }
    cfg.update(over)
    return cfg


@pytest.mark.parametrize("task,kind", [("classification", "gin"), ("regression", "gcn")])
def test_trainer_learns_and_tests_from_the_checkpoint(dev, tmp_path, task, kind):
    from molclr_amd.dataset_test import MolTestDatasetWrapper
    from molclr_amd.finetune import FineTune
    write_csv(tmp_path / "data.csv", task)
    cfg = config_of(tmp_path, task, kind)
    ft = FineTune(MolTestDatasetWrapper(cfg["batch_size"], **cfg["dataset"]), cfg)
    ft.train()
    assert len(ft.epoch_train_loss) == 3
    print("epoch losses", ft.epoch_train_loss)
    assert ft.epoch_train_loss[-1] < ft.epoch_train_loss[0]
    assert os.path.exists(os.path.join(ft.log_dir, "checkpoints", "model.pth"))
    if task == "classification":
        print("roc_auc", ft.roc_auc)
        assert np.isfinite(ft.roc_auc) and ft.roc_auc > 0.5
    else:
        print("rmse", ft.rmse)
        assert np.isfinite(ft.rmse)


def test_trainer_loads_a_pretraining_checkpoint_and_checks_labels(dev, tmp_path):
    from molclr_amd.dataset_test import collate_labelled
    from molclr_amd.data import Data
    from molclr_amd.finetune import FineTune
    from molclr_amd.ginet_molclr import GINet as PreGINet
    torch.manual_seed(9)
    pre = PreGINet(num_layer=2, emb_dim=64, feat_dim=128)
    for bn in pre.batch_norms:
        bn.running_mean.uniform_(-1, 1)
    folder = tmp_path / "ckpt" / "pre" / "checkpoints"
    folder.mkdir(parents=True)
    torch.save(pre.state_dict(), folder / "model.pth")
    ft = FineTune(None, config_of(tmp_path, "classification", fine_tune_from="pre"))
    model = ft.build_model()
    sd, own = pre.state_dict(), model.state_dict()
    shared = [k for k in sd if not k.startswith("out_lin.")]
    assert shared and set(shared) == {k for k in own if not k.startswith("pred_head.")}
    for k in shared:
        assert torch.equal(own[k].cpu(), sd[k]), k

    rng = np.random.default_rng(1)
    items = []
    for i, y in enumerate([0, 1, 5, 1]):  # 5: outside the two classes
        m = random_molecule(rng)
        items.append(Data(x=torch.from_numpy(m.x), edge_index=torch.from_numpy(m.edge_index),
                          edge_attr=torch.from_numpy(m.edge_attr),
                          y=torch.tensor([[y]], dtype=torch.long), mol_index=i))
    good = collate_labelled(items[:2] + items[3:]).to(dev)
    ft._step(model, good)
    ft.check_inputs()
    ft._step(model, collate_labelled(items).to(dev))
    with pytest.raises(ValueError, match="class label"):
        ft.check_inputs()
