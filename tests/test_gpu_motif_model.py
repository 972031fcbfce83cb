"""The motif fine-tuning model and its trainer on the GPU against the oracle's
GIN encoder with the motif readout restated (tests/motif_ref.RefMotifGINet:
fp64 on the CPU, same weights), at the bounds tests/test_gpu_models.py holds
the pre-training models to."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from .motif_ref import RefMotifGINet
from .test_gpu_finetune import batch6, config_of, criterion, target_of, write_csv
from .test_gpu_models import TOL, check_grads, pre_bn_bias, rel

pytestmark = pytest.mark.gpu
L, FEAT, NUM = 2, 128, 9


def motif_args(seed=3):
    """0-4 motifs for each of the 6 molecules, in the reference's layout."""
    rng = np.random.default_rng(seed)
    counts = [0, 4, 1, 2, 3, 0]
    clique = np.concatenate([rng.choice(NUM, n, replace=False) for n in counts]).astype(np.int64)
    mol = np.concatenate([np.repeat(np.arange(6), counts), np.arange(6)])
    return torch.from_numpy(mol), torch.from_numpy(clique)


def mine_model(task, D, drop=0.0, **kw):
    from molclr_amd.ginet_finetune_mp import GINet
    return GINet(NUM, task, L, D, FEAT, drop, **kw)


@pytest.mark.parametrize("task,D", [("classification", 64), ("regression", 64),
                                    ("classification", 62), ("regression", 62)])
def test_model_matches_oracle(dev, task, D):
    torch.manual_seed(0)
    ref = RefMotifGINet(NUM, task, L, D, FEAT)
    ref64 = copy.deepcopy(ref).double()
    mine = mine_model(task, D)
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(dev)
    data, t = batch6(), target_of(task)
    mol, clique = motif_args()

    for m in (ref, ref64, mine):
        m.eval()
    with torch.no_grad():
        h6, p6 = ref64(data, mol, clique)
        hm, pm = mine(data.to(dev), mol.to(dev), clique.to(dev))
    assert hm.shape == (6, 2 * FEAT) and pm.shape == (6, 2 if task == "classification" else 1)
    assert rel(hm, h6) < TOL and rel(pm, p6) < TOL

    for m in (ref, ref64, mine):
        m.train()
    _, pr = ref(data, mol, clique)
    criterion(task, pr, t).backward()
    _, p6 = ref64(data, mol, clique)
    l6 = criterion(task, p6, t)
    l6.backward()
    hm, pm, lm = mine.loss(data.to(dev), mol.to(dev), clique.to(dev), t.to(dev))
    lm.backward()
    assert rel(lm, l6) < TOL and rel(pm, p6) < TOL
    g64 = dict(ref64.named_parameters())
    err32 = {}
    for n, p in ref.named_parameters():  # the reference's own fp32 error
        e = (p.grad.double() - g64[n].grad).norm().item()
        err32[n] = {"err32": e, "err32_identity": e}
    # The gate bias's gradient is the sum of d loss / d gate over each segment's
    # softmax: exactly 0, so fp64's own 1e-17 is rounding noise and no measure.
    # It is held to the absolute bound tests/test_gpu_motif_pool.py holds dc to.
    n = "motif_pool.gate_nn.0.bias"
    bound = 2 * err32[n]["err32"] + 1e-6 * ref64.gate_logits.grad.abs().sum().item()
    err32[n] = {"err32": bound, "err32_identity": bound}
    check_grads(mine, ref64, err32, record="finetune_gin_motif")
    for name, buf in ref.named_buffers():
        assert rel(dict(mine.named_buffers())[name].float(), buf.float()) < TOL, name


def test_pred_stays_differentiable_for_a_user_criterion(dev):
    torch.manual_seed(1)
    a = mine_model("classification", 64).to(dev)
    b = copy.deepcopy(a)
    data, t = batch6().to(dev), target_of("classification").to(dev)
    mol, clique = (x.to(dev) for x in motif_args())
    a.loss(data, mol, clique, t)[2].backward()
    F.cross_entropy(b(data, mol, clique)[1], t).backward()
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    for n in ga:
        assert gb[n].grad is not None, n
        if pre_bn_bias(n):
            continue
        assert (ga[n].grad - gb[n].grad).norm() <= 1e-5 * ga[n].grad.norm() + 1e-9, n


def test_dropout_training_and_eval(dev):
    torch.manual_seed(4)
    m = mine_model("classification", 64, drop=0.3).to(dev)
    data, t = batch6().to(dev), target_of("classification").to(dev)
    mol, clique = (x.to(dev) for x in motif_args())
    m.train()
    h, pred, loss = m.loss(data, mol, clique, t)
    loss.backward()
    assert torch.isfinite(h).all() and torch.isfinite(pred).all() and torch.isfinite(loss)
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    m.eval()
    with torch.no_grad():
        h1, p1 = m(data, mol, clique)
        h2, p2 = m(data, mol, clique)
    assert torch.equal(h1, h2) and torch.equal(p1, p2)


def test_bf16_precision_accepted_and_index_lengths_checked(dev):
    torch.manual_seed(6)
    m = mine_model("regression", 64, precision="bf16").to(dev)
    data, t = batch6().to(dev), target_of("regression").to(dev)
    mol, clique = (x.to(dev) for x in motif_args())
    h, pred, loss = m.loss(data, mol, clique, t)
    loss.backward()
    assert h.dtype == torch.float32 and pred.dtype == torch.float32 and torch.isfinite(loss)
    with pytest.raises(ValueError, match="mol_idx"):
        m(data, mol[:-1], clique)


def _trainer(tmp_path, **over):
    from molclr_amd.dataset_test import MolTestDatasetWrapper
    from molclr_amd.finetune import FineTune
    cfg = config_of(tmp_path, "classification", "gin_motif", epochs=2, **over)
    return FineTune(MolTestDatasetWrapper(cfg["batch_size"], **cfg["dataset"]), cfg)


def test_trainer_end_to_end_builtin_and_json(dev, tmp_path):
    from molclr_amd import motifs
    from molclr_amd.ginet_finetune import GINet as PlainGINet
    from molclr_amd.ginet_finetune_mp import GINet
    write_csv(tmp_path / "data.csv", "classification", n=120)
    ft = _trainer(tmp_path, motifs="builtin")
    model = ft.train()
    assert len(ft.epoch_train_loss) == 2 and np.isfinite(ft.epoch_train_loss).all()
    assert np.isfinite(ft.roc_auc)
    sd = torch.load(os.path.join(ft.log_dir, "checkpoints", "model.pth"), weights_only=True)
    for k in ("motif_embedding.weight", "motif_lin.weight", "motif_pool.gate_nn.0.bias"):
        assert k in sd
    fresh = GINet(len(ft.vocabulary), "classification", **ft.config["model"])
    fresh.load_state_dict(sd, strict=True)
    assert isinstance(model, GINet) and len(ft.vocabulary) > 3

    # the motif table starts as the plain model's h of the vocabulary's graphs
    smiles_data = ft.dataset.get_data_loaders()[0]
    torch.manual_seed(0)
    built = ft.build_model()
    torch.manual_seed(0)
    plain = PlainGINet("classification", **ft.config["model"]).to(dev)
    rows, feats = ft.embed_vocabulary(plain)
    assert rows.tolist() == list(range(len(ft.vocabulary)))
    assert torch.equal(built.motif_embedding.weight.detach(), feats)
    assert feats.shape == (len(ft.vocabulary), 128) and torch.isfinite(feats).all()

    # the JSON source written from the builtin assignments: the same first step
    path = tmp_path / "motifs.json"
    motifs.write_json(path, smiles_data, ft.vocabulary, ft.assignments)
    losses = []
    for source in ("builtin", str(path)):
        run = _trainer(tmp_path, motifs=source)
        torch.manual_seed(0)
        np.random.seed(0)
        _, loader, _, _ = run.dataset.get_data_loaders()
        run.load_motifs(smiles_data)
        m = run.build_model()
        data = next(iter(loader))
        data, motif = run._to_device(data)
        losses.append(run._step(m, data, motif)[1].item())
        run.check_inputs()
    assert np.isfinite(losses[0]) and losses[0] == losses[1]
