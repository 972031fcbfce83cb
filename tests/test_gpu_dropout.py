"""Dropout inside the encoder executors (molclr_amd/csrc/dropout.h) on the GPU.

The mask is a pure function of (seed, call, layer, row, column unit), so the
tests export the kernels' own masks (molclr_dropout_mask), check them against
the numpy restatement (tests/philox.py), and feed them to the fp64 oracle in
place of F.dropout: the executors' forward and backward are then held to the
bounds tests/test_gpu_models.py and tests/test_gpu_bf16.py hold the dropout-0
models to."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import oracle.reference_cpu as ref_cpu
from molclr_amd import ops
from molclr_amd.dataset import SyntheticPairBatches, collate_views, random_molecule
from oracle.reference_cpu import RefGCN, RefGINet

from . import philox
from .test_gpu_bf16 import BF16_TOL
from .test_gpu_models import TOL, check_grads, pre_bn_bias, rel

pytestmark = pytest.mark.gpu
FEAT = 128
SEED = -0x1234567890ABCDEF  # a seed with both halves set (and the sign bit)


def star(centre_neighbours=6):
    """A centre atom with 6 neighbours: its row walks the CSR (degree > 4)."""
    n = centre_neighbours + 1
    x = np.stack([np.full(n, 5), np.zeros(n, dtype=np.int64)], 1).astype(np.int64)
    row = np.empty(2 * (n - 1), dtype=np.int64)
    col = np.empty(2 * (n - 1), dtype=np.int64)
    row[0::2], col[0::2] = 0, np.arange(1, n)
    row[1::2], col[1::2] = np.arange(1, n), 0
    attr = np.zeros((2 * (n - 1), 2), dtype=np.int64)
    attr[:, 0] = np.repeat(np.arange(n - 1) % 4, 2)
    return x, np.stack([row, col]), attr


def batch7(seed=5):
    """tests/test_gpu_finetune.py's batch6 plus the star."""
    rng = np.random.default_rng(seed)
    mols = [random_molecule(rng) for _ in range(6)]
    return collate_views([(m.x, m.edge_index, m.edge_attr) for m in mols] + [star()])


def state(dev, call=0, seed=SEED):
    return torch.tensor([seed, call], dtype=torch.long, device=dev)


class MaskFeed:
    """F.dropout for the oracle: h * mask_l / (1 - p) with the kernels' masks,
    consumed in layer order; view(rows) starts a forward over those rows."""

    def __init__(self, masks, p):
        self.masks, self.p = [m.cpu() for m in masks], p
        self.view(slice(None))

    def view(self, rows):
        self.rows, self.layer = rows, 0

    def __call__(self, h, p=0.5, training=True, inplace=False):
        assert training and p == self.p
        m = self.masks[self.layer][self.rows, :h.shape[1]]
        self.layer += 1
        assert m.shape == h.shape
        return h * m.to(h.dtype) / (1 - p)


def export_masks(model, p, N):
    """The masks of the model's NEXT training forward, one per layer, at the
    executor's (padded) width."""
    D = model.emb_dim + model._dim_pad()
    return [ops.dropout_mask(model.dropout_state, l, p, N, D) for l in range(model.num_layer)]


# ---------------------------------------------------------------------------
# the mask itself
# ---------------------------------------------------------------------------
N_MASK, D_MASK, P_MASK = 4096, 64, 0.3


@pytest.fixture(scope="module")
def masks(dev):
    """{(layer, call): [N, D] uint8 from molclr_dropout_mask}, computed once."""
    return {(l, c): ops.dropout_mask(state(dev, c), l, P_MASK, N_MASK, D_MASK).cpu().numpy()
            for l in (0, 1) for c in (0, 1)}


def test_mask_matches_numpy_restatement(dev, masks):
    for (l, c), m in masks.items():
        want = philox.dropout_mask(SEED, c, l, P_MASK, N_MASK, D_MASK)
        assert m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1}
        assert np.array_equal(m, want), (l, c, int((m != want).sum()))
    # the high counter word reaches the key: call 2^32 is not call 0
    hi = ops.dropout_mask(state(dev, 1 << 32), 0, P_MASK, 64, D_MASK).cpu().numpy()
    assert np.array_equal(hi, philox.dropout_mask(SEED, 1 << 32, 0, P_MASK, 64, D_MASK))
    assert not np.array_equal(hi, masks[(0, 0)][:64])


def test_mask_statistics(masks):
    n = N_MASK * D_MASK
    bound = 5 * math.sqrt(P_MASK * (1 - P_MASK) / n)  # 0.0045 at n = 262144
    for key, m in masks.items():
        kept = m.mean()
        print(f"mask {key}: kept share {kept:.5f} (bound {bound:.5f} around {1 - P_MASK})")
        assert abs(kept - (1 - P_MASK)) < bound, key


def test_masks_independent_across_layers_and_calls(masks):
    n = N_MASK * D_MASK
    q = P_MASK ** 2 + (1 - P_MASK) ** 2  # two independent masks agree on this share
    bound = 5 * math.sqrt(q * (1 - q) / n)
    for a, b in (((0, 0), (1, 0)), ((0, 0), (0, 1)), ((1, 0), (1, 1)), ((0, 1), (1, 1))):
        agree = (masks[a] == masks[b]).mean()
        print(f"masks {a} / {b}: agree on {agree:.5f} (bound {bound:.5f} around {q:.2f})")
        assert abs(agree - q) < bound, (a, b)  # a key blind to layer or call: 1.0


def test_next_key_returns_the_state_and_advances_by_one(dev):
    from molclr_amd import _lib
    st = state(dev, call=41)
    key = torch.zeros(2, dtype=torch.long, device=dev)
    for k in (41, 42):
        _lib.call("molclr_dropout_next_key", st.data_ptr(), key.data_ptr(), _lib.stream_of(dev))
        assert key.tolist() == [SEED, k] and st.tolist() == [SEED, k + 1]


# ---------------------------------------------------------------------------
# the executors against the fp64 oracle with the kernels' own masks
# ---------------------------------------------------------------------------
def ref_finetune(kind, L, D, p):
    """tests/test_gpu_finetune.py's ref_model (classification) with the
    reference's dropout after every BatchNorm (models/ginet_finetune.py)."""
    base = RefGINet if kind == "gin" else RefGCN

    class Ref(base):
        def __init__(self):
            super().__init__(L, D, FEAT, drop_ratio=p)
            del self.out_lin
            head = [nn.Linear(FEAT, FEAT // 2), nn.Softplus()]
            if kind == "gin":
                head += [nn.Linear(FEAT // 2, FEAT // 2), nn.Softplus()]
            head.append(nn.Linear(FEAT // 2, 2))
            setattr(self, "pred_head" if kind == "gin" else "pred_lin", nn.Sequential(*head))

        def forward(self, data):
            h = self.x_embedding1(data.x[:, 0]) + self.x_embedding2(data.x[:, 1])
            for l in range(self.num_layer):
                h = self.batch_norms[l](self.gnns[l](h, data.edge_index, data.edge_attr))
                if l != self.num_layer - 1:
                    h = F.relu(h)
                h = ref_cpu.F.dropout(h, self.drop_ratio, training=self.training)
            h = self.feat_lin(self.pool(h, data.batch))
            return h, (self.pred_head if kind == "gin" else self.pred_lin)(h)

    return Ref()


def mine_finetune(kind, L, D, p, **kw):
    from molclr_amd.gcn_finetune import GCN
    from molclr_amd.ginet_finetune import GINet
    if kind == "gin":
        return GINet("classification", L, D, FEAT, p, **kw)
    return GCN("classification", L, D, FEAT, p)


def targets(n, seed=2):
    return torch.randint(0, 2, (n,), generator=torch.Generator().manual_seed(seed))


def err32_of(ref, ref64):
    g64 = dict(ref64.named_parameters())
    out = {}
    for n, p in ref.named_parameters():  # the reference's own fp32 error
        e = (p.grad.double() - g64[n].grad).norm().item()
        out[n] = {"err32": e, "err32_identity": e}
    return out


FT_CASES = [("gin", 2, 64), ("gin", 3, 64), ("gcn", 2, 64), ("gin", 2, 62), ("gcn", 2, 62)]
P = 0.3


@pytest.mark.parametrize("kind,L,D", FT_CASES)
def test_finetune_model_matches_oracle_under_its_masks(dev, monkeypatch, kind, L, D):
    torch.manual_seed(0)
    ref = ref_finetune(kind, L, D, P)
    ref64 = copy.deepcopy(ref).double()
    mine = mine_finetune(kind, L, D, P)
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(dev).train()
    data = batch7()
    t = targets(7)
    N = data.x.shape[0]
    mine.dropout_state = state(dev, call=3)
    feed = MaskFeed(export_masks(mine, P, N), P)
    monkeypatch.setattr(ref_cpu.F, "dropout", feed)

    feed.view(slice(None))
    _, pr = ref(data)
    F.cross_entropy(pr, t).backward()
    feed.view(slice(None))
    h6, p6 = ref64(data)
    l6 = F.cross_entropy(p6, t)
    l6.backward()
    assert mine._executor_ok()
    hm, pm, lm = mine.loss(data.to(dev), t.to(dev))
    lm.backward()
    assert mine.dropout_state.tolist() == [SEED, 4]
    print(f"{kind} L={L} D={D}: h {rel(hm, h6):.2e} pred {rel(pm, p6):.2e} loss {rel(lm, l6):.2e}")
    assert rel(hm, h6) < TOL and rel(pm, p6) < TOL and rel(lm, l6) < TOL
    check_grads(mine, ref64, err32_of(ref, ref64), record=f"finetune_{kind}")
    for name, buf in ref.named_buffers():
        assert rel(dict(mine.named_buffers())[name].float(), buf.float()) < TOL, name


@pytest.mark.parametrize("kind,L,D", [("gin", 3, 64), ("gcn", 2, 64)])
def test_paired_forward_matches_oracle_under_its_masks(dev, monkeypatch, kind, L, D):
    """forward_pair: per-view BatchNorm segments, the mask's row is the row in
    the union of both views."""
    from molclr_amd.gcn_molclr import GCN
    from molclr_amd.ginet_molclr import GINet
    torch.manual_seed(1)
    ref = (RefGINet if kind == "gin" else RefGCN)(L, D, FEAT, drop_ratio=P)
    ref64 = copy.deepcopy(ref).double()
    mine = (GINet if kind == "gin" else GCN)(L, D, FEAT, drop_ratio=P)
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(dev).train()
    xi, xj = batch7(5), batch7(6)
    ni, nj = xi.x.shape[0], xj.x.shape[0]
    mine.dropout_state = state(dev)
    feed = MaskFeed(export_masks(mine, P, ni + nj), P)
    monkeypatch.setattr(ref_cpu.F, "dropout", feed)

    def both(model):
        feed.view(slice(0, ni))
        hi, oi = model(xi)
        feed.view(slice(ni, ni + nj))
        hj, oj = model(xj)
        return torch.cat([hi, hj]), torch.cat([oi, oj])

    h_r, out_r = both(ref)
    h_6, out_6 = both(ref64)
    h_m, out_m = mine.forward_pair(xi.to(dev), xj.to(dev))
    print(f"paired {kind}: h {rel(h_m, h_6):.2e} out {rel(out_m, out_6):.2e}")
    assert rel(h_m, h_6) < TOL and rel(out_m, out_6) < TOL
    torch.manual_seed(3)
    w1, w2 = torch.randn_like(h_r), torch.randn_like(out_r)
    ((h_r * w1).sum() + (out_r * w2).sum()).backward()
    ((h_6 * w1.double()).sum() + (out_6 * w2.double()).sum()).backward()
    ((h_m * w1.to(dev)).sum() + (out_m * w2.to(dev)).sum()).backward()
    check_grads(mine, ref64, err32_of(ref, ref64), record=f"{kind}_paired")
    for name, buf in ref.named_buffers():
        assert rel(dict(mine.named_buffers())[name].float(), buf.float()) < TOL, name


def test_bf16_matches_oracle_under_its_masks(dev, monkeypatch):
    """precision='bf16' with dropout, held to tests/test_gpu_bf16.py's bounds
    for the fp64 reference (h, out, loss, worst gradient)."""
    L, D = 2, 64
    torch.manual_seed(0)
    ref64 = ref_finetune("gin", L, D, P).double()
    mine = mine_finetune("gin", L, D, P, precision="bf16")
    mine.load_state_dict({k: v.float() if v.is_floating_point() else v
                          for k, v in ref64.state_dict().items()})
    mine = mine.to(dev).train()
    data = batch7()
    t = targets(7)
    mine.dropout_state = state(dev, call=1)
    feed = MaskFeed(export_masks(mine, P, data.x.shape[0]), P)
    monkeypatch.setattr(ref_cpu.F, "dropout", feed)
    h6, p6 = ref64(data)
    l6 = F.cross_entropy(p6, t)
    l6.backward()
    hm, pm, lm = mine.loss(data.to(dev), t.to(dev))
    lm.backward()
    g64 = dict(ref64.named_parameters())
    gerr = {n: rel(p.grad, g64[n].grad) for n, p in mine.named_parameters() if not pre_bn_bias(n)}
    errs = {"h": rel(hm, h6), "out": rel(pm, p6), "loss": rel(lm, l6), "grad": max(gerr.values())}
    print("bf16 with dropout:", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v < BF16_TOL[k], (k, v, sorted(gerr.items(), key=lambda kv: -kv[1])[:4])


# ---------------------------------------------------------------------------
# determinism, freshness, eval, exact zeros
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("gin", "gcn"))
def test_fresh_masks_replayable_and_eval_unchanged(dev, kind):
    torch.manual_seed(4)
    m = mine_finetune(kind, 2, 64, 0.3).to(dev).train()
    data = batch7().to(dev)
    h1, _ = m(data)
    assert m.dropout_state is not None and int(m.dropout_state[1]) == 1
    h2, _ = m(data)
    assert int(m.dropout_state[1]) == 2 and not torch.equal(h1, h2)
    m.dropout_state[1] = 0
    h3, _ = m(data)
    assert torch.equal(h1, h3)
    # torch.manual_seed repeats the lazily drawn seed
    torch.manual_seed(8)
    m.dropout_state = None
    m(data)
    s = int(m.dropout_state[0])
    torch.manual_seed(8)
    m.dropout_state = None
    m(data)
    assert int(m.dropout_state[0]) == s
    # eval: no dropout, the outputs of a drop_ratio = 0 copy
    plain = mine_finetune(kind, 2, 64, 0.0).to(dev)
    plain.load_state_dict(m.state_dict())
    m.eval()
    plain.eval()
    before = m.dropout_state.clone()
    with torch.no_grad():
        (ha, pa), (hb, pb) = m(data), plain(data)
    assert torch.equal(ha, hb) and torch.equal(pa, pb)
    assert torch.equal(m.dropout_state, before)


def test_exact_zeros_where_the_mask_drops(dev):
    """One GIN layer: the stored-h apply of the last layer (no ReLU).  h == 0
    exactly where the exported mask is 0; elsewhere h is 1 / (1 - p) x the
    BatchNorm output of a dropout-free twin on the same input."""
    from molclr_amd.ginet_molclr import GINet
    p = 0.3
    torch.manual_seed(5)
    m = GINet(1, 64, FEAT, drop_ratio=p).to(dev).train()
    plain = copy.deepcopy(m)
    plain.drop_ratio = 0.0
    data = batch7().to(dev)
    m.dropout_state = state(dev, 6)
    keep = export_masks(m, p, data.x.shape[0])[0].bool()
    h, _ = m.encode(data)
    y, _ = plain.encode(data)
    assert bool((h[~keep] == 0).all()) and bool((y[~keep] != 0).any())
    assert rel(h[keep], y[keep] / (1 - p)) < TOL


# ---------------------------------------------------------------------------
# the captured training step
# ---------------------------------------------------------------------------
def test_captured_step_with_dropout_follows_eager(dev):
    """tests/test_gpu_graph_step.py::test_captured_step_follows_eager with
    drop_ratio = 0.2: a deep-copied twin with the same dropout_state, stepped
    eagerly from the same state, lands on the same loss, gradients and
    parameters; every replay advances the device counter by one."""
    from molclr_amd.ginet_molclr import GINet
    from molclr_amd.graph_step import CapturedTrainStep
    from molclr_amd.nt_xent import NTXentLoss
    from molclr_amd.optim import FusedAdam

    from .test_gpu_graph_step import _eager_step, _sync, _to
    B = 8
    batches = [_to(p, dev) for p in SyntheticPairBatches(B, seed=11).take(3)]
    torch.manual_seed(5)
    ref = GINet(num_layer=2, emb_dim=64, feat_dim=64, drop_ratio=0.2).to(dev)
    cap = copy.deepcopy(ref)
    cap.dropout_state = state(dev)
    ref.dropout_state = state(dev)
    opt_r = FusedAdam(ref.parameters(), 5e-4, weight_decay=1e-5)
    opt_c = FusedAdam(cap.parameters(), 5e-4, weight_decay=1e-5)
    crit = NTXentLoss(dev, B, 0.1, True)
    step = CapturedTrainStep(cap, opt_c, crit, node_quantum=128, edge_quantum=512, node_slack=0)
    for i, (xi, xj) in enumerate(batches):
        _sync(ref, opt_r, cap, opt_c)
        lr_ = _eager_step(ref, opt_r, crit, xi, xj)
        lc = step(xi, xj).clone()
        torch.cuda.synchronize()
        assert abs(lc.item() - lr_.item()) <= 1e-6 * abs(lr_.item()), (i, lc.item(), lr_.item())
        assert rel(opt_c.flat_grad, opt_r.flat_grad) < 1e-5, i
        for bc, br in zip(cap.batch_norms, ref.batch_norms):
            assert rel(bc.running_mean, br.running_mean) < 1e-6, i
            assert rel(bc.running_var, br.running_var) < 1e-6, i
        assert cap.dropout_state.tolist() == [SEED, i + 1] == ref.dropout_state.tolist()
    assert step.replays == 3 and step.captures >= 1
    assert int(cap.dropout_state[1]) == 3  # captures record, they run nothing
    worst = max((rel(pc, pr), n) for (n, pc), pr in zip(cap.named_parameters(), ref.parameters())
                if not pre_bn_bias(n))  # those: exact gradient 0, Adam steps on rounding noise
    print("parameters after 3 steps, worst:", worst)
    assert worst[0] < 1e-5, worst
