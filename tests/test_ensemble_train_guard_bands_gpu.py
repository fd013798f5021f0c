"""Guard-band cases (tests/guard_bands.py) of the DatasetGAN training entries (csrc/pixel_ensemble_train.h): operands, results
and workspaces between 0xFF bands, results born NaN.  References and bounds as tests/test_ensemble_train_gpu.py: gather
1e-6 * max|feature|, the two GEMMs 2e-5 * max|ref|, the tail against the float64 model (1e-4 of max|ref|, the label pass's bound)."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import guard_bands as G
from test_guard_bands_gpu import T, _mk, _rel

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_session():
    G.reset()
    yield
    G.reset()


def test_gather(device, monkeypatch):
    import sis_hip
    t = T(device, monkeypatch)
    gen = torch.Generator().manual_seed(3)
    layers = [_mk(gen, 2, 32, r, r) for r in (4, 16, 8)]
    pixels = torch.stack([torch.randint(0, 2, (77,), generator=gen), torch.randint(0, 16, (77,), generator=gen),
                          torch.randint(0, 16, (77,), generator=gen)], 1).int()
    pixels[:4] = torch.tensor([[0, 0, 0], [1, 0, 15], [0, 15, 0], [1, 15, 15]])
    ref = torch.cat([F.interpolate(a.double(), size=(16, 16), mode="bilinear", align_corners=False) for a in layers], 1)
    ref = ref[pixels[:, 0].long(), :, pixels[:, 1].long(), pixels[:, 2].long()]
    got = t.run(sis_hip.pe_train_gather, [t.put(a) for a in layers], t.put(pixels), 16)
    assert _rel(got, ref) <= 1e-6, _rel(got, ref)


@pytest.mark.parametrize("pixels,features,members", [(130, 96, 2), (128, 32, 1)])   # a partial row tile; full tiles only
def test_l1_forward(device, monkeypatch, pixels, features, members):
    import sis_hip
    t = T(device, monkeypatch)
    gen = torch.Generator().manual_seed(pixels)
    x, w, b = _mk(gen, pixels, features), _mk(gen, members * 128, features), _mk(gen, members * 128)
    got = t.run(sis_hip.pe_train_l1_forward, t.put(x), t.put(w), t.put(b))
    assert _rel(got, torch.relu(x.double() @ w.double().t() + b.double())) <= 2e-5


@pytest.mark.parametrize("pixels,features,members", [(130, 96, 2),     # partial K chunk, a feature tile of 96 of 128 columns
                                                      (2100, 160, 1)])  # two slabs in the workspace, the second one partial
def test_l1_wgrad(device, monkeypatch, pixels, features, members):
    import sis_hip
    t = T(device, monkeypatch)
    gen = torch.Generator().manual_seed(pixels)
    x, dz = _mk(gen, pixels, features), _mk(gen, pixels, members * 128)
    dw, db = t.run(sis_hip.pe_train_l1_wgrad, t.put(dz), t.put(x))
    assert _rel(dw, dz.double().t() @ x.double()) <= 2e-5 and _rel(db, dz.double().sum(0)) <= 2e-5


@pytest.mark.parametrize("pixels,members,classes", [(131, 2, 3), (300, 1, 31)])   # partial tiles of every tail kernel
def test_tail(device, monkeypatch, pixels, members, classes):
    """The float64 reference is the model's own tail: ReLU output a1 -> BatchNorm1d -> Linear -> ReLU -> BatchNorm1d -> Linear ->
    nn.CrossEntropyLoss, differentiated by autograd down to a1 and gated by a1 > 0."""
    import sis_hip
    t = T(device, monkeypatch)
    gen = torch.Generator().manual_seed(pixels)
    a1 = torch.relu(_mk(gen, pixels, members * 128))
    labels = torch.randint(0, classes, (pixels,), generator=gen)
    params = {"g1": 1 + 0.2 * _mk(gen, members, 128), "be1": 0.2 * _mk(gen, members, 128), "w2": 0.2 * _mk(gen, members, 32, 128),
              "b2": 0.2 * _mk(gen, members, 32), "g2": 1 + 0.2 * _mk(gen, members, 32), "be2": 0.2 * _mk(gen, members, 32),
              "w3": 0.3 * _mk(gen, members, classes, 32), "b3": 0.2 * _mk(gen, members, classes)}
    running = {"mean1": _mk(gen, members, 128), "var1": 1 + torch.rand(members, 128, generator=gen), "mean2": _mk(gen, members, 32),
               "var2": 1 + torch.rand(members, 32, generator=gen), "tracked1": torch.full((members,), 4, dtype=torch.int64),
               "tracked2": torch.full((members,), 9, dtype=torch.int64)}
    dev_running = {k: t.put(v, inplace=True) for k, v in running.items()}
    out = t.run(sis_hip.pe_train_tail, t.put(a1), t.put(labels), {k: t.put(v) for k, v in params.items()}, classes,
                running=dev_running, want_logits=True)
    for n in range(members):
        bn1, lin2, bn2, lin3 = nn.BatchNorm1d(128), nn.Linear(128, 32), nn.BatchNorm1d(32), nn.Linear(32, classes)
        net = nn.Sequential(bn1, lin2, nn.ReLU(), bn2, lin3).double()
        with torch.no_grad():
            for mod, w, b in ((bn1, "g1", "be1"), (lin2, "w2", "b2"), (bn2, "g2", "be2"), (lin3, "w3", "b3")):
                mod.weight.copy_(params[w][n])
                mod.bias.copy_(params[b][n])
            for mod, m, v in ((bn1, "mean1", "var1"), (bn2, "mean2", "var2")):
                mod.running_mean.copy_(running[m][n])
                mod.running_var.copy_(running[v][n])
        a = a1[:, n * 128:(n + 1) * 128].double().requires_grad_()
        logits = net(a)
        loss = nn.CrossEntropyLoss()(logits, labels)
        loss.backward()
        bound = 1e-4
        assert _rel(out["logits"][n], logits) <= bound and abs(out["loss"][n].item() - loss.item()) <= bound * logits.abs().max().item()
        assert _rel(out["dz1"][:, n * 128:(n + 1) * 128], a.grad * (a > 0)) <= bound
        for mod, w, b in ((bn1, "g1", "be1"), (lin2, "w2", "b2"), (bn2, "g2", "be2"), (lin3, "w3", "b3")):
            assert _rel(out["grads"]["d" + w][n], mod.weight.grad) <= bound, w
            assert _rel(out["grads"]["d" + b][n], mod.bias.grad) <= bound, b
        for mod, m, v in ((bn1, "mean1", "var1"), (bn2, "mean2", "var2")):
            assert _rel(dev_running[m][n], mod.running_mean) <= 1e-6 and _rel(dev_running[v][n], mod.running_var) <= 1e-6
    assert dev_running["tracked1"].tolist() == [5] * members and dev_running["tracked2"].tolist() == [10] * members
