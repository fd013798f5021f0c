"""DatasetGAN ensemble training on the device (csrc/pixel_ensemble_train.h, training/ensemble_step.py) against the float64 oracle
of tests/ensemble_train_checks.py.  Every test prints the figures it asserts on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ensemble_train_checks as C

pytestmark = pytest.mark.gpu


def _relmax(got, ref):
    d = (got.detach().double().cpu() - ref.detach().double().cpu()).abs().max().item()
    return (d if d == d else float("inf")) / max(ref.detach().double().abs().max().item(), 1e-300)


# ---------------------------------------------------------------------------------------------------- gather
def test_gather_matches_bilinear_upsampling(device):
    """Layers at 4^2, 8^2 and full 16^2, 32 channels each, two images; every pixel (the four corners and the edge rows among
    them) within 1e-6 * max|feature| of F.interpolate(bilinear, align_corners=False) in float64."""
    import sis_hip
    gen = torch.Generator().manual_seed(11)
    layers = [torch.randn(2, 32, r, r, generator=gen) for r in (4, 8, 16)]
    ref = torch.cat([F.interpolate(t.double(), size=(16, 16), mode="bilinear", align_corners=False) for t in layers], 1)
    img, y, x = torch.meshgrid(torch.arange(2), torch.arange(16), torch.arange(16), indexing="ij")
    pixels = torch.stack([img.reshape(-1), y.reshape(-1), x.reshape(-1)], 1)
    order = torch.randperm(pixels.shape[0], generator=gen)
    pixels = torch.cat([torch.tensor([[0, 0, 0], [0, 0, 15], [1, 15, 0], [1, 15, 15]]), pixels[order]]).int()
    got = sis_hip.pe_train_gather([t.to(device) for t in layers], pixels.to(device), 16)
    want = ref[pixels[:, 0].long(), :, pixels[:, 1].long(), pixels[:, 2].long()]
    err = (got.double().cpu() - want).abs().max().item()
    print(f"gather: max err {err:.3e}, bound {1e-6 * want.abs().max().item():.3e}")
    assert tuple(got.shape) == (516, 96) and err <= 1e-6 * want.abs().max().item()
    assert torch.equal(got[:, 64:].cpu(), layers[2][pixels[:, 0].long(), :, pixels[:, 1].long(), pixels[:, 2].long()])   # plain reads


# ---------------------------------------------------------------------------------------------------- the two GEMMs alone
SHAPES = [(4, 64, 1), (130, 96, 3), (257, 64, 10)]


@pytest.mark.parametrize("pixels,features,members", SHAPES)
def test_layer1_forward_alone(device, pixels, features, members):
    import sis_hip
    gen = torch.Generator().manual_seed(pixels + features)
    x, w, b = torch.randn(pixels, features, generator=gen), torch.randn(members * 128, features, generator=gen), torch.randn(members * 128, generator=gen)
    ref = torch.relu(x.double() @ w.double().t() + b.double())
    got = sis_hip.pe_train_l1_forward(x.to(device), w.to(device), b.to(device))
    err = _relmax(got, ref)
    print(f"l1 forward {(pixels, features, members)}: {err:.3e} of max|ref|")
    assert err <= 2e-5


@pytest.mark.parametrize("pixels,features,members", SHAPES + [(2100, 64, 1)])   # 2100: two slabs, the second one partial
def test_layer1_weight_gradient_alone(device, pixels, features, members):
    import sis_hip
    gen = torch.Generator().manual_seed(pixels + features + 1)
    x, dz = torch.randn(pixels, features, generator=gen), torch.randn(pixels, members * 128, generator=gen)
    dw, db = sis_hip.pe_train_l1_wgrad(dz.to(device), x.to(device))
    ew, eb = _relmax(dw, dz.double().t() @ x.double()), _relmax(db, dz.double().sum(0))
    print(f"l1 wgrad {(pixels, features, members)}: dW1 {ew:.3e}, db1 {eb:.3e} of max|ref|")
    assert ew <= 2e-5 and eb <= 2e-5


# ---------------------------------------------------------------------------------------------------- whole step
def _fused_run(device, seed, steps, pixels, features, members, classes, want_logits=False):
    """The fused counterpart of C.aten_steps."""
    from training.ensemble_step import FusedEnsembleStep
    e = C.make_ensemble(seed, classes, features, members, device=device)
    opts = C.make_optimizers(e)
    fused = FusedEnsembleStep(e, opts)
    p0 = {k: v.detach().clone() for k, v in fused.stacks.items()}
    out = []
    for step in range(steps):
        x, t = C.batch(seed, step, pixels, features, classes)
        loss, logits = fused.forward_backward(x.to(device), t.to(device), want_logits=want_logits)
        rec = {"loss": loss.clone(), "logits": logits, "grads": {k: v.clone() for k, v in fused.grads.items()}}
        for i in range(members):
            opts[f"optimizer_{i}"].step()
        rec["running"] = {k: fused.buffers[k].clone().view(members, -1) for k in C.RUNNING}
        rec["tracked"] = fused.buffers["tracked1"].tolist() + fused.buffers["tracked2"].tolist()
        out.append(rec)
    return out, p0, {k: v.detach().clone() for k, v in fused.stacks.items()}, e


@pytest.mark.parametrize("seed", C.GATE_SEEDS)
def test_whole_step_against_the_oracle(device, seed):
    """P = 64, F = 64, N = 3, 3 classes, 3 consecutive steps.  Gradients of all ten parameter kinds, running statistics, losses
    and the update p_3 - p_0: relative L2 error against the float64 oracle at most 8 x that of the ATen fp32 step on the device.
    The inputs keep every ReLU gate clear of zero (asserted on the oracle; nothing is excluded from the comparison)."""
    shape = dict(steps=3, pixels=64, features=64, members=3, classes=3)
    assert C.gates_clear(seed, **shape)
    oracle, o0, o3 = C.oracle_run(seed, *shape.values())
    e = C.make_ensemble(seed, 3, 64, 3, device=device)
    aten, a0, a3 = C.aten_steps(e, C.make_optimizers(e), seed, device=device, **shape)
    fused, f0, f3, _ = _fused_run(device, seed, **shape)
    failures = []

    def check(what, got, lib, ref):
        ef, ea = C.rel_l2(got, ref), C.rel_l2(lib, ref)
        print(f"seed {seed} {what}: fused {ef:.3e}, ATen fp32 {ea:.3e}")
        if not ef <= 8 * ea:
            failures.append((what, ef, ea))

    for s in range(3):
        for k in C.KINDS:
            for n in range(3):
                check(f"step {s} d{k}[{n}]", fused[s]["grads"][k][n], aten[s]["grads"][k][n], oracle[s]["grads"][k][n])
        for k in C.RUNNING:
            check(f"step {s} running {k}", fused[s]["running"][k], aten[s]["running"][k], oracle[s]["running"][k])
        check(f"step {s} loss", fused[s]["loss"], aten[s]["loss"], oracle[s]["loss"])
        assert fused[s]["tracked"] == [s + 1] * 6
    for k in C.KINDS:
        for n in range(3):
            check(f"update {k}[{n}]", (f3[k] - f0[k])[n], (a3[k] - a0[k])[n], (o3[k] - o0[k])[n])
    assert not failures, failures


@pytest.mark.parametrize("pixels", [2, 131])
def test_odd_pixel_counts(device, pixels):
    """P below one tile and P that is no multiple of it, N = 1: losses and logits within 1e-4 * max|logit| of the oracle."""
    oracle, _, _ = C.oracle_run(7, 1, pixels, 64, 1, 3)
    fused, _, _, e = _fused_run(device, 7, 1, pixels, 64, 1, 3, want_logits=True)
    bound = 1e-4 * oracle[0]["logits"].abs().max().item()
    el = (fused[0]["logits"].double().cpu() - oracle[0]["logits"]).abs().max().item()
    eo = (fused[0]["loss"].double().cpu() - oracle[0]["loss"]).abs().max().item()
    print(f"P = {pixels}: logits {el:.3e}, loss {eo:.3e}, bound {bound:.3e}")
    assert el <= bound and eo <= bound
    m = e.networks["network_0"]
    assert int(m.layers[2].num_batches_tracked) == 1 and int(m.layers[5].num_batches_tracked) == 1


def _bits(rec, members=slice(None)):
    out = {"loss": rec["loss"][members], **{"d" + k: v[members] for k, v in rec["grads"].items()},
           **{k: v[members] for k, v in rec["running"].items()}}
    return {k: v.cpu() for k, v in out.items()}


def test_two_identical_steps_give_identical_bits(device):
    a, _, a1, _ = _fused_run(device, 5, 2, 300, 96, 3, 3)
    b, _, b1, _ = _fused_run(device, 5, 2, 300, 96, 3, 3)
    for s in range(2):
        for k, v in _bits(a[s]).items():
            assert torch.equal(v, _bits(b[s])[k]), (s, k)
    assert all(torch.equal(a1[k], b1[k]) for k in a1)


def test_a_member_does_not_see_its_neighbours(device):
    """Member 0 trained alone = member 0 trained inside an ensemble of 3 with the same weights and batch, bit for bit."""
    three, _, p3, _ = _fused_run(device, 5, 2, 300, 96, 3, 3)
    one, _, p1, _ = _fused_run(device, 5, 2, 300, 96, 1, 3)   # the same seed: member 0 is constructed first, from the same draws
    for s in range(2):
        for k, v in _bits(one[s]).items():
            assert torch.equal(v, _bits(three[s], slice(0, 1))[k]), (s, k)
    assert all(torch.equal(p1[k], p3[k][:1]) for k in p1)


# ---------------------------------------------------------------------------------------------------- errors
def test_unsupported_shapes_raise(device):
    import sis_hip
    from networks.pixel_classifier.model import PixelEnsembleClassifier
    from training.ensemble_step import FusedEnsembleStep
    e = C.make_ensemble(0, 3, 64, 1, device=device)
    fused = FusedEnsembleStep(e, C.make_optimizers(e))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        fused.forward_backward(torch.randn(1, 64, device=device), torch.zeros(1, dtype=torch.int64, device=device))
    with pytest.raises(RuntimeError, match="unsupported shape: 1 pixels"):
        sis_hip.pe_train_tail(torch.rand(1, 128, device=device), torch.zeros(1, dtype=torch.int64, device=device),
                              {k: fused.stacks[k] for k in sis_hip.PE_TRAIN_PARAMS}, 3)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        sis_hip.pe_train_l1_forward(torch.randn(4, 40, device=device), torch.randn(128, 40, device=device), torch.randn(128, device=device))
    with pytest.raises(RuntimeError, match="11 members"):
        sis_hip.pe_train_l1_forward(torch.randn(4, 32, device=device), torch.randn(11 * 128, 32, device=device),
                                    torch.randn(11 * 128, device=device))
    with pytest.raises(ValueError, match="11 members"):
        FusedEnsembleStep(PixelEnsembleClassifier(3, 32, 11))


# ---------------------------------------------------------------------------------------------------- end to end
def test_train_then_label_end_to_end(device, tmp_path):
    """A separable 16^2 set of 2 images: 200 fused steps at P = 64 through dataset, loader, builder and updater; the loss falls
    below half its first value; the snapshot, loaded into DatasetGANSegmenter, labels at least 95 % of the training pixels
    correctly through the fused label pass.  (tests/test_ensemble_train_cpu.py: the ATen loop alone reaches both marks.)"""
    from segmentation.dataset_gan_segmenter import DatasetGANSegmenter, dataset_gan_upsamplers
    losses, snapshot, dataset, builder, updater = C.e2e_train(str(tmp_path), device, fused=True)
    assert updater.fused_step is not None
    print(f"end to end: first losses {losses[0].tolist()}, last {losses[-1].tolist()}")
    assert (losses[-1] < 0.5 * losses[0]).all()
    acts = {i: t for i, t in enumerate(dataset.layers)}
    seg = DatasetGANSegmenter(base_dir=tmp_path, image_size=C.E2E["size"], class_to_color_map=C.COLOURS, classifier_path=snapshot,
                              feature_size=dataset.get_feature_vector_length(), upsamplers=dataset_gan_upsamplers(acts, C.E2E["size"]))
    labels = seg.predict_labels_from_activations(acts)
    share = (labels.cpu().numpy() == dataset.pixel_labels).mean()
    print(f"end to end: {share:.4f} of the training pixels labelled correctly")
    assert share >= 0.95
