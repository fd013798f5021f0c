"""Shared pieces of the DatasetGAN ensemble-training tests (tests/test_ensemble_train_{cpu,gpu}.py).

The oracle is the repository's own ``PixelClassifier`` in float64 on the CPU with ``nn.CrossEntropyLoss`` and the CPU path of
``GradientClipAdam`` in float64 (tests/golden/dataset_gan.npz pins that model to the reference).  ``oracle_run`` is cached: the
tests that share a recipe share one run, and nobody changes what it returns.
"""
import functools
import json
import os

import numpy as np
import torch
from torch import nn

KINDS = {"w1": "layers.0.weight", "b1": "layers.0.bias", "g1": "layers.2.weight", "be1": "layers.2.bias", "w2": "layers.3.weight",
         "b2": "layers.3.bias", "g2": "layers.5.weight", "be2": "layers.5.bias", "w3": "layers.6.weight", "b3": "layers.6.bias"}
RUNNING = {"mean1": "layers.2.running_mean", "var1": "layers.2.running_var", "mean2": "layers.5.running_mean",
           "var2": "layers.5.running_var"}
ADAM = dict(lr=5e-4, betas=(0.5, 0.999), weight_decay=1e-4)
# Seeds whose ReLU gates stay clear of zero under THIS module's recipe (make_ensemble + batch), found by scanning 0..119 on the
# float64 oracle: 19, 55, 57, 90, 91, 97, 102, 111.  The two with the widest margin (1.3e-5 and 1.7e-5 of max|pre-activation|) are
# used; the CPU suite re-checks the condition.
GATE_SEEDS = (19, 57)


def make_ensemble(seed, classes, features, members, dtype=torch.float32, device="cpu"):
    """The recipe of the whole-step tests: seed, construct (the constructor calls init_weights), convert."""
    from networks.pixel_classifier.model import PixelEnsembleClassifier
    torch.manual_seed(seed)
    e = PixelEnsembleClassifier(classes, features, members)
    for m in e.get_networks().values():
        m.to(device=device, dtype=dtype)
    return e


def make_optimizers(ensemble):
    from training.fused_adam import GradientClipAdam
    return {f"optimizer_{i}": GradientClipAdam(m.parameters(), **ADAM) for i, m in enumerate(ensemble.get_networks().values())}


def batch(seed, step, pixels, features, classes):
    gen = torch.Generator().manual_seed(1000 * seed + step)
    x = torch.randn(pixels, features, generator=gen)
    return x, torch.randint(0, classes, (pixels,), generator=gen)


def param(member, dotted):
    obj = member
    for part in dotted.split("."):
        obj = getattr(obj, part) if not part.isdigit() else obj[int(part)]
    return obj


def aten_steps(ensemble, optimizers, seed, steps, pixels, features, classes, device="cpu", dtype=torch.float32, record_pre=False,
               members=None):
    """The reference's per-member loop -> per step {"grads": {kind: [N, ...]}, "loss": [N], "running": {...}, "logits": [N, P, C],
    "pre": [max|z|, min|z|] per hidden layer}, and the parameters before and after."""
    members = list(ensemble.get_networks().values())
    ce = nn.CrossEntropyLoss()
    snap = lambda: {k: torch.stack([param(m, d).detach().clone() for m in members]) for k, d in KINDS.items()}   # noqa: E731
    p0, out = snap(), []
    for step in range(steps):
        x, t = batch(seed, step, pixels, features, classes)
        x, t = x.to(device=device, dtype=dtype), t.to(device)
        rec = {"loss": [], "logits": [], "pre": []}
        for i, m in enumerate(members):
            opt = optimizers[f"optimizer_{i}"]
            opt.zero_grad()
            if record_pre:
                with torch.no_grad():
                    z1 = m.layers[0](x)
                    bn = m.layers[2]
                    a = torch.relu(z1)
                    y1 = bn.weight * (a - a.mean(0)) / torch.sqrt(a.var(0, unbiased=False) + bn.eps) + bn.bias
                    z2 = m.layers[3](y1)
                    rec["pre"].append([(z.abs().min().item(), z.abs().max().item()) for z in (z1, z2)])
            logits = m(x)
            loss = ce(logits, t)
            loss.backward()
            rec["loss"].append(loss.detach().clone())
            rec["logits"].append(logits.detach().clone())
        rec["grads"] = {k: torch.stack([param(m, d).grad.detach().clone() for m in members]) for k, d in KINDS.items()}
        for i in range(len(members)):
            optimizers[f"optimizer_{i}"].step()
        rec["running"] = {k: torch.stack([param(m, d).detach().clone() for m in members]) for k, d in RUNNING.items()}
        rec["tracked"] = [int(m.layers[2].num_batches_tracked) for m in members]
        rec["loss"], rec["logits"] = torch.stack(rec["loss"]), torch.stack(rec["logits"])
        out.append(rec)
    return out, p0, snap()


@functools.lru_cache(maxsize=None)
def oracle_run(seed, steps, pixels, features, members, classes):
    e = make_ensemble(seed, classes, features, members, dtype=torch.float64)
    return aten_steps(e, make_optimizers(e), seed, steps, pixels, features, classes, dtype=torch.float64, record_pre=True)


def gates_clear(seed, steps=3, pixels=64, features=64, members=3, classes=3, margin=1e-5):
    """No hidden pre-activation of either layer, at any step, within ``margin`` * max|pre-activation| of zero (on the oracle)."""
    recs, _, _ = oracle_run(seed, steps, pixels, features, members, classes)
    return all(lo >= margin * hi for rec in recs for member in rec["pre"] for lo, hi in member)


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    d = torch.linalg.vector_norm(got - ref).item()
    return (d if d == d else float("inf")) / max(torch.linalg.vector_norm(ref).item(), 1e-300)


# ---------------------------------------------------------------------------------------------------- a tiny dataset on disk
COLOURS = {"background": "#000000", "printed_text": "#0000FF", "handwritten_text": "#FF0000"}
RGB = np.array([[0, 0, 0], [0, 0, 255], [255, 0, 0]], dtype=np.uint8)


def class_maps(images, size, seed=3):
    """Vertical bands of the three classes, shifted per image, with a few random pixels so that no class is a rectangle."""
    rng = np.random.default_rng(seed)
    maps = np.zeros((images, size, size), dtype=np.uint8)
    for i in range(images):
        cols = (np.arange(size) * 3 // size + i) % 3
        maps[i] = cols[None, :]
        flip = rng.random((size, size)) < 0.05
        maps[i][flip] = rng.integers(0, 3, size=int(flip.sum()))
    return maps


def separable_activations(maps, channels=32, offset=4.0, seed=5):
    """Generator-shaped layers {0: 4^2, 1: 8^2, 2: full} of ``channels`` each; on the full-resolution layer the pixels of class c
    carry ``offset`` on channel c."""
    images, size = maps.shape[0], maps.shape[1]
    gen = torch.Generator().manual_seed(seed)
    per_image = []
    for i in range(images):
        acts = {0: torch.randn(channels, size // 4, size // 4, generator=gen), 1: torch.randn(channels, size // 2, size // 2, generator=gen),
                2: torch.randn(channels, size, size, generator=gen)}
        for c in range(3):
            acts[2][c] += offset * torch.from_numpy((maps[i] == c).astype(np.float32))
        per_image.append({k: v.numpy() for k, v in acts.items()})
    return per_image


def write_dataset(tmp_path, maps, per_image, latents=None):
    """tensors.npz, train.json, map.json and the label PNGs in the reference's layout -> (json path, npz path, map path)."""
    from PIL import Image
    entries = []
    for i, m in enumerate(maps):
        Image.fromarray(RGB[m]).save(os.path.join(tmp_path, f"label_{i}.png"))
        Image.fromarray(np.zeros((*m.shape, 3), dtype=np.uint8)).save(os.path.join(tmp_path, f"image_{i}.png"))
        entries.append({"image": f"image_{i}.png", "label": f"label_{i}.png", "activations": i, "latent": i})
    stored = np.empty(len(per_image), dtype=object)
    for i, a in enumerate(per_image):
        stored[i] = a
    np.savez(os.path.join(tmp_path, "tensors.npz"), activations=stored,
             latent_codes=np.zeros((len(maps), 4), dtype=np.float32) if latents is None else latents)
    with open(os.path.join(tmp_path, "train.json"), "w") as f:
        json.dump(entries, f)
    with open(os.path.join(tmp_path, "map.json"), "w") as f:
        json.dump(COLOURS, f)
    return os.path.join(tmp_path, "train.json"), os.path.join(tmp_path, "tensors.npz"), os.path.join(tmp_path, "map.json")


E2E = dict(images=2, size=16, pixels=64, steps=200, seed=0)


def e2e_config(tmp_path):
    return {"numpy_class": 3, "num_models": 3, "lr": ADAM["lr"], "beta1": 0.5, "beta2": 0.999, "weight_decay": 1e-4,
            "log_dir": os.path.join(tmp_path, "logs"), "snapshot_save_iter": E2E["steps"], "batch_size": E2E["pixels"]}


def e2e_train(tmp_path, device, fused):
    """Dataset on disk -> loader -> builder -> updater -> E2E['steps'] updates -> (losses of every step [steps, N], snapshot path,
    dataset, builder)."""
    from data.dataset_gan_dataset import DeviceDatasetGANDataset, PixelBatchLoader
    from training.loop import get_current_reporter
    from training_builder.pixel_ensemble_train_builder import PixelEnsembleTrainBuilder
    maps = class_maps(E2E["images"], E2E["size"])
    json_path, npz, cmap = write_dataset(tmp_path, maps, separable_activations(maps))
    dataset = DeviceDatasetGANDataset(json_path, npz, cmap, E2E["size"], device=device)
    loader = PixelBatchLoader(dataset, E2E["pixels"], seed=E2E["seed"])
    config = {**e2e_config(tmp_path), "fused": fused}
    torch.manual_seed(E2E["seed"])
    builder = PixelEnsembleTrainBuilder(config, loader, None)
    if torch.device(device).type == "cpu":
        builder.device = lambda: torch.device("cpu")
        for m in builder.segmentation_network.get_networks().values():
            m.cpu()
    updater = builder.get_updater()
    snapshotter = builder.get_snapshotter()
    losses = []
    for it in range(1, E2E["steps"] + 1):
        updater.update()
        obs = get_current_reporter().observations
        losses.append(torch.stack([obs[f"loss/CrossEntropyLoss_network_{i}"].detach().float().reshape(()) for i in range(3)]))
        snapshotter.maybe_save(it)
    return torch.stack(losses).cpu(), os.path.join(config["log_dir"], f"{E2E['steps']:06d}.pt"), dataset, builder, updater
