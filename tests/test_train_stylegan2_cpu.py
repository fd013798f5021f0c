"""CPU: GAN training from an image list (train_stylegan_2.py) -- the algebra of the polyphase downsampling layer in float64, the
entry point's options / optimizers / schedule, the image list loader against a PIL restatement, and the C ABI of the new kernels."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch
import yaml

import gan_train_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "synthesis-in-style_amd")

NEW_SYMBOLS = {"sis_gan_image_batch", "sis_phase_split_supported", "sis_phase_split", "sis_phase_merge",
               "sis_down_weight_compose_supported", "sis_down_weight_compose", "sis_down_weight_compose_adjoint"}

# the options of the reference's train_stylegan_2.py:187-203, in its order
REFERENCE_OPTIONS = [("config",), ("--resume-ckpt",), ("--images",), ("--val-images",), ("--device",), ("-l", "--log-dir"),
                     ("-ln", "--log-name"), ("--local_rank",), ("--mpi-backend",), ("--cache-root",), ("-s", "--stylegan-variant"),
                     ("--wandb-project-name",), ("--wandb-entity",)]


# ---- the polyphase identity ---------------------------------------------------------------------------------------------

def _operands(b, cin, cout, h, w, seed=0):
    gen = torch.Generator().manual_seed(seed + b + cin + cout + h + w)
    x = torch.randn(b, cin, h, w, generator=gen, dtype=torch.float64)
    wt = torch.randn(cout, cin, 3, 3, generator=gen, dtype=torch.float64)
    gy = torch.randn(b, cout, h // 2, w // 2, generator=gen, dtype=torch.float64)
    return x, wt, gy, 1 / math.sqrt(cin * 9)


def _rel(got, want):
    return C.max_abs(got, want) / want.abs().max().item()


@pytest.mark.parametrize("shape", [(2, 8, 16, 8, 8), (1, 3, 5, 6, 10)])
@pytest.mark.parametrize("taps", ["1331", "asymmetric"])
def test_polyphase_identity_float64(shape, taps):
    """Blur(pad 2) + stride-2 conv == stride-1 conv of the phase split with the composed weight: forward, dx, dW and the R1-style
    second derivative d/dW |d(sum y^2)/dx|^2, within 1e-12 relative.  The asymmetric FIR pins the flip of the blur (a true
    convolution), which [1, 3, 3, 1] cannot see."""
    x, wt, gy, scale = _operands(*shape)
    f = C.fir_taps() if taps == "1331" else C.fir_taps(torch.arange(1.0, 17.0).view(4, 4).tolist())
    results = []
    for fn in (C.library_down, C.polyphase_down):
        xx, ww = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
        y = fn(xx, ww, f, scale)
        dx, dw = torch.autograd.grad(y, (xx, ww), gy, retain_graph=True)
        g, = torch.autograd.grad(y.pow(2).sum(), xx, create_graph=True)
        r1_w, = torch.autograd.grad(g.pow(2).sum(), ww)
        results.append((y.detach(), dx, dw, r1_w))
    assert tuple(results[0][0].shape) == (shape[0], shape[2], shape[3] // 2, shape[4] // 2)
    for name, want, got in zip(("y", "dx", "dW", "d/dW |d y^2/dx|^2"), *results):
        assert _rel(got, want) < 1e-12, (name, _rel(got, want))


def test_compose_restatements_are_adjoint():
    """``ref_compose_adjoint`` (written out) is the transpose of ``ref_compose``: autograd's, and the dot-product identity."""
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(5, 3, 3, 3, generator=gen, dtype=torch.float64, requires_grad=True)
    g = torch.randn(5, 12, 3, 3, generator=gen, dtype=torch.float64)
    f = C.fir_taps(torch.arange(1.0, 17.0).view(4, 4).tolist())
    composed = C.ref_compose(w, f, 0.37)
    assert tuple(composed.shape) == (5, 12, 3, 3) and bool((composed != 0).all())   # all 36 taps of every pair carry weight
    want, = torch.autograd.grad(composed, w, g)
    got = C.ref_compose_adjoint(g, f, 0.37)
    assert _rel(got, want) < 1e-14
    assert abs((composed.detach() * g).sum().item() - (w.detach() * got).sum().item()) < 1e-12 * (composed.detach() * g).abs().sum().item()


# ---- the entry point ----------------------------------------------------------------------------------------------------

def test_option_names_are_the_references():
    import train_stylegan_2 as T
    import argparse
    parser_actions = []
    real = argparse.ArgumentParser.add_argument

    def spy(self, *names, **kw):
        parser_actions.append(tuple(names))
        return real(self, *names, **kw)

    argparse.ArgumentParser.add_argument = spy
    try:
        args = T.parse_args(["cfg.yaml", "--images", "train.json"])
    finally:
        argparse.ArgumentParser.add_argument = real
    own = [a for a in parser_actions if a != ("-h", "--help")]
    assert own[:len(REFERENCE_OPTIONS)] == REFERENCE_OPTIONS
    assert own[len(REFERENCE_OPTIONS):] == [("--max-iter",)]
    assert (args.device, args.log_dir, args.log_name, args.local_rank, args.mpi_backend, args.stylegan_variant) == \
        ("cuda", "training", "training", 0, "gloo", "2")
    assert args.resume_ckpt is None and args.max_iter is None and args.wandb_project_name == "StyleGAN Training"
    with pytest.raises(SystemExit):
        T.parse_args(["cfg.yaml"])   # --images is required
    assert T.parse_args(["c", "--images", "i", "-s", "SWAGAN"]).stylegan_variant == "swagan"


def _config():
    with open(os.path.join(SRC, "configs", "stylegan", "stylegan_256px.yaml")) as f:
        return yaml.safe_load(f)


def test_yaml_carries_the_reference_values():
    cfg = _config()
    want = dict(image_save_iter=1000, display_size=16, snapshot_save_iter=10000, log_iter=10, max_iter=100000, batch_size=24, lr=0.001,
                latent_size=512, n_mlp=8, channel_multiplier=2, style_mixing_prob=0.9, freeze_stochastic_noise_layers=[0, 1, 2, 3, 4, 5],
                input_dim=3, image_size=256, regularization=dict(g_interval=4, d_interval=16, r1_weight=10, path_reg_weight=2))
    for key, value in want.items():
        assert cfg[key] == value, key
    assert isinstance(cfg["polyphase_downsample"], bool)


def test_optimizers_and_schedule():
    import train_stylegan_2 as T
    from training.fused_adam import GradientClipAdam
    cfg = _config()
    cfg["max_iter"] = 10
    g, d = torch.nn.Linear(3, 2), torch.nn.Linear(2, 1)
    opts = T.build_optimizers(cfg, g, d)
    assert set(opts) == {"generator", "discriminator"} and all(isinstance(o, GradientClipAdam) for o in opts.values())
    for name, r in (("generator", 4 / 5), ("discriminator", 16 / 17)):
        group = opts[name].param_groups[0]
        assert group["lr"] == 0.001 * r and tuple(group["betas"]) == (0.0, 0.99 ** r) and group["weight_decay"] == 0.0
    scheds = T.build_schedulers(cfg, opts)
    for name, r in (("generator", 4 / 5), ("discriminator", 16 / 17)):
        lr0, seen = 0.001 * r, []
        for it in range(11):
            seen.append(opts[name].param_groups[0]["lr"])
            for p in (g if name == "generator" else d).parameters():
                p.grad = torch.zeros_like(p)
            opts[name].step()   # (CPU parameters: the plain torch path)
            scheds[name].step()
        closed = [1e-8 + (lr0 - 1e-8) * (1 + math.cos(math.pi * t / 10)) / 2 for t in range(11)]
        np.testing.assert_allclose(seen, closed, rtol=1e-9, atol=1e-15)
        assert seen[0] == lr0 and abs(seen[5] - (1e-8 + (lr0 - 1e-8) / 2)) < 1e-12 and abs(seen[10] - 1e-8) < 1e-15


def test_variant_1_raises_and_snapshot_keys():
    import train_stylegan_2 as T
    cfg = dict(_config(), stylegan_variant="1")
    with pytest.raises(NotImplementedError, match="StyleGAN1 is not on the MI355X hot path"):
        T.build_networks(cfg)
    assert T.SNAPSHOT_KEYS == ("generator", "discriminator", "g_ema", "generator_optimizer", "discriminator_optimizer")
    assert T.reg_ratio("4") == 0.8


def test_sample_latents_are_fixed_by_the_seed():
    import train_stylegan_2 as T
    cfg = dict(display_size=5, latent_size=7, seed=3)
    a, b = T.sample_latents(cfg, "cpu"), T.sample_latents(cfg, "cpu")
    assert tuple(a.shape) == (5, 7) and torch.equal(a, b) and not torch.equal(a, T.sample_latents(dict(cfg, seed=4), "cpu"))


# ---- the loader ---------------------------------------------------------------------------------------------------------

def _write_images(folder, sizes, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    names = []
    for i, (w, h) in enumerate(sizes):
        name = f"sub/img_{i:02d}.png" if i % 2 else f"img_{i:02d}.png"
        os.makedirs(os.path.dirname(os.path.join(folder, name)), exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(folder, name))
        names.append(name)
    return names


def test_dataset_decodes_resizes_and_keeps_uint8(tmp_path, capsys):
    from PIL import Image
    from data.gan_image_dataset import DeviceImageDataset
    names = _write_images(str(tmp_path), [(32, 32), (40, 36), (32, 32)])
    (tmp_path / "broken.png").write_bytes(b"not a png")
    (tmp_path / "train.json").write_text(json.dumps(names + ["broken.png"]))
    ds = DeviceImageDataset(tmp_path / "train.json", 32, device="cpu")
    assert len(ds) == 4 and ds.pixels.dtype == torch.uint8 and tuple(ds.pixels.shape) == (4, 3, 32, 32) and ds.resident
    for i, name in enumerate(names):   # the PIL / numpy restatement of transforms.Resize((S, S)) on a PIL image
        with Image.open(tmp_path / name) as im:
            im = im.convert("RGB")
            if im.size != (32, 32):
                im = im.resize((32, 32), Image.BILINEAR)
            want = np.asarray(im).transpose(2, 0, 1)
        assert np.array_equal(ds.pixels[i].numpy(), want), name
    assert not ds.pixels[3].any()   # the unreadable file: the reference's black image ...
    out = capsys.readouterr().out
    assert out.count("Could not load") == 1 and "broken.png" in out   # ... with one warning
    with pytest.raises(ValueError, match="input_dim"):
        DeviceImageDataset(tmp_path / "train.json", 32, input_dim=1, device="cpu")
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        ds.get_batch([0])   # no CPU path for the batch kernel
    with pytest.raises(IndexError):
        ds.get_batch([4])
    small = DeviceImageDataset(tmp_path / "train.json", 32, device="cpu", max_resident_bytes=100)
    assert not small.resident


def test_epoch_order_is_reproducible_and_sharded(tmp_path):
    from data.gan_image_dataset import DeviceImageDataset, DeviceImageLoader
    (tmp_path / "train.json").write_text(json.dumps([f"{i}.png" for i in range(14)]))
    ds = DeviceImageDataset(tmp_path / "train.json", 32, load=False)
    a, b = DeviceImageLoader(ds, 4, seed=5), DeviceImageLoader(ds, 4, seed=5)
    assert a.indices(0) == b.indices(0) and a.indices(1) == b.indices(1) and a.indices(0) != a.indices(1)
    assert sorted(a.indices(0)) == list(range(14)) and len(a) == 3
    assert DeviceImageLoader(ds, 4, seed=6).indices(0) != a.indices(0)
    r0, r1 = DeviceImageLoader(ds, 4, rank=0, world_size=2, seed=5), DeviceImageLoader(ds, 4, rank=1, world_size=2, seed=5)
    assert not set(r0.indices(0)) & set(r1.indices(0)) and sorted(r0.indices(0) + r1.indices(0)) == list(range(14))
    assert len(r0) == 1 and len(DeviceImageLoader(ds, 4, drop_last=False, rank=0, world_size=2)) == 2
    with pytest.raises(ValueError):
        DeviceImageLoader(ds, 4, rank=2, world_size=2)


def test_loader_restarts_with_the_next_epoch(tmp_path):
    """One pass = one epoch with drop_last; ``Updater.next_batch`` (which ``Stylegan2Updater.update_core`` reads its images
    through) starts the next pass, with the next epoch's order."""
    from data.gan_image_dataset import DeviceImageDataset, DeviceImageLoader
    from training.loop import Updater
    (tmp_path / "train.json").write_text(json.dumps([f"{i}.png" for i in range(10)]))
    ds = DeviceImageDataset(tmp_path / "train.json", 32, load=False)
    ds.get_batch = lambda idx: {"image": list(idx)}
    loader = DeviceImageLoader(ds, 4, seed=1)
    up = Updater({"images": loader}, {}, {})
    got = [up.next_batch("images")["image"] for _ in range(5)]
    e0, e1, e2 = loader.indices(0), loader.indices(1), loader.indices(2)
    assert got == [e0[0:4], e0[4:8], e1[0:4], e1[4:8], e2[0:4]]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

def test_new_symbols_declared_and_exported():
    import sis_hip
    text = open(os.path.join(ROOT, "include", "sis_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sis_[a-z0-9_]+)\s*\(", text))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(sis_hip.exported_symbols())
    lib = ctypes.CDLL(sis_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    L = sis_hip.lib()
    assert L.sis_phase_split_supported(8, 8) and L.sis_phase_split_supported(6, 10)
    assert not L.sis_phase_split_supported(7, 8) and not L.sis_phase_split_supported(8, 0)
    assert L.sis_down_weight_compose_supported(4, 4) and not L.sis_down_weight_compose_supported(3, 3)
    assert not L.sis_down_weight_compose_supported(4, 6)
    assert not sis_hip.down_weight_compose_supported(torch.ones(2, 2) / 4) and sis_hip.down_weight_compose_supported(torch.ones(4, 4) / 16)
    names = sis_hip.own_kernel_names()
    for kernel in ("gan_image_batch_kernel", "phase_split_kernel", "down_weight_compose_kernel", "down_weight_adjoint_kernel"):
        assert kernel in names, kernel


def test_entries_reject_bad_arguments_before_any_launch():
    """Null pointers, odd sizes and a FIR that is not 4 x 4 are refused by the entry points themselves (no device needed)."""
    import sis_hip
    L = sis_hip.lib()
    assert L.sis_phase_split(None, None, 1, 1, 8, 8, None) == 1 and b"null pointer" in L.sis_last_error()
    one = ctypes.c_void_p(16)
    assert L.sis_phase_split(one, one, 1, 1, 7, 8, None) == 1 and b"even" in L.sis_last_error()
    assert L.sis_down_weight_compose(one, one, one, 3, 3, 1.0, 8, 8, None) == 1 and b"4 x 4 only" in L.sis_last_error()
    assert L.sis_down_weight_compose_adjoint(one, one, one, 4, 5, 1.0, 8, 8, None) == 1 and b"4 x 4 only" in L.sis_last_error()
    assert L.sis_gan_image_batch(one, one, one, 0, 1, 8, None) == 1 and L.sis_gan_image_batch(None, one, one, 1, 1, 8, None) == 1


def test_polyphase_switch_defaults_off():
    import networks.stylegan2.discriminator as D
    assert D._POLYPHASE is (os.environ.get("SIS_GAN_POLYPHASE", "0") == "1")   # read once, at import; unset means off
    assert _config()["polyphase_downsample"] in (False, True)
    layer = D.ConvLayer(8, 16, 3, downsample=True)
    assert list(layer.state_dict()) == ["0.kernel", "1.weight", "2.bias"] and layer._down3x3   # children and keys as before
    assert not D.ConvLayer(8, 16, 1, downsample=True, activate=False, bias=False)._down3x3 and not D.ConvLayer(8, 8, 3)._down3x3
