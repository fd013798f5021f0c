"""The projection encoders and autoencoders on the CPU (plain ATen formulation) against the reference's recorded outputs
(tests/golden/encoder32.npz), the factories of ``networks`` and the new library symbols."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

import encoder_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["WPlusEncoder", "WWPlusEncoder", "WEncoder", "WPlusNoNoiseEncoder", "WNoNoiseEncoder", "NoiseEncoder"]
NEW_SYMBOLS = {"sis_enc_conv3x3_s2_supported", "sis_enc_conv3x3_s2_packed_floats", "sis_enc_conv3x3_s2_pack", "sis_enc_conv3x3_s2",
               "sis_enc_stem_supported", "sis_enc_stem", "sis_enc_block_tail_supported", "sis_enc_block_tail_tiles", "sis_enc_block_tail_workspace_floats", "sis_enc_block_tail",
               "sis_enc_latent_heads_supported", "sis_enc_latent_heads"}
NEW_KERNELS = {"enc_conv3x3_s2_kernel", "enc_s2_pack_kernel", "enc_stem_kernel", "enc_block_tail_kernel", "enc_noise_finish_kernel", "enc_latent_heads_kernel"}


def test_fixture_lists_every_class():
    assert [str(c) for c in C.fixture()["classes"]] == CLASSES
    assert os.path.getsize(C.GOLDEN) < 512 * 1024


@pytest.mark.parametrize("cls", CLASSES)
def test_state_dict_names_and_shapes(cls):
    import networks.encoder.u_net_like_encoder as E
    size, latent, input_dim, channels = C.config()[:4]
    enc = getattr(E, cls)(size, latent, input_dim, channels, stylegan_variant=2)
    ours, want = enc.state_dict(), C.state_dict(cls)
    assert list(ours.keys()) == C.state_keys(cls)
    for k, v in ours.items():
        assert tuple(v.shape) == tuple(want[k].shape), k
    # torchvision's attribute names
    block = enc.resnet_blocks[1]
    assert [n for n, _ in block.named_children()] == ["conv1", "bn1", "relu", "conv2", "bn2", "downsample"] and block.stride == 2
    assert block.conv1.bias is None and block.conv1.padding == (1, 1) and block.conv1.stride == (2, 2)
    assert enc.resnet_blocks[0] is enc.start_block


@pytest.mark.parametrize("cls", CLASSES)
def test_cpu_forward_reproduces_the_reference(cls):
    """Same ATen formulation on both sides: the forward tolerance of tests/test_segmentation_oracle_cpu.py (rtol 1e-3, atol 1e-4)."""
    enc = C.build(cls)
    x = torch.from_numpy(C.fixture()["input"])
    with torch.no_grad():
        got = C.named_outputs(enc(x))
    want = C.named_expected(cls)
    assert sorted(got) == sorted(want) and want
    for name, ref in want.items():
        assert got[name].dtype == torch.float32 and tuple(got[name].shape) == ref.shape, name
        np.testing.assert_allclose(got[name].numpy(), ref, rtol=1e-3, atol=1e-4, err_msg=f"{cls} {name}")
    # under autograd and in training mode the same module differentiates
    if cls == "WPlusEncoder":
        enc.train()
        out = enc(x)
        (out.latent.sum() + sum(n.sum() for n in out.noise)).backward()
        assert enc.start_block.conv1.weight.grad is not None and enc.to_noise[0].weight.grad is not None


def test_autoencoder_reconstruction_on_the_cpu_formulation():
    """encode on the CPU reproduces the reference's latents; the decoder needs a HIP device (tests/test_encoder_gpu.py)."""
    from networks.encoder.autoencoder import StyleganAutoencoder
    auto = StyleganAutoencoder(C.build("WPlusEncoder"), C.generator()).eval()
    with torch.no_grad():
        latents = auto.encode(torch.from_numpy(C.fixture()["input"]))
    assert auto.is_wplus(latents) and tuple(latents.latent.shape) == (2, auto.decoder.n_latent, 32)
    assert [tuple(n.shape[-2:]) for n in latents.noise] == [tuple(n.shape[-2:]) for n in auto.decoder.make_noise()]
    assert auto.use_generated_noise is True


def test_unbuilt_encoders_raise_with_a_reason():
    import networks.encoder.u_net_like_encoder as E
    size, latent, input_dim, channels = C.config()[:4]
    with pytest.raises(NotImplementedError, match="StyleGAN1"):
        E.WPlusResnetNoiseEncoder(size, latent, input_dim, channels)
    with pytest.raises(NotImplementedError, match="StyleGAN1"):
        E.WCodeEncoder(10, size, latent, input_dim, channels)


CFG = {"stylegan_variant": 2, "image_size": 16, "latent_size": 32, "input_dim": 3, "n_mlp": 2, "channel_multiplier": 1}


@pytest.mark.parametrize("extra,auto_cls,enc_cls", [
    ({}, "StyleganAutoencoder", "WPlusEncoder"),
    ({"w_only": True}, "StyleganAutoencoder", "WWPlusEncoder"),
    ({"dropout_autoencoder": True}, "DropoutStyleganAutoencoder", "WPlusEncoder"),
    ({"dropout_autoencoder": True, "w_only": True}, "DropoutStyleganAutoencoder", "WWPlusEncoder"),
    ({"two_stem": True, "disable_update_for": "none"}, "TwoStemStyleganAutoencoder", "WPlusNoNoiseEncoder"),
    ({"two_stem": True, "w_only": True, "disable_update_for": "latent"}, "TwoStemStyleganAutoencoder", "WNoNoiseEncoder"),
    ({"stylegan_variant": "swagan", "w_only": True}, "StyleganAutoencoder", "WWPlusEncoder"),
    ({"input_dim": 1}, "StyleganAutoencoder", "WPlusEncoder"),
])
def test_get_autoencoder_builds_the_reference_classes(extra, auto_cls, enc_cls):
    import networks
    import networks.encoder.u_net_like_encoder as E
    auto = networks.get_autoencoder({**CFG, **extra})
    assert type(auto).__name__ == auto_cls and type(auto.encoder) is getattr(E, enc_cls)
    assert auto.encoder.size_channel_map == auto.decoder.channels and auto.encoder.stylegan_variant == 2
    assert auto.encoder.start_block.conv1.in_channels == {**CFG, **extra}["input_dim"]
    if auto_cls == "TwoStemStyleganAutoencoder":
        assert type(auto.noise_encoder) is E.NoiseEncoder and auto.encoder is auto.latent_encoder
        disabled = extra["disable_update_for"]
        assert (auto.update_latent, auto.update_noise) == (disabled in ("noise", "none"), disabled in ("latent", "none"))
    assert networks.StyleganAutoencoder is __import__("networks.encoder.autoencoder", fromlist=["x"]).StyleganAutoencoder


def test_get_autoencoder_rejects_what_the_reference_rejects():
    import networks
    with pytest.raises(NotImplementedError):
        networks.get_autoencoder({**CFG, "stylegan_variant": 1})
    with pytest.raises(NotImplementedError, match="code dim"):
        networks.get_autoencoder({**CFG, "code_dim": 4})
    with pytest.raises(AssertionError):
        networks.get_autoencoder({**CFG, "two_stem": True, "disable_update_for": "bogus"})


def test_autoencoder_checkpoint_round_trip(tmp_path):
    import networks
    cfg = {**CFG, "stylegan_checkpoint": "unused.pt"}
    torch.manual_seed(3)
    auto = networks.get_autoencoder(cfg)
    with torch.no_grad():
        for bn in [m for m in auto.encoder.modules() if isinstance(m, torch.nn.BatchNorm2d)]:
            bn.running_mean.normal_()
    ckpt = tmp_path / "auto.pt"
    torch.save({"autoencoder": auto.state_dict()}, ckpt)
    loaded = networks.load_autoencoder_or_generator(argparse.Namespace(device="cpu", checkpoint=str(ckpt)), cfg)
    assert type(loaded) is type(auto) and list(loaded.state_dict()) == list(auto.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(auto.state_dict().values(), loaded.state_dict().values()))
    # a file without the 'autoencoder' entry: the reference's fall-through is not provided
    bare = tmp_path / "bare.pt"
    torch.save(auto.state_dict(), bare)
    with pytest.raises(NotImplementedError, match="'autoencoder' entry"):
        networks.load_autoencoder_or_generator(argparse.Namespace(device="cpu", checkpoint=str(bare)), cfg)


def test_trainable_parameter_groups():
    from networks.encoder.autoencoder import StyleganAutoencoder, TwoStemStyleganAutoencoder
    enc = C.build("WPlusEncoder")
    auto = StyleganAutoencoder(enc, C.generator())
    assert [id(p) for p in auto.trainable_parameters()] == [id(p) for p in enc.parameters()]
    groups = auto.trainable_parameters(as_groups=[["to_noise"], ["to_latent", "bn"]])
    names = dict(enc.named_parameters())
    want_noise = [p for n, p in names.items() if "to_noise" in n]
    want_second = [p for n, p in names.items() if "to_noise" not in n and ("to_latent" in n or "bn" in n)]
    assert [sorted(g) for g in groups] == [["params"]] * 3
    assert [id(p) for p in groups[1]["params"]] == [id(p) for p in want_noise] and len(want_noise) == 16  # 4 + 4 one-channel heads (the last intermediate one is built, never called), weight and bias
    assert [id(p) for p in groups[2]["params"]] == [id(p) for p in want_second]
    assert sum(len(g["params"]) for g in groups) == len(names)
    assert not {id(p) for p in groups[0]["params"]} & {id(p) for p in want_noise + want_second}
    # two stems: a stem whose update is disabled is left out
    two = TwoStemStyleganAutoencoder(C.build("WPlusNoNoiseEncoder"), C.build("NoiseEncoder"), C.generator(), update_latent=False)
    assert [id(p) for p in two.trainable_parameters()] == [id(p) for p in two.noise_encoder.parameters()]
    groups = two.trainable_parameters(as_groups=[["to_noise"]])
    assert len(groups) == 2 and len(groups[1]["params"]) == 16
    with pytest.raises(AssertionError):
        TwoStemStyleganAutoencoder(None, None, None, update_latent=False, update_noise=False)


def test_importing_networks_does_not_load_the_encoders():
    import subprocess
    import sys
    src = os.path.join(ROOT, "synthesis-in-style_amd")
    code = ("import sys, networks; assert networks.StyleganAutoencoder.__module__ == 'networks.encoder.autoencoder'; "
            "assert 'networks.encoder.u_net_like_encoder' not in sys.modules and 'sis_hip' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=src, env={**os.environ, "PYTHONPATH": src})


def test_generate_images_takes_what_the_reference_takes():
    """A dict batch goes through autoencoder.encode; anything else but Latents is refused; a generator-only holder cannot encode."""
    import networks
    from utils.dataset_creation import generate_images
    with pytest.raises(NotImplementedError):
        generate_images([1, 2], None)
    holder = networks.get_autoencoder({k: v for k, v in CFG.items() if k != "input_dim"})
    assert holder.encoder is None
    with pytest.raises(NotImplementedError, match="generator only"):
        generate_images({"input_image": torch.zeros(1, 3, 16, 16)}, holder, device="cpu")


def test_header_ctypes_table_and_library_agree():
    import sis_hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sis_hip.h")).read(), flags=re.S)
    assert NEW_SYMBOLS <= set(re.findall(r"\b(sis_[a-z0-9_]+)\s*\(", header)) and NEW_SYMBOLS <= set(sis_hip.exported_symbols())
    L = sis_hip.lib()
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert decl.count(",") + 1 == len(sis_hip._SIGNATURES[name][0]), name
        assert hasattr(L, name)
    assert NEW_KERNELS <= sis_hip.own_kernel_names()
    # the queries (no device needed)
    assert L.sis_enc_conv3x3_s2_supported(128, 256, 256, 256) and L.sis_enc_conv3x3_s2_supported(512, 512, 8, 8)
    assert L.sis_enc_conv3x3_s2_supported(16, 24, 12, 20) and L.sis_enc_conv3x3_s2_supported(40, 72, 36, 36)
    assert not L.sis_enc_conv3x3_s2_supported(3, 8, 32, 32) and not L.sis_enc_conv3x3_s2_supported(8, 8, 9, 8)
    assert not L.sis_enc_conv3x3_s2_supported(8, 8, 512, 512)
    assert L.sis_enc_conv3x3_s2_packed_floats(16, 24, 1) == 16 * 10 * 64 and L.sis_enc_conv3x3_s2_packed_floats(16, 72, 0) == 16 * 9 * 128
    assert L.sis_enc_stem_supported(1, 8, 8, 12) and L.sis_enc_stem_supported(3, 128, 256, 256) and not L.sis_enc_stem_supported(5, 8, 8, 8)
    assert L.sis_enc_block_tail_supported(8, 16) and not L.sis_enc_block_tail_supported(8, 18)
    assert [L.sis_enc_block_tail_tiles(n) for n in (16, 256, 260)] == [1, 1, 2]
    # channel slices (of at least 8 channels, for about 512 workgroups per sample): 40 channels -> 5 slices; 8 channels -> one, no workspace
    assert L.sis_enc_block_tail_workspace_floats(3, 40, 240) == 3 * 5 * 240 and L.sis_enc_block_tail_workspace_floats(1, 8, 16) == 0
    assert L.sis_enc_block_tail_workspace_floats(7, 128, 65536) == 7 * 2 * 65536 and L.sis_enc_block_tail_workspace_floats(7, 512, 16) == 7 * 64 * 16
    assert not L.sis_enc_conv3x3_s2_supported(8, 8, 8, 404) and L.sis_enc_conv3x3_s2_supported(8, 8, 8, 200)   # the gate is the LDS byte count
    assert L.sis_enc_latent_heads_supported(512, 512) and not L.sis_enc_latent_heads_supported(12000, 512)
