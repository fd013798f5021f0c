"""Golden vectors of the projection encoders from the UNMODIFIED reference networks/encoder/u_net_like_encoder.py and
autoencoder.py, loaded by file path.  The two modules they import are stand-ins: ``torchvision.models.resnet`` is this
repository's restatement of BasicBlock (torchvision is not installed; the block is torchvision's, not the reference's),
``latent_projecting`` is this repository's ``Latents`` container.  The generator of the autoencoder case is the UNMODIFIED
reference networks/stylegan2/model.py on the oracle's CPU ops (oracle/load_reference.py).  Needs the reference tree, so it
runs on the development box only.

    python tests/golden/make_golden_encoder.py      -> tests/golden/encoder32.npz

Per encoder class, at image_size 32, latent_size 32, 3 input channels, map {32: 8, 16: 16, 8: 24, 4: 32}, stylegan_variant 2,
eval(), BatchNorm statistics and affine parameters drawn away from (0, 1): the state_dict's names in order per class, its
values once for all classes under ``sd/<name>`` (each tensor is drawn from its name, so the classes share the block ladder and
their common heads; float16-representable, stored as float16), the reference's outputs for one input [2, 3, 32, 32] in float32
and, with the module cast to double, in float64 (``<class>/latent``; the noise maps, equal for every class that has them, once
under ``noise<i>``).  For
StyleganAutoencoder(WPlusEncoder, Generator(32, 32, n_mlp=2, channel_multiplier=1)) the reconstructed image, both precisions
(generator weights: oracle.stylegan2_ref.seeded_state_dict(32, 32, 2, 1, seed=GEN_SEED), not stored).
"""
import importlib.util
import os
import sys
import types
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SRC = os.path.join(ROOT, "synthesis-in-style_amd")
for p in (ROOT, SRC):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import stylegan2_ref as R  # noqa: E402
from oracle.load_reference import REFERENCE_ROOT, load_reference_stylegan2  # noqa: E402

CLASSES = ["WPlusEncoder", "WWPlusEncoder", "WEncoder", "WPlusNoNoiseEncoder", "WNoNoiseEncoder", "NoiseEncoder"]
SIZE, LATENT, INPUT_DIM, CHANNELS = 32, 32, 3, {32: 8, 16: 16, 8: 24, 4: 32}
GEN_SEED, GEN_N_MLP, GEN_CM = 41, 2, 1


def load_reference_encoders():
    from latent_projecting import Latents
    from networks.encoder.u_net_like_encoder import BasicBlock
    saved = {k: sys.modules.get(k) for k in ("torchvision", "torchvision.models", "torchvision.models.resnet", "latent_projecting")}
    tv, tvm, tvr = types.ModuleType("torchvision"), types.ModuleType("torchvision.models"), types.ModuleType("torchvision.models.resnet")
    tvr.BasicBlock = BasicBlock
    tv.models, tvm.resnet = tvm, tvr
    lp = types.ModuleType("latent_projecting")
    lp.Latents, lp.CodeLatents = Latents, type("CodeLatents", (), {})
    sys.modules.update({"torchvision": tv, "torchvision.models": tvm, "torchvision.models.resnet": tvr, "latent_projecting": lp})
    try:
        mods = []
        for name in ("u_net_like_encoder", "autoencoder"):
            path = os.path.join(REFERENCE_ROOT, "networks", "encoder", name + ".py")
            spec = importlib.util.spec_from_file_location("reference_encoder_" + name, path)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            mods.append(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mods


def randomise(module):
    """Every tensor from a generator seeded by its NAME (so the classes share their trunk and their common heads), at the
    initial scale of a convolution; BatchNorm statistics and affine parameters away from (0, 1).  Values are rounded to
    float16-representable numbers: the fixture stores them as float16, exactly."""
    with torch.no_grad():
        for name, t in sorted(dict(module.state_dict()).items()):
            if name.endswith("num_batches_tracked"):
                continue
            gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
            if name.endswith("running_var"):
                v = 0.5 + torch.rand(t.shape, generator=gen)
            elif name.endswith("running_mean"):
                v = 0.3 * torch.randn(t.shape, generator=gen)
            elif ".bn" in name or "downsample.1" in name:
                v = (0.8 + 0.4 * torch.rand(t.shape, generator=gen)) if name.endswith("weight") else 0.2 * torch.randn(t.shape, generator=gen)
            elif name.endswith("bias"):
                v = 0.1 * torch.randn(t.shape, generator=gen)
            else:
                v = torch.randn(t.shape, generator=gen) * (2.0 / t[0].numel()) ** 0.5
            t.copy_(v.half().float())


def put(out, key, value):
    """Store once; a second class's tensor under the same key must be bit-equal (shared trunk, shared heads)."""
    if key in out:
        assert out[key].dtype == value.dtype and np.array_equal(out[key], value), key
    else:
        out[key] = value


def record(out, cls, latents, suffix):
    if latents.latent is not None:
        out[f"{cls}/latent{suffix}"] = latents.latent.numpy()
    if latents.noise is not None:
        out[f"{cls}/num_noise"] = np.asarray(len(latents.noise))
        for i, n in enumerate(latents.noise):
            put(out, f"noise{i}{suffix}", n.numpy())   # the same for every class that has noise heads


def main():
    enc_mod, auto_mod = load_reference_encoders()
    x = torch.from_numpy(np.random.RandomState(7).uniform(-1, 1, (2, INPUT_DIM, SIZE, SIZE)).astype(np.float32))
    out = {"input": x.numpy(), "classes": np.asarray(CLASSES), "cfg": np.asarray([SIZE, LATENT, INPUT_DIM, GEN_SEED, GEN_N_MLP, GEN_CM]),
           "channel_sizes": np.asarray(sorted(CHANNELS)), "channel_values": np.asarray([CHANNELS[k] for k in sorted(CHANNELS)])}
    for cls in CLASSES:
        enc = getattr(enc_mod, cls)(SIZE, LATENT, INPUT_DIM, CHANNELS, stylegan_variant=2)
        randomise(enc)
        enc.eval()
        sd = enc.state_dict()
        out[f"{cls}/state_keys"] = np.asarray(list(sd.keys()))
        for k, v in sd.items():
            if k.startswith("resnet_blocks.0."):   # the same tensors as start_block.*
                assert torch.equal(v, sd["start_block." + k[len("resnet_blocks.0."):]])
            elif k.endswith("num_batches_tracked"):
                put(out, f"sd/{k}", v.numpy())
            else:
                assert torch.equal(v.half().float(), v), k
                put(out, f"sd/{k}", v.half().numpy())
        with torch.no_grad():
            record(out, cls, enc(x), "")
            record(out, cls, enc.double()(x.double()), "_f64")
        enc.float()
        if cls == "WPlusEncoder":
            ref = load_reference_stylegan2()
            g = ref.Generator(SIZE, LATENT, GEN_N_MLP, channel_multiplier=GEN_CM)
            g.load_state_dict(R.seeded_state_dict(SIZE, LATENT, GEN_N_MLP, GEN_CM, seed=GEN_SEED), strict=True)
            auto = auto_mod.StyleganAutoencoder(enc, g).eval()
            with torch.no_grad():
                out["autoencoder/image"] = auto(x).numpy()
                out["autoencoder/image_f64"] = auto.double()(x.double()).numpy()
            auto.float()
    path = os.path.join(ROOT, "tests", "golden", "encoder32.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
