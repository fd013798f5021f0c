"""Shared by the encoder tests: the fixture tests/golden/encoder32.npz (tests/golden/make_golden_encoder.py) as modules of
this repository carrying the fixture's weights, and float64 torch restatements of the four encoder kernels."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder32.npz")


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def config():
    g = fixture()
    size, latent, input_dim, gen_seed, gen_n_mlp, gen_cm = (int(v) for v in g["cfg"])
    channels = {int(k): int(v) for k, v in zip(g["channel_sizes"], g["channel_values"])}
    return size, latent, input_dim, channels, gen_seed, gen_n_mlp, gen_cm


def state_keys(cls):
    return [str(k) for k in fixture()[f"{cls}/state_keys"]]


def state_dict(cls):
    g, sd = fixture(), {}
    for k in state_keys(cls):
        stored = "start_block." + k[len("resnet_blocks.0."):] if k.startswith("resnet_blocks.0.") else k
        v = torch.from_numpy(g[f"sd/{stored}"])
        sd[k] = v.float() if v.dtype == torch.float16 else v
    return sd


def build(cls):
    """This repository's encoder of that class with the fixture's weights, eval()."""
    import networks.encoder.u_net_like_encoder as E
    size, latent, input_dim, channels = config()[:4]
    enc = getattr(E, cls)(size, latent, input_dim, channels, stylegan_variant=2)
    enc.load_state_dict(state_dict(cls), strict=True)
    return enc.eval()


def expected(cls, suffix=""):
    """(latent or None, [noise maps] or None) the reference computed; suffix "_f64": with the module in double."""
    g = fixture()
    latent = g.get(f"{cls}/latent{suffix}")
    noise = [g[f"noise{i}{suffix}"] for i in range(int(g[f"{cls}/num_noise"]))] if f"{cls}/num_noise" in g else None
    return latent, noise


def named_outputs(latents):
    """{name: tensor} of a Latents result, as ``expected`` orders them."""
    out = {}
    if latents.latent is not None:
        out["latent"] = latents.latent
    for i, n in enumerate(latents.noise or []):
        out[f"noise{i}"] = n
    return out


def named_expected(cls, suffix=""):
    latent, noise = expected(cls, suffix)
    out = {} if latent is None else {"latent": latent}
    for i, n in enumerate(noise or []):
        out[f"noise{i}"] = n
    return out


def generator():
    """Generator(32) of the fixture's autoencoder case (weights from the oracle's seeded schema, as the fixture's script)."""
    from networks.stylegan2.model import Generator
    from oracle import stylegan2_ref as R
    size, latent, _, _, gen_seed, gen_n_mlp, gen_cm = config()
    g = Generator(size, latent, gen_n_mlp, channel_multiplier=gen_cm)
    g.load_state_dict(R.seeded_state_dict(size, latent, gen_n_mlp, gen_cm, seed=gen_seed), strict=True)
    return g.eval()


# ---- float64 restatements of the kernels (folded BatchNorm: scale, shift per channel)

def _cs(v):
    return v.double().view(1, -1, 1, 1)


def ref_conv3x3_s2(x, w1, scale1, shift1, wd=None, scale_d=None, shift_d=None):
    main = torch.relu(F.conv2d(x.double(), w1.double(), None, 2, 1) * _cs(scale1) + _cs(shift1))
    short = None if wd is None else F.conv2d(x.double(), wd.double(), None, 2) * _cs(scale_d) + _cs(shift_d)
    return main, short


def ref_stem(x, w1, scale1, shift1, wd, bias_d, scale_d, shift_d):
    main = torch.relu(F.conv2d(x.double(), w1.double(), None, 1, 1) * _cs(scale1) + _cs(shift1))
    short = F.conv2d(x.double(), wd.double(), None if bias_d is None else bias_d.double()) * _cs(scale_d) + _cs(shift_d)
    return main, short


def ref_block_tail(c, residual, scale, shift, noise_w=None, noise_b=None):
    y = c.double() * _cs(scale) + _cs(shift)
    y = torch.relu(y if residual is None else y + residual.double())
    noise = None if noise_w is None else F.conv2d(y, noise_w.double(), noise_b.double())
    return y, noise, y.mean(dim=(2, 3))


def ref_latent_heads(pooled, weights, biases):
    """pooled[i] [B, C_i] -> [B, latent] per head."""
    return [p.double() @ w.double().view(w.shape[0], -1).t() + b.double() for p, w, b in zip(pooled, weights, biases)]
