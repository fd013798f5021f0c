"""Encoder + generator pairs of the reference (networks/encoder/autoencoder.py): ``StyleganAutoencoder`` (:13-52),
``DropoutStyleganAutoencoder`` (:55-68) and ``TwoStemStyleganAutoencoder`` (:137-196) with their ``forward``, ``encode``,
``is_wplus``, ``trainable_parameters(as_groups=...)`` and ``use_generated_noise``.  The code-, style- and super-resolution
variants belong to the StyleGAN1 factories and are not rebuilt.  ``encoder`` may be ``None``: the generator-only holder
``networks.get_autoencoder`` returns for configs without an ``input_dim``; ``encode`` then raises."""
import random
from itertools import chain
from typing import Dict, Iterator, List, Sequence, Union

import torch
from torch import nn
from torch.nn import Parameter

from latent_projecting import Latents


def _grouped(networks, recurse, as_groups) -> List[Dict[str, list]]:
    """[{'params': everything no group claims}, {'params': group 0}, ...]: a parameter joins the first group one of whose keys
    is a substring of its name."""
    rest, groups = [], [[] for _ in as_groups]
    for network in networks:
        for name, param in network.named_parameters(recurse=recurse):
            hit = next((i for i, keys in enumerate(as_groups) if any(key in name for key in keys)), None)
            (rest if hit is None else groups[hit]).append(param)
    return [{'params': params} for params in [rest] + groups]


class StyleganAutoencoder(nn.Module):

    def __init__(self, encoder, decoder):
        super().__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.use_generated_noise = True

    def is_wplus(self, latents: Latents) -> bool:
        return len(latents.latent.shape) == 3

    def encode(self, x: torch.Tensor) -> Latents:
        if self.encoder is None:
            raise NotImplementedError("this autoencoder holds a generator only: build it from a config with 'input_dim' "
                                      "(networks.get_autoencoder) to get an encoder")
        return self.encoder(x)

    def decode(self, latents: Latents, noise=None) -> torch.Tensor:
        image, _ = self.decoder([latents.latent], input_is_latent=self.is_wplus(latents), noise=latents.noise if noise is None else noise)
        return image

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        latents = self.encode(x)
        if not self.use_generated_noise:
            latents.noise = self.decoder.make_noise()
        return self.decode(latents)

    def trainable_parameters(self, recurse: bool = True, as_groups: Sequence[Sequence[str]] = None) \
            -> Union[Iterator[Parameter], List[Dict[str, list]]]:
        if as_groups is None:
            return self.encoder.parameters(recurse=recurse)
        return _grouped([self.encoder], recurse, as_groups)


class DropoutStyleganAutoencoder(StyleganAutoencoder):
    """Each predicted noise map is replaced by a random one with probability ``dropout_ratio`` (Python's ``random``)."""

    def __init__(self, *args, dropout_ratio=0.5, **kwargs):
        super().__init__(*args, **kwargs)
        self.dropout_ratio = dropout_ratio

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        latents = self.encode(x)
        mixed = [predicted if random.random() > self.dropout_ratio else drawn
                 for predicted, drawn in zip(latents.noise, self.decoder.make_noise())]
        return self.decode(latents, noise=mixed)


class TwoStemStyleganAutoencoder(nn.Module):
    """Latents from one encoder, noise maps from another; a stem whose update is disabled is left out of
    ``trainable_parameters`` (the noise stem is then not run: random noise takes its place).

    One deliberate difference from the reference's ``encode`` (:187-196): it wraps the latent stem in
    ``torch.set_grad_enabled(self.update_latent)``, which also switches autograd ON inside a caller's ``torch.no_grad()``.  Here
    the stem runs under ``update_latent and torch.is_grad_enabled()``: a disabled stem is still cut off from autograd, but an
    inference call stays an inference call (and so stays on the encoder kernels)."""

    def __init__(self, latent_encoder, noise_encoder, decoder, update_latent=True, update_noise=True):
        super().__init__()
        self.latent_encoder = latent_encoder
        self.noise_encoder = noise_encoder
        self.decoder = decoder
        self.update_latent = update_latent
        self.update_noise = update_noise
        assert update_latent or update_noise, "'update_latent' or 'update_noise' must be true for Two Stem Autoencoder"

    @property
    def encoder(self):
        return self.latent_encoder

    def is_wplus(self, latents: Latents) -> bool:
        return len(latents.latent.shape) == 3

    def encode(self, x: torch.Tensor) -> Latents:
        with torch.set_grad_enabled(self.update_latent and torch.is_grad_enabled()):
            latent = self.latent_encoder(x).latent
        noise = self.noise_encoder(x).noise if self.update_noise else self.decoder.make_noise()
        return Latents(latent=latent, noise=noise)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        latents = self.encode(x)
        image, _ = self.decoder([latents.latent], input_is_latent=self.is_wplus(latents), noise=latents.noise)
        return image

    def _stems(self):
        return ([self.latent_encoder] if self.update_latent else []) + ([self.noise_encoder] if self.update_noise else [])

    def trainable_parameters(self, recurse: bool = True, as_groups: Sequence[Sequence[str]] = None) \
            -> Union[Iterator[Parameter], List[Dict[str, list]]]:
        if as_groups is None:
            return chain.from_iterable(network.parameters(recurse=recurse) for network in self._stems())
        return _grouped(self._stems(), recurse, as_groups)
