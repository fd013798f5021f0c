"""Network factories of the synthesis path, under the reference's names
(/root/reference/stylegan_code_finder/networks/__init__.py):

* ``load_weights`` (:22-29)                      checkpoint dict -> ``network.load_state_dict`` (optional ``key``, ``strict``);
* ``get_stylegan2_generator`` (:36-41)           ``Generator(image_size, latent_size, n_mlp, channel_multiplier)`` + ``g_ema`` weights;
* ``get_swagan_generator`` (:354-362)            the same for the wavelet generator;
* ``get_autoencoder`` (:326-353, :390-412) / ``load_autoencoder_or_generator`` (:415-423)
                                                 the object ``generate_images(batch, autoencoder, ...)`` and
                                                 ``build_latent_and_noise_generator(autoencoder, ...)`` are handed.  With an
                                                 ``input_dim`` in the config the encoder the reference would build for
                                                 ``stylegan_variant`` 2 / ``'swagan'`` is built on the generator's own channel
                                                 map (``w_only``, ``two_stem`` + ``disable_update_for``, ``dropout_autoencoder``);
                                                 without one the holder carries the generator alone (``encode`` raises).  A config
                                                 with ``stylegan_checkpoint`` loads the whole autoencoder from the checkpoint's
                                                 ``'autoencoder'`` entry; the reference's fall-through for files without that
                                                 entry (the file itself as a bare state_dict) is not provided.

Imports of the model modules are deferred into the functions: ``networks`` is the package every model module lives in.  The one
exception is ``networks.encoder.autoencoder`` (torch and the ``Latents`` container only), whose classes are re-exported here
under the reference's names; the encoders themselves are imported where they are built.
"""
import argparse
from pathlib import Path
from typing import Union

import torch
from torch import nn


def load_weights(network: nn.Module, model_file: Union[str, Path], *, key: str = None, strict: bool = True,
                 convert: bool = False) -> nn.Module:
    if convert:
        raise NotImplementedError("convert_autoencoder_checkpoint belongs to the encoder research code (out of scope)")
    weights = torch.load(model_file, map_location='cpu')
    if key is not None and key in weights:
        weights = weights[key]
    network.load_state_dict(weights, strict=strict)
    return network


def get_stylegan2_generator(image_size, latent_size, n_mlp=8, channel_multiplier=2, init_ckpt=None, ckpt_key='g_ema',
                            strict=True):
    from networks.stylegan2.model import Generator
    generator = Generator(image_size, latent_size, n_mlp, channel_multiplier=channel_multiplier)
    if init_ckpt is not None:
        load_weights(generator, init_ckpt, key=ckpt_key, strict=strict)
    return generator


def get_swagan_generator(image_size, latent_size, n_mlp=8, channel_multiplier=2, init_ckpt=None, ckpt_key='g_ema',
                         strict=True):
    from networks.swagan.model import Generator
    generator = Generator(image_size, latent_size, n_mlp, channel_multiplier=channel_multiplier)
    if init_ckpt is not None:
        load_weights(generator, init_ckpt, key=ckpt_key, strict=strict)
    return generator


from networks.encoder.autoencoder import DropoutStyleganAutoencoder, StyleganAutoencoder, TwoStemStyleganAutoencoder  # noqa: E402,F401


def _encoder_classes(config: dict):
    """(autoencoder class, encoder class(es)) the reference's get_stylegan_2_based_autoencoder / get_swagan_based_autoencoder
    pick (:326-353, :390-393)."""
    from networks.encoder.u_net_like_encoder import NoiseEncoder, WNoNoiseEncoder, WPlusEncoder, WPlusNoNoiseEncoder, WWPlusEncoder
    w_only = bool(config.get('w_only', False))
    if config['stylegan_variant'] == 2:
        if config.get('two_stem', False):
            return TwoStemStyleganAutoencoder, (WNoNoiseEncoder if w_only else WPlusNoNoiseEncoder, NoiseEncoder)
        if config.get('code_dim', 0) > 0:
            raise NotImplementedError("stylegan2 code dim training not yet implemented")   # the reference's own message
        if config.get('dropout_autoencoder', False):
            return DropoutStyleganAutoencoder, (WWPlusEncoder if w_only else WPlusEncoder,)
    return StyleganAutoencoder, (WWPlusEncoder if w_only else WPlusEncoder,)


def get_autoencoder(config: dict, init_ckpt: str = None) -> Union[StyleganAutoencoder, TwoStemStyleganAutoencoder]:
    assert config['stylegan_variant'] in [1, 2, 'swagan'], "Stylegan Variant Unknown"
    if config['stylegan_variant'] == 1:
        raise NotImplementedError("StyleGAN1 is not on the MI355X hot path (SURVEY.md §2)")
    make = get_swagan_generator if config['stylegan_variant'] == 'swagan' else get_stylegan2_generator
    generator = make(config['image_size'], config['latent_size'], n_mlp=config.get('n_mlp', 8),
                     channel_multiplier=config.get('channel_multiplier', 2), init_ckpt=init_ckpt, strict=False)
    if config.get('input_dim') is None:
        return StyleganAutoencoder(None, generator)   # generator-only configs of the dataset tools
    autoencoder_class, encoder_classes = _encoder_classes(config)
    encoders = [cls(config['image_size'], config['latent_size'], config['input_dim'], generator.channels, stylegan_variant=2)
                for cls in encoder_classes]
    if autoencoder_class is TwoStemStyleganAutoencoder:
        disabled = config.get('disable_update_for', 'none')
        return TwoStemStyleganAutoencoder(*encoders, generator, update_latent=disabled in ['noise', 'none'],
                                          update_noise=disabled in ['latent', 'none'])
    return autoencoder_class(encoders[0], generator)


def load_autoencoder_or_generator(args: argparse.Namespace, config: dict) -> Union[StyleganAutoencoder, TwoStemStyleganAutoencoder]:
    autoencoder = get_autoencoder(config).to(args.device)
    # the reference decides by this key whether the checkpoint holds a full autoencoder or just the generator
    if 'stylegan_checkpoint' in config:
        if config.get('input_dim') is None:
            raise NotImplementedError("a full autoencoder checkpoint needs 'input_dim' in the config (the encoder's input channels)")
        weights = torch.load(args.checkpoint, map_location='cpu')
        if 'autoencoder' not in weights:
            raise NotImplementedError("the checkpoint has no 'autoencoder' entry: the reference then loads the file itself as a "
                                      "bare state_dict, which is not provided here; generator checkpoints ('g_ema') are "
                                      "loaded by configs without 'stylegan_checkpoint'")
        autoencoder.load_state_dict(weights['autoencoder'], strict=True)
        return autoencoder
    autoencoder.decoder = load_weights(autoencoder.decoder, args.checkpoint, key='g_ema')
    return autoencoder
