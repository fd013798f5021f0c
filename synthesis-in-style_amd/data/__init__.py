import argparse


def get_dataset_class(args: argparse.Namespace):
    """The autoencoder dataset a training / evaluation config asks for (reference: data/__init__.py:8-15): ``denoising`` first,
    then ``black_and_white_denoising``, else the plain one.  The import is deferred: ``data`` is the package the loaders of every
    other workload live in, and they need neither the library nor a device to be imported."""
    from data.autoencoder_dataset import AutoencoderDataset, BlackAndWhiteDenoisingAutoencoderDataset, DenoisingAutoencoderDataset
    if getattr(args, 'denoising', False):
        return DenoisingAutoencoderDataset
    if getattr(args, 'black_and_white_denoising', False):
        return BlackAndWhiteDenoisingAutoencoderDataset
    return AutoencoderDataset
