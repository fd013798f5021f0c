"""Maker of tests/golden/dataset_gan.npz: the UNMODIFIED reference PixelClassifier / PixelEnsembleClassifier
(networks/pixel_classifier/model.py of the reference tree) on the CPU, imported by file path with the bare packages of
oracle/load_reference.py (a fresh process).

Restated here, not imported: ``scale_activations`` (data/dataset_gan_dataset.py:12-34; its module needs torchvision) with the
feature tensor allocated on the CPU instead of 'cuda' (:22), and ``PixelEnsembleClassifier.predict_classes`` with its
prediction stack allocated on the CPU instead of 'cuda' (model.py:41).  Everything else is the reference's code.

Config: B = 2 activations of a 32^2 generator-like dict (two layers each at 4, 8, 16 and 32 pixels, F = 384), an ensemble of
N = 3 members with 3 classes; weights and activations come from the seeded numpy functions below, so the archive holds only
outputs: the state_dict keys / shapes of both hidden variants, every member's logits, the voted labels, and the CPU
``torch.mode`` results of tie rows.  The GPU test imports this module for ``seeded_member`` / ``seeded_activations`` /
``CONFIG`` (the reference is imported only inside ``main``).

    python tests/golden/make_golden_dataset_gan.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIG = dict(batch=2, size=32, layers=((0, 64, 4), (1, 64, 4), (2, 64, 8), (3, 64, 8), (4, 32, 16), (5, 32, 16),
                                        (6, 32, 32), (7, 32, 32)), classes=3, members=3)


def member_schema(classes, dim):
    h1, h2 = (128, 32) if classes < 32 else (256, 128)
    return [('layers.0.weight', (h1, dim)), ('layers.0.bias', (h1,)),
            ('layers.2.weight', (h1,)), ('layers.2.bias', (h1,)), ('layers.2.running_mean', (h1,)),
            ('layers.2.running_var', (h1,)), ('layers.2.num_batches_tracked', ()),
            ('layers.3.weight', (h2, h1)), ('layers.3.bias', (h2,)),
            ('layers.5.weight', (h2,)), ('layers.5.bias', (h2,)), ('layers.5.running_mean', (h2,)),
            ('layers.5.running_var', (h2,)), ('layers.5.num_batches_tracked', ()),
            ('layers.6.weight', (classes, h2)), ('layers.6.bias', (classes,))]


def seeded_member(classes, dim, seed):
    """A member state_dict with non-trivial BatchNorm statistics: Linear weights ~ N(0, 1/fan_in), biases ~ 0.1 N(0, 1),
    BN scales ~ U(0.5, 1.5), shifts ~ 0.1 N(0, 1), running means ~ 0.3 N(0, 1), running variances ~ U(0.2, 2).  Linear
    weight rows are centred."""
    rng = np.random.RandomState(seed)
    sd = {}
    for key, shape in member_schema(classes, dim):
        if key.endswith('num_batches_tracked'):
            sd[key] = torch.tensor(10, dtype=torch.int64)
        elif key.endswith('running_mean'):
            sd[key] = torch.from_numpy((0.3 * rng.randn(*shape)).astype(np.float32))
        elif key.endswith('running_var'):
            sd[key] = torch.from_numpy(rng.uniform(0.2, 2.0, shape).astype(np.float32))
        elif key in ('layers.2.weight', 'layers.5.weight'):
            sd[key] = torch.from_numpy(rng.uniform(0.5, 1.5, shape).astype(np.float32))
        elif key.endswith('bias'):
            sd[key] = torch.from_numpy((0.1 * rng.randn(*shape)).astype(np.float32))
        else:   # rows of zero mean: the classes' mean logits stay close, so the labels vary over the image
            w = rng.randn(*shape) / np.sqrt(shape[1])
            sd[key] = torch.from_numpy((w - w.mean(1, keepdims=True)).astype(np.float32))
    return sd


def seeded_activations(layers=None, batch=None, seed=11):
    """{key: float32 [B, c, r, r]} ~ N(0, 1) for ``layers`` = ((key, c, r), ...)."""
    rng = np.random.RandomState(seed)
    batch = CONFIG['batch'] if batch is None else batch
    return {k: torch.from_numpy(rng.randn(batch, c, r, r).astype(np.float32)) for k, c, r in (layers or CONFIG['layers'])}


def tie_rows():
    """Member-label rows whose majority is tied: every order of three distinct labels (N = 3) and 2-2 splits (N = 4)."""
    import itertools
    rows3 = [list(p) for p in itertools.permutations([0, 1, 2])] + [list(p) for p in itertools.permutations([1, 4, 2])]
    rows4 = [list(p) for p in sorted(set(itertools.permutations([0, 0, 2, 2])))] + \
        [list(p) for p in sorted(set(itertools.permutations([1, 3, 3, 1])))]
    return np.array(rows3, dtype=np.float32), np.array(rows4, dtype=np.float32)


def scale_activations_cpu(activations, upsamplers):
    """data/dataset_gan_dataset.py:12-34 with the tensor on the CPU (the reference allocates it on 'cuda', :22)."""
    scaled = []
    for entry in activations:
        batch_size = entry[0].shape[0]
        image_size = entry[0].shape[2] * int(upsamplers[0].scale_factor)
        feature_size = sum([e.shape[1] for e in entry.values()])
        image_activations = torch.empty((batch_size, image_size, image_size, feature_size))
        feature_index = 0
        for idx, activation in entry.items():
            up = upsamplers[idx](activation).squeeze()
            new_index = feature_index + up.shape[1]
            image_activations[:, :, :, feature_index:new_index] = torch.moveaxis(up, 1, -1)
            feature_index = new_index
        scaled.append(image_activations)
    return scaled


def ensemble_predict_classes_cpu(ensemble, x):
    """model.py:40-49 with the prediction stack on the CPU (the reference allocates it on 'cuda', :41)."""
    predictions = torch.zeros((x.shape[0], len(ensemble.networks)))
    for i, model in enumerate(ensemble.networks.values()):
        predictions[:, i] = model.predict_classes(x).squeeze()
    return torch.mode(predictions).values


def main():
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle.load_reference import load_reference_segmenters
    load_reference_segmenters()
    R = importlib.import_module('networks.pixel_classifier.model')
    torch.manual_seed(0)
    out = {}
    dim = sum(c for _, c, _ in CONFIG['layers'])
    for tag, classes in (('small', 3), ('large', 34)):
        sd = R.PixelClassifier(classes, dim).state_dict()
        out[f'keys_{tag}'] = np.array(list(sd))
        out[f'shapes_{tag}'] = np.array([','.join(map(str, t.shape)) for t in sd.values()])
    ensemble = R.PixelEnsembleClassifier(CONFIG['classes'], CONFIG['size'], 0)
    for n in range(CONFIG['members']):
        m = R.PixelClassifier(CONFIG['classes'], dim)
        m.load_state_dict(seeded_member(CONFIG['classes'], dim, seed=100 + n))
        m.eval()
        ensemble.add_network(m)
    acts = seeded_activations()
    upsamplers = [torch.nn.Upsample(scale_factor=CONFIG['size'] / a.shape[-1], mode='bilinear') for a in acts.values()]
    with torch.no_grad():
        scaled = scale_activations_cpu([acts], upsamplers)[0]
        x = scaled.reshape(-1, dim)
        out['logits'] = np.stack([m(x).numpy() for m in ensemble.networks.values()])
        out['labels'] = ensemble_predict_classes_cpu(ensemble, x).reshape(CONFIG['batch'], CONFIG['size'],
                                                                          CONFIG['size']).numpy()
    rows3, rows4 = tie_rows()
    out['mode_cpu3'] = torch.mode(torch.from_numpy(rows3)).values.numpy()
    out['mode_cpu4'] = torch.mode(torch.from_numpy(rows4)).values.numpy()
    np.savez_compressed(os.path.join(HERE, 'dataset_gan.npz'), **out)


if __name__ == '__main__':
    main()
