"""Fit the k-means activation catalogs of a trained generator on the MI355X: the reference's create_semantic_segmentation.py
(main :164-187, get_activations :67-93, find_and_render_clusters :114-129, save_* :132-161).

Seeded latents are streamed through the generator as the dataset CLI does; each batch's activations are copied into
preallocated per-layer device buffers ``[n, C, H, W]`` (the reference moves all of them to the host: 12.3 GB for -n 100); per
layer every cluster count of the range is fitted in one batched run (MiniBatchSphericalKMeans.fit_many); written under the
destination:

  catalogs/{k}/centres_{layer}.npy   float32 [k, C] unit centres
  catalogs/{k}.json                  {"catalogs": {layer: path}, "id_to_size_map", "n_iter", "inertia", "counts"}: its "catalogs"
                                     entry is what create_dataset_for_segmentation.py's config takes
  cluster_arrays/{k}.npz             per layer the colour rendering uint8 [n, 3, H, W] of the label map (and the images)
  cluster_images/{k}.png             the renderings, nearest-resized to the largest layer, one row per layer

``-i FILE`` (a JSON list of image paths, relative to the file) fits the catalogs on real pages instead: each image goes through the
reference's transform (utils/data_loading.py:38-42: PIL resize to image_size x image_size, / 255, (x - 0.5) / 0.5), the
projection autoencoder encodes it, and the activations are those of decoding its latents (get_activations :74-86).  It needs
a checkpoint with an ``'autoencoder'`` entry (``--w-only`` / ``--two-stem`` say which encoder the entry belongs to); without one
``-i`` raises ``NotImplementedError``.

Not reproduced: the pickled catalog objects (the .npy / .json pair replaces them).
"""
import argparse
import json
from pathlib import Path

import numpy
import torch

import sis_hip
from create_dataset_for_segmentation import add_generator_precision_argument, apply_generator_precision, load_generator
from segmentation.gan_local_edit.spherical_kmeans import MiniBatchSphericalKMeans
from utils.dataset_creation import seeded_latents

# the reference's COLOR_MAP (:23-46) as RGB triples
COLOR_MAP = [(0, 179, 255), (117, 62, 128), (0, 104, 255), (215, 189, 166), (32, 0, 193), (98, 162, 206), (102, 112, 129),
             (52, 125, 0), (142, 118, 246), (138, 83, 0), (92, 122, 255), (122, 55, 83), (0, 142, 255), (81, 40, 179),
             (0, 200, 244), (13, 24, 127), (0, 170, 147), (21, 51, 89), (19, 58, 241), (22, 44, 35)]


def palette(k, device=None):
    """uint8 [k, 3]: colour of cluster id i (the map repeats after 20)."""
    return torch.tensor([COLOR_MAP[i % len(COLOR_MAP)] for i in range(k)], dtype=torch.uint8, device=device)


def render_clusters(labels, k):
    """int64 [n, H, W] label map -> uint8 [n, 3, H, W] colours (cluster_id_to_image :100-111, from the label map)."""
    return palette(k, labels.device)[labels].permute(0, 3, 1, 2).contiguous()


def prepare_output_dir(args):
    dest = Path(args.destination)
    if not dest.is_absolute() and args.checkpoint:
        dest = Path(args.checkpoint).parent.parent / dest
    dest.mkdir(exist_ok=True, parents=True)
    return dest


def get_activations(args, g, device):
    """-> ({layer: float32 [n, C, H, W] on the device}, uint8 [n, 3, S, S] images on the host)."""
    n, buffers, images = args.num_samples, None, []
    torch.random.manual_seed(args.seed)
    with torch.no_grad():
        for first in range(0, n, args.batch_size):
            m = min(args.batch_size, n - first)
            z = seeded_latents(args.batch_size, g.style_dim, device)[:m]
            image, acts = g([z.to(device, non_blocking=True)], noise=g.make_noise(), return_intermediate_activations=True)
            if buffers is None:
                buffers = {key: torch.empty((n,) + tuple(a.shape[1:]), dtype=torch.float32, device=device) for key, a in acts.items()
                           if args.strip_activations_from is None
                           or (a.shape[-2] > args.strip_activations_from and a.shape[-1] > args.strip_activations_from)}
            for key, buf in buffers.items():
                buf[first:first + m] = acts[key]
            images.append(sis_hip.make_image_u8(image).permute(0, 3, 1, 2).cpu())
    return buffers, torch.cat(images).numpy()


def load_image_batch(paths, image_size, input_dim, device):
    """The reference's data-loader transform (utils/data_loading.py:38-42) for a list of files -> float32 [n, input_dim, S, S]."""
    from PIL import Image
    out = torch.empty((len(paths), input_dim, image_size, image_size), dtype=torch.float32)
    for i, path in enumerate(paths):
        with Image.open(path) as handle:
            image = handle.convert('L' if input_dim == 1 else 'RGB').resize((image_size, image_size), Image.BILINEAR)
        pixels = torch.from_numpy(numpy.asarray(image, dtype=numpy.uint8).reshape(image_size, image_size, input_dim).copy())
        out[i] = (pixels.permute(2, 0, 1).float() / 255 - 0.5) / 0.5
    return out.to(device)


def load_autoencoder(args, device):
    """The projection autoencoder of a checkpoint's 'autoencoder' entry (networks.load_autoencoder_or_generator, which raises
    NotImplementedError for a checkpoint without the entry); without a checkpoint there is nothing to encode with."""
    import networks
    if not args.checkpoint:
        raise NotImplementedError("-i/--images needs the projection autoencoder: a checkpoint that holds an 'autoencoder' entry")
    config = {'stylegan_variant': 2, 'image_size': args.image_size, 'latent_size': args.latent_size, 'n_mlp': args.n_mlp,
              'channel_multiplier': args.channel_multiplier, 'input_dim': args.input_dim, 'w_only': args.w_only,
              'two_stem': args.two_stem, 'disable_update_for': 'none', 'stylegan_checkpoint': args.checkpoint}
    return networks.load_autoencoder_or_generator(argparse.Namespace(device=device, checkpoint=args.checkpoint), config).eval()


def get_image_activations(args, autoencoder, device):
    """``get_activations`` for ``-i``: encode the listed images, decode the latents, keep the decode's activations."""
    from utils.dataset_creation import generate_images
    list_file = Path(args.images)
    with open(list_file) as f:
        paths = [str(list_file.parent / p) for p in json.load(f)][:args.num_samples]
    if not paths:
        raise ValueError(f"{list_file} lists no images")
    n, buffers, images = len(paths), None, []
    for first in range(0, n, args.batch_size):
        batch = {'input_image': load_image_batch(paths[first:first + args.batch_size], args.image_size, args.input_dim, device)}
        acts, image = generate_images(batch, autoencoder, device)
        if buffers is None:
            buffers = {key: torch.empty((n,) + tuple(a.shape[1:]), dtype=torch.float32, device=device) for key, a in acts.items()
                       if args.strip_activations_from is None
                       or (a.shape[-2] > args.strip_activations_from and a.shape[-1] > args.strip_activations_from)}
        for key, buf in buffers.items():
            buf[first:first + image.shape[0]] = acts[key]
        images.append(sis_hip.make_image_u8(image).permute(0, 3, 1, 2).cpu())
    return buffers, torch.cat(images).numpy()


def find_clusters(activations, cluster_counts, **fit_args):
    """{k: {layer: fitted MiniBatchSphericalKMeans}}: per layer one batched run over all cluster counts."""
    found = {k: {} for k in cluster_counts}
    for layer, act in activations.items():
        for k, model in zip(cluster_counts, MiniBatchSphericalKMeans.fit_many(act, list(cluster_counts), compute_labels=True, **fit_args)):
            found[k][layer] = model
    return found


def save_catalogs(models, activations, k, dest_dir):
    cat_dir = dest_dir / 'catalogs' / str(k)
    cat_dir.mkdir(parents=True, exist_ok=True)
    meta = {"catalogs": {}, "id_to_size_map": {}, "n_iter": {}, "inertia": {}, "counts": {}}
    for layer, model in models.items():
        path = (cat_dir / f"centres_{layer}.npy").resolve()
        numpy.save(str(path), model.cluster_centers_)
        meta["catalogs"][str(layer)] = str(path)
        meta["id_to_size_map"][str(layer)] = f"{activations[layer].shape[-2]}x{activations[layer].shape[-1]}"
        meta["n_iter"][str(layer)] = model.n_iter_
        meta["inertia"][str(layer)] = model.inertia_
        meta["counts"][str(layer)] = [int(c) for c in model.label_counts_]
    with open(dest_dir / 'catalogs' / f"{k}.json", "w") as f:
        json.dump(meta, f, indent=1)


def save_cluster_visualizations(rendered, k, dest_dir):
    """rendered: {key: uint8 [n, 3, H, W]} (numpy)."""
    from PIL import Image
    array_path = dest_dir / 'cluster_arrays' / f"{k}.npz"
    array_path.parent.mkdir(parents=True, exist_ok=True)
    numpy.savez_compressed(str(array_path), **{str(key): v for key, v in rendered.items()})
    largest = max(v.shape[-1] for v in rendered.values())
    rows = []
    for v in rendered.values():
        rep = largest // v.shape[-1]
        up = v.repeat(rep, axis=2).repeat(rep, axis=3) if rep > 1 else v   # nearest
        rows.append(numpy.concatenate(list(up.transpose(0, 2, 3, 1)), axis=1))   # samples side by side
    image_path = dest_dir / 'cluster_images' / f"{k}.png"
    image_path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(numpy.concatenate(rows, axis=0)).save(str(image_path))


def main(args):
    lo, hi = args.cluster_range
    if not 1 <= lo < hi <= sis_hip.SKM_KMAX + 1:
        raise ValueError(f"cluster range {lo} {hi}: counts 1 .. {sis_hip.SKM_KMAX} are supported (the upper end is exclusive)")
    device = torch.device('cuda', 0)
    if args.images is not None:
        autoencoder = load_autoencoder(args, device)   # raises without an 'autoencoder' checkpoint, before anything is written
        torch.cuda.set_device(device)
        dest = prepare_output_dir(args)
        activations, images = get_image_activations(args, autoencoder, device)
    else:
        torch.cuda.set_device(device)
        dest = prepare_output_dir(args)
        g = load_generator(args.checkpoint, args.image_size, args.latent_size, args.n_mlp, args.channel_multiplier, device)
        apply_generator_precision(g, args)
        activations, images = get_activations(args, g, device)
    if not activations:
        raise ValueError("no activation layer is left after --strip-activations-from")
    counts = list(range(lo, hi))
    found = find_clusters(activations, counts, random_state=args.random_state)
    for k in counts:
        save_catalogs(found[k], activations, k, dest)
        rendered = {layer: render_clusters(m.labels_.reshape(activations[layer].shape[0], *activations[layer].shape[-2:]), k).cpu().numpy()
                    for layer, m in found[k].items()}
        rendered[max(rendered.keys()) + 1] = images
        save_cluster_visualizations(rendered, k, dest)
    torch.cuda.synchronize()
    return dest, found


def build_parser():
    parser = argparse.ArgumentParser(description="Fit k-means catalogs on the activations of a StyleGAN2 generator on MI355X")
    parser.add_argument("checkpoint", nargs='?', default=None, help="generator checkpoint holding 'g_ema' (omit: random weights)")
    parser.add_argument("--destination", default='semantic_segmentation',
                        help="where to save; a relative path is taken from the second parent directory of the checkpoint")
    parser.add_argument("-b", "--batch-size", default=10, type=int, help="batch size for generation of images")
    parser.add_argument("-n", "--num-samples", default=100, type=int, help="number of samples the clusters are fitted on")
    parser.add_argument("-c", "--cluster-range", nargs=2, default=[3, 24], type=int, help="cluster counts LO .. HI - 1")
    parser.add_argument("-i", "--images", help="JSON list of image paths (relative to the file): fit on the activations of their "
                                               "reconstructions; needs a checkpoint with an 'autoencoder' entry")
    parser.add_argument("--input-dim", type=int, default=3, choices=[1, 3], help="channels of the images the encoder takes")
    parser.add_argument("--w-only", action="store_true", help="the checkpoint's encoder predicts one W latent (WWPlusEncoder)")
    parser.add_argument("--two-stem", action="store_true", help="the checkpoint holds a two-stem autoencoder")
    parser.add_argument("-s", "--strip-activations-from", type=int, help="drop all activations of this size or smaller")
    parser.add_argument("--image-size", type=int, default=256)
    parser.add_argument("--latent-size", type=int, default=512)
    parser.add_argument("--n-mlp", type=int, default=8)
    parser.add_argument("--channel-multiplier", type=int, default=2)
    parser.add_argument("--seed", type=int, default=1, help="seed of the latent stream")
    parser.add_argument("--random-state", type=int, default=0, help="seed of the fit plans")
    add_generator_precision_argument(parser)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
