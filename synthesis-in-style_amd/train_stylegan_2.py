"""Train a StyleGAN2 / SWAGAN generator from a list of images: stage 1 of the pipeline (reference: train_stylegan_2.py:29-214).

    python train_stylegan_2.py configs/stylegan/stylegan_256px.yaml --images train.json -l logs -ln my_run

``--images`` is the JSON ``scripts/create_stylegan_train_dataset.py`` of the reference writes (image paths relative to the JSON).
The result -- ``{generator, discriminator, g_ema, generator_optimizer, discriminator_optimizer}`` snapshots under
``<log-dir>/<log-name>/`` -- is what ``create_dataset_for_segmentation.py`` and the catalog tools load (key ``g_ema``).

Wiring as the reference (:57-183): generator, discriminator and the averaged generator ``g_ema``; ``GradientClipAdam`` with the
lazy-regularisation correction ``lr * r``, ``betas = (0 ** r, 0.99 ** r)``, ``r = interval / (interval + 1)``; ``Stylegan2Updater``;
``accumulate(generator, 0)`` before the first step; ``CosineAnnealingLR(T_max = max_iter, eta_min = 1e-8)`` stepped every
iteration; a grid of ``display_size`` fixed latents rendered by ``g_ema`` every ``image_save_iter``; snapshots every
``snapshot_save_iter``.  What replaces the reference's third-party pieces:

* ``pytorch_training`` trainer / extensions -> the plain loop of ``train.py`` with its stdout log line;
* ``JSONDataset`` + ``DataLoader`` workers   -> ``data.gan_image_dataset``: every image decoded once, resident as uint8, a batch is
  one ``sis_gan_image_batch`` launch;
* wandb, ``--cache-root``                    -> accepted and ignored (one printed line);
* the FID extension (``--val-images``)        -> not built: it needs ``pytorch_fid`` and its Inception weights.

Differences kept small on purpose: the run directory is ``<log-dir>/<log-name>`` (the reference appends a time stamp under
``logs/``), and the grid uses the stored noise buffers of ``g_ema`` (``randomize_noise=False``), so a snapshot reproduces its grid.
More than one process (``torch.distributed.run``: RANK / WORLD_SIZE / LOCAL_RANK from the environment) wraps both networks in
DistributedDataParallel as the reference does and shards the image list by rank; that path has NOT been run on hardware.
"""
import argparse
import logging
import math
import os
import time
from pathlib import Path

import torch
import torch.distributed as dist
from torch.optim.lr_scheduler import CosineAnnealingLR

from train import load_yaml_config, merge_config_and_args, setup_distributed
from training.loop import get_current_reporter

SNAPSHOT_KEYS = ('generator', 'discriminator', 'g_ema', 'generator_optimizer', 'discriminator_optimizer')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Train a Stylegan 2 Generator")
    parser.add_argument("config", help="Path to yaml file holding train config")
    parser.add_argument("--resume-ckpt", default=None, type=str, help="Path to a snapshot to resume training from.")
    parser.add_argument("--images", required=True, help="path to json file holding a list of all images to use")
    parser.add_argument("--val-images", help="path to json holding validation images (accepted; the FID extension is not built)")
    parser.add_argument("--device", choices=['cpu', 'cuda'], default='cuda', help='Device to use')
    parser.add_argument('-l', '--log-dir', default='training', help="outputs path")
    parser.add_argument('-ln', '--log-name', default='training', help='name of the train run')
    parser.add_argument('--local_rank', type=int, default=0)
    parser.add_argument('--mpi-backend', default='gloo', choices=['nccl', 'gloo'], help="backend of torch.distributed")
    parser.add_argument('--cache-root', help='path to local cache (accepted and ignored: the images are resident on the device)')
    parser.add_argument("-s", "--stylegan-variant", type=str.lower, choices=["1", "2", 'swagan'], default="2",
                        help="which stylegan variant to use")
    parser.add_argument("--wandb-project-name", default="StyleGAN Training", help="accepted and ignored (no wandb)")
    parser.add_argument("--wandb-entity", help="accepted and ignored (no wandb)")
    parser.add_argument('--max-iter', dest='max_iter', type=int, help='stop after this many iterations')
    return parser.parse_args(argv)


def reg_ratio(interval) -> float:
    """Lazy regularisation (reference :79-80): a regulariser run every ``interval`` steps rescales lr and betas by this ratio."""
    return int(interval) / (int(interval) + 1)


def build_networks(config: dict):
    """(generator, discriminator, g_ema) on the CPU, ``g_ema`` in eval mode (reference :52-73)."""
    variant = str(config['stylegan_variant'])
    if variant == '1':
        raise NotImplementedError("StyleGAN1 is not on the MI355X hot path (SURVEY.md §2)")
    if variant == 'swagan':
        from networks.swagan import Discriminator, Generator
    else:
        from networks.stylegan2 import Discriminator, Generator
    make = lambda: Generator(config['image_size'], config['latent_size'], config['n_mlp'],   # noqa: E731
                             channel_multiplier=config['channel_multiplier'])
    generator, g_ema = make(), make()
    discriminator = Discriminator(config['image_size'], channel_multiplier=config['channel_multiplier'])
    g_ema.eval()
    return generator, discriminator, g_ema


def resume(networks: dict, path):
    """``--resume-ckpt``: the three networks from a snapshot (reference :75-77; the optimizers start fresh, as there, and the
    ``accumulate(generator, 0)`` that follows sets g_ema's parameters to the resumed generator's, as there)."""
    weights = torch.load(path, map_location='cpu')
    for name, network in networks.items():
        network.load_state_dict(weights[name], strict=True)


def build_optimizers(config: dict, generator, discriminator) -> dict:
    from training.fused_adam import GradientClipAdam
    out = {}
    for name, network, key in (('generator', generator, 'g_interval'), ('discriminator', discriminator, 'd_interval')):
        r = reg_ratio(config['regularization'][key])
        out[name] = GradientClipAdam(network.parameters(), lr=float(config['lr']) * r, betas=(0 ** r, 0.99 ** r))
    return out


def build_schedulers(config: dict, optimizers: dict) -> dict:
    # (the fused Adam copies lr / betas of its param_groups to the device at every eager step -- ``push_hyper`` -- so the value
    # the scheduler writes is the one the next step uses)
    return {name: CosineAnnealingLR(opt, int(config['max_iter']), eta_min=1e-8) for name, opt in optimizers.items()}


def build_loader(config: dict, device, rank: int = 0, world_size: int = 1):
    from data.gan_image_dataset import DeviceImageDataset, DeviceImageLoader
    dataset = DeviceImageDataset(config['images'], config['image_size'], input_dim=config.get('input_dim', 3), device=device)
    loader = DeviceImageLoader(dataset, int(config['batch_size']), shuffle=True, drop_last=True, rank=rank, world_size=world_size,
                               seed=int(config.get('seed', 0)))
    if len(loader) == 0:
        raise ValueError(f"batch_size {config['batch_size']} is larger than this rank's share of the {len(dataset)} images")
    return loader


def sample_latents(config: dict, device) -> torch.Tensor:
    """The fixed latents of the sample grid: ``display_size`` rows, seeded by the config's ``seed`` (default 0)."""
    rng = torch.Generator().manual_seed(int(config.get('seed', 0)))
    return torch.randn(int(config.get('display_size', 16)), int(config['latent_size']), generator=rng).to(device)


def render_grid(g_ema, sample_z: torch.Tensor, batch_size: int):
    """uint8 [rows * S, cols * S, 3] (host): ``g_ema`` on the fixed latents with its stored noise, cols = ceil(sqrt(n))."""
    import numpy
    import sis_hip
    tiles = []
    with torch.no_grad():
        for lo in range(0, len(sample_z), batch_size):
            image, _ = g_ema([sample_z[lo:lo + batch_size]], randomize_noise=False)
            tiles.append(sis_hip.make_image_u8(image).cpu().numpy())
    tiles = numpy.concatenate(tiles, 0)
    n, s = tiles.shape[0], tiles.shape[1]
    cols = math.ceil(math.sqrt(n))
    rows = -(-n // cols)
    grid = numpy.zeros((rows * s, cols * s, 3), dtype=numpy.uint8)
    for i in range(n):
        r, c = divmod(i, cols)
        grid[r * s:(r + 1) * s, c * s:(c + 1) * s] = tiles[i]
    return grid


def save_grid(grid, path: Path):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(grid).save(path, format='PNG')


def main(args: argparse.Namespace, rank: int = 0, world_size: int = 1):
    """Returns the logged observations of rank 0: [(iteration, {name: value})]."""
    from training_builder.base_train_builder import Snapshotter
    from updater.stylegan_2_updater import Stylegan2Updater
    config = merge_config_and_args(load_yaml_config(args.config), args)
    if config['device'] != 'cuda' or not torch.cuda.is_available():
        raise RuntimeError("train_stylegan_2.py needs a HIP device: the networks run on this project's kernels, there is no CPU path")
    if rank == 0:
        if config.get('cache_root') is not None or config.get('wandb_entity') is not None:
            print("--cache-root / --wandb-*: accepted and ignored (images are resident on the device; logging goes to stdout)", flush=True)
        if config.get('val_images'):
            print("--val-images: accepted and unused (the FID extension is not built)", flush=True)
    if world_size > 1:
        setup_distributed(args.mpi_backend, rank, world_size)
    local_rank = int(os.environ.get('LOCAL_RANK', args.local_rank)) if world_size > 1 else torch.cuda.current_device()
    device = torch.device('cuda', local_rank % torch.cuda.device_count())
    torch.cuda.set_device(device)
    if 'polyphase_downsample' in config:
        import networks.stylegan2.discriminator as discriminator_module
        discriminator_module._POLYPHASE = bool(config['polyphase_downsample'])

    generator, discriminator, g_ema = build_networks(config)
    if config.get('resume_ckpt') is not None:
        resume({'generator': generator, 'discriminator': discriminator, 'g_ema': g_ema}, config['resume_ckpt'])
    generator, discriminator, g_ema = generator.to(device), discriminator.to(device), g_ema.to(device)
    optimizers = build_optimizers(config, generator, discriminator)
    bare = {'generator': generator, 'discriminator': discriminator}
    if world_size > 1:
        from torch.nn.parallel import DistributedDataParallel as DDP
        generator = DDP(generator, device_ids=[device.index], broadcast_buffers=False, output_device=device.index)
        discriminator = DDP(discriminator, device_ids=[device.index], broadcast_buffers=False, output_device=device.index)
    loader = build_loader(config, device, rank, world_size)
    updater = Stylegan2Updater(iterators={'images': loader}, networks={'generator': generator, 'discriminator': discriminator},
                               optimizers=optimizers, device=device, copy_to_device=world_size == 1,
                               regularization_options=config['regularization'],   # (as is: the key quirk of SURVEY.md §567 is kept)
                               style_mixing_prob=float(config['style_mixing_prob']), latent_size=int(config['latent_size']), g_ema=g_ema,
                               freeze_stochastic_noise_layers=config.get('freeze_stochastic_noise_layers', False))
    updater.accumulate(generator, 0)
    schedulers = build_schedulers(config, optimizers)
    run_dir = Path(config['log_dir']) / config['log_name']
    snapshotter = sample_z = None
    if rank == 0:
        snapshotter = Snapshotter({**bare, 'g_ema': g_ema, 'generator_optimizer': optimizers['generator'],
                                   'discriminator_optimizer': optimizers['discriminator']}, run_dir, int(config['snapshot_save_iter']))
        sample_z = sample_latents(config, device)
    if world_size > 1:
        dist.barrier()
    logging.info('Setup complete. Starting training...')
    history, t0 = [], time.perf_counter()
    try:
        for it in range(1, int(config['max_iter']) + 1):
            updater.update()
            for scheduler in schedulers.values():
                scheduler.step()
            if rank != 0:
                continue
            snapshotter.maybe_save(it)
            if it % int(config['image_save_iter']) == 0:
                save_grid(render_grid(g_ema, sample_z, int(config['batch_size'])), run_dir / 'images' / f"{it:06d}.png")
            if it % int(config.get('log_iter', 10)) == 0:
                obs = get_current_reporter().scalars()
                rate = it * int(config['batch_size']) * world_size / (time.perf_counter() - t0)
                print(f"iter {it} " + " ".join(f"{k}={v:.5f}" for k, v in obs.items()) + f" images/s={rate:.1f}", flush=True)
                history.append((it, obs))
    finally:
        if world_size > 1:
            dist.destroy_process_group()
    logging.info('Training finished')
    return history


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    cli = parse_args()
    if 'RANK' in os.environ:   # launched by torch.distributed.run: one process per GPU
        main(cli, int(os.environ['RANK']), int(os.environ.get('WORLD_SIZE', '1')))
    else:
        main(cli, 0, 1)
