"""Device half of the weight-state family (tests/weight_state_checks.py): after every way this project writes weights, the next
forward of the fused inference paths -- the generator's, the projection encoder's -- computes what a freshly constructed module
with the same state computes, bit for bit and in every intermediate activation; a forward with no write in front of it launches no
prepack kernel.  The reference is the same kernels on the same weights, so there is no tolerance anywhere.

Then the two places where a stale image was a wrong training run: the generator as the discriminator step sees it
(``UpdateDisabler``, grad enabled) after two ``update()`` calls with the optimizers ``train_stylegan_2.py`` builds, and the second
sample grid of a ``train_stylegan_2.main`` run against the snapshot written at the same iteration."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

import weight_state_checks as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "synthesis-in-style_amd")
SMALL = dict(image_size=32, batch_size=4, n_mlp=2, latent_size=64, channel_multiplier=1, max_iter=4, snapshot_save_iter=2, image_save_iter=2,
             log_iter=1, display_size=4)   # the end-to-end test's configuration (tests/test_train_stylegan2_gpu.py), one iteration longer
BATCH = 2


@pytest.fixture
def records(monkeypatch):
    """Every launch of the library's kernels while the test runs: (kernel, flops, bytes, event, event)."""
    import sis_hip
    for name in ("SIS_WINOGRAD", "SIS_WINO24", "SIS_GEN_PRECISION", "SIS_ENCODER_HIP", "SIS_UP_FIR"):
        monkeypatch.delenv(name, raising=False)
    out = []
    sis_hip.set_profiler(out)
    yield out
    sis_hip.set_profiler(None)


def _prepacks(records):
    return [r[0] for r in records if "prepack" in r[0]]


def _convolutions(records):
    return [r[0] for r in records if "modconv" in r[0] and "prepack" not in r[0]]


# ---------------------------------------------------------------------------------------------------------------- the generator
def _generator(seed, device, precision=None, size=SMALL["image_size"]):
    from networks.stylegan2.model import Generator
    g = W.seeded(lambda: Generator(size, SMALL["latent_size"], SMALL["n_mlp"], channel_multiplier=SMALL["channel_multiplier"]), seed)
    return g.set_matrix_precision(precision).to(device).eval()


def _generator_inputs(device, size):
    gen = torch.Generator().manual_seed(17)
    z = torch.randn(BATCH, SMALL["latent_size"], generator=gen).to(device)
    sides = [4] + [2 ** i for i in range(3, size.bit_length()) for _ in range(2)]   # 32: 4, 8, 8, 16, 16, 32, 32
    noise = [torch.randn(1, 1, s, s, generator=gen).to(device) for s in sides]
    return z, noise


def _fused_run(device, records, grad=False, must_contain=(), size=SMALL["image_size"]):
    """``run`` of ``assert_follows``: the generator's fused path on fixed latents and noise, every activation and the image.  That
    the modulated-convolution kernels ran is read from the profiler records: the autograd formulation launches none of them."""
    z, noise = _generator_inputs(device, size)

    def run(g):
        seen = len(records)
        with torch.set_grad_enabled(grad):
            image, acts = g([z], noise=noise, return_intermediate_activations=True)
        torch.cuda.synchronize(device)
        kernels = _convolutions(records[seen:])
        assert len(kernels) >= 4 and not image.requires_grad, f"the fused path did not run: {sorted(set(r[0] for r in records[seen:]))}"
        for name in must_contain:
            assert any(name in k for k in kernels), (name, sorted(set(kernels)))
        return {**{f"activation {k}": v for k, v in acts.items()}, "image": image}

    return run


@pytest.mark.parametrize("name", list(W.WRITERS))
def test_generator_follows_every_writer(device, records, name):
    g, other = _generator(1, device), _generator(2, device)
    W.assert_follows(_fused_run(device, records), g, W.writer(name), other, builds=lambda: len(_prepacks(records)))


@pytest.mark.parametrize("name", ["accumulate_half", "clip_adam_step"])
def test_generator_follows_the_invisible_writers_in_bf16(device, records, name):
    import sis_hip
    g, other = _generator(1, device, "bf16"), _generator(2, device, "bf16")
    run = _fused_run(device, records, must_contain=(sis_hip.BF16_KERNEL,))
    W.assert_follows(run, g, W.writer(name), other, builds=lambda: len(_prepacks(records)))
    assert "modconv_prepack_bf16" in _prepacks(records)


@pytest.mark.parametrize("name", ["accumulate_half", "clip_adam_step"])
def test_fast_fir_image_follows_the_invisible_writers(device, records, name):
    """At 32 x 32 the fast-FIR images are built and rebuilt but no launch reads them: that kernel takes inputs of 32 x 32 and
    larger.  The 64 x 64 generator is the smallest whose last up-convolution (512 -> 256 channels, 32^2 -> 64^2) runs on it."""
    g, other = _generator(1, device, size=64), _generator(2, device, size=64)
    run = _fused_run(device, records, must_contain=("upfir",), size=64)
    W.assert_follows(run, g, W.writer(name), other, builds=lambda: len(_prepacks(records)))


def test_generator_builds_all_five_images_once(device, records):
    """The configuration is the smallest that holds every kind of image; three forwards with no write build each once."""
    run = _fused_run(device, records)
    g = _generator(1, device)
    first = run(g)
    built = _prepacks(records)
    assert built.count("modconv_prepack") == 7, built   # one (wpk, wsq) per styled convolution
    assert {"modconv_prepack_wino", "modconv_prepack_wino24", "modconv_up_fir_prepack"} <= set(built), built
    for _ in range(2):
        assert W.first_difference(run(g), first) is None
    assert _prepacks(records) == built
    g.set_matrix_precision("bf16")   # drops the packs: everything is built again, now with the bf16 image
    run(g)
    assert "modconv_prepack_bf16" in _prepacks(records)[len(built):]
    built = _prepacks(records)
    run(g)
    assert _prepacks(records) == built


def _updater(device):
    """As tests/test_gan_gpu.py::test_update_core_runs_the_schedule builds it, with the optimizers train_stylegan_2.py builds."""
    import train_stylegan_2 as T
    from networks.stylegan2.model import Discriminator
    from updater.stylegan_2_updater import Stylegan2Updater
    torch.manual_seed(0)
    g, g_ema = _generator(3, device).train(), _generator(4, device)
    g_ema.load_state_dict(g.state_dict())
    d = Discriminator(32, channel_multiplier=1).to(device)
    config = {"lr": 2e-3, "regularization": {"g_interval": 4, "d_interval": 16}}
    images = torch.rand(4, 3, 32, 32, generator=torch.Generator().manual_seed(5)) * 2 - 1

    def batches():
        while True:
            yield {"image": images.clone()}

    return Stylegan2Updater(iterators={"images": batches()}, networks={"generator": g, "discriminator": d},
                            optimizers=T.build_optimizers(config, g, d), device=device, g_ema=g_ema, latent_size=64,
                            regularization_options={"d_reg_interval": 2, "g_reg_interval": 4})


def test_discriminator_step_sees_the_current_generator(device, records):
    """After two iterations, under ``update_discriminator``'s conditions (grad enabled, the generator's parameters switched off by
    ``UpdateDisabler``: its fused path), the generator computes what a fresh module with its parameters computes.  Its optimizer is
    ``GradientClipAdam``, whose device step writes the parameters from a kernel."""
    from training.fused_adam import GradientClipAdam
    from training.loop import UpdateDisabler
    up = _updater(device)
    assert isinstance(up.optimizers["generator"], GradientClipAdam)
    up.update()
    up.update()
    g = up.networks["generator"]
    run = _fused_run(device, records, grad=True)
    fresh = W.fresh_like(g)
    assert g.training and fresh.training and all(p.requires_grad for p in g.parameters())
    with UpdateDisabler(g):
        got = run(g)
    with UpdateDisabler(fresh):
        want = run(fresh)
    stale = W.first_difference(got, want)
    assert stale is None, f"the discriminator step's fakes: '{stale}' comes from weights the optimizer has since changed"


def test_averaged_generator_follows_the_updates(device, records):
    up = _updater(device)
    run = _fused_run(device, records)
    before = run(up.g_ema)   # packs g_ema, as the first sample grid does
    up.update()
    up.update()
    got, want = run(up.g_ema), run(W.fresh_like(up.g_ema))
    assert not torch.equal(before["image"], want["image"])
    stale = W.first_difference(got, want)
    assert stale is None, f"g_ema: '{stale}' comes from weights averaged away since"


@pytest.fixture(scope="module")
def trained_run(tmp_path_factory, device):
    """One 4-iteration run of train_stylegan_2.main from 12 random 32 x 32 PNGs: grids and snapshots at iterations 2 and 4."""
    from PIL import Image
    import networks.stylegan2.discriminator as D
    import train_stylegan_2 as T
    from training.loop import get_current_reporter
    root = tmp_path_factory.mktemp("weight_state_run")
    rng = np.random.default_rng(7)
    names = [f"img_{i:02d}.png" for i in range(12)]
    for name in names:
        Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(root / name)
    (root / "train.json").write_text(json.dumps(names))
    with open(os.path.join(SRC, "configs", "stylegan", "stylegan_256px.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(SMALL)
    (root / "config.yaml").write_text(yaml.safe_dump(cfg))
    saved = D._POLYPHASE
    try:
        args = T.parse_args([str(root / "config.yaml"), "--images", str(root / "train.json"), "-l", str(root / "logs"), "-ln", "run"])
        get_current_reporter().observations.clear()
        torch.manual_seed(11)
        T.main(args, 0, 1)
    finally:
        D._POLYPHASE = saved
    return root / "logs" / "run", cfg


@pytest.mark.parametrize("iteration", [2, 4])
def test_every_grid_is_its_snapshots_grid(device, trained_run, iteration, tmp_path):
    """The grid saved at an iteration has the bytes ``render_grid`` makes from the snapshot of that iteration.  2 is the render that
    packs g_ema's weights (the comparison tests/test_train_stylegan2_gpu.py makes); 4 is the first one after the weight average has
    moved them."""
    import train_stylegan_2 as T
    from create_dataset_for_segmentation import load_generator
    run_dir, cfg = trained_run
    assert sorted(p.name for p in run_dir.glob("*.pt")) == ["000002.pt", "000004.pt"]
    g = load_generator(str(run_dir / f"{iteration:06d}.pt"), 32, 64, 2, 1, device)
    T.save_grid(T.render_grid(g, T.sample_latents(cfg, device), cfg["batch_size"]), tmp_path / "again.png")
    assert (tmp_path / "again.png").read_bytes() == (run_dir / "images" / f"{iteration:06d}.png").read_bytes()
    if iteration == 4:
        assert (run_dir / "images" / "000004.png").read_bytes() != (run_dir / "images" / "000002.png").read_bytes()


# ---------------------------------------------------------------------------------------------------------------- the encoder
ENCODER = (32, 32, 3, {32: 8, 16: 16, 8: 24, 4: 32})   # the smallest map the encoder's tests use (tests/golden/make_golden_encoder.py)


def _encoder(seed, device):
    from networks.encoder.u_net_like_encoder import WPlusEncoder
    enc = W.seeded(lambda: WPlusEncoder(*ENCODER, stylegan_variant=2), seed)
    with torch.no_grad():
        gen = torch.Generator().manual_seed(seed)
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.3 * torch.randn(m.running_mean.shape, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))
    return enc.to(device).eval()


def _running_statistics(enc, other):
    """A train-mode forward: moves the BatchNorm buffers (a control: the buffers' ``_version`` sees it)."""
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(next(enc.parameters()).device)
    enc.train()
    with torch.no_grad():
        enc(x)
    enc.eval()


def _statistics(enc):
    out = []
    for j, block in enumerate(enc._blocks()):
        out += [(f"block{j}.bn1.running_mean", block.bn1.running_mean), (f"block{j}.bn2.running_var", block.bn2.running_var)]
    return out


@pytest.mark.parametrize("name", list(W.WRITERS) + ["running_statistics"])
def test_encoder_follows_every_writer(device, records, name, monkeypatch):
    import sis_hip
    built = []   # the encoder's Winograd images and folded BatchNorms are no profiler records: their builders are counted

    def counted(fn):
        def call(*args, **kwargs):
            built.append(fn.__name__)
            return fn(*args, **kwargs)
        return call

    for fn in (sis_hip.conv3x3_prepack, sis_hip.fold_batch_norm, sis_hip.enc_conv3x3_s2_pack):
        monkeypatch.setattr(sis_hip, fn.__name__, counted(fn))
    builds = lambda: len(built) + len(_prepacks(records))   # noqa: E731
    x = (torch.rand(BATCH, 3, 32, 32, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(device)

    def run(enc):
        seen = len(records)
        sis_hip.library_calls(reset=True)
        with torch.no_grad():
            out = enc(x)
        torch.cuda.synchronize(device)
        kernels = [r[0] for r in records[seen:]]
        assert kernels.count("enc_stem_kernel") == 1 and kernels.count("enc_block_tail_kernel") == 8 and kernels.count("enc_latent_heads_kernel") == 1, kernels
        assert not sis_hip.library_calls(reset=True)["fallback"]
        return {**{f"noise {i}": n for i, n in enumerate(out.noise)}, "latent": out.latent}

    enc, other = _encoder(1, device), _encoder(2, device)
    if name == "running_statistics":
        W.assert_follows(run, enc, _running_statistics, other, builds=builds, layers=_statistics)
    else:
        W.assert_follows(run, enc, W.writer(name), other, builds=builds)
    assert {"conv3x3_prepack", "fold_batch_norm", "enc_conv3x3_s2_pack"} <= set(built) and "enc_conv3x3_s2_prepack" in _prepacks(records)
