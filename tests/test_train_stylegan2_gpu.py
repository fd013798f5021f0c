"""GPU: GAN training from an image list -- the loader's batch kernel, the phase split / merge, the composed downsampling weight,
``down_conv3x3`` to second order, the discriminator switch against the reference golden, and train_stylegan_2.py end to end.

Bounds.  Gather / split / merge copy or apply one correctly rounded formula: bit-equal.  Compose / adjoint: sums of at most 9 (16)
fp32 products plus one scale -> 1e-6 * max|ref|.  ``down_conv3x3`` (Winograd F(2x2,3x3) over 4 Cin channels): the error of the
library's direct fp32 formulation against float64 is MEASURED on the same operands and the polyphase route is allowed 4 x that
(the Winograd-over-direct factor of DESIGN.md §13.3), never more than 1e-4 * max|ref| (tests/gan_train_checks.py)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import gan_train_checks as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "synthesis-in-style_amd")
ASYMMETRIC = torch.arange(1.0, 17.0).view(4, 4).tolist()


@pytest.mark.parametrize("size", [8, 6])   # 6: rows of 24 bytes, no multiple of 16
def test_gan_image_batch_is_bit_equal(device, size):
    import sis_hip
    gen = torch.Generator().manual_seed(size)
    images = torch.randint(0, 256, (7, 3, size, size), generator=gen, dtype=torch.uint8)
    images.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)   # every byte value at least once (samples 0 .. 2)
    ids = torch.tensor([3, 0, 6, 3, 1], dtype=torch.int32)   # a repeated id, the last sample of the list
    got = sis_hip.gan_image_batch(images.to(device), ids.to(device))
    want = C.ref_image_batch(images, ids)
    assert got.dtype == torch.float32 and tuple(got.shape) == (5, 3, size, size)
    assert torch.equal(got.cpu(), want)
    assert got.min().item() >= -1.0 and got.max().item() <= 1.0


def test_gan_image_batch_odd_size_and_bad_id(device):
    """3 * 5 * 5 bytes per sample: the one-element-per-thread kernel; an id outside the list is a NaN sample, not a read."""
    import sis_hip
    gen = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (3, 3, 5, 5), generator=gen, dtype=torch.uint8)
    ids = torch.tensor([2, 0], dtype=torch.int32)
    assert torch.equal(sis_hip.gan_image_batch(images.to(device), ids.to(device)).cpu(), C.ref_image_batch(images, ids))
    for side in (5, 4):   # both kernels
        bad = sis_hip.gan_image_batch(images[:, :, :side, :side].contiguous().to(device), torch.tensor([1, 3, -1], dtype=torch.int32).to(device)).cpu()
        assert torch.isfinite(bad[0]).all() and torch.isnan(bad[1]).all() and torch.isnan(bad[2]).all()


@pytest.mark.parametrize("shape", [(2, 8, 8, 8), (1, 3, 6, 10), (3, 24, 4, 8)])   # W % 8 == 0: 16-byte path; 10: element path
def test_phase_split_and_merge_are_bit_equal(device, shape):
    import sis_hip
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape)))
    split = sis_hip.phase_split(x.to(device))
    assert torch.equal(split.cpu(), F.pixel_unshuffle(x, 2))
    p = torch.randn(*split.shape, generator=torch.Generator().manual_seed(1 + sum(shape)))
    assert torch.equal(sis_hip.phase_merge(p.to(device)).cpu(), F.pixel_shuffle(p, 2))
    assert torch.equal(sis_hip.phase_merge(split).cpu(), x)


def test_phase_functions_differentiate_to_any_order(device):
    from networks.hip_conv import phase_merge, phase_split
    x = torch.randn(2, 8, 8, 8, device=device, requires_grad=True)
    g = torch.randn(2, 32, 4, 4, device=device, requires_grad=True)
    dx, = torch.autograd.grad(phase_split(x), x, g, create_graph=True)
    assert torch.equal(dx, F.pixel_shuffle(g, 2)) and dx.grad_fn is not None
    ddg, = torch.autograd.grad(dx, g, x)   # the adjoint of the adjoint: the split again
    assert torch.equal(ddg, F.pixel_unshuffle(x, 2))
    assert torch.equal(phase_merge(phase_split(x)), x)


@pytest.mark.parametrize("cout,cin", [(16, 8), (40, 24), (5, 3), (64, 300)])   # (64, 300): 75 workgroups
@pytest.mark.parametrize("taps", ["1331", "asymmetric"])
def test_compose_and_adjoint_against_float64(device, cout, cin, taps):
    import sis_hip
    gen = torch.Generator().manual_seed(cout + cin)
    w, g = torch.randn(cout, cin, 3, 3, generator=gen), torch.randn(cout, 4 * cin, 3, 3, generator=gen)
    f32 = C.fir_taps(dtype=torch.float32) if taps == "1331" else C.fir_taps(ASYMMETRIC, dtype=torch.float32)
    scale = 1 / math.sqrt(cin * 9)
    composed = sis_hip.down_weight_compose(w.to(device), f32.to(device), scale)
    adjoint = sis_hip.down_weight_compose_adjoint(g.to(device), f32.to(device), scale)
    ref_c, ref_a = C.ref_compose(w, f32, scale), C.ref_compose_adjoint(g, f32, scale)
    ec, ea = C.max_abs(composed, ref_c), C.max_abs(adjoint, ref_a)
    print(f"compose {cout}x{cin} {taps}: err {ec:.3e} of max {ref_c.abs().max().item():.3e}; adjoint err {ea:.3e} of max {ref_a.abs().max().item():.3e}")
    assert tuple(composed.shape) == (cout, 4 * cin, 3, 3) and ec <= 1e-6 * ref_c.abs().max().item()
    assert tuple(adjoint.shape) == (cout, cin, 3, 3) and ea <= 1e-6 * ref_a.abs().max().item()
    # <compose(W), G> = <W, adjoint(G)>, both sides accumulated in float64 from the kernels' fp32 outputs.  Each output element is
    # within 1e-6 * max|.| of the exact linear map (above), so the two sides differ by at most
    # 1e-6 * (max|compose| * sum|G| + max|adjoint| * sum|W|).
    lhs = (composed.double().cpu() * g.double()).sum().item()
    rhs = (w.double() * adjoint.double().cpu()).sum().item()
    slack = 1e-6 * (ref_c.abs().max().item() * g.double().abs().sum().item() + ref_a.abs().max().item() * w.double().abs().sum().item())
    assert abs(lhs - rhs) <= slack, (lhs, rhs, slack)


def test_compose_declines_other_firs(device):
    import sis_hip
    w = torch.randn(8, 8, 3, 3, device=device)
    for taps in ([1.0, 2.0, 1.0], [1.0] * 6):
        fir = C.fir_taps(taps, dtype=torch.float32).to(device)
        assert not sis_hip.down_weight_compose_supported(fir)
        with pytest.raises(RuntimeError, match="4 x 4 only"):
            sis_hip.down_weight_compose(w, fir, 1.0)


DOWN_SHAPES = [(2, 8, 16, 8, 8),        # the smallest shape the Winograd path takes (half resolution 4 x 4, 32 input channels)
               (3, 24, 40, 12, 16),     # channel counts and sizes that are no multiple of the 64-wide tiles, odd batch
               (2, 64, 64, 16, 16)]     # 256 -> 64 channels at 8 x 8: the % 64 Winograd weight-gradient kernel engages


def _down_operands(shape):
    b, cin, cout, h, w = shape
    gen = torch.Generator().manual_seed(sum(shape))
    return (torch.randn(b, cin, h, w, generator=gen), torch.randn(cout, cin, 3, 3, generator=gen),
            torch.randn(b, cout, h // 2, w // 2, generator=gen), torch.randn(cout, cin, 3, 3, generator=gen), 1 / math.sqrt(cin * 9))


@pytest.mark.parametrize("shape", DOWN_SHAPES)
def test_down_conv3x3_to_second_order(device, shape):
    import sis_hip
    from networks.hip_conv import down_conv3x3, down_conv3x3_supported
    from networks.stylegan2.op import upfirdn2d
    x, w, gy, probe, scale = _down_operands(shape)
    f64, f32 = C.fir_taps(), C.fir_taps(dtype=torch.float32).to(device)
    ref = C.first_and_second_order(lambda a, k: C.library_down(a, k, f64, scale), x.double(), w.double(), gy.double(), probe.double())
    on_device = [t.to(device) for t in (x, w, gy, probe)]
    assert down_conv3x3_supported(on_device[0], on_device[1], f32)
    if shape[1] * 4 % 64 == 0 and shape[2] % 64 == 0:
        assert sis_hip.conv3x3_wgrad_supported(shape[0], 4 * shape[1], shape[2], shape[3] // 2, shape[4] // 2)
    sis_hip.library_calls(reset=True)
    got = C.first_and_second_order(lambda a, k: down_conv3x3(a, k, f32, scale), *on_device)
    assert "gan.down_conv3x3" not in sis_hip.library_calls(reset=True)["fallback"]
    lib = C.first_and_second_order(lambda a, k: F.conv2d(upfirdn2d(a, f32, pad=(2, 2)), k * scale, stride=2), *on_device)
    failures = []
    for name, g, l, r in zip(C.ORDER_NAMES, got, lib, ref):
        bound, lib_err = C.winograd_bound(l, r)
        err = C.max_abs(g, r)
        print(f"down_conv3x3 {shape} {name}: polyphase err {err:.3e}, library fp32 err {lib_err:.3e}, bound {bound:.3e}, max|ref| {r.abs().max().item():.3e}")
        if not err <= bound:
            failures.append((name, err, bound))
    assert not failures, failures


def test_declined_shape_runs_the_library_formulation(device, monkeypatch):
    """(2, 8, 16, 4, 4): half resolution 2 x 2, which the Winograd tile plan declines -- the layer runs blur + library convolution,
    the same numbers as with the switch off, and the fallback is counted."""
    import sis_hip
    import networks.stylegan2.discriminator as D
    torch.manual_seed(3)
    layer = D.ConvLayer(8, 16, 3, downsample=True).to(device)
    x = torch.randn(2, 8, 4, 4, device=device, requires_grad=True)
    results = []
    for switch in (False, True):
        monkeypatch.setattr(D, "_POLYPHASE", switch)
        sis_hip.library_calls(reset=True)
        y = layer(x)
        grads = torch.autograd.grad(y.pow(2).sum(), [x] + list(layer.parameters()))
        results.append((y.detach(),) + grads)
        assert sis_hip.library_calls(reset=True)["fallback"].get("gan.down_conv3x3", 0) == (1 if switch else 0)
    for a, b in zip(*results):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape", DOWN_SHAPES[1:])
def test_two_runs_are_bit_equal(device, shape):
    from networks.hip_conv import down_conv3x3
    x, w, gy, _, scale = _down_operands(shape)
    f32 = C.fir_taps(dtype=torch.float32).to(device)
    runs = []
    for _ in range(2):
        a, k = x.to(device).requires_grad_(True), w.to(device).requires_grad_(True)
        y = down_conv3x3(a, k, f32, scale)
        runs.append((y.detach(),) + torch.autograd.grad(y, (a, k), gy.to(device)))
    for u, v in zip(*runs):
        assert torch.equal(u, v)


def _spy_on_route(monkeypatch):
    import sis_hip
    import networks.stylegan2.discriminator as D
    calls = []
    real = D.down_conv3x3

    def spy(input, weight, fir, scale):
        calls.append(tuple(input.shape))
        return real(input, weight, fir, scale)

    monkeypatch.setattr(D, "_POLYPHASE", True)
    monkeypatch.setattr(D, "down_conv3x3", spy)
    sis_hip.library_calls(reset=True)
    return calls


def test_substeps_match_reference_golden_with_polyphase(device, golden_dir, monkeypatch):
    """The D step, R1, G step (and path-length) assertions of tests/test_gan_gpu.py against tests/golden/gan32.npz, same tolerances
    (2e-4 / 2e-3), with the discriminator's three downsampling layers (512 -> 512 at 32^2, 16^2, 8^2) on the polyphase route."""
    import sis_hip
    import test_gan_gpu
    calls = _spy_on_route(monkeypatch)
    test_gan_gpu.test_four_substeps_match_reference_golden(device, golden_dir)
    assert len(calls) >= 3 * 4 and {c[1:] for c in calls} == {(512, 32, 32), (512, 16, 16), (512, 8, 8)}
    assert "gan.down_conv3x3" not in sis_hip.library_calls(reset=True)["fallback"]


def test_swagan_discriminator_takes_the_route(device, golden_dir, monkeypatch):
    import sis_hip
    import test_swagan_gpu
    calls = _spy_on_route(monkeypatch)
    test_swagan_gpu.test_discriminator_matches_reference_golden(device, golden_dir)
    assert calls
    assert "gan.down_conv3x3" not in sis_hip.library_calls(reset=True)["fallback"]


# ---- train_stylegan_2.py end to end ---------------------------------------------------------------------------------------

SMALL = dict(image_size=32, batch_size=4, n_mlp=2, latent_size=64, channel_multiplier=1, max_iter=3, snapshot_save_iter=2, image_save_iter=2,
             log_iter=1, display_size=4)


def _small_config(**overrides):
    with open(os.path.join(SRC, "configs", "stylegan", "stylegan_256px.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(SMALL)
    cfg.update(overrides)
    return cfg


@pytest.fixture(scope="module")
def trained(tmp_path_factory, device):
    """One 3-iteration run per switch position from 12 random 32 x 32 PNGs and two 40 x 36 ones."""
    from PIL import Image
    import networks.stylegan2.discriminator as D
    import train_stylegan_2 as T
    from training.loop import get_current_reporter
    root = tmp_path_factory.mktemp("gan_train")
    rng = np.random.default_rng(7)
    names = []
    for i in range(14):
        w, h = (40, 36) if i >= 12 else (32, 32)
        names.append(f"img_{i:02d}.png")
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / names[-1])
    (root / "train.json").write_text(json.dumps(names))
    runs, saved = {}, D._POLYPHASE
    try:
        for switch in (False, True):
            cfg_path = root / f"config_{int(switch)}.yaml"
            cfg_path.write_text(yaml.safe_dump(_small_config(polyphase_downsample=switch)))
            args = T.parse_args([str(cfg_path), "--images", str(root / "train.json"), "-l", str(root / "logs"), "-ln", f"run_{int(switch)}"])
            get_current_reporter().observations.clear()
            torch.manual_seed(11)
            history = T.main(args, 0, 1)
            assert D._POLYPHASE is switch
            runs[switch] = (root / "logs" / f"run_{int(switch)}", history)
    finally:
        D._POLYPHASE = saved
    return root, runs


@pytest.mark.parametrize("switch", [False, True])
def test_end_to_end_run(device, trained, switch, tmp_path):
    import train_stylegan_2 as T
    from create_dataset_for_segmentation import load_generator
    run_dir, history = trained[1][switch]
    assert [it for it, _ in history] == [1, 2, 3]
    for _, obs in history:
        assert obs and all(math.isfinite(v) for v in obs.values()), obs
    first = history[0][1]   # iteration 0 runs all four sub-steps
    assert {"discriminator/discriminator_loss", "discriminator/r1_loss", "generator/generator_loss", "generator/perceputal_path_loss"} <= set(first)
    assert sorted(p.name for p in run_dir.glob("*.pt")) == ["000002.pt"]
    snapshot = torch.load(run_dir / "000002.pt", map_location="cpu")
    assert set(snapshot) == set(T.SNAPSHOT_KEYS)
    assert len(snapshot["generator_optimizer"]["state"]) > 0 and "exp_avg" in next(iter(snapshot["discriminator_optimizer"]["state"].values()))
    # the snapshot's g_ema through the loader create_dataset_for_segmentation.py uses, and the grid it rendered at that iteration
    cfg = _small_config()
    g = load_generator(str(run_dir / "000002.pt"), 32, 64, 2, 1, device)
    T.save_grid(T.render_grid(g, T.sample_latents(cfg, device), cfg["batch_size"]), tmp_path / "again.png")
    assert (tmp_path / "again.png").read_bytes() == (run_dir / "images" / "000002.png").read_bytes()
    from PIL import Image
    with Image.open(run_dir / "images" / "000002.png") as im:
        assert im.size == (64, 64) and np.asarray(im).std() > 0


def test_resume_starts_from_the_snapshot(device, trained, tmp_path):
    """A second process with --resume-ckpt and lr 0: after one iteration G and D are bit-equal to the snapshot's (the step size is
    zero).  g_ema: the reference calls ``updater.accumulate(generator, 0)`` after loading, which sets the average to the resumed
    generator (its stored noise stays the snapshot's); one averaging step of an unchanged generator then leaves it there."""
    root, runs = trained
    snap_path = runs[False][0] / "000002.pt"
    cfg_path = tmp_path / "resume.yaml"
    cfg_path.write_text(yaml.safe_dump(_small_config(lr=0.0, max_iter=1, snapshot_save_iter=1, image_save_iter=1000, polyphase_downsample=True)))
    done = subprocess.run([sys.executable, os.path.join(SRC, "train_stylegan_2.py"), str(cfg_path), "--images", str(root / "train.json"),
                           "--resume-ckpt", str(snap_path), "-l", str(tmp_path / "logs"), "-ln", "resumed", "--val-images", "val.json"],
                          capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    assert "iter 1 " in done.stdout and "--val-images: accepted and unused" in done.stdout
    before = torch.load(snap_path, map_location="cpu")
    after = torch.load(tmp_path / "logs" / "resumed" / "000001.pt", map_location="cpu")
    for net in ("generator", "discriminator"):
        assert list(after[net]) == list(before[net])
        for key, value in before[net].items():
            assert torch.equal(after[net][key], value), (net, key)
    params = {name for name, _ in __import__("networks").get_stylegan2_generator(32, 64, 2, 1).named_parameters()}
    assert params and params < set(before["g_ema"])
    for key, value in before["g_ema"].items():
        if key in params:   # decay * G + (1 - decay) * G in fp32: within two roundings of G
            np.testing.assert_allclose(after["g_ema"][key].numpy(), before["generator"][key].numpy(), rtol=3e-7, atol=0, err_msg=key)
        else:
            assert torch.equal(after["g_ema"][key], value), key
