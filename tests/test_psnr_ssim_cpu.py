"""CPU checks of the reconstruction metrics and the denoising loader: the restatement against an independent
torch formulation, the grey formula against PIL, the C boundary, the script's bookkeeping, and the conditions the GPU tests
(tests/test_psnr_ssim_gpu.py, tests/test_autoencoder_dataset_gpu.py) rely on for their inputs."""
import argparse
import json
import os
import re

import numpy as np
import pytest
import torch

import psnr_ssim_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "synthesis-in-style_amd")
NEW_SYMBOLS = {"sis_psnr_ssim_tile", "sis_psnr_ssim_workspace_bytes", "sis_psnr_ssim", "sis_autoencoder_batch"}
PRODUCT_MODULES = ["evaluation/psnr_ssim.py", "data/autoencoder_dataset.py", "data/__init__.py", "scripts/evaluate_checkpoints.py",
                   "utils/config.py"]


def _shapes():
    import sis_hip
    return [R.resolve_shape(s, sis_hip.psnr_ssim_tile()) for s in R.SHAPES]


# ---------------------------------------------------------------------------------------------------------------- formulas

@pytest.mark.parametrize("content", R.CONTENTS)
def test_restatement_equals_the_torch_formulation_in_float64(content):
    """Separable scipy filters against one 2-D grouped conv2d on a reflect-padded input: to 1e-12 (relative for the dB values)."""
    for shape in _shapes():
        x, y = R.case(shape, content)
        psnr, ssim, s = R.reference(shape, content)
        t_psnr, t_ssim, t_s = R.aten_psnr_ssim(torch.from_numpy(x).double(), torch.from_numpy(y).double(), window=shape[4])
        assert np.abs(t_s.numpy() - s).max() <= 1e-12, (shape, content)
        assert np.abs(t_ssim.numpy() - ssim).max() <= 1e-12, (shape, content)
        finite = np.isfinite(psnr)
        assert np.array_equal(np.isinf(t_psnr.numpy()), ~finite), (shape, content)
        assert np.all(np.abs(t_psnr.numpy()[finite] - psnr[finite]) <= 1e-12 * np.maximum(1.0, np.abs(psnr[finite]))), (shape, content)


def test_exact_cases_of_the_restatement():
    for shape in _shapes():
        psnr, ssim, s = R.reference(shape, "identical")
        assert np.all(np.isposinf(psnr)) and np.abs(ssim - 1).max() <= 1e-12
        _, ssim, s = R.reference(shape, "inverted")
        assert (s < 0).all() and np.all(ssim == 0), shape   # every s negative: the kernel's ssim is then exactly 0


def test_mixed_sign_case_has_both_signs():
    for shape in _shapes():
        _, ssim, s = R.reference(shape, "independent")
        negative = (s < 0).mean()
        assert 0.10 <= negative <= 0.90, (shape, negative)
        # what the clamp changes is far outside the bound of the GPU test: a missing clamp fails there
        assert abs(ssim.mean() - s.mean()) > 100 * R.bound(R.aten_error(shape, "independent")[1]), shape


def test_unnormalise_decisions_of_the_mixed_cases():
    for shape in _shapes():
        x, y = R.case(shape, "mixed_range")
        assert [float(v.min()) < 0 for v in x] == [b % 2 == 0 for b in range(shape[0])] == [float(v.min()) < 0 for v in y]
        assert np.abs(x[0]).max() > 1   # the clamp has something to do
        x, y = R.case(shape, "target_negative")
        assert all(v.min() >= 0 for v in x) and all(v.min() < 0 for v in y)
        for content in ("noisy", "smooth", "independent", "inverted", "identical", "constant_target"):
            assert min(v.min() for v in R.case(shape, content)) >= 0, (shape, content)


def test_grey_formula_is_pils():
    from PIL import Image
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (64, 48, 3), dtype=np.uint8)
    rgb[0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 0, 255]]
    pil = np.asarray(Image.fromarray(rgb).convert('L').convert('RGB'))
    ours = R.grey_levels(rgb.transpose(2, 0, 1))
    assert np.array_equal(pil, np.repeat(ours[:, :, None], 3, axis=2))


# ------------------------------------------------------------------------------------- conditions on the loader's inputs

def test_share_of_pixels_near_a_rounding_boundary():
    """The noise comparison leaves out the pixels whose value before rounding is within 2^-8 of a half-integer: at most 2 %."""
    for size, per_channel, grey, scales, seeds in R.noise_cases():
        _, _, ambiguous = R.autoencoder_batch(R.noise_images(size), R.NOISE_IDS, scales, [per_channel] * 3, seeds, [grey] * 3)
        assert ambiguous.mean() <= 0.02, (size, per_channel, grey, scales, ambiguous.mean())


def test_restated_noise_is_standard_normal():
    """The bounds of the GPU statistics test, on the restatement's own z (n = 3 * 64 * 64)."""
    z = np.concatenate([R.normal(R.STATISTICS_SEED, c, 64 * 64) for c in range(3)])
    n = z.size
    assert n == 12288 and abs(z.mean()) <= 4 / np.sqrt(n) and abs(z.var() - 1) <= 4 * np.sqrt(2 / n)
    levels, _, _ = R.autoencoder_batch(np.full((1, 3, 64, 64), 128, dtype=np.uint8), [0], [50.0], [1], [R.STATISTICS_SEED], [0])
    recovered = (levels - 128) / 50.0
    assert abs(recovered.mean()) <= 4 / np.sqrt(n) and abs(recovered.var() - 1) <= 4 * np.sqrt(2 / n)


def test_scale_zero_and_clip_of_the_restatement():
    images = R.noise_images(8)
    levels, outputs, ambiguous = R.autoencoder_batch(images, [3, 1], [0.0, 0.0], [1, 0], [1, 2], [0, 0])
    assert np.array_equal(levels, outputs) and not ambiguous.any()
    levels, _, _ = R.autoencoder_batch(images, [3], [50.0], [1], [9], [0])
    assert levels.min() == 0 and levels.max() == 255


# ---------------------------------------------------------------------------------------------------------------- boundary

def test_new_symbols_are_declared_and_bound():
    import sis_hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sis_hip.h")).read(), flags=re.S)
    assert NEW_SYMBOLS <= set(re.findall(r"\b(sis_[a-z0-9_]+)\s*\(", header)) and NEW_SYMBOLS <= set(sis_hip.exported_symbols())
    assert sis_hip.psnr_ssim_tile() >= 8
    assert sis_hip.lib().sis_psnr_ssim_workspace_bytes(2, 3, 33, 65) >= 2 * 3 * 2 * 3 * 16


def test_product_modules_do_not_import_the_test_libraries():
    for name in PRODUCT_MODULES:
        text = open(os.path.join(SRC, name)).read()
        assert not re.search(r"^\s*(import|from)\s+(scipy|kornia|imgaug|pytorch_training)\b", text, flags=re.M), name


def test_cpu_tensors_raise():
    import sis_hip
    from evaluation.psnr_ssim import PSNRSSIMEvaluator
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        sis_hip.psnr_ssim(x, x)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        PSNRSSIMEvaluator().psnr_and_ssim(x, x)
    with pytest.raises(AssertionError, match="Batch size"):
        PSNRSSIMEvaluator().psnr_and_ssim(torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8))
    ids = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        sis_hip.autoencoder_batch(torch.zeros(1, 3, 4, 4, dtype=torch.uint8), ids, torch.zeros(1), ids, ids, ids)


def test_dataset_class_choice():
    from data import get_dataset_class
    from data.autoencoder_dataset import AutoencoderDataset, BlackAndWhiteDenoisingAutoencoderDataset, DenoisingAutoencoderDataset
    assert get_dataset_class(argparse.Namespace()) is AutoencoderDataset
    assert get_dataset_class(argparse.Namespace(denoising=True, black_and_white_denoising=True)) is DenoisingAutoencoderDataset
    assert get_dataset_class(argparse.Namespace(black_and_white_denoising=True)) is BlackAndWhiteDenoisingAutoencoderDataset


# ---------------------------------------------------------------------------------------------------------- script plumbing

class _Identity:
    def to(self, device):
        return self

    def eval(self):
        return self

    def __call__(self, x):
        return x


class _StubEvaluator:
    calls = 0

    def psnr_and_ssim_batch(self, image, target):
        type(self).calls += 1
        value = image.mean(dim=(1, 2, 3))
        return 20 + value, value / 10


def _run(tmp_path, monkeypatch, *flags):
    import scripts.evaluate_checkpoints as E
    run = tmp_path / "run"
    (run / "checkpoints").mkdir(parents=True, exist_ok=True)
    (run / "config").mkdir(exist_ok=True)
    (run / "checkpoints" / "100.pt").write_bytes(b"")
    (run / "config" / "config.json").write_text(json.dumps({"image_size": 8, "latent_size": 8, "stylegan_variant": 2}))
    (run / "config" / "args.json").write_text(json.dumps({"denoising": True, "input_dim": 3}))
    (tmp_path / "checkpoints.txt").write_text(str(run / "checkpoints" / "100.pt") + "\n")
    (tmp_path / "datasets.json").write_text(json.dumps([{"name": "pages", "test": "test.json", "train": "train.json"}]))
    # five images in batches of 2, 2, 1 with per-image means 0 .. 4
    batches = [{"input_image": torch.full((n, 3, 4, 4), 0.0) + torch.arange(lo, lo + n).view(n, 1, 1, 1).float(),
                "output_image": torch.zeros(n, 3, 4, 4)} for lo, n in ((0, 2), (2, 2), (4, 1))]
    seen = {}

    def loaders(dataset, config, batch_size):
        seen.update(config=config, dataset=dataset, batch_size=batch_size)
        return {"test": batches}

    monkeypatch.setattr(E, "get_autoencoder", lambda config: _Identity())
    monkeypatch.setattr(E, "load_weights", lambda network, path, **kwargs: network)
    monkeypatch.setattr(E, "build_data_loaders", loaders)
    monkeypatch.setattr(E, "PSNRSSIMEvaluator", _StubEvaluator)
    args = E.build_parser().parse_args([str(tmp_path / "checkpoints.txt"), str(tmp_path / "datasets.json"), *flags])
    failed = E.main(args)
    return run, failed, seen


def test_script_writes_reconstruction_json_and_skips_what_is_done(tmp_path, monkeypatch, capsys):
    _StubEvaluator.calls = 0
    run, failed, seen = _run(tmp_path, monkeypatch, "--skip-fid", "--batch-size", "2")
    assert failed == [] and seen["batch_size"] == 2 and seen["config"]["denoising"] is True and seen["config"]["image_size"] == 8
    assert list(seen["dataset"]) == ["test"]
    result = json.loads((run / "evaluation" / "reconstruction.json").read_text())
    assert list(result) == ["100.pt"] and list(result["100.pt"]) == ["pages"] and set(result["100.pt"]["pages"]) == {"psnr", "ssim"}
    assert result["100.pt"]["pages"]["psnr"] == pytest.approx(22.0, abs=1e-12) and result["100.pt"]["pages"]["ssim"] == pytest.approx(0.2, abs=1e-7)
    assert not (run / "evaluation" / "fid.json").exists() and _StubEvaluator.calls == 3
    assert "FID" not in capsys.readouterr().out
    _, failed, _ = _run(tmp_path, monkeypatch, "--skip-fid")   # the finished combination is skipped
    assert failed == [] and _StubEvaluator.calls == 3


def test_script_says_that_fid_is_not_built_and_goes_on(tmp_path, monkeypatch, capsys):
    _StubEvaluator.calls = 0
    run, failed, _ = _run(tmp_path, monkeypatch)
    out = capsys.readouterr().out
    assert failed == [] and "failed" not in out
    assert [line for line in out.splitlines() if "FID" in line] == [__import__("scripts.evaluate_checkpoints").evaluate_checkpoints.FID_NOT_BUILT]
    assert "psnr" in json.loads((run / "evaluation" / "reconstruction.json").read_text())["100.pt"]["pages"]
    assert not (run / "evaluation" / "fid.json").exists()
    _, failed, _ = _run(tmp_path, monkeypatch, "--skip-reconstruction")   # FID alone: one line, nothing computed, no failure
    assert failed == [] and _StubEvaluator.calls == 3
