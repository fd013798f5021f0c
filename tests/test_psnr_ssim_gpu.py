"""``sis_hip.psnr_ssim`` (csrc/eval_ops.h) against the float64 restatement (tests/psnr_ssim_restatement.py), the evaluator on top
of it, and scripts/evaluate_checkpoints.py end to end.

Bounds.  For the SSIM map, ssim[b] and a finite psnr[b] (in dB): max|device - ref64| <= max(4 E, 2^-19), E the same
maximum for the float32 ATen formulation (2-D taps by grouped conv2d, computed here on the CPU) against ref64.  4 is the margin
for a different but equally accurate summation order (separable against 2-D taps), fixed before any run; 2^-19 is 16 ulp of 1 for
the cases where E is 0.  The exact cases (+inf, 0, 1) are compared for equality.

Measured on an MI355X over all cases: the kernel accumulates in double and rounds once, so its error is the float32 rounding of
the result -- map <= 2.98e-8, ssim <= 2.86e-8, psnr <= 1.51e-6 dB -- against E up to 5.06e-4 (map, smooth case at window 11),
1.39e-5 (ssim) and 3.08e-6 dB (psnr).  The test prints every figure.
"""
import json

import numpy as np
import pytest
import torch

import psnr_ssim_restatement as R

pytestmark = pytest.mark.gpu

FLOOR = R.FLOOR


def _shape(shape):
    import sis_hip
    return R.resolve_shape(shape, sis_hip.psnr_ssim_tile())


def _run(device, shape, content):
    import sis_hip
    x, y = R.case(shape, content)
    return sis_hip.psnr_ssim(torch.from_numpy(x).to(device), torch.from_numpy(y).to(device), window=shape[4], return_map=True)


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_against_the_restatement(device, shape, content):
    shape = _shape(shape)
    ref_psnr, ref_ssim, ref_s = R.reference(shape, content)
    e_map, e_ssim, e_psnr = R.aten_error(shape, content)
    psnr, ssim, smap = (t.double().cpu().numpy() for t in _run(device, shape, content))
    finite = np.isfinite(ref_psnr)
    d_map, d_ssim = np.abs(smap - ref_s).max(), np.abs(ssim - ref_ssim).max()
    d_psnr = np.abs(psnr[finite] - ref_psnr[finite]).max() if finite.any() else 0.0
    print(f"psnr_ssim {shape} {content}: map {d_map:.2e} (E {e_map:.2e}) ssim {d_ssim:.2e} (E {e_ssim:.2e}) "
          f"psnr {d_psnr:.2e} dB (E {e_psnr:.2e})")
    assert np.isfinite(smap).all()
    assert d_map <= R.bound(e_map)
    assert d_ssim <= R.bound(e_ssim)
    assert np.array_equal(np.isposinf(psnr), ~finite) and d_psnr <= R.bound(e_psnr)
    if content == "identical":
        assert np.all(ssim == 1.0) and np.all(np.isposinf(psnr))
    if content == "inverted":
        assert np.all(ssim == 0.0)
    if content == "independent":   # a missing clamp must fail: the unclamped mean is far outside the bound
        assert abs(ssim.mean() - ref_s.mean()) > 100 * R.bound(e_ssim)


@pytest.mark.parametrize("content", ["smooth", "mixed_range"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_two_runs_give_equal_bits_and_the_evaluator_is_the_kernel(device, shape, content):
    from evaluation.psnr_ssim import PSNRSSIMEvaluator
    shape = _shape(shape)
    first, second = _run(device, shape, content), _run(device, shape, content)
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    x, y = (torch.from_numpy(v).to(device) for v in R.case(shape, content))
    evaluator = PSNRSSIMEvaluator(ssim_kernel_size=shape[4])
    b_psnr, b_ssim = evaluator.psnr_and_ssim_batch(x, y)
    assert torch.equal(b_psnr, first[0]) and torch.equal(b_ssim, first[1])
    for b in range(shape[0]):
        psnr, ssim = evaluator.psnr_and_ssim(x[b:b + 1], y[b:b + 1])
        assert psnr.dim() == 0 and torch.equal(psnr, b_psnr[b]) and torch.equal(ssim, b_ssim[b])
        assert torch.equal(evaluator.psnr(x[b:b + 1], y[b:b + 1]), b_psnr[b]) and torch.equal(evaluator.ssim(x[b:b + 1], y[b:b + 1]), b_ssim[b])


def test_forced_modes(device):
    import sis_hip
    shape = _shape(R.SHAPES[2])
    x, y = R.case(shape, "target_negative")
    dx, dy = torch.from_numpy(x).to(device), torch.from_numpy(y).to(device)
    for mode in (sis_hip.UNNORMALIZE_ALWAYS, sis_hip.UNNORMALIZE_NEVER):
        ref_psnr, ref_ssim, ref_s = R.psnr_ssim(x, y, window=shape[4], mode=mode)
        psnr, ssim, smap = (t.double().cpu().numpy() for t in sis_hip.psnr_ssim(dx, dy, window=shape[4], unnormalize=mode, return_map=True))
        assert np.abs(smap - ref_s).max() <= FLOOR and np.abs(ssim - ref_ssim).max() <= FLOOR
        assert np.abs(psnr - ref_psnr).max() <= 4 * FLOOR   # half an ulp of a float32 below 128 dB


def test_declines_with_a_message(device):
    import sis_hip
    x = torch.zeros(1, 3, 2, 8, device=device)
    with pytest.raises(RuntimeError, match="window"):
        sis_hip.psnr_ssim(x, x, window=5)      # H = 2 is not larger than 5 // 2
    with pytest.raises(RuntimeError, match="window"):
        sis_hip.psnr_ssim(x, x, window=4)
    with pytest.raises(RuntimeError, match="one shape"):
        sis_hip.psnr_ssim(x, x[:, :2], window=3)


# ------------------------------------------------------------------------------------------------------------- end to end

def test_evaluate_checkpoints_end_to_end(device, tmp_path):
    from PIL import Image

    import scripts.evaluate_checkpoints as E
    from evaluation.psnr_ssim import PSNRSSIMEvaluator
    from networks import get_autoencoder, load_weights
    config = {"stylegan_variant": 2, "image_size": 32, "latent_size": 32, "n_mlp": 2, "channel_multiplier": 1}
    run_args = {"input_dim": 3, "denoising": False}
    torch.manual_seed(3)
    autoencoder = get_autoencoder({**config, **run_args})
    run = tmp_path / "run"
    (run / "checkpoints").mkdir(parents=True)
    (run / "config").mkdir()
    torch.save({"autoencoder": autoencoder.state_dict()}, run / "checkpoints" / "7.pt")
    (run / "config" / "config.json").write_text(json.dumps(config))
    (run / "config" / "args.json").write_text(json.dumps(run_args))
    rng = np.random.default_rng(17)
    names = []
    for i in range(6):
        names.append(f"{i}.png")
        Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(tmp_path / names[-1])
    (tmp_path / "test.json").write_text(json.dumps(names))
    (tmp_path / "checkpoints.txt").write_text(str(run / "checkpoints" / "7.pt") + "\n")
    (tmp_path / "datasets.json").write_text(json.dumps([{"name": "pages", "test": str(tmp_path / "test.json"), "train": str(tmp_path / "test.json")}]))
    args = E.build_parser().parse_args([str(tmp_path / "checkpoints.txt"), str(tmp_path / "datasets.json"), "--skip-fid", "--batch-size", "4"])
    assert E.main(args) == []
    result = json.loads((run / "evaluation" / "reconstruction.json").read_text())["7.pt"]["pages"]
    assert set(result) == {"psnr", "ssim"}

    # the per-image loop of the reference on the same reconstructions
    loaded = load_weights(get_autoencoder({**config, **run_args}).to(device), run / "checkpoints" / "7.pt", key='autoencoder').eval()
    dataset = E.get_dataset_class(E.argparse.Namespace(**config, **run_args))(str(tmp_path / "test.json"), 32)
    evaluator, psnr, ssim = PSNRSSIMEvaluator(), [], []
    for lo in (0, 4):   # the script's batches (the autoencoder's own kernels may depend on the batch size in the last bits)
        batch = dataset.get_batch(list(range(lo, min(lo + 4, 6))))
        with torch.no_grad():
            reconstructed = loaded(batch["input_image"])
        for b in range(len(reconstructed)):
            p, s = evaluator.psnr_and_ssim(reconstructed[b:b + 1], batch["output_image"][b:b + 1])
            psnr.append(float(p.cpu()))
            ssim.append(float(s.cpu()))
    assert np.isfinite(psnr).all() and 0 <= min(ssim) and max(ssim) <= 1
    assert result["psnr"] == pytest.approx(np.mean(psnr), rel=1e-6) and result["ssim"] == pytest.approx(np.mean(ssim), rel=1e-6)
