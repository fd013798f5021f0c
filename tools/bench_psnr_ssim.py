"""PSNR / SSIM of a batch and the denoising loader's batch on one MI355X.

* ``sis_hip.psnr_ssim`` at B = 32, 3 x 256 x 256, window 5 and 11 -- with the unnormalise decision (inputs in [-1, 1]: the minima
  launch reads both tensors a second time) and without (``unnormalize=2``: both tensors read once) -- against the same metric in
  ATen (tests/psnr_ssim_restatement.py ``aten_psnr_ssim``: reflect pad, one grouped conv2d per moment, element-wise ops): batched
  without a host sync, and per image as the reference's evaluator runs it (two ``min() < 0`` syncs and one ``.cpu()`` per metric).
  The variants alternate in this process, five runs each after warm-up, device events around a window of at least 0.2 s; median
  and range.  Every iteration takes the next of several input sets that together exceed the 256 MiB Infinity Cache, so the
  tensors come from HBM.
* the share of the HBM roofline: the time to read the two tensors once at the achievable 6.3 TB/s (MI355X_MICROARCH: 8 TB/s peak)
  over the measured time of a call.  A call is three launches issued from Python; the figure is the call's, not a kernel's.
* ``sis_hip.autoencoder_batch`` beside ``sis_hip.gan_image_batch`` (B = 32 of 256 resident 3 x 256 x 256 images).

Writes profiles/psnr_ssim_bench.json and prints it.

    python tools/bench_psnr_ssim.py [--runs 5] [--out profiles/psnr_ssim_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))   # the ATen formulation the tests measure E with

import torch  # noqa: E402

BATCH, CHANNELS, SIZE = 32, 3, 256
HBM_ACHIEVABLE = 6.3e12
WINDOW_SECONDS = 0.2


def timed(fn, sets, iters):
    """ms per call over ``iters`` calls cycling through the input sets, by device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fn(*sets[i % len(sets)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(variants, sets, runs):
    """{name: {median_ms, min_ms, max_ms, iters}}: warm-up, a pilot to size the window, then ``runs`` alternating rounds."""
    iters = {}
    for name, fn in variants.items():
        timed(fn, sets, 3)
        pilot = timed(fn, sets, 5)
        iters[name] = int(min(5000, max(5, WINDOW_SECONDS * 1e3 / max(pilot, 1e-3))))
    samples = {name: [] for name in variants}
    for _ in range(runs):
        for name, fn in variants.items():
            samples[name].append(timed(fn, sets, iters[name]))
    return {name: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5), "iters": iters[name]}
            for name, v in samples.items()}


def per_image_aten(window):
    from psnr_ssim_restatement import aten_psnr_ssim

    def unnormalize(image):   # the reference's PSNRSSIMEvaluator.unnormalize: a host sync
        return (image.clamp(-1, 1) + 1) / 2 if image.min() < 0 else image

    def run(image, target):
        out = []
        for b in range(image.shape[0]):
            x, y = unnormalize(image[b:b + 1]), unnormalize(target[b:b + 1])
            psnr, ssim, _ = aten_psnr_ssim(x, y, window=window, mode=2)
            out.append((float(psnr.cpu()), float(ssim.cpu())))
        return out
    return run


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--runs", type=int, default=5)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "psnr_ssim_bench.json"))
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_psnr_ssim: a HIP device is required (no CPU timing is meaningful)")
    import sis_hip
    from psnr_ssim_restatement import aten_psnr_ssim
    device = torch.device("cuda:0")
    gen = torch.Generator(device=device).manual_seed(0)
    shape = (BATCH, CHANNELS, SIZE, SIZE)
    pair_bytes = 2 * 4 * BATCH * CHANNELS * SIZE * SIZE
    n_sets = -(-(288 << 20) // pair_bytes)   # together past the 256 MiB Infinity Cache
    sets = []
    for _ in range(n_sets):
        target = torch.rand(shape, generator=gen, device=device) * 2 - 1
        sets.append(((target + 0.1 * torch.randn(shape, generator=gen, device=device)).contiguous(), target))
    sets01 = [((x.clamp(-1, 1) + 1) / 2, (y + 1) / 2) for x, y in sets[:n_sets]]
    roofline_ms = pair_bytes / HBM_ACHIEVABLE * 1e3
    result = {"device": torch.cuda.get_device_name(0), "shape": {"batch": BATCH, "channels": CHANNELS, "height": SIZE, "width": SIZE},
              "input_sets": n_sets, "bytes_of_both_tensors": pair_bytes, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
              "roofline_ms_reading_both_once": round(roofline_ms, 5), "runs": args.runs, "windows": {}}
    for window in (5, 11):
        k_psnr, k_ssim = sis_hip.psnr_ssim(*sets[0], window=window)
        a_psnr, a_ssim, _ = aten_psnr_ssim(*sets[0], window=window)
        agreement = {"max_abs_psnr_db": float((k_psnr - a_psnr).abs().max()), "max_abs_ssim": float((k_ssim - a_ssim).abs().max())}
        variants = {
            "kernel": lambda x, y, w=window: sis_hip.psnr_ssim(x, y, window=w),
            "aten_batched": lambda x, y, w=window: aten_psnr_ssim(x, y, window=w),
            "aten_per_image": per_image_aten(window),
        }
        times = measure(variants, sets, args.runs)
        times["kernel_unnormalize_never"] = measure({"k": lambda x, y, w=window: sis_hip.psnr_ssim(x, y, window=w, unnormalize=2)},
                                                    sets01, args.runs)["k"]
        for name in ("kernel", "kernel_unnormalize_never"):
            times[name]["share_of_hbm_roofline"] = round(roofline_ms / times[name]["median_ms"], 4)
        times["kernel_over_aten_batched"] = round(times["kernel"]["median_ms"] / times["aten_batched"]["median_ms"], 4)
        times["kernel_over_aten_per_image"] = round(times["kernel"]["median_ms"] / times["aten_per_image"]["median_ms"], 5)
        times["kernel_against_aten_float32"] = agreement
        result["windows"][str(window)] = times
    del sets, sets01

    n_images = 256
    images = torch.randint(0, 256, (n_images, 3, SIZE, SIZE), generator=gen, device=device, dtype=torch.uint8)
    id_sets = [(torch.randint(0, n_images, (BATCH,), generator=gen, device=device, dtype=torch.int32),) for _ in range(8)]
    scale = torch.full((BATCH,), 25.0, device=device)
    ones = torch.ones(BATCH, dtype=torch.int32, device=device)
    zeros = torch.zeros(BATCH, dtype=torch.int32, device=device)
    seed = torch.arange(BATCH, dtype=torch.int32, device=device)
    loader = measure({
        "gan_image_batch": lambda ids: sis_hip.gan_image_batch(images, ids),
        "autoencoder_batch_per_channel": lambda ids: sis_hip.autoencoder_batch(images, ids, scale, ones, seed, zeros),
        "autoencoder_batch_shared_grey": lambda ids: sis_hip.autoencoder_batch(images, ids, scale, zeros, seed, ones),
    }, id_sets, args.runs)
    result["loader_batch"] = {"batch": BATCH, "resident_images": n_images, "size": SIZE, **loader}
    text = json.dumps(result, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
