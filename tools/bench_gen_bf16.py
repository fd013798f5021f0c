"""The generator's opt-in bf16 matrix-core route against its fp32 default on one MI355X.

* Two ``Generator(256)`` instances with the same weights in one process, one in each mode, at B = 32: the whole forward
  (no grad, fixed latents and noise maps), by device events after warm-up, five runs each, alternating.
* Per eligible stride-1 3x3 layer shape of that generator: the bf16 launch (``sis_modconv2d_bf16``) against the launch the default
  takes (``sis_modconv2d_wino24_rgb``: F(2x4,3x3) with the ToRGB sums in its epilogue) and the plain F(2x4,3x3) launch, same
  operands, fused tail, alternating in the same way.  A shape passes the gate when every bf16 run is below every run of the
  default's launch.  The bf16 route pays a separate ToRGB pass that the default does not; that is inside the whole-forward time.
* On the same latents: per returned activation and for the image max|bf16 - fp32| / max|fp32|; the share of differing bytes after
  ``sis_make_image_u8``; PSNR between the two uint8 images through ``sis_psnr_ssim``.

Writes profiles/gen_bf16.json and prints it.

    python tools/bench_gen_bf16.py [--runs 5] [--batch 32] [--size 256] [--out profiles/gen_bf16.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))

import torch  # noqa: E402

WINDOW_SECONDS = 0.2
CACHE_BYTES = 288 << 20   # input sets of a layer together exceed the 256 MiB Infinity Cache


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(variants, runs):
    """{name: [ms per call, one per run]}: warm-up, a pilot to size the window, then ``runs`` alternating rounds."""
    iters = {}
    for name, fn in variants.items():
        timed(fn, 3)
        pilot = timed(fn, 5)
        iters[name] = int(min(2000, max(5, WINDOW_SECONDS * 1e3 / max(pilot, 1e-3))))
    samples = {name: [] for name in variants}
    for _ in range(runs):
        for name, fn in variants.items():
            samples[name].append(round(timed(fn, iters[name]), 5))
    return samples, iters


def summary(samples):
    return {"runs_ms": samples, "median_ms": round(statistics.median(samples), 5), "min_ms": min(samples), "max_ms": max(samples)}


def every_run_below(a, b):
    return max(a) < min(b)


def bench_layer(sis_hip, device, batch, cin, cout, res, runs, gen):
    mk = lambda *s: torch.randn(*s, generator=gen, device=device)
    weight = mk(1, cout, cin, 3, 3)
    wpk, wsq = sis_hip.modconv_prepack(weight)
    u24, packed = sis_hip.modconv_prepack_wino24(weight), sis_hip.modconv_prepack_bf16(weight)
    s = 1 + 0.3 * mk(batch, cin)
    ds = sis_hip.modconv_demod(s, wsq, 1 / (cin * 9) ** 0.5, True)
    noise, nw, bias = mk(1, 1, res, res), 0.3 * mk(1), 0.2 * mk(cout)
    rgb_w, rgb_s = mk(3 * cout), 1 + 0.3 * mk(batch, cout)
    part = torch.empty(sis_hip.rgb_part_shape(batch, cout, res, res), device=device)
    n_sets = max(1, -(-CACHE_BYTES // (4 * batch * (cin + cout) * res * res)))
    xs = [mk(batch, cin, res, res) for _ in range(n_sets)]
    outs = [torch.empty(batch, cout, res, res, device=device) for _ in range(n_sets)]
    call = lambda i, **kw: sis_hip.modconv2d(xs[i % n_sets], wpk, s, ds, 3, noise, nw, bias, fuse_act=True, out=outs[i % n_sets], **kw)
    variants = {"bf16": lambda i: call(i, bf16_w=packed),
                "fp32_default_wino24_rgb": lambda i: call(i, wino24_u=u24, rgb=(rgb_w, rgb_s, 1 / cout ** 0.5, part)),
                "fp32_wino24": lambda i: call(i, wino24_u=u24)}
    samples, iters = measure(variants, runs)
    y_bf16 = call(0, bf16_w=packed).clone()
    y_fp32 = call(0, wino24_u=u24)
    flops = 2.0 * batch * cout * cin * 9 * res * res
    row = {"cin": cin, "cout": cout, "map": res, "batch": batch, "input_sets": n_sets, "direct_form_flops": flops, "iters": iters,
           **{name: summary(v) for name, v in samples.items()}}
    row["bf16_tflops_direct_form"] = round(flops / (row["bf16"]["median_ms"] * 1e-3) / 1e12, 1)
    row["bf16_over_default"] = round(row["bf16"]["median_ms"] / row["fp32_default_wino24_rgb"]["median_ms"], 4)
    row["every_bf16_run_below_every_default_run"] = every_run_below(samples["bf16"], samples["fp32_default_wino24_rgb"])
    row["layer_max_abs_diff_over_max_abs_fp32"] = float((y_bf16 - y_fp32).abs().max() / y_fp32.abs().max())
    return row


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--runs", type=int, default=5)
    parser.add_argument("--batch", type=int, default=32)
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_bf16.json"))
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gen_bf16: a HIP device is required (no CPU timing is meaningful)")
    import sis_hip
    from networks.stylegan2.model import Generator
    device = torch.device("cuda:0")
    gen = torch.Generator(device=device).manual_seed(0)
    torch.manual_seed(0)
    g32 = Generator(args.size, 512, 8, channel_multiplier=2).to(device).eval()
    g16 = Generator(args.size, 512, 8, channel_multiplier=2).to(device).eval()
    # random weights at the magnitudes of an initialised generator, noise injection switched on (its weight is zero at init)
    with torch.no_grad():
        for name, p in g32.named_parameters():
            if name.endswith("noise.weight"):
                p.fill_(0.1)
    g16.load_state_dict(g32.state_dict(), strict=True)
    g32.set_matrix_precision("fp32")
    g16.set_matrix_precision("bf16")
    z = torch.randn(args.batch, 512, generator=gen, device=device)
    noise = g32.make_noise()

    def forward(g):
        with torch.no_grad():
            return g([z], noise=noise, return_intermediate_activations=True)

    result = {"device": torch.cuda.get_device_name(0), "generator": {"size": args.size, "batch": args.batch, "style_dim": 512, "n_mlp": 8},
              "runs": args.runs, "timing": "device events around a window of at least 0.2 s after warm-up; the modes alternate"}

    # ---- deviation on the same latents (and which kernels each mode launches)
    rec32, rec16 = [], []
    sis_hip.set_profiler(rec32)
    img32, acts32 = forward(g32)
    sis_hip.set_profiler(rec16)
    img16, acts16 = forward(g16)
    sis_hip.set_profiler(None)
    torch.cuda.synchronize()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    u32, u16 = sis_hip.make_image_u8(img32.clamp(-1, 1)), sis_hip.make_image_u8(img16.clamp(-1, 1))
    f32, f16 = (u32.permute(0, 3, 1, 2).float() / 255).contiguous(), (u16.permute(0, 3, 1, 2).float() / 255).contiguous()
    psnr, ssim = sis_hip.psnr_ssim(f16, f32, unnormalize=2)
    result["deviation"] = {
        "bf16_launches_per_forward": sum(r[0] == sis_hip.BF16_KERNEL for r in rec16),
        "bf16_launches_in_fp32_mode": sum(r[0] == sis_hip.BF16_KERNEL for r in rec32),
        "activation_max_abs_diff_over_max_abs_fp32": {str(k): rel(acts16[k], acts32[k]) for k in sorted(acts32)},
        "image_max_abs_diff_over_max_abs_fp32": rel(img16, img32),
        "image_abs_max_fp32": float(img32.abs().max()),
        "uint8_bytes_differing_share": float((u32 != u16).float().mean()),
        "uint8_max_abs_diff": int((u32.int() - u16.int()).abs().max()),
        "uint8_psnr_db_per_image": {"min": float(psnr.min()), "median": float(psnr.median()), "max": float(psnr.max())},
        "uint8_ssim_per_image_min": float(ssim.min()),
        "all_finite": bool(torch.isfinite(img16).all()) and all(bool(torch.isfinite(a).all()) for a in acts16.values()),
    }
    del acts32, acts16, rec32, rec16

    # ---- the whole forward in both modes
    samples, iters = measure({"fp32": lambda i: forward(g32), "bf16": lambda i: forward(g16)}, args.runs)
    result["forward"] = {"iters": iters, **{name: summary(v) for name, v in samples.items()},
                         "bf16_over_fp32": round(statistics.median(samples["bf16"]) / statistics.median(samples["fp32"]), 4),
                         "every_bf16_run_below_every_fp32_run": every_run_below(samples["bf16"], samples["fp32"])}
    del g32, g16, img32, img16
    torch.cuda.empty_cache()

    # ---- per eligible layer shape (the stride-1 3x3 layers of the generator from 32^2 up)
    channels = Generator.get_channels(2)
    result["layers"] = []
    res = 32
    while res <= args.size:
        c = channels[res]
        if sis_hip.modconv_bf16_eligible(c, c, res, res):
            result["layers"].append(bench_layer(sis_hip, device, args.batch, c, c, res, args.runs, gen))
            torch.cuda.empty_cache()
        res *= 2
    text = json.dumps(result, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
