"""Discriminator downsampling layers on one MI355X: the polyphase route (``networks.hip_conv.down_conv3x3``: phase split +
composed weight + Winograd convolution) against today's blur + library stride-2 convolution.

The six downsampling layers of ``Discriminator(256)`` at the training batch (B = 24): 128 -> 256 @256^2, 256 -> 512 @128^2,
512 -> 512 @64^2, 32^2, 16^2, 8^2.  Per layer and formulation three timed regions, as a training iteration runs them:

  forward    y = layer(x, W) with autograd recording
  backward   dL/dx and dL/dW from dL/dy (the D step)
  r1         the double backward of the R1 penalty: d/dW |d<y, gy>/dx|^2 (the first-order graph is built outside the region)

Device events around ``--reps`` calls after ``--warmup`` untimed ones; the two formulations alternate inside each of ``--runs``
runs in one process; the table gives the median and the spread (min .. max) over the runs.  ``--loader`` adds one line: the
image loader's batch (ids upload + ``sis_gan_image_batch``) at 24 x 3 x 256 x 256.

    python tools/bench_gan_down.py [--batch 24] [--runs 5] [--out profiles/gan_polyphase_layers.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))

LAYERS = [(128, 256, 256), (256, 512, 128), (512, 512, 64), (512, 512, 32), (512, 512, 16), (512, 512, 8)]   # (Cin, Cout, H = W)


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def measure(layer_fn, x, w, gy, reps, warmup):
    """ms of (forward, backward, r1) for one formulation."""
    x, w = x.detach().requires_grad_(True), w.detach().requires_grad_(True)
    out = {}

    def forward():
        return layer_fn(x, w)

    for _ in range(warmup):
        forward()
    out["forward"] = timed(forward, reps)

    state = {}

    def fresh_forward():
        state["y"] = layer_fn(x, w)

    def backward():
        torch.autograd.grad(state["y"], (x, w), gy, retain_graph=True)

    fresh_forward()
    for _ in range(warmup):
        backward()
    out["backward"] = timed(backward, reps)

    def r1_graph():
        y = layer_fn(x, w)
        g, = torch.autograd.grad(y, x, gy, create_graph=True)
        state["penalty"] = g.pow(2).sum()

    def r1():
        torch.autograd.grad(state["penalty"], w, retain_graph=True)

    r1_graph()
    for _ in range(warmup):
        r1()
    out["r1"] = timed(r1, reps)
    state.clear()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, nargs="*", help="indices into the layer list (default: all six)")
    ap.add_argument("--loader", action="store_true", help="also time the image loader's batch")
    ap.add_argument("--out", help="write the JSON result here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gan_down.py needs a HIP device (a CPU run says nothing about these kernels)")
    import sis_hip
    from networks.hip_conv import down_conv3x3, down_conv3x3_supported
    from networks.stylegan2.model import make_kernel
    from networks.stylegan2.op import upfirdn2d
    device = torch.device("cuda:0")
    fir = make_kernel([1, 3, 3, 1]).to(device)
    result = {"batch": args.batch, "runs": args.runs, "reps": args.reps, "device": torch.cuda.get_device_name(0), "layers": []}
    print(f"{'layer':>22} {'region':>9} {'library ms (min..max)':>28} {'polyphase ms (min..max)':>28} {'ratio':>6}")
    for index in (args.layers if args.layers else range(len(LAYERS))):
        cin, cout, size = LAYERS[index]
        scale = 1 / math.sqrt(cin * 9)
        gen = torch.Generator(device="cpu").manual_seed(index)
        x = torch.randn(args.batch, cin, size, size, generator=gen).to(device)
        w = torch.randn(cout, cin, 3, 3, generator=gen).to(device)
        gy = torch.randn(args.batch, cout, size // 2, size // 2, generator=gen).to(device)
        if not down_conv3x3_supported(x, w, fir):
            sys.exit(f"layer {index}: the polyphase route declines {tuple(x.shape)}")
        formulations = {
            "library": lambda a, k: F.conv2d(upfirdn2d(a, fir, pad=(2, 2)), k * scale, stride=2),
            "polyphase": lambda a, k: down_conv3x3(a, k, fir, scale),
        }
        sis_hip.library_calls(reset=True)
        samples = {name: {"forward": [], "backward": [], "r1": []} for name in formulations}
        for _ in range(args.runs):
            for name, fn in formulations.items():   # alternating
                for region, ms in measure(fn, x, w, gy, args.reps, args.warmup).items():
                    samples[name][region].append(ms)
        assert "gan.down_conv3x3" not in sis_hip.library_calls(reset=True)["fallback"]
        row = {"cin": cin, "cout": cout, "size": size, "ms": samples}
        result["layers"].append(row)
        for region in ("forward", "backward", "r1"):
            lib, poly = samples["library"][region], samples["polyphase"][region]
            fmt = lambda v: f"{statistics.median(v):8.3f} ({min(v):.3f}..{max(v):.3f})"   # noqa: E731
            print(f"{f'{cin}->{cout} @{size}^2':>22} {region:>9} {fmt(lib):>28} {fmt(poly):>28} {statistics.median(poly) / statistics.median(lib):6.2f}",
                  flush=True)
        del x, w, gy
        torch.cuda.empty_cache()
    if args.loader:
        pixels = torch.randint(0, 256, (240, 3, 256, 256), dtype=torch.uint8).to(device)
        order = torch.randperm(240).tolist()

        def batch():
            ids = torch.tensor(order[:args.batch], dtype=torch.int32).to(device, non_blocking=True)
            return sis_hip.gan_image_batch(pixels, ids)

        for _ in range(3):
            batch()
        ms = [timed(batch, 20) for _ in range(args.runs)]
        result["loader_ms_per_batch"] = ms
        print(f"loader: batch of {args.batch} x 3 x 256 x 256 from 240 resident images: median {statistics.median(ms):.3f} ms "
              f"({min(ms):.3f}..{max(ms):.3f})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
