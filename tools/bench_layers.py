"""Per-layer timing of the generator's convolution kernels (development tool, GPU box).
usage: python tools/bench_layers.py [batch] [reps] [layer, e.g. conv64]   -> one line per layer: ms, TFLOP/s
SIS_WINOGRAD=0: direct kernel; SIS_WINO24=0: F(2x2,3x3) where F(2x4,3x3) would run (the generator's own switches).
SIS_LAYER_LAUNCHES=1: per-launch times instead (median, min, max), the form the per-layer selection rule of DESIGN 3.2 reads.
SIS_WINO24_TPW=n: n tiles per workgroup on the F(2x4,3x3) layers instead of the launcher's choice.
SIS_WINO24_RGB=1: the F(2x4,3x3) layers also form the ToRGB channel sum (modconv_wino24_kernel<true>).
SIS_LAYER_AB=1: the ship-list rule of DESIGN 3.2e -- on every layer both kernels take, launches of modconv_wino24_kernel<true> and
modconv_wino44_kernel<true> alternate in this process; per kernel the median, min and max of REPS launches."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))
import torch  # noqa: E402
import sis_hip  # noqa: E402

if os.environ.get("SIS_HIP_LIB"):  # same-box A/B of kernel builds (tools/build_variant.sh)
    sis_hip.LIB_PATH = os.path.join(ROOT, "synthesis-in-style_amd", "lib", os.environ["SIS_HIP_LIB"])

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
only = sys.argv[3] if len(sys.argv) > 3 else ""
WINO = os.environ.get("SIS_WINOGRAD", "1") != "0"
WINO24 = WINO and os.environ.get("SIS_WINO24", "1") != "0"
LAUNCHES = os.environ.get("SIS_LAYER_LAUNCHES", "0") == "1"
AB = os.environ.get("SIS_LAYER_AB", "0") == "1"
dev = torch.device("cuda:0")
layers = [("conv", 512, 512, 4), ("up", 512, 512, 4), ("conv", 512, 512, 8), ("up", 512, 512, 8),
          ("conv", 512, 512, 16), ("up", 512, 512, 16), ("conv", 512, 512, 32), ("up", 512, 512, 32),
          ("conv", 512, 512, 64), ("up", 512, 256, 64), ("conv", 256, 256, 128), ("up", 256, 128, 128),
          ("conv", 128, 128, 256)]
tot = 0.0
for kind, cin, cout, h in layers:
    if only and only != f"{kind}{h}":
        continue
    x = torch.randn(B, cin, h, h, device=dev)
    w = torch.randn(1, cout, cin, 3, 3, device=dev)
    s = 1 + 0.1 * torch.randn(B, cin, device=dev)
    wpk, wsq = sis_hip.modconv_prepack(w)
    ds = sis_hip.modconv_demod(s, wsq, 1 / (cin * 9) ** 0.5, True)
    oh = h if kind == "conv" else 2 * h
    noise = torch.randn(1, 1, oh, oh, device=dev)
    nw = torch.full((1,), 0.1, device=dev)
    bias = torch.zeros(cout, device=dev)
    if AB:
        if kind != "conv" or not (sis_hip.modconv_wino24_eligible(cin, cout, h, h) and sis_hip.modconv_wino44_eligible(cin, cout, h, h)):
            continue
        rgb = (torch.randn(3, cout, device=dev), 1 + 0.1 * torch.randn(B, cout, device=dev), 1 / cout ** 0.5,
               torch.empty(sis_hip.rgb_part_shape(B, cout, h, h), device=dev))
        packs = {"wino24": {"wino24_u": sis_hip.modconv_prepack_wino24(w)}, "wino44": {"wino44_u": sis_hip.modconv_prepack_wino44(w)}}
        ts = {name: [] for name in packs}
        for it in range(REPS + 2):
            for name, pack in packs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                sis_hip.modconv2d(x, wpk, s, ds, 3, noise, nw, bias, fuse_act=True, rgb=rgb, **pack)
                e1.record()
                torch.cuda.synchronize()
                if it >= 2:
                    ts[name].append(e0.elapsed_time(e1))
        fl = 2.0 * B * cout * cin * 9 * h * h
        for name, factor in (("wino24", 24 / 72), ("wino44", 36 / 144)):
            t = sorted(ts[name])
            med = t[len(t) // 2]
            print(f"{kind:5s} {cin:4d}->{cout:4d} @{h:3d}  {name}  median {med:8.3f} ms  min {t[0]:8.3f}  max {t[-1]:8.3f}  "
                  f"executed {factor * fl / med / 1e9:6.1f} TFLOP/s", flush=True)
        continue
    if kind == "conv" and WINO24 and sis_hip.modconv_wino24_eligible(cin, cout, h, h):
        kw = {"wino24_u": sis_hip.modconv_prepack_wino24(w), "wino24_tiles_per_wg": int(os.environ.get("SIS_WINO24_TPW", "0"))}
        if os.environ.get("SIS_WINO24_RGB", "0") == "1":
            kw["rgb"] = (torch.randn(3, cout, device=dev), 1 + 0.1 * torch.randn(B, cout, device=dev), 1 / cout ** 0.5,
                         torch.empty(sis_hip.rgb_part_shape(B, cout, h, h), device=dev))
    else:
        kw = {"wino_u": sis_hip.modconv_prepack_wino(w) if (WINO and kind == "conv") else None}
    f = (lambda: sis_hip.modconv2d(x, wpk, s, ds, 3, noise, nw, bias, fuse_act=True, **kw)) if kind == "conv" else \
        (lambda: sis_hip.modconv2d_up(x, wpk, s, ds))
    f()
    torch.cuda.synchronize()
    if LAUNCHES:
        ts = []
        for _ in range(REPS + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts = sorted(ts[2:])
        print(f"{kind:5s} {cin:4d}->{cout:4d} @{h:3d}  {sis_hip.lib().sis_last_kernel().decode():24s} median {ts[len(ts) // 2]:8.3f} ms  "
              f"min {ts[0]:8.3f}  max {ts[-1]:8.3f}", flush=True)
        continue
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        f()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / REPS
    fl = 2.0 * B * cout * cin * 9 * h * h
    tot += ms
    print(f"{kind:5s} {cin:4d}->{cout:4d} @{h:3d}  {ms:8.3f} ms  {fl / ms / 1e9:7.2f} TFLOP/s", flush=True)
print(f"total {tot:.3f} ms")
