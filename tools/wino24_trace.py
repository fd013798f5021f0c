"""Development tool (GPU box): cycles per tile of modconv_wino24_kernel between two chunk loops, from the trace build
(tools/wino_trace.sh): where a workgroup that walks several tiles spends the time in which no MFMA runs.
usage: python tools/wino24_trace.py [h=256] [cin=128] [cout=128] [batch=32]"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))
import torch  # noqa: E402
import sis_hip  # noqa: E402

sis_hip.LIB_PATH = os.path.join(ROOT, "synthesis-in-style_amd", "lib", "libsis_hip_trace%s.so" % os.environ.get("SIS_TRACE_SUFFIX", ""))
h = int(sys.argv[1]) if len(sys.argv) > 1 else 256
cin = int(sys.argv[2]) if len(sys.argv) > 2 else 128
cout = int(sys.argv[3]) if len(sys.argv) > 3 else 128
B = int(sys.argv[4]) if len(sys.argv) > 4 else 32
dev = torch.device("cuda:0")
x = torch.randn(B, cin, h, h, device=dev)
w = torch.randn(1, cout, cin, 3, 3, device=dev)
s = 1 + 0.1 * torch.randn(B, cin, device=dev)
wpk, wsq = sis_hip.modconv_prepack(w)
ds = sis_hip.modconv_demod(s, wsq, 1 / (cin * 9) ** 0.5, True)
noise = torch.randn(1, 1, h, h, device=dev)
nw = torch.full((1,), 0.1, device=dev)
bias = torch.zeros(cout, device=dev)
u = sis_hip.modconv_prepack_wino24(w)
L = sis_hip.lib()
L.sis_wino24_trace_tile_read.argtypes = [ctypes.c_void_p]


f = lambda: sis_hip.modconv2d(x, wpk, s, ds, 3, noise, nw, bias, fuse_act=True, wino24_u=u)  # noqa: E731
for _ in range(3):
    f()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(10):
    f()
e1.record()
torch.cuda.synchronize()
buf = np.zeros((4, 8, 16, 8), dtype=np.uint32)
assert L.sis_wino24_trace_tile_read(buf.ctypes.data) == 0
print(f"{cin}->{cout} @{h} B={B}, {e0.elapsed_time(e1) / 10:.3f} ms per launch (trace build)")
names = ["exchange + barrier", "finalise + stores", "barrier + DMA/loads issued", "vmcnt(0) + barrier", "V(0) + barrier -> loop"]
d = lambda a, b: (b - a) & 0xFFFFFFFF  # noqa: E731
for g in range(4):
    t = buf[g].astype(np.int64)  # [wave][tile][slot]
    ks = [k for k in range(1, 16) if t[0, k, 0] and t[0, k, 1] and t[0, k - 1, 1]]
    if not ks:
        print(f"  workgroup {g}: one tile per workgroup, no tile boundary")
        continue
    # stamps in program order from tile k - 1's last MFMA to tile k's first
    pts = lambda k: [t[:, k - 1, 1], t[:, k - 1, 2], t[:, k - 1, 3], t[:, k, 4], t[:, k, 5], t[:, k, 0]]  # noqa: E731
    sp = np.stack([np.stack([d(a, b) for a, b in zip(pts(k)[:-1], pts(k)[1:])], axis=-1) for k in ks])  # [tile][wave][span]
    loop = np.stack([d(t[:, k - 1, 0], t[:, k - 1, 1]) for k in ks])
    tile = np.stack([d(t[:, k - 1, 0], t[:, k, 0]) for k in ks])
    med = np.median(sp.reshape(-1, sp.shape[-1]), axis=0).astype(int)
    gap = int(np.median(sp.sum(-1)))
    print(f"  workgroup {g}: {len(ks)} boundaries; cycles per tile {int(np.median(tile))}, chunk loop {int(np.median(loop))}, "
          f"gap {gap} ({100.0 * gap / np.median(tile):.1f} %)")
    print("    " + " | ".join(f"{n} {m}" for n, m in zip(names, med)))
