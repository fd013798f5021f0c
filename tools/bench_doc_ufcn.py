"""DocUFCN training step on one MI355X: the graphed step of the HIP path against the same step on plain ATen (torch's modules,
``F.cross_entropy(weight=...)``, ``clip_grad_norm_`` + ``torch.optim.Adam``), same process, same shapes.

Config: reference configs/segmenter/stylegan2_doc_ufcn_segmenter.yaml -- DocUFCN('base')(3, 3), B = 8, 256^2, dropout 0.4,
GradientClipAdam(lr, betas=(beta1, beta2), weight_decay), class weights of three classes.  Prints one JSON line:
images/s of both, and the profiler's own-vs-library kernel time split of one eager step of the HIP path.

    python tools/bench_doc_ufcn.py [--batch 8] [--size 256] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

CONFIG = dict(lr=1e-3, beta1=0.9, beta2=0.999, weight_decay=1e-4, class_weights=[1.0, 2.0, 0.5])


def _batches(n, b, size, dev):
    g = torch.Generator().manual_seed(0)
    return [{'images': torch.randn(b, 3, size, size, generator=g).to(dev),
             'segmented': torch.randint(0, 3, (b, 1, size, size), generator=g).to(dev)} for _ in range(n)]


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import sis_hip
    from networks.doc_ufcn import get_doc_ufcn
    from training.fused_adam import GradientClipAdam
    from updater.segmentation_updater import StandardUpdater

    dev = torch.device("cuda:0")
    batches = _batches(4, args.batch, args.size, dev)
    torch.manual_seed(0)
    net = get_doc_ufcn('base')(3, 3).to(dev).train()
    opt = GradientClipAdam(net.parameters(), lr=CONFIG['lr'], betas=(CONFIG['beta1'], CONFIG['beta2']),
                           weight_decay=CONFIG['weight_decay'])
    up = StandardUpdater(iterators={'images': batches}, networks={'segmentation': net}, optimizers={'main': opt}, device=dev,
                         class_weights=CONFIG['class_weights'], hip_graph=True)
    up._step_graph.strict = True   # a capture that fails must fail the run, not pass as an eager measurement
    own_s = _time(up.update, args.steps, args.warmup)
    if up._step_graph.graph is None:
        raise RuntimeError("the DocUFCN step was not captured")

    # own-vs-library split of one eager step of the same path
    eager = StandardUpdater(iterators={'images': batches}, networks={'segmentation': net}, optimizers={'main': opt}, device=dev,
                            class_weights=CONFIG['class_weights'], hip_graph=False)
    eager.update()
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        eager.update()
        torch.cuda.synchronize()
    own_us = lib_us = 0.0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            t = getattr(e, "device_time", None)
            t = e.cuda_time if t is None else t
            if sis_hip.is_own_kernel(e.name):
                own_us += t
            else:
                lib_us += t

    # plain ATen formulation of the same step
    torch.manual_seed(0)
    ref = get_doc_ufcn('base')(3, 3).to(dev).train()
    ref_opt = torch.optim.Adam(ref.parameters(), lr=CONFIG['lr'], betas=(CONFIG['beta1'], CONFIG['beta2']),
                               weight_decay=CONFIG['weight_decay'])
    wts = torch.tensor(CONFIG['class_weights'], device=dev)
    it = [0]

    def aten_step():
        batch = batches[it[0] % len(batches)]
        it[0] += 1
        ref_opt.zero_grad()
        loss = F.cross_entropy(ref._forward_torch(batch['images']), batch['segmented'][:, 0], weight=wts)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
        ref_opt.step()

    aten_s = _time(aten_step, args.steps, args.warmup)
    print(json.dumps({
        "workload": f"DocUFCN train step B={args.batch} {args.size}^2 fp32 dropout 0.4",
        "own_images_per_s": round(args.batch / own_s, 1), "own_step_ms": round(own_s * 1e3, 3), "own_hip_graph": True,
        "aten_images_per_s": round(args.batch / aten_s, 1), "aten_step_ms": round(aten_s * 1e3, 3),
        "speedup": round(aten_s / own_s, 3),
        "eager_step_own_kernel_ms": round(own_us / 1e3, 3), "eager_step_library_kernel_ms": round(lib_us / 1e3, 3),
        "library_fallbacks": sis_hip.library_calls()["fallback"],
        "device": torch.cuda.get_device_name(0),
    }))


if __name__ == "__main__":
    main()
