"""The projection encoder on one MI355X (networks/encoder/u_net_like_encoder.py, csrc/encoder_ops.h).

A WPlusEncoder on Generator(256, channel_multiplier=2)'s channel map (3 input channels, latent size 512, 14 BasicBlocks), eval(),
torch.no_grad(), float32, at B = 1 and 8:
  * ms per encode on the library's kernels (default) and with SIS_ENCODER_HIP=0 (the ATen / MIOpen formulation: the only way
    to run this network before these kernels existed), in one process, alternating, five runs each (a run = ``--steps`` timed
    encodes after ``--warmup``); the median run is reported, all runs are listed;
  * ms per encode per layer class (stem, stride-2, Winograd, tail, heads) from device events around each launch
    (``sis_hip.set_profiler``; sis_bn_act_fwd and the subsampling copies are not bracketed and show in ``unbracketed_ms`` with
    the launch gaps; where the encoder dispatches a stride-2 layer to the dense-and-subsample route, its 3x3 part counts as a
    Winograd launch and its shortcut as ``stride2_shortcut_1x1``);
  * per stride-2 layer, ``sis_enc_conv3x3_s2`` (main + shortcut output, one read of the input) against the dense-and-subsample
    route as the encoder dispatches it (``UNetLikeEncoder._conv1_stride2_dense``: Winograd stride-1 convolution, subsample,
    sis_bn_act_fwd; the shortcut as subsample + sis_conv1x1_f32 + sis_bn_act_fwd), alternating, five runs each;
  * the 14 block tails (with their noise heads and pool partials) and the latent heads launch against their ATen counterparts
    (affine + add + relu, Conv2d to one channel, adaptive_avg_pool2d; 14 Conv2d on the pooled maps + stack), summed over the
    encoder's block outputs, alternating, five runs each;
  * encode + decode images/s (StyleganAutoencoder.forward) beside bare synthesis of the same Generator(256), B = 8.
Writes profiles/encoder_bench.json (``--out``) and prints it.  ``--stride2-route k1`` puts every stride-2 layer of the
whole-encoder figures on ``sis_enc_conv3x3_s2``: profiles/encoder_bench_k1_only.json, the measurement the dispatch rests on.

    python tools/bench_encoder.py [--steps 10] [--warmup 3] [--stride2-route k1 --out profiles/encoder_bench_k1_only.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))

import torch  # noqa: E402

SIZE, LATENT, RUNS = 256, 512, 5


def _events_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _alternate(fns, steps, warmup):
    """{name: [ms per call of each of the five runs]}, the variants taking turns."""
    runs = {name: [] for name in fns}
    for _ in range(RUNS):
        for name, fn in fns.items():
            runs[name].append(round(_events_ms(fn, steps, warmup), 4))
    return runs


def _switch(value):
    if value is None:
        os.environ.pop("SIS_ENCODER_HIP", None)
    else:
        os.environ["SIS_ENCODER_HIP"] = value


def _layer_class(kernel):
    if kernel == "enc_stem_kernel":
        return "stem"
    if kernel == "enc_conv3x3_s2_kernel":
        return "stride2"
    if kernel == "enc_block_tail_kernel":
        return "tail"
    if kernel == "enc_latent_heads_kernel":
        return "heads"
    if "conv1x1_f32" in kernel:
        return "stride2_shortcut_1x1"   # the dense-and-subsample route's shortcut; its 3x3 part is among the Winograd launches
    return "winograd" if "wino" in kernel else kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stride2-route", choices=["measured", "k1"], default="measured",
                    help="k1: every stride-2 layer of the whole-encoder figures on sis_enc_conv3x3_s2 (the measurement the dispatch rests on)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_bench.json"))
    args = ap.parse_args()
    import sis_hip
    from networks.encoder.autoencoder import StyleganAutoencoder
    import networks.encoder.u_net_like_encoder as E
    from networks.encoder.u_net_like_encoder import WPlusEncoder
    E.STRIDE2_ROUTE = args.stride2_route
    from networks.stylegan2.model import Generator
    assert torch.cuda.is_available(), "bench_encoder.py needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = Generator(SIZE, LATENT, 8, channel_multiplier=2).to(dev).eval()
    enc = WPlusEncoder(SIZE, LATENT, 3, g.channels, stylegan_variant=2)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
    enc = enc.to(dev).eval()
    auto = StyleganAutoencoder(enc, g).eval()
    out = {"workload": "WPlusEncoder on Generator(256, channel_multiplier=2)'s channel map, 3 input channels, latent 512, eval, fp32",
           "device": torch.cuda.get_device_name(0), "stride2_route": args.stride2_route, "runs": RUNS, "steps_per_run": args.steps, "batch": {}}

    def encode(x, switch):
        def fn():
            _switch(switch)
            with torch.no_grad():
                return enc(x)
        return fn

    for batch in (1, 8):
        x = torch.rand(batch, 3, SIZE, SIZE, device=dev) * 2 - 1
        runs = _alternate({"hip": encode(x, None), "aten": encode(x, "0")}, args.steps, args.warmup)
        _switch(None)
        a, b = encode(x, None)(), encode(x, "0")()
        _switch(None)
        err = max((a.latent - b.latent).abs().max().item() / b.latent.abs().max().item(),
                  max((p - q).abs().max().item() / q.abs().max().item() for p, q in zip(a.noise, b.noise)))
        # per layer class: one bracketed encode pass, averaged over the steps
        records = []
        sis_hip.library_calls(reset=True)
        sis_hip.set_profiler(records)
        for _ in range(args.steps):
            encode(x, None)()
        sis_hip.set_profiler(None)
        torch.cuda.synchronize()
        classes, launches = {}, {}
        for kernel, _, _, e0, e1 in records:
            c = _layer_class(kernel)
            classes[c] = classes.get(c, 0.0) + e0.elapsed_time(e1) / args.steps
            launches[c] = launches.get(c, 0) + 1
        hip = statistics.median(runs["hip"])
        out["batch"][str(batch)] = {
            "hip_ms_per_encode": hip, "hip_runs_ms": runs["hip"], "aten_ms_per_encode": statistics.median(runs["aten"]),
            "aten_runs_ms": runs["aten"], "speedup": round(statistics.median(runs["aten"]) / hip, 3),
            "max_rel_difference_hip_vs_aten": float(f"{err:.3e}"),
            "layer_class_ms": {k: round(v, 4) for k, v in sorted(classes.items())},
            "layer_class_launches": {k: v // args.steps for k, v in sorted(launches.items())},
            "unbracketed_ms": round(hip - sum(classes.values()), 4),
            "declined_layers": {k: v for k, v in sis_hip.LIBRARY_CALLS.items() if "encoder" in k}}

    # ---- K1 against the dense-and-subsample route, per stride-2 layer: the dispatched code itself (_conv1_stride2_dense)
    out["stride2_layers"] = {}
    packs = enc._packs()["packs"]
    s2 = [(b, p) for b, p in zip(enc._blocks(), packs) if b.stride == 2]
    for batch in (1, 8):
        size = SIZE
        for block, p in s2:
            cin, cout = block.conv1.in_channels, block.conv1.out_channels
            x = torch.randn(batch, cin, size, size, device=dev)
            packed = enc._stride2_image(block, dict(p, s2=None), "s2")
            fns = {"k1": lambda: sis_hip.enc_conv3x3_s2(x, packed, cout, *p["bn1"], *p["bnd"])}
            scratch = dict(p)   # (the Winograd image this builds is dropped with the dict)
            E.STRIDE2_ROUTE = "measured"
            dense_ok = enc._conv1_stride2_dense(x, block, scratch) is not None
            if dense_ok:
                fns["dense_subsample"] = lambda: enc._conv1_stride2_dense(x, block, scratch)
            runs = _alternate(fns, args.steps, args.warmup)
            row = {"k1_ms": statistics.median(runs["k1"]), "k1_runs_ms": runs["k1"],
                   "k1_tflops": round(2.0 * batch * cout * cin * 10 * (size // 2) ** 2 / statistics.median(runs["k1"]) / 1e9, 2)}
            if dense_ok:
                row.update({"dense_subsample_ms": statistics.median(runs["dense_subsample"]), "dense_subsample_runs_ms": runs["dense_subsample"]})
                (m, s), (dm, ds) = fns["k1"](), fns["dense_subsample"]()
                row["max_rel_difference"] = float(f"{max((m - dm).abs().max().item() / dm.abs().max().item(), (s - ds).abs().max().item() / ds.abs().max().item()):.3e}")
            out["stride2_layers"][f"B{batch} {cin}->{cout} {size}x{size}"] = row
            size //= 2
    E.STRIDE2_ROUTE = args.stride2_route

    # ---- the block tails and the latent heads against their ATen counterparts, summed over the 14 block outputs
    out["tail_and_heads"] = {}
    for batch in (1, 8):
        cases, size = [], SIZE
        for j, (block, p) in enumerate(zip(enc._blocks(), packs)):
            if block.stride == 2:
                size //= 2
            ch = block.conv1.out_channels
            cases.append((torch.randn(batch, ch, size, size, device=dev), torch.randn(batch, ch, size, size, device=dev), p["bn2"],
                          enc._noise_head(j), enc._latent_head(j), size * size))
        partials = {}

        def tails_hip():
            for j, (c, r, bn2, nh, lh, hw) in enumerate(cases):
                _, _, partials[j] = sis_hip.enc_block_tail(c, r, *bn2, nh.weight.detach() if nh is not None else None,
                                                           nh.bias.detach() if nh is not None else None, want_pool=True)

        pooled = {}

        def tails_aten():
            with torch.no_grad():
                for j, (c, r, bn2, nh, lh, hw) in enumerate(cases):
                    y = torch.relu(c * bn2[0].view(1, -1, 1, 1) + bn2[1].view(1, -1, 1, 1) + r)
                    if nh is not None:
                        nh(y)
                    pooled[j] = torch.nn.functional.adaptive_avg_pool2d(y, (1, 1))
        tails_hip()
        tails_aten()
        n = len(cases)
        table = sis_hip.enc_heads_table(sorted(((partials[j], cases[j][5], cases[j][4].weight.detach(), cases[j][4].bias.detach(), n - 1 - j)
                                                for j in range(n)), key=lambda r: r[4]), dev)

        def heads_aten():
            with torch.no_grad():
                return torch.stack([cases[j][4](pooled[j]) for j in range(n)][::-1], dim=1).squeeze(3).squeeze(3)
        runs = _alternate({"tail_hip": tails_hip, "tail_aten": tails_aten, "heads_hip": lambda: sis_hip.enc_latent_heads(table), "heads_aten": heads_aten},
                          args.steps, args.warmup)
        out["tail_and_heads"][str(batch)] = {k + "_ms": statistics.median(v) for k, v in runs.items()}
        out["tail_and_heads"][str(batch)].update({k + "_runs_ms": v for k, v in runs.items()})

    # ---- encode + decode beside bare synthesis
    batch = 8
    x = torch.rand(batch, 3, SIZE, SIZE, device=dev) * 2 - 1
    z = torch.randn(batch, LATENT, device=dev)
    noise = g.make_noise()

    def synth():
        with torch.no_grad():
            return g([z], noise=noise)

    def auto_fwd():
        with torch.no_grad():
            return auto(x)
    runs = _alternate({"synthesis": synth, "encode_decode": auto_fwd}, args.steps, args.warmup)
    out["images_per_s_b8"] = {"synthesis": round(1000 * batch / statistics.median(runs["synthesis"]), 1), "synthesis_runs_ms": runs["synthesis"],
                              "encode_decode": round(1000 * batch / statistics.median(runs["encode_decode"]), 1),
                              "encode_decode_runs_ms": runs["encode_decode"]}
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
