"""Catalog fitting on one MI355X -> profiles/semantic_clusters_bench.json.

Generator(256) (random weights: the timings depend on shapes, the iteration counts on the data) activations of --samples
samples; for layers 8/9 (512 x 64^2) and 12/13 (128 x 256^2) and k = 3 .. 23 in one batched run per layer: seconds of
plan + init, loop (and per iteration), label passes.  The fused label pass alone against the same pass written in ATen
(F.normalize of the permuted activation, matmul, argmax), alternated in this process, with its HBM rate against the 8 TB/s
roofline and its fp32 MFMA rate.  The compute part of the whole CLI stage (activations + every layer x every k) and the file
writing of ONE cluster count.  Host comparison: scikit-learn's MiniBatchKMeans on the normalised rows of layer 8, one cluster
count, if scikit-learn is installed.  Everything is timed after a warm-up of the same shape, with device synchronisation.
"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))
import sis_hip  # noqa: E402
import create_semantic_segmentation as S  # noqa: E402
from segmentation.gan_local_edit.spherical_kmeans import MiniBatchSphericalKMeans  # noqa: E402


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def aten_label_pass(x, cen):
    b, c, h, w = x.shape
    rows = torch.nn.functional.normalize(x.permute(0, 2, 3, 1).reshape(-1, c), dim=1)
    return (rows @ cen.t()).argmax(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--batch-size", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semantic_clusters_bench.json"))
    ap.add_argument("--host-k", type=int, default=8)
    ap.add_argument("--skip-host", action="store_true")
    opt = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    args = S.build_parser().parse_args(["-n", str(opt.samples), "-b", str(opt.batch_size), "--image-size", "256"])
    g = S.load_generator(None, 256, 512, 8, 2, dev)
    t_act, (acts, images) = timed(lambda: S.get_activations(args, g, dev), 1)
    ks = list(range(3, 24))
    out = {"device": torch.cuda.get_device_name(0), "samples": opt.samples, "generator": "Generator(256), random weights",
           "cluster_counts": [ks[0], ks[-1]], "activations_s": t_act, "layers": {}}
    MiniBatchSphericalKMeans.fit_many(acts[4], ks)   # warm-up: library load, LDS attributes
    for layer in (8, 9, 12, 13):
        x = acts[layer]
        b, c, h, w = x.shape
        MiniBatchSphericalKMeans.fit_many(x, ks)   # warm-up of this shape
        timings = {}
        models = MiniBatchSphericalKMeans.fit_many(x, ks, timings=timings)
        iters = [m.n_iter_ for m in models]
        cen = torch.from_numpy(models[5].cluster_centers_).to(dev)   # k = 8
        sis_hip.skm_label(x, cen)
        aten_label_pass(x, cen)
        fused, atn = [], []
        for _ in range(3):   # alternated
            fused.append(timed(lambda: sis_hip.skm_label(x, cen), 5)[0])
            atn.append(timed(lambda: aten_label_pass(x, cen), 5)[0])
        lab, _ = sis_hip.skm_label(x, cen)
        same = float((lab == aten_label_pass(x, cen)).float().mean())
        f, a = min(fused), min(atn)
        out["layers"][str(layer)] = {
            "shape": [b, c, h, w], "fits": len(ks), "n_iter_min_max": [min(iters), max(iters)],
            "plan_init_s": timings["plan_init_s"], "loop_s": timings["loop_s"], "label_passes_s": timings["label_pass_s"],
            "loop_us_per_iteration_all_fits": 1e6 * timings["loop_s"] / max(iters),
            "label_pass_fused_ms": 1e3 * f, "label_pass_aten_ms": 1e3 * a, "aten_over_fused": a / f,
            "label_pass_tb_per_s": x.numel() * 4 / f / 1e12, "label_pass_fraction_of_8_tb_per_s": x.numel() * 4 / f / 8e12,
            "label_pass_mfma_tflops_padded_to_32_centres": 2.0 * b * h * w * c * 32 / f / 1e12,
            "labels_equal_to_aten": same}
        print(layer, json.dumps(out["layers"][str(layer)]), flush=True)
    # ---- the compute part of the whole stage: every layer, every cluster count
    t_fit, found = timed(lambda: S.find_clusters(acts, ks), 1)
    out["stage"] = {"layers": len(acts), "cluster_counts": len(ks), "fits": len(acts) * len(ks), "activations_s": t_act,
                    "fit_all_layers_all_counts_s": t_fit}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        S.save_catalogs(found[8], acts, 8, Path(tmp))
        rendered = {layer: S.render_clusters(m.labels_.reshape(acts[layer].shape[0], *acts[layer].shape[-2:]), 8).cpu().numpy()
                    for layer, m in found[8].items()}
        rendered[max(rendered) + 1] = images
        S.save_cluster_visualizations(rendered, 8, Path(tmp))
        out["stage"]["write_files_of_one_cluster_count_s"] = time.perf_counter() - t0
    out["stage"]["note"] = "the stage writes the files of every cluster count (21 here); only one was timed"
    print("stage", json.dumps(out["stage"]), flush=True)
    # ---- host comparison
    if not opt.skip_host:
        try:
            from sklearn.cluster import MiniBatchKMeans
        except ImportError:
            out["host_scikit_learn"] = "not measured: scikit-learn is not installed"
        else:
            x = acts[8]
            t0 = time.perf_counter()
            rows = torch.nn.functional.normalize(x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]), dim=1).cpu().numpy()
            t_copy = time.perf_counter() - t0
            t0 = time.perf_counter()
            km = MiniBatchKMeans(n_clusters=opt.host_k, random_state=0, batch_size=100, max_iter=100, n_init=3, max_no_improvement=10,
                                 reassignment_ratio=0.01, tol=0.0).fit(rows)
            out["host_scikit_learn"] = {"layer": 8, "k": opt.host_k, "samples": opt.samples, "rows": len(rows), "threads": os.environ.get("OMP_NUM_THREADS"),
                                        "normalise_on_device_and_copy_s": t_copy, "fit_s": time.perf_counter() - t0, "n_iter_epochs": int(km.n_iter_), "n_steps": int(km.n_steps_),
                                        "note": "one fit of one cluster count on one layer; the stage has layers x counts of them"}
        print("host", json.dumps(out.get("host_scikit_learn")), flush=True)
    with open(opt.out, "w") as fjson:
        json.dump(out, fjson, indent=1)
    print("wrote", opt.out)


if __name__ == "__main__":
    main()
