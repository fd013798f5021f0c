"""DatasetGAN ensemble training, the parts that need no GPU: the updater's ATen path, the builder's snapshot, the dataset's
sampling, the stacked parameters of ``FusedEnsembleStep``, the C boundary and the CLI."""
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import ensemble_train_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"sis_pe_train_workspace_bytes", "sis_pe_train_gather", "sis_pe_train_l1_forward", "sis_pe_train_tail",
               "sis_pe_train_l1_wgrad"}
NEW_KERNELS = {"pe_gather_kernel", "pe_l1_fwd_kernel", "pe_colsum_kernel", "pe_colsum_finish_kernel", "pe_bn_finish_kernel",
               "pe_l2_fwd_kernel", "pe_l3_ce_kernel", "pe_finish3_kernel", "pe_l2_bwd_kernel", "pe_finish2_kernel", "pe_dz1_kernel",
               "pe_l1_wgrad_kernel", "pe_slab_sum_kernel"}


class _ListLoader:
    def __init__(self, batches):
        self.batches, self.dataset = batches, None

    def __iter__(self):
        return iter(self.batches)


def test_updater_aten_path_equals_a_hand_written_loop():
    from training.loop import get_current_reporter
    from updater.dataset_gan_updater import DatasetGANUpdater
    seed, steps, pixels, features, classes = 4, 3, 16, 32, 3
    batches = [dict(zip(("activations", "label"), C.batch(seed, s, pixels, features, classes))) for s in range(steps)]
    e = C.make_ensemble(seed, classes, features, 2)
    opts = C.make_optimizers(e)
    assert sorted(opts) == ["optimizer_0", "optimizer_1"]
    updater = DatasetGANUpdater(iterators={"feature_vectors": _ListLoader(batches)}, networks=e.get_networks(), optimizers=opts,
                                device="cpu")
    assert updater.fused_step is None and "HIP" in updater.fused_reason
    for _ in range(steps):
        updater.update()
    obs = get_current_reporter().observations
    assert {"loss/CrossEntropyLoss_network_0", "loss/CrossEntropyLoss_network_1"} <= set(obs)

    ref = C.make_ensemble(seed, classes, features, 2)
    ref_opts = C.make_optimizers(ref)
    ce = nn.CrossEntropyLoss()
    for b in batches:
        for i, m in enumerate(ref.get_networks().values()):
            ref_opts[f"optimizer_{i}"].zero_grad()
            loss = ce(m(b["activations"]), b["label"])
            loss.backward()
            ref_opts[f"optimizer_{i}"].step()
    for name in e.get_networks():
        for (k, a), (_, b) in zip(e.networks[name].state_dict().items(), ref.networks[name].state_dict().items()):
            assert torch.equal(a, b), (name, k)
    assert float(obs["loss/CrossEntropyLoss_network_1"]) == float(loss.detach())


def test_reset_calls_reset_dataset_where_it_exists():
    from updater.dataset_gan_updater import DatasetGANUpdater
    calls = []

    class _Dataset:
        def reset_dataset(self):
            calls.append(1)

    loader = _ListLoader([])
    loader.dataset = _Dataset()
    e = C.make_ensemble(0, 3, 32, 1)
    updater = DatasetGANUpdater(iterators={"feature_vectors": loader, "other": _ListLoader([])}, networks=e.get_networks(),
                                optimizers=C.make_optimizers(e), device="cpu")
    updater.reset()
    assert calls == [1]


def test_gate_seeds_keep_the_relu_gates_clear_of_zero():
    for seed in C.GATE_SEEDS:
        assert C.gates_clear(seed), seed


def _dataset(tmp_path, images=2, size=8, **kw):
    from data.dataset_gan_dataset import DeviceDatasetGANDataset
    maps = C.class_maps(images, size)
    per_image = [{0: np.random.default_rng(i).standard_normal((32, size // 2, size // 2)).astype(np.float32),
                  1: np.random.default_rng(9 + i).standard_normal((1, 32, size, size)).astype(np.float32)} for i in range(images)]
    json_path, npz, cmap = C.write_dataset(str(tmp_path), maps, per_image)
    return DeviceDatasetGANDataset(json_path, npz, cmap, size, device="cpu", **kw), maps, per_image


def test_dataset_epoch_and_validation_order(tmp_path):
    from data.dataset_gan_dataset import PixelBatchLoader
    ds, maps, per_image = _dataset(tmp_path)
    assert ds.get_feature_vector_length() == 64 and [tuple(t.shape) for t in ds.layers] == [(2, 32, 4, 4), (2, 32, 8, 8)]
    assert np.array_equal(ds.class_maps.numpy(), maps) and not hasattr(ds, "pixel_activations")
    total, b = 2 * 8 * 8, 24
    loader = PixelBatchLoader(ds, b, seed=1)
    assert len(loader) == total // b
    seen = []
    for batch in loader:
        assert batch["pixels"].dtype == torch.int32 and tuple(batch["pixels"].shape) == (b, 3) and batch["label"].dtype == torch.int64
        img, y, x = batch["pixels"].numpy().T
        assert np.array_equal(batch["label"].numpy(), maps[img, y, x])
        seen += list(img * 64 + y * 8 + x)
    assert len(seen) == len(set(seen)) == (total // b) * b          # at most once each, all but the last partial batch
    second = [tuple(batch["pixels"][0].tolist()) for batch in loader]
    first = [tuple(p) for p in np.stack([np.array(seen) // 64, np.array(seen) // 8 % 8, np.array(seen) % 8], 1)[::b]]
    assert second != first                                          # the next epoch is another permutation
    val = PixelBatchLoader(ds, b, shuffle=False, drop_last=False)
    flat = np.concatenate([bt["pixels"].numpy() @ np.array([64, 8, 1]) for bt in val])
    assert np.array_equal(flat, np.arange(total))
    # the features the ATen loop trains on are the reference's upsampled activations at those pixels
    pixels = next(iter(val))["pixels"]
    up = torch.nn.functional.interpolate(torch.from_numpy(np.stack([a[0] for a in per_image])), size=(8, 8), mode="bilinear",
                                         align_corners=False)
    img, y, x = pixels.long().T
    feats = ds.features(pixels)
    assert torch.allclose(feats[:, :32], up[img, :, y, x], atol=1e-6)
    assert torch.equal(feats[:, 32:], torch.from_numpy(np.stack([a[1][0] for a in per_image]))[img, :, y, x])


def test_dataset_random_sampling_follows_class_probabilities(tmp_path):
    from data.dataset_gan_dataset import PixelBatchLoader
    probabilities = [0.6, 0.3, 0.1]
    ds, maps, _ = _dataset(tmp_path, class_probabilities=probabilities, random_sampling=True)
    loader = PixelBatchLoader(ds, 32, seed=2)
    labels = np.concatenate([b["label"].numpy() for _ in range(8) for b in loader])
    n = labels.size
    assert n == 8 * 4 * 32
    for c, p in enumerate(probabilities):
        # 5 standard deviations of a binomial share: a correct sampler fails once in 1.7 million runs (and the seed is fixed)
        assert abs((labels == c).mean() - p) <= 5 * np.sqrt(p * (1 - p) / n), (c, (labels == c).mean())
    batch = next(iter(loader))
    img, y, x = batch["pixels"].numpy().T
    assert np.array_equal(batch["label"].numpy(), maps[img, y, x])


def test_fused_step_keeps_state_dict_keys_and_views_the_stacks():
    from training.ensemble_step import FusedEnsembleStep
    e = C.make_ensemble(1, 3, 64, 3)
    before = {name: {k: v.clone() for k, v in m.state_dict().items()} for name, m in e.get_networks().items()}
    params = {name: list(m.parameters()) for name, m in e.get_networks().items()}
    opts = C.make_optimizers(e)
    step = FusedEnsembleStep(e, opts)
    for name, m in e.get_networks().items():
        assert list(m.state_dict()) == list(before[name])
        assert all(a is b for a, b in zip(m.parameters(), params[name]))   # the optimizers' parameters are still the members'
        for k, v in m.state_dict().items():
            assert torch.equal(v, before[name][k]), (name, k)
    for kind, dotted in C.KINDS.items():
        stack, grad = step.stacks[kind], step.grads[kind]
        assert stack.shape[0] == 3 and stack.is_contiguous()
        for i, m in enumerate(e.get_networks().values()):
            p = C.param(m, dotted)
            assert p.data_ptr() == stack[i].data_ptr() and p.is_contiguous() and tuple(p.shape) == tuple(stack.shape[1:])
            assert p.grad.data_ptr() == grad[i].data_ptr() and p.grad.is_contiguous()
    m0 = e.networks["network_0"]
    assert m0.layers[2].running_var.data_ptr() == step.buffers["var1"][0].data_ptr()
    assert m0.layers[5].num_batches_tracked.data_ptr() == step.buffers["tracked2"][0].data_ptr()
    with torch.no_grad():
        step.stacks["b3"][1].fill_(7.0)
    assert float(e.networks["network_1"].layers[6].bias.detach()[0]) == 7.0
    with pytest.raises(RuntimeError, match="HIP device"):
        step.forward_backward(torch.zeros(4, 64), torch.zeros(4, dtype=torch.int64))


def test_fused_step_names_what_it_does_not_cover():
    from networks.pixel_classifier.model import PixelEnsembleClassifier
    from training.ensemble_step import FusedEnsembleStep
    assert FusedEnsembleStep.unsupported(PixelEnsembleClassifier(3, 64, 2)) is None
    assert "11 members" in FusedEnsembleStep.unsupported(PixelEnsembleClassifier(3, 32, 11))
    assert "multiple of 32" in FusedEnsembleStep.unsupported(PixelEnsembleClassifier(3, 40, 1))
    assert "wide variant" in FusedEnsembleStep.unsupported(PixelEnsembleClassifier(40, 64, 1))
    with pytest.raises(ValueError, match="wide variant"):
        FusedEnsembleStep(PixelEnsembleClassifier(40, 64, 1))


def test_header_and_ctypes_table_agree_on_the_new_symbols():
    import sis_hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sis_hip.h")).read(), flags=re.S)
    assert NEW_SYMBOLS <= set(re.findall(r"\b(sis_[a-z0-9_]+)\s*\(", header)) and NEW_SYMBOLS <= set(sis_hip.exported_symbols())
    for name in NEW_SYMBOLS:
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert decl.count(",") + 1 == len(sis_hip._SIGNATURES[name][0]), name
    L = sis_hip.lib()
    assert L.sis_pe_train_workspace_bytes(0, 1, 64, 1) == -1 and L.sis_pe_train_workspace_bytes(0, 64, 40, 1) == -1
    assert L.sis_pe_train_workspace_bytes(1, 64, 64, 11) == -1 and L.sis_pe_train_workspace_bytes(0, 64, 64, 3) > 0
    # the weight gradient's slabs: none up to 2048 pixels, then one [N*128, F] slab per 2048 pixels, at most 8
    small, large = L.sis_pe_train_workspace_bytes(1, 2048, 64, 1), L.sis_pe_train_workspace_bytes(1, 2049, 64, 1)
    assert large - small >= 2 * 128 * 64 * 4 > small


def test_new_kernels_count_as_own():
    import sis_hip
    assert NEW_KERNELS <= sis_hip.own_kernel_names()
    assert sis_hip.is_own_kernel("void (anonymous namespace)::pe_colsum_kernel<true>(float const*, double*, int, int)")


def test_cli_parses_its_arguments_and_the_config_has_the_reference_values():
    import yaml
    import train_pixel_ensemble as cli
    args = cli.parse_args(["cfg.yaml", "--images", "train.json", "--val-images", "val.json", "--class-to-color-map", "map.json",
                           "-l", "out"])
    assert (args.config, args.train_json, args.validation_json, args.class_to_color_map, args.log_dir) == \
        ("cfg.yaml", "train.json", "val.json", "map.json", "out")
    with open(os.path.join(ROOT, "synthesis-in-style_amd", "configs", "pixel_ensemble", "dataset_gan_ensemble.yaml")) as f:
        config = yaml.safe_load(f)
    assert (config["lr"], config["beta1"], config["beta2"], config["weight_decay"], config["num_models"], config["numpy_class"],
            config["batch_size"]) == (5e-4, 0.5, 0.999, 1e-4, 3, 3, 4)


def test_both_lookups_still_refuse_and_name_the_entry_point(tmp_path):
    import train
    from training_builder.train_builder_selection import get_train_builder_class
    from utils.data_loading import get_data_loader
    with pytest.raises(NotImplementedError, match="train_pixel_ensemble.py"):
        get_train_builder_class({"network": "PixelEnsemble"})
    args = train.parse_args(["cfg.yaml", "--images", "train.json", "--class-to-color-map", "map.json"])
    with pytest.raises(NotImplementedError, match="train_pixel_ensemble.py"):
        get_data_loader(tmp_path / "train.json", "dataset_gan", args, {})


def test_aten_loop_reaches_the_end_to_end_marks_and_the_snapshot_loads(tmp_path):
    """The oracle side of the GPU end-to-end test (same dataset, seed and step count, the ATen loop on CPU tensors): the loss
    falls below half its first value and the voted labels of the training pixels are at least 95 % right.  The builder's snapshot
    loads through ``DatasetGANSegmenter.load_ensemble`` with equal weights."""
    from segmentation.dataset_gan_segmenter import DatasetGANSegmenter
    losses, snapshot, dataset, builder, updater = C.e2e_train(str(tmp_path), "cpu", fused=False)
    assert updater.fused_step is None
    assert (losses[-1] < 0.5 * losses[0]).all(), (losses[0], losses[-1])
    checkpoint = torch.load(snapshot, map_location="cpu")
    assert sorted(checkpoint) == ["network_0", "network_1", "network_2", "optimizer_0", "optimizer_1", "optimizer_2"]
    seg = DatasetGANSegmenter.__new__(DatasetGANSegmenter)
    seg.class_to_color_map, seg.image_size = C.COLOURS, C.E2E["size"]
    ensemble = seg.load_ensemble(snapshot, dataset.get_feature_vector_length())
    assert len(ensemble.networks) == 3
    for loaded, trained in zip(ensemble.networks.values(), builder.segmentation_network.get_networks().values()):
        for (k, a), (_, b) in zip(loaded.state_dict().items(), trained.state_dict().items()):
            assert torch.equal(a.cpu(), b.cpu()), k
    ensemble.networks = {k: v.cpu() for k, v in ensemble.networks.items()}
    val = dataset.batch(np.arange(dataset.num_pixels()))
    with torch.no_grad():
        voted = ensemble.predict_classes(dataset.features(val["pixels"]))
    assert (voted.long() == val["label"]).float().mean().item() >= 0.95
