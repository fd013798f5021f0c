"""DatasetGAN labelling, CPU side: reference schema, checkpoint loading, the eval forward and BatchNorm folding against
float64, the reference labels through ``predict_labels(scale_activations(...))``, and the colour table."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_dataset_gan as G  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "dataset_gan.npz")
DIM = sum(c for _, c, _ in G.CONFIG['layers'])
COLOURS = {"background": "#000000", "printed_text": "#0000FF", "handwritten_text": "#FF0000"}


def _checkpoint(tmp_path, n=3, classes=3, dim=DIM):
    ck = {f"network_{i}": G.seeded_member(classes, dim, seed=100 + i) for i in range(n)}
    ck.update({f"optimizer_{i}": {"state": {}, "param_groups": []} for i in range(n)})
    path = tmp_path / "ensemble.pth"
    torch.save(ck, path)
    return path


def _segmenter(tmp_path, size=G.CONFIG['size']):
    from segmentation.dataset_gan_segmenter import DatasetGANSegmenter, dataset_gan_upsamplers
    acts = G.seeded_activations()
    return DatasetGANSegmenter(base_dir=tmp_path, image_size=size, class_to_color_map=COLOURS,
                               classifier_path=str(_checkpoint(tmp_path)), feature_size=DIM,
                               upsamplers=dataset_gan_upsamplers(acts, size)), acts


def test_state_dict_schema_matches_reference():
    from networks.pixel_classifier import PixelClassifier
    gold = np.load(GOLD)
    for tag, classes in (("small", 3), ("large", 34)):
        sd = PixelClassifier(classes, DIM).state_dict()
        assert list(sd) == list(gold[f"keys_{tag}"])
        assert [",".join(map(str, t.shape)) for t in sd.values()] == list(gold[f"shapes_{tag}"])
        assert [(k, tuple(t.shape)) for k, t in sd.items()] == G.member_schema(classes, DIM)


def test_ensemble_naming_and_init():
    from networks.pixel_classifier import PixelClassifier, PixelEnsembleClassifier, ensemble_eval_mode
    torch.manual_seed(0)
    e = PixelEnsembleClassifier(3, 64, 2)
    assert list(e.get_networks()) == ["network_0", "network_1"] and e.last_net_id == 2
    e.add_network(PixelClassifier(3, 64))
    assert list(e.get_networks())[-1] == "network_3"
    m = e.networks["network_0"]
    w, bias = m.layers[0].weight.detach(), m.layers[0].bias.detach()
    assert float(bias.abs().max()) == 0.0 and abs(float(w.std()) - 0.02) < 2e-3
    assert float(m.layers[2].weight.detach().min()) == 1.0   # BatchNorm1d keeps its default init (the BatchNorm2d branch never fires)
    with ensemble_eval_mode(e):
        assert not any(n.training for n in e.networks.values())
    assert all(n.training for n in e.networks.values())


def test_load_ensemble_strict_skips_optimizer(tmp_path):
    seg, _ = _segmenter(tmp_path)
    nets = seg.ensemble.get_networks()
    assert len(nets) == 3 and all(not n.training for n in nets.values())
    for i, n in enumerate(nets.values()):
        ref = G.seeded_member(3, DIM, seed=100 + i)
        for k, v in n.state_dict().items():
            assert torch.equal(v.cpu(), ref[k]), k
    bad = tmp_path / "bad.pth"
    sd = G.seeded_member(3, DIM, seed=1)
    sd.pop("layers.6.bias")
    torch.save({"network_0": sd}, bad)
    with pytest.raises(RuntimeError):
        seg.load_ensemble(str(bad), DIM)


def _fp64_member(sd, x):
    d = {k: v.double() for k, v in sd.items()}

    def bn(h, p):
        return (h - d[p + "running_mean"]) / torch.sqrt(d[p + "running_var"] + 1e-5) * d[p + "weight"] + d[p + "bias"]
    h = bn(torch.relu(x @ d["layers.0.weight"].t() + d["layers.0.bias"]), "layers.2.")
    h = bn(torch.relu(h @ d["layers.3.weight"].t() + d["layers.3.bias"]), "layers.5.")
    return h @ d["layers.6.weight"].t() + d["layers.6.bias"]


@pytest.mark.parametrize("classes", [3, 34])
def test_eval_forward_and_folding_match_fp64(classes):
    from networks.pixel_classifier import PixelEnsembleClassifier, PixelClassifier
    dim = 96
    x = torch.from_numpy(np.random.RandomState(3).randn(500, dim).astype(np.float32))
    e = PixelEnsembleClassifier(classes, dim, 0)
    for i in range(2):
        m = PixelClassifier(classes, dim)
        m.load_state_dict(G.seeded_member(classes, dim, seed=7 + i))
        e.add_network(m.eval())
    fw = e.fused_weights([(64, 8), (32, 16)], 16, "cpu")
    h1 = fw["hidden1"]
    for n, m in enumerate(e.networks.values()):
        ref = _fp64_member(m.state_dict(), x.double())
        with torch.no_grad():
            got = m(x).double()
        assert (got - ref).abs().max() <= 1e-5 * ref.abs().max()
        # the folded weights applied in float64 in the kernels' order: W1 (k-major per group), + b1, ReLU, W2', ReLU, W3'
        assert fw["full"] == [1] and [idx for idx, _ in fw["groups"]] == [[0]]
        w1 = torch.cat([fw["w1f"], fw["groups"][0][1]], 0).double()[:, n * h1:(n + 1) * h1]   # full resolution, then 8
        xg = torch.cat([x[:, 64:], x[:, :64]], 1).double()
        h = torch.relu(xg @ w1 + fw["b1"].double()[n * h1:(n + 1) * h1])
        h = torch.relu(h @ fw["w2t"][n].double() + fw["b2"][n].double())
        z = (h @ fw["w3t"][n].double() + fw["b3"][n].double())[:, :classes]
        assert (z - ref).abs().max() <= 1e-5 * ref.abs().max()
        assert float(fw["w3t"][n][:, classes:].abs().max()) == 0.0


def test_fused_weights_reject_wrong_feature_count():
    from networks.pixel_classifier import PixelEnsembleClassifier, PixelClassifier
    e = PixelEnsembleClassifier(3, 96, 0)
    e.add_network(PixelClassifier(3, 96).eval())
    with pytest.raises(ValueError, match="96 features"):
        e.fused_weights([(64, 8), (64, 16)], 16, "cpu")


def test_predict_labels_reproduces_reference(tmp_path):
    from data.dataset_gan_dataset import scale_activations
    seg, acts = _segmenter(tmp_path)
    seg.ensemble.networks = {k: v.cpu() for k, v in seg.ensemble.networks.items()}
    scaled = scale_activations([acts], seg.upsamplers)[0]
    gold = np.load(GOLD)
    with torch.no_grad():
        logits = np.stack([m(scaled.reshape(-1, DIM)).numpy() for m in seg.ensemble.networks.values()])
    assert np.abs(logits - gold["logits"]).max() <= 1e-4 * np.abs(gold["logits"]).max()
    labels = seg.predict_labels(scaled).numpy()
    top2 = np.sort(gold["logits"], axis=2)
    clear = ((top2[..., -1] - top2[..., -2]) > 1e-3).all(0).reshape(labels.shape)
    assert clear.mean() > 0.9
    assert np.array_equal(labels[clear], gold["labels"][clear])


def test_cpu_mode_tie_rule_matches_fixture():
    gold = np.load(GOLD)
    rows3, rows4 = G.tie_rows()
    assert np.array_equal(torch.mode(torch.from_numpy(rows3)).values.numpy(), gold["mode_cpu3"])
    assert np.array_equal(torch.mode(torch.from_numpy(rows4)).values.numpy(), gold["mode_cpu4"])


def test_colour_table_and_reference_colouring(tmp_path):
    from PIL import ImageColor
    seg, _ = _segmenter(tmp_path)
    table = seg.colour_table()
    assert table.dtype == np.uint8 and table.tolist() == [list(ImageColor.getrgb(c)) for c in COLOURS.values()]
    assert seg.class_id_map == {"background": 0, "printed_text": 1, "handwritten_text": 2}
    lab = torch.from_numpy(np.random.RandomState(0).randint(0, 3, (2, 1, 8, 8)))
    assert np.array_equal(seg.label_images_to_color_images(lab), table[lab[:, 0].numpy()])


def test_upsampler_mode_and_count(tmp_path):
    seg, acts = _segmenter(tmp_path)
    seg.upsamplers = [torch.nn.Upsample(scale_factor=u.scale_factor, mode='nearest') for u in seg.upsamplers]
    with pytest.raises(NotImplementedError):
        seg.predict_labels_from_activations(acts)
    seg.upsamplers = seg.upsamplers[:-1]
    with pytest.raises(ValueError):
        seg.predict_labels_from_activations(acts)


def test_pixel_ensemble_builder_stays_out_of_scope():
    from training_builder.train_builder_selection import get_train_builder_class
    with pytest.raises(NotImplementedError):
        get_train_builder_class({'network': 'PixelEnsemble'})


def test_kernels_are_own_and_exported():
    import sis_hip
    assert {"pe_project_kernel", "pe_head_kernel"} <= sis_hip.own_kernel_names()
    assert sis_hip.is_own_kernel("void (anonymous namespace)::pe_head_kernel<128, 32, 32>((anonymous namespace)::PeHeadParams)")
    assert {"sis_pixel_ensemble_project", "sis_pixel_ensemble_head"} <= set(sis_hip.exported_symbols())
