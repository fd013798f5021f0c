"""DatasetGAN labelling on the device (csrc/pixel_ensemble.hip): member logits against a float64 oracle of the reference
order (upsample, concatenate, Linear, ReLU, BatchNorm, ...), the reference fixture, the vote's tie rule against torch.mode on
the device, bit-identity across calls / batch compositions / streams, peak memory, the dataset loop end to end, errors."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_dataset_gan as G  # noqa: E402

pytestmark = pytest.mark.gpu
COLOURS = {"background": "#000000", "printed_text": "#0000FF", "handwritten_text": "#FF0000"}
# Generator(256, channel_multiplier=2): (key, channels, resolution); F = 10 * 512 + 2 * 256 + 2 * 128 = 5888
GEN256 = tuple((k, c, r) for k, (c, r) in enumerate([(512, 4)] * 2 + [(512, 8)] * 2 + [(512, 16)] * 2 + [(512, 32)] * 2 +
                                                      [(512, 64)] * 2 + [(256, 128)] * 2 + [(128, 256)] * 2))
# a dict without a full-resolution layer (SWAGAN-like: the image is one inverse wavelet step above the last activation)
TOP4 = ((0, 256, 128), (1, 256, 128), (2, 128, 256), (3, 128, 256))
NOFULL = tuple((k, c, r) for k, (c, r) in enumerate([(512, 4)] * 2 + [(512, 8)] * 2 + [(256, 16)] * 2 + [(128, 32)] * 2))


def _segmenter(tmp_path, layers, size, members, classes, seed=100, colours=None):
    from segmentation.dataset_gan_segmenter import DatasetGANSegmenter
    dim = sum(c for _, c, _ in layers)
    colours = colours or {f"c{i}": f"#{(37 * i) % 256:02x}{(91 * i) % 256:02x}{(53 * i) % 256:02x}" for i in range(classes)}
    path = tmp_path / f"ens_{members}_{classes}_{seed}.pth"
    torch.save({f"network_{i}": G.seeded_member(classes, dim, seed=seed + i) for i in range(members)}, path)
    ups = [torch.nn.Upsample(scale_factor=size / r, mode='bilinear') for _, _, r in layers]
    return DatasetGANSegmenter(base_dir=tmp_path, image_size=size, class_to_color_map=colours, classifier_path=str(path),
                               feature_size=dim, upsamplers=ups)


def _acts(layers, batch, device, seed=11):
    g = torch.Generator(device=device).manual_seed(seed)
    return {k: torch.randn(batch, c, r, r, device=device, generator=g) for k, c, r in layers}


def _fp64_logits(seg, acts, size):
    """Reference order in float64: bilinear upsampling of every layer, concatenation, then each member's layers."""
    out = []
    for b in range(next(iter(acts.values())).shape[0]):
        feats = torch.cat([F.interpolate(a[b:b + 1].double(), scale_factor=size // a.shape[-1], mode='bilinear',
                                         align_corners=False) for a in acts.values()], 1)
        x = feats[0].reshape(feats.shape[1], -1).t()
        per = []
        for m in seg.ensemble.networks.values():
            d = {k: v.double() for k, v in m.state_dict().items()}

            def bn(h, p):
                return (h - d[p + "running_mean"]) / torch.sqrt(d[p + "running_var"] + 1e-5) * d[p + "weight"] + d[p + "bias"]
            h = bn(torch.relu(x @ d["layers.0.weight"].t() + d["layers.0.bias"]), "layers.2.")
            h = bn(torch.relu(h @ d["layers.3.weight"].t() + d["layers.3.bias"]), "layers.5.")
            per.append(h @ d["layers.6.weight"].t() + d["layers.6.bias"])
        out.append(torch.stack(per))
    return torch.stack(out, 1)   # [N, B, P, C]


def _check_against(logits, labels, ref, ref_labels=None):
    """Member logits within eps = 1e-4 max|logit| of the float64 oracle; labels equal wherever every member's top-2 gap
    exceeds 2 eps.  -> measured relative error."""
    n, b, p, c = ref.shape
    got = logits.reshape(n, b, p, c).double()
    eps = 1e-4 * ref.abs().max()
    err = (got - ref).abs().max()
    assert err <= eps, f"logit error {err / ref.abs().max():.3e} of max|logit|"
    top2 = ref.topk(2, dim=3).values
    clear = ((top2[..., 0] - top2[..., 1]) > 2 * eps).all(0)                       # [B, P]
    member = ref.argmax(3)                                                           # [N, B, P]
    want = torch.mode(member.permute(1, 2, 0).float(), dim=2).values.long() if ref_labels is None else ref_labels
    assert clear.float().mean() > 0.9
    assert torch.equal(labels.reshape(b, p)[clear], want.reshape(b, p)[clear])
    return float(err / ref.abs().max())


@pytest.mark.parametrize("layers,size,members,classes", [(GEN256, 256, 1, 3), (GEN256, 256, 3, 3), (GEN256, 256, 10, 3),
                                                         (GEN256, 256, 3, 34), (NOFULL, 64, 3, 3)])
def test_logits_and_labels_match_fp64(device, tmp_path, layers, size, members, classes):
    seg = _segmenter(tmp_path, layers, size, members, classes)
    acts = _acts(layers, 2, device)
    labels, rgb, logits = seg.label_activations(acts, want_logits=True)
    torch.cuda.synchronize()
    assert labels.dtype == torch.int64 and labels.shape == (2, size, size)
    err = _check_against(logits, labels, _fp64_logits(seg, acts, size))
    assert torch.equal(rgb, torch.from_numpy(seg.colour_table()).to(device)[labels])
    print(f"[dataset_gan] {len(layers)} layers -> {size}^2, N={members}, C={classes}: logit error {err:.2e} of max|logit|")


def test_reference_fixture(device, tmp_path):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "dataset_gan.npz"))
    cfg = G.CONFIG
    seg = _segmenter(tmp_path, cfg['layers'], cfg['size'], cfg['members'], cfg['classes'], colours=COLOURS)
    acts = {k: v.to(device) for k, v in G.seeded_activations().items()}
    labels, _, logits = seg.label_activations(acts, want_logits=True)
    ref = torch.from_numpy(gold["logits"]).double().to(device).reshape(cfg['members'], cfg['batch'], -1, cfg['classes'])
    _check_against(logits, labels, ref, torch.from_numpy(gold["labels"]).long().to(device))
    assert torch.equal(seg.predict_labels_from_activations(acts), labels)


def _constant_member(classes, dim, label):
    """A member whose logits are its last bias alone: every pixel gets ``label``."""
    sd = {k: torch.zeros(s) if not k.endswith("num_batches_tracked") else torch.tensor(0)
          for k, s in G.member_schema(classes, dim)}
    sd["layers.2.running_var"] = torch.ones_like(sd["layers.2.running_var"])
    sd["layers.5.running_var"] = torch.ones_like(sd["layers.5.running_var"])
    sd["layers.6.bias"][label] = 1.0
    return sd


def test_vote_ties_follow_device_torch_mode(device, tmp_path):
    from segmentation.dataset_gan_segmenter import DatasetGANSegmenter
    layers = ((0, 32, 8), (1, 32, 16))
    acts = _acts(layers, 1, device)
    rows3, rows4 = G.tie_rows()
    rng = np.random.RandomState(4)   # ties among up to ten members: the device's rule is neither the smallest nor the largest
    extra = [[0, 2, 2, 2, 1, 0, 1, 1, 1, 2]] + [list(rng.randint(0, 3, n)) for n in (5, 6, 7, 8, 9, 10, 10, 10, 10)]
    for row in list(rows3) + list(rows4) + extra:
        path = tmp_path / "tie.pth"
        torch.save({f"network_{i}": _constant_member(5, 64, int(v)) for i, v in enumerate(row)}, path)
        seg = DatasetGANSegmenter(base_dir=tmp_path, image_size=16, class_to_color_map={f"c{i}": "#000000" for i in range(5)},
                                  classifier_path=str(path), feature_size=64,
                                  upsamplers=[torch.nn.Upsample(scale_factor=16 / r, mode='bilinear') for _, _, r in layers])
        got = seg.predict_labels_from_activations(acts)
        want = torch.mode(torch.tensor(row, device=device).reshape(1, -1).repeat(256, 1)).values.long()
        assert torch.equal(got.reshape(-1), want), (row, got.reshape(-1)[0].item(), want[0].item())


def test_bit_identity_batches_and_streams(device, tmp_path, monkeypatch):
    from utils.dataset_creation import label_and_encode
    seg = _segmenter(tmp_path, GEN256, 256, 3, 3)
    acts = _acts(GEN256, 8, device)
    l8 = seg.predict_labels_from_activations(acts)
    assert torch.equal(l8, seg.predict_labels_from_activations(acts))
    l4 = seg.predict_labels_from_activations({k: v[3:7].contiguous() for k, v in acts.items()})
    assert torch.equal(l8[3:7], l4)
    for i in range(3, 7):
        assert torch.equal(l8[i:i + 1], seg.predict_labels_from_activations({k: v[i:i + 1].contiguous() for k, v in acts.items()}))
    image = torch.rand(8, 3, 256, 256, device=device) * 2 - 1
    monkeypatch.setenv("SIS_LABEL_STREAM", "0")
    _, same, _ = label_and_encode(image, acts, {}, seg)
    monkeypatch.setenv("SIS_LABEL_STREAM", "1")
    _, side, ready = label_and_encode(image, acts, {}, seg)
    ready.synchronize()
    assert torch.equal(same["dataset_gan"], side["dataset_gan"])


def test_peak_memory(device, tmp_path):
    seg = _segmenter(tmp_path, GEN256, 256, 3, 3)
    acts = _acts(GEN256, 8, device)
    seg.predict_labels_from_activations(acts)   # weights packed and cached
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    seg.predict_labels_from_activations(acts)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 400e6


def test_dataset_loop_end_to_end(device, tmp_path):
    from PIL import Image
    import create_dataset_for_segmentation as cds
    from networks import get_stylegan2_generator
    from segmentation.dataset_gan_segmenter import DatasetGANSegmenter
    torch.manual_seed(0)
    g = get_stylegan2_generator(32, 512, n_mlp=2)
    ckpt = tmp_path / "g.pt"
    torch.save({"g_ema": g.state_dict()}, ckpt)
    dim = 512 * 8
    ens = tmp_path / "ens.pth"
    torch.save({**{f"network_{i}": G.seeded_member(3, dim, seed=40 + i) for i in range(3)},
                **{f"optimizer_{i}": {} for i in range(3)}}, ens)
    cfg = {"image_size": 32, "latent_size": 512, "n_mlp": 2, "seed": 3, "segmenter_type": "dataset_gan",
           "class_to_color_map": COLOURS}
    args = argparse.Namespace(checkpoint=str(ckpt), config=None, num_images=7, save_to=str(tmp_path / "out"), batch_size=3,
                              truncate=False, classifier_path=str(ens))
    assert cds.build_dataset(args, cfg, rank=0, world_size=2)[1] == (0, 4)
    assert cds.build_dataset(args, cfg, rank=1, world_size=2)[1] == (4, 7)
    single = argparse.Namespace(**{**vars(args), "save_to": str(tmp_path / "single")})
    assert cds.build_dataset(single, cfg, rank=0, world_size=1) == (7, (0, 7))
    files = sorted((tmp_path / "out").rglob("*.png"))
    assert len(files) == 7
    for f in files:
        twin = tmp_path / "single" / f.relative_to(tmp_path / "out")
        assert np.array_equal(np.asarray(Image.open(f)), np.asarray(Image.open(twin))), f.name
    # the label halves: only the map's colours, equal to the colour rendering of the fused labels of the same batch
    g = cds.load_generator(str(ckpt), 32, 512, 2, 2, device)
    seg = cds.dataset_gan_segmenter(g, str(ens), cfg, None, device)
    assert isinstance(seg, DatasetGANSegmenter) and len(seg.upsamplers) == 8
    torch.random.manual_seed(3)
    from utils.dataset_creation import seeded_latents
    with torch.no_grad():
        z = seeded_latents(3, 512, device)
        _, acts = g([z.to(device)], noise=g.make_noise(), return_intermediate_activations=True)
    colours = seg.colour_table()[seg.predict_labels_from_activations(acts).cpu().numpy()]
    table = {tuple(c) for c in seg.colour_table().tolist()}
    for i in range(3):
        im = np.asarray(Image.open(tmp_path / "single" / "0" / "0" / f"{i:04d}.png"))
        assert {tuple(p) for p in im[:, 32:].reshape(-1, 3).tolist()} <= table
        assert np.array_equal(im[:, 32:], colours[i])


def test_errors(device, tmp_path):
    seg = _segmenter(tmp_path, TOP4, 256, 3, 3)
    acts = _acts(TOP4, 1, device)
    seg.predict_labels_from_activations(acts)
    bad = dict(acts)
    bad[0] = torch.randn(1, 256, 48, 48, device=device)            # not a power-of-two fraction of 256
    with pytest.raises(ValueError):
        seg.predict_labels_from_activations(bad)
    with pytest.raises(ValueError):                                   # F of the ensemble != the activations' channels
        seg.predict_labels_from_activations({**acts, 0: torch.randn(1, 128, 128, 128, device=device)})
    odd = _segmenter(tmp_path, ((0, 48, 8), (1, 48, 16)), 16, 2, 3)   # channel counts the tiles do not take
    with pytest.raises(RuntimeError):
        odd.predict_labels_from_activations(_acts(((0, 48, 8), (1, 48, 16)), 1, device))
    many = _segmenter(tmp_path, TOP4, 256, 11, 3)              # 11 members
    with pytest.raises(RuntimeError):
        many.predict_labels_from_activations(acts)
    wide = _segmenter(tmp_path, TOP4, 256, 2, 65)              # 65 classes
    with pytest.raises(RuntimeError):
        wide.predict_labels_from_activations(acts)
    with pytest.raises(RuntimeError):
        seg.label_activations({k: v.cpu() for k, v in acts.items()})
