"""The projection encoders' kernels (csrc/encoder_ops.h) against float64 torch restatements, and whole encoders / the
autoencoder against the reference's float64 outputs (tests/golden/encoder32.npz).

Bounds.  Single kernels: the project's per-layer fp32 bound, 2e-5 * max|ref| (tests/test_hip_conv_gpu.py).  Whole networks:
per tensor MULTIPLE = 16 times the error of the reference's own float32 run against its float64 run, and never above
1e-4 * max|ref64| (the project's loosest multi-layer fp32 forward bound).  16 = 4 x 4: the inference path computes its stride-1
3x3 layers by Winograd F(2x2,3x3), whose fp32 error is up to about 4 times a direct convolution's (Barabasz et al., "Error
analysis and improving the accuracy of Winograd convolution for deep neural networks", 2018), and the maximum error over
the few hundred elements of a tensor is itself a statistic that varies by a small factor between two equally accurate
evaluation orders (folded BatchNorm, another summation order).  The measured reference errors are listed in DESIGN.md §13."""
import functools
import json

import numpy as np
import pytest
import torch

import encoder_checks as C

pytestmark = pytest.mark.gpu

MULTIPLE = 16


def _mk(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _fold(gen, c):
    return 0.5 + torch.rand(c, generator=gen), 0.3 * torch.randn(c, generator=gen)


def _rel(got, ref):
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    d = (got.detach().double().cpu() - ref.double()).abs().max().item()
    return (d if d == d else float("inf")) / max(ref.double().abs().max().item(), 1e-30)


# ---------------------------------------------------------------------------------------------------------------- K1
S2_CASES = [(2, 8, 8, 8, 8),        # smallest
            (1, 16, 24, 12, 20),    # non-square, channel and pixel remainders
            (3, 40, 72, 36, 36),    # several K chunks, pixel tiles and channel tiles
            (1, 128, 256, 64, 64)]  # a real layer


@functools.lru_cache(maxsize=None)
def _s2_case(b, cin, cout, h, w):
    gen = torch.Generator().manual_seed(1000 * b + cin + cout + h)
    x, w1, wd = _mk(gen, b, cin, h, w), _mk(gen, cout, cin, 3, 3) / (3 * cin ** 0.5), _mk(gen, cout, cin, 1, 1) / cin ** 0.5
    f1, fd = _fold(gen, cout), _fold(gen, cout)
    return x, w1, wd, f1, fd, C.ref_conv3x3_s2(x, w1, *f1, wd, *fd)


@pytest.mark.parametrize("shortcut", [True, False])
@pytest.mark.parametrize("b,cin,cout,h,w", S2_CASES)
def test_conv3x3_s2(device, b, cin, cout, h, w, shortcut):
    import sis_hip
    x, w1, wd, f1, fd, (ref_main, ref_short) = _s2_case(b, cin, cout, h, w)
    assert sis_hip.enc_conv3x3_s2_supported(cin, cout, h, w)
    d = lambda *ts: [t.to(device) for t in ts]   # noqa: E731
    packed = sis_hip.enc_conv3x3_s2_pack(w1.to(device), wd.to(device) if shortcut else None)
    y, ys = sis_hip.enc_conv3x3_s2(x.to(device), packed, cout, *d(*f1), *(d(*fd) if shortcut else ()))
    assert sis_hip.lib().sis_last_kernel().decode() == "enc_conv3x3_s2_kernel"
    print(f"conv3x3_s2 {(b, cin, cout, h, w)} shortcut={shortcut}: main {_rel(y, ref_main):.2e}" + (f" short {_rel(ys, ref_short):.2e}" if shortcut else ""))
    assert _rel(y, ref_main) < 2e-5
    if shortcut:
        assert _rel(ys, ref_short) < 2e-5
    else:
        assert ys is None


def test_conv3x3_s2_declines_with_a_message(device):
    import sis_hip
    x = torch.zeros(1, 8, 9, 8, device=device)
    packed = sis_hip.enc_conv3x3_s2_pack(torch.zeros(8, 8, 3, 3, device=device))
    one = torch.ones(8, device=device)
    with pytest.raises(RuntimeError, match="not supported"):
        sis_hip.enc_conv3x3_s2(x, packed, 8, one, one)


# ---------------------------------------------------------------------------------------------------------------- K2
@pytest.mark.parametrize("cin", [1, 3])
@pytest.mark.parametrize("h,w", [(8, 12), (32, 32)])
@pytest.mark.parametrize("bias", [True, False])
def test_stem(device, cin, h, w, bias):
    import sis_hip
    b, cout = 2, 40   # two channel groups of 32, the second partial
    gen = torch.Generator().manual_seed(cin * 100 + h)
    x, w1, wd = _mk(gen, b, cin, h, w), _mk(gen, cout, cin, 3, 3) / 3, _mk(gen, cout, cin, 1, 1)
    bd = _mk(gen, cout) if bias else None
    f1, fd = _fold(gen, cout), _fold(gen, cout)
    ref_main, ref_short = C.ref_stem(x, w1, *f1, wd, bd, *fd)
    d = lambda t: None if t is None else t.to(device)   # noqa: E731
    y, ys = sis_hip.enc_stem(d(x), d(w1), d(f1[0]), d(f1[1]), d(wd), d(bd), d(fd[0]), d(fd[1]))
    print(f"stem cin={cin} {h}x{w} bias={bias}: main {_rel(y, ref_main):.2e} short {_rel(ys, ref_short):.2e}")
    assert _rel(y, ref_main) < 2e-5 and _rel(ys, ref_short) < 2e-5


# ---------------------------------------------------------------------------------------------------------------- K3
# (8, 4x4): one channel slice; (40, 12x20): five slices of 8 channels, the noise through its workspace; (6, 20x20): two pixel
# tiles, channels % 4 != 0; (72, 36x36): six pixel tiles x nine slices, the last tile partial
@pytest.mark.parametrize("b,ch,h,w", [(3, 8, 4, 4), (3, 40, 12, 20), (1, 6, 20, 20), (2, 72, 36, 36)])
@pytest.mark.parametrize("noise", [True, False])
@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("residual", [True, False])
def test_block_tail(device, b, ch, h, w, noise, pool, residual):
    import sis_hip
    gen = torch.Generator().manual_seed(b + ch + h)
    c, res = _mk(gen, b, ch, h, w), (_mk(gen, b, ch, h, w) if residual else None)
    scale, shift = _fold(gen, ch)
    nw, nb = (_mk(gen, 1, ch, 1, 1), _mk(gen, 1)) if noise else (None, None)
    ref_y, ref_noise, ref_pool = C.ref_block_tail(c, res, scale, shift, nw, nb)
    d = lambda t: None if t is None else t.to(device)   # noqa: E731
    run = lambda: sis_hip.enc_block_tail(d(c), d(res), d(scale), d(shift), d(nw), d(nb), want_pool=pool)   # noqa: E731
    y, nz, partial = run()
    assert _rel(y, ref_y) < 2e-5
    assert (nz is None) == (not noise) and (partial is None) == (not pool)
    if noise:
        assert tuple(nz.shape) == (b, 1, h, w) and _rel(nz, ref_noise) < 2e-5
    if pool:
        assert tuple(partial.shape) == (b, ch, sis_hip.enc_block_tail_tiles(h * w))
        assert _rel(partial.sum(dim=2) / (h * w), ref_pool) < 2e-5
    y2, nz2, partial2 = run()   # no atomics, fixed order: bit-equal
    assert torch.equal(y, y2) and (not noise or torch.equal(nz, nz2)) and (not pool or torch.equal(partial, partial2))
    # the split of the channels over workgroups does not depend on the batch: a sample alone gives the same bits
    y1, nz1, partial1 = sis_hip.enc_block_tail(d(c[:1]), d(res[:1]) if residual else None, d(scale), d(shift), d(nw), d(nb), want_pool=pool)
    assert torch.equal(y1, y[:1]) and (not noise or torch.equal(nz1, nz[:1])) and (not pool or torch.equal(partial1, partial[:1]))


# ---------------------------------------------------------------------------------------------------------------- K4
@pytest.mark.parametrize("n_heads,channels", [(1, [32]), (4, [8, 24, 40, 24]), (14, [8, 8, 16, 16, 24, 24, 32, 32, 40, 40, 72, 72, 264, 264])])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("sum_heads", [False, True])
def test_latent_heads(device, n_heads, channels, batch, sum_heads):
    import sis_hip
    latent = 48
    gen = torch.Generator().manual_seed(n_heads * 10 + batch)
    hws = [4 * (3 + 70 * (i % 3)) for i in range(n_heads)]   # 12, 292 (two tiles), 572 (three tiles) pixels
    partials = [_mk(gen, batch, c, sis_hip.enc_block_tail_tiles(hw)) for c, hw in zip(channels, hws)]
    weights = [_mk(gen, latent, c, 1, 1) / c ** 0.5 for c in channels]
    biases = [_mk(gen, latent) for _ in channels]
    slots = [n_heads - 1 - i for i in range(n_heads)]
    ref = C.ref_latent_heads([p.double().sum(dim=2) / hw for p, hw in zip(partials, hws)], weights, biases)
    dev = [[t.to(device) for t in ts] for ts in (partials, weights, biases)]
    rows = sorted(zip(dev[0], hws, dev[1], dev[2], slots), key=lambda r: r[4])
    table = sis_hip.enc_heads_table(rows, device)
    assert table.max_channels == max(channels) and table.slots == sorted(slots) and (table.batch, table.latent) == (batch, latent)
    out = sis_hip.enc_latent_heads(table, sum_heads=sum_heads)
    if sum_heads:
        want = torch.stack(ref, dim=1).sum(dim=1)
        assert tuple(out.shape) == (batch, latent)
    else:
        want = torch.stack(ref[::-1], dim=1)   # head i sits in row n - 1 - i
        assert tuple(out.shape) == (batch, n_heads, latent)
    assert _rel(out, want) < 2e-5, _rel(out, want)
    assert torch.equal(out, sis_hip.enc_latent_heads(table, sum_heads=sum_heads))


def test_latent_heads_refuses_rows_it_would_not_write(device):
    import sis_hip
    mk = lambda c, slot: (torch.zeros(2, c, 1, device=device), 16, torch.zeros(48, c, device=device), torch.zeros(48, device=device), slot)   # noqa: E731
    with pytest.raises(RuntimeError, match="do not fit"):
        sis_hip.enc_latent_heads(sis_hip.enc_heads_table([mk(8, 0), mk(8, 2)], device))            # slot 2 of 2 rows
    with pytest.raises(RuntimeError, match="do not fit"):
        sis_hip.enc_latent_heads(sis_hip.enc_heads_table([mk(8, 0), mk(16, 0)], device))           # two heads, one row
    with pytest.raises(RuntimeError, match="do not fit the kernel"):
        sis_hip.enc_latent_heads(sis_hip.enc_heads_table([mk(12280, 0)], device))                  # pool + outputs beyond the LDS budget
    with pytest.raises(RuntimeError, match="partials"):
        sis_hip.enc_heads_table([(torch.zeros(2, 8, 3, device=device), 16, torch.zeros(48, 8, device=device), torch.zeros(48, device=device), 0)], device)


# ---------------------------------------------------------------------------------------- whole encoders, the autoencoder
def _bound(name, ref64, ref32):
    err32 = np.abs(ref32.astype(np.float64) - ref64).max()
    return min(MULTIPLE * err32, 1e-4 * np.abs(ref64).max()), err32


def _check_outputs(what, got, cls):
    want64, want32 = C.named_expected(cls, "_f64"), C.named_expected(cls)
    assert sorted(got) == sorted(want64) and want64
    for name, ref in want64.items():
        bound, err32 = _bound(name, ref, want32[name])
        err = np.abs(got[name].double().cpu().numpy() - ref).max()
        print(f"{what} {cls} {name}: err {err:.3e}, reference float32 err {err32:.3e}, bound {bound:.3e}")
        assert got[name].dtype == torch.float32 and err == err and err <= bound, (cls, name, err, bound)


def _kernels_of(fn):
    import sis_hip
    records = []
    sis_hip.set_profiler(records)
    try:
        out = fn()
    finally:
        sis_hip.set_profiler(None)
    return out, [r[0] for r in records]


CLASSES = ["WPlusEncoder", "WWPlusEncoder", "WEncoder", "WPlusNoNoiseEncoder", "WNoNoiseEncoder", "NoiseEncoder"]


@pytest.mark.parametrize("cls", CLASSES)
def test_encoder_against_the_reference_in_float64(device, cls, monkeypatch):
    import sis_hip
    monkeypatch.delenv("SIS_ENCODER_HIP", raising=False)
    enc = C.build(cls).to(device)
    x = torch.from_numpy(C.fixture()["input"]).to(device)
    sis_hip.library_calls(reset=True)
    with torch.no_grad():
        out, kernels = _kernels_of(lambda: enc(x))
    _check_outputs("hip", C.named_outputs(out), cls)
    # the path ran on the library's kernels: no layer was declined at these shapes
    assert not [k for k in sis_hip.LIBRARY_CALLS if k.startswith("fallback:encoder")], dict(sis_hip.LIBRARY_CALLS)
    assert kernels.count("enc_stem_kernel") == 1 and kernels.count("enc_conv3x3_s2_kernel") == 3 and kernels.count("enc_block_tail_kernel") == 8
    assert kernels.count("enc_latent_heads_kernel") == (0 if cls == "NoiseEncoder" else 1)
    with torch.no_grad():   # cached packs and head tables: the second encode is bit-equal
        again = C.named_outputs(enc(x))
    assert all(torch.equal(again[k], v) for k, v in C.named_outputs(out).items())
    # the switch: the plain ATen formulation, same bound, none of the encoder kernels
    monkeypatch.setenv("SIS_ENCODER_HIP", "0")
    with torch.no_grad():
        plain, kernels = _kernels_of(lambda: enc(x))
    assert not [k for k in kernels if k and k.startswith("enc_")]
    _check_outputs("aten", C.named_outputs(plain), cls)


def test_stride2_dispatch_on_wide_layers(device, monkeypatch):
    """Channels % 32 == 0: the stride-2 layers take the dense-and-subsample route (dispatch by measurement).
    Reference: the same module in float64 on the CPU; bound: the project's multi-layer fp32 forward bound, 1e-4 * max|ref|."""
    import copy
    import networks.encoder.u_net_like_encoder as E
    monkeypatch.delenv("SIS_ENCODER_HIP", raising=False)
    torch.manual_seed(11)
    enc = E.WPlusEncoder(16, 64, 3, {16: 32, 8: 64, 4: 64}, stylegan_variant=2)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
    enc.eval()
    x = torch.rand(3, 3, 16, 16) * 2 - 1
    with torch.no_grad():
        want = C.named_outputs(copy.deepcopy(enc).double()(x.double()))
        got, kernels = _kernels_of(lambda: enc.to(device)(x.to(device)))
    assert kernels.count("enc_conv3x3_s2_kernel") == 0 and kernels.count("enc_block_tail_kernel") == 6
    assert sum("conv1x1_f32" in k for k in kernels) == 2
    for name, ref in want.items():
        assert _rel(C.named_outputs(got)[name], ref) < 1e-4, name


def test_packs_follow_the_parameters(device, monkeypatch):
    monkeypatch.delenv("SIS_ENCODER_HIP", raising=False)
    enc = C.build("WPlusEncoder").to(device)
    x = torch.from_numpy(C.fixture()["input"]).to(device)
    with torch.no_grad():
        before = enc(x)
        enc.resnet_blocks[1].conv1.weight.mul_(0.5)          # a packed stride-2 weight
        enc.resnet_blocks[2].bn2.running_mean.add_(0.25)     # a folded buffer
        after = enc(x)
        monkeypatch.setenv("SIS_ENCODER_HIP", "0")
        plain = enc(x)
    assert not torch.equal(before.latent, after.latent)
    scale = plain.latent.abs().max().item()
    assert (after.latent - plain.latent).abs().max().item() <= 1e-4 * scale


def test_autoencoder_reconstruction(device):
    from networks.encoder.autoencoder import StyleganAutoencoder
    g = C.fixture()
    auto = StyleganAutoencoder(C.build("WPlusEncoder"), C.generator()).to(device).eval()
    with torch.no_grad():
        image = auto(torch.from_numpy(g["input"]).to(device))
    bound, err32 = _bound("image", g["autoencoder/image_f64"], g["autoencoder/image"])
    err = np.abs(image.double().cpu().numpy() - g["autoencoder/image_f64"]).max()
    print(f"autoencoder image: err {err:.3e}, reference float32 err {err32:.3e}, bound {bound:.3e}")
    assert err == err and err <= bound, (err, bound)


def test_generate_images_with_a_dict_batch(device):
    from networks.encoder.autoencoder import StyleganAutoencoder
    from utils.dataset_creation import generate_images
    g = C.fixture()
    auto = StyleganAutoencoder(C.build("WPlusEncoder"), C.generator()).to(device).eval()
    x = torch.from_numpy(g["input"])
    acts, image = generate_images({"input_image": x}, auto, device)
    with torch.no_grad():
        latents = auto.encode(x.to(device))
        want_image, want_acts = auto.decoder([latents.latent], input_is_latent=True, noise=latents.noise, return_intermediate_activations=True)
    assert sorted(acts) == sorted(want_acts) and torch.equal(image, want_image)
    assert all(torch.equal(acts[k], want_acts[k]) for k in acts)
    bound, _ = _bound("image", g["autoencoder/image_f64"], g["autoencoder/image"])
    assert np.abs(image.double().cpu().numpy() - g["autoencoder/image_f64"]).max() <= bound


def test_cli_fits_catalogs_on_images(device, tmp_path):
    import networks
    import create_semantic_segmentation as S
    from PIL import Image
    rng = np.random.RandomState(3)
    names = []
    for i in range(4):
        page = np.full((40, 48, 3), 235, dtype=np.uint8)
        for _ in range(6):   # dark "text lines" on a light page
            y0, x0 = rng.randint(2, 34), rng.randint(2, 20)
            page[y0:y0 + 3, x0:x0 + rng.randint(8, 26)] = rng.randint(0, 80)
        names.append(f"page_{i}.png")
        Image.fromarray(page).save(tmp_path / names[-1])
    with open(tmp_path / "images.json", "w") as f:
        json.dump(names, f)
    torch.manual_seed(5)
    cfg = {"stylegan_variant": 2, "image_size": 32, "latent_size": 32, "input_dim": 3, "n_mlp": 2, "channel_multiplier": 1}
    auto = networks.get_autoencoder(cfg).to(device)
    (tmp_path / "run" / "checkpoints").mkdir(parents=True)
    ckpt = tmp_path / "run" / "checkpoints" / "auto.pt"
    torch.save({"autoencoder": auto.state_dict()}, ckpt)
    common = ["--destination", str(tmp_path / "out"), "-n", "4", "-b", "2", "-c", "3", "5", "-s", "8", "--image-size", "32",
              "--latent-size", "32", "--n-mlp", "2", "--channel-multiplier", "1", "-i", str(tmp_path / "images.json")]
    dest, found = S.main(S.build_parser().parse_args([str(ckpt)] + common))
    assert sorted(found) == [3, 4] and sorted(found[3]) == [4, 5, 6, 7]      # the 16^2 and 32^2 layers (-s 8 drops the smaller ones)
    meta = json.load(open(dest / "catalogs" / "3.json"))
    assert meta["id_to_size_map"] == {"4": "16x16", "5": "16x16", "6": "32x32", "7": "32x32"}
    arrays = np.load(dest / "cluster_arrays" / "3.npz")
    assert arrays["8"].shape == (4, 3, 32, 32) and arrays["8"].dtype == np.uint8   # the reconstructions
    # the activations are those of encode -> decode of the listed images
    x = S.load_image_batch([str(tmp_path / n) for n in names], 32, 3, device)
    assert x.min().item() >= -1 and x.max().item() <= 1 and tuple(x.shape) == (4, 3, 32, 32)
    from utils.dataset_creation import generate_images
    acts, image = generate_images({"input_image": x}, auto.eval(), device)
    import sis_hip
    assert np.array_equal(sis_hip.make_image_u8(image).permute(0, 3, 1, 2).cpu().numpy(), arrays["8"])
    # a generator checkpoint cannot encode
    gen_ckpt = tmp_path / "run" / "checkpoints" / "gen.pt"
    torch.save({"g_ema": auto.decoder.state_dict()}, gen_ckpt)
    with pytest.raises(NotImplementedError, match="'autoencoder' entry"):
        S.main(S.build_parser().parse_args([str(gen_ckpt)] + common))
