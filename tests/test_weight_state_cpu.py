"""Host half of the weight-state family (tests/weight_state_checks.py): with the pack functions of ``sis_hip`` replaced by stubs
that return clones and count their calls, every image a ``ModulatedConv2d`` keeps, the generator's modulation plan, the encoder's
packs and the bf16 shadow copies are rebuilt after every way this project writes weights -- and by nothing else.

A stub's "image" is a clone of the weight, so "the image belongs to the weights as they are now" is ``torch.equal(image, weight)``.
``FusedSGD`` has no host path and is in the device file only; ``GradientClipAdam`` takes its plain torch path here."""
import collections

import pytest
import torch

import weight_state_checks as W

IMAGES = ("pack", "wino", "wino24", "bf16", "fir")


@pytest.fixture
def stubs(monkeypatch):
    """Counter of pack calls by kind; ``stubs.route`` chooses what the two eligibility predicates answer."""
    import sis_hip
    calls = collections.Counter()
    calls.route = {"wino24": False, "bf16": False}

    def clone_as(kind):
        def stub(weight, *more, **kw):
            calls[kind] += 1
            return weight.detach().clone()
        return stub

    def prepack(weight):
        calls["pack"] += 1
        return weight.detach().clone(), weight.detach().clone()

    def s2_pack(weight, shortcut_weight=None):
        calls["s2"] += 1
        return weight.detach().clone(), None if shortcut_weight is None else shortcut_weight.detach().clone()

    real_fold = calls.real_fold = sis_hip.fold_batch_norm

    def fold(bn, conv_bias=None):
        calls["fold"] += 1
        return real_fold(bn, conv_bias)   # plain torch: runs on the host

    for name in ("SIS_WINOGRAD", "SIS_WINO24", "SIS_GEN_PRECISION"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(sis_hip, "modconv_prepack", prepack)
    monkeypatch.setattr(sis_hip, "modconv_prepack_wino", clone_as("wino"))
    monkeypatch.setattr(sis_hip, "modconv_prepack_wino24", clone_as("wino24"))
    monkeypatch.setattr(sis_hip, "modconv_prepack_bf16", clone_as("bf16"))
    monkeypatch.setattr(sis_hip, "modconv_prepack_up_fir", clone_as("fir"))
    monkeypatch.setattr(sis_hip, "modconv_wino24_eligible", lambda *a: calls.route["wino24"])
    monkeypatch.setattr(sis_hip, "modconv_bf16_eligible", lambda *a: calls.route["bf16"])
    monkeypatch.setattr(sis_hip, "fold_batch_norm", fold)
    monkeypatch.setattr(sis_hip, "conv3x3_prepack", clone_as("conv3x3"))
    monkeypatch.setattr(sis_hip, "enc_conv3x3_s2_pack", s2_pack)
    return calls


def _layer(image, seed):
    from networks.stylegan2.model import ModulatedConv2d
    if image == "fir":   # the fast-FIR image: an up-convolution with Cin % 8 == 0 and Cout % 64 == 0
        layer = W.seeded(lambda: ModulatedConv2d(8, 64, 3, 16, upsample=True), seed)
    else:
        layer = W.seeded(lambda: ModulatedConv2d(8, 8, 3, 16), seed)
    if image == "bf16":
        layer.set_matrix_precision("bf16")
    return layer


def _use(layer, image, stubs):
    """The image as the fused path asks for it."""
    stubs.route.update(wino24=image == "wino24", bf16=image == "bf16")
    if image == "pack":
        return layer.packed_weights()[0]
    if image == "fir":
        return layer.fir_weights()
    assert layer.route(32, 32) == image
    operand = layer.winograd_operand(32, 32)
    assert list(operand) == [{"wino": "wino_u", "wino24": "wino24_u", "bf16": "bf16_w"}[image]], operand
    return operand[list(operand)[0]]


@pytest.mark.parametrize("image", IMAGES)
@pytest.mark.parametrize("name", W.HOST_WRITERS)
def test_every_image_follows_every_writer(stubs, name, image):
    layer, other = _layer(image, 1), _layer(image, 2)
    first = _use(layer, image, stubs)
    assert first is not None and torch.equal(first, layer.weight) and stubs[image] == 1 and stubs["pack"] == 1
    old = layer.weight.detach().clone()
    W.writer(name)(layer, other)
    assert not torch.equal(old, layer.weight)
    again = _use(layer, image, stubs)
    assert again is not None and torch.equal(again, layer.weight), f"the {image} image is the one of the weights before {name}"
    wpk, wsq = layer.packed_weights()
    assert torch.equal(wpk, layer.weight) and torch.equal(wsq, layer.weight)
    assert stubs[image] == 2 and stubs["pack"] == 2
    for _ in range(3):   # and nothing is rebuilt without a write
        assert _use(layer, image, stubs) is again
    assert stubs[image] == 2 and stubs["pack"] == 2


@pytest.mark.parametrize("image", IMAGES)
def test_no_write_means_no_repack(stubs, image):
    layer = _layer(image, 3)
    uses = [_use(layer, image, stubs) for _ in range(3)]
    assert uses[0] is uses[1] is uses[2] and stubs[image] == 1 and stubs["pack"] == 1
    assert sum(stubs.values()) == (1 if image == "pack" else 2)


@pytest.mark.parametrize("name", W.HOST_WRITERS)
def test_forward_follows_every_writer(stubs, name):
    """``assert_follows`` on the host formulation: the pack a forward would use next to the layer's output.  Also what shows, without
    a device, that each writer and seed moves the result (the sensitivity step)."""
    gen = torch.Generator().manual_seed(5)
    x, style = torch.randn(2, 8, 6, 6, generator=gen), torch.randn(2, 16, generator=gen)

    def run(layer):   # grad enabled: under no_grad the modulation would go to its kernel, which needs a device
        wpk, wsq = layer.packed_weights()
        return {"wpk": wpk, "wsq": wsq, "out": layer._forward_autograd(x, style).detach()}

    W.assert_follows(run, _layer("pack", 1), W.writer(name), _layer("pack", 2), builds=lambda: sum(stubs.values()))


def _small_generator(seed):
    from networks.stylegan2.model import Generator
    return W.seeded(lambda: Generator(8, 16, 1, channel_multiplier=1), seed)


def _plan_points_into_the_packs(g):
    from networks.stylegan2.model import StyledConv
    plan = g._modulation_plan(2, torch.device("cpu"))
    styled = [m.conv for m, _ in g._layer_sequence() if isinstance(m, StyledConv)]
    assert plan["n_dem"] == len(styled) == 3
    assert plan["dem"][:, 0].tolist() == [conv.packed_weights()[1].data_ptr() for conv in styled]
    assert plan["mod"][:, 0].tolist() == [m.conv.modulation.weight.data_ptr() for m, _ in g._layer_sequence()]
    for conv in styled:
        assert torch.equal(conv.packed_weights()[1], conv.weight), "wsq is the one of the weights before the write"
    return plan


@pytest.mark.parametrize("name", W.HOST_WRITERS)
def test_modulation_plan_points_into_the_current_packs(stubs, name):
    g, other = _small_generator(1), _small_generator(2)
    plan = _plan_points_into_the_packs(g)
    assert g._modulation_plan(2, torch.device("cpu")) is plan and stubs["pack"] == 3
    held = [g.conv1.conv.packed_weights()[1]] + [m.conv.packed_weights()[1] for m in g.convs]   # alive: their addresses cannot come back
    W.writer(name)(g, other)
    after = _plan_points_into_the_packs(g)
    assert after is not plan and stubs["pack"] == 6 and len(held) == 3
    assert g._modulation_plan(2, torch.device("cpu")) is after and stubs["pack"] == 6


def test_set_matrix_precision_keeps_the_fp32_operands(stubs):
    """The layer's documented behaviour: the fp32 operands (wpk, wsq) stay, the bf16 image is dropped, so that a plan that holds
    their addresses stays valid; the generator's call drops the packs and its plan with them."""
    layer = _layer("bf16", 1)
    image = _use(layer, "bf16", stubs)
    pack = layer.packed_weights()
    layer.set_matrix_precision("fp32")
    assert layer.packed_weights() is pack and "bf16" not in layer._images and stubs["pack"] == 1
    stubs.route.update(bf16=True)
    assert not layer.bf16_takes(32, 32) and "bf16_w" not in layer.winograd_operand(32, 32)
    layer.set_matrix_precision("bf16")
    assert layer.packed_weights() is pack and _use(layer, "bf16", stubs) is not image and stubs["bf16"] == 2 and stubs["pack"] == 1
    g = _small_generator(1)
    plan = _plan_points_into_the_packs(g)
    g.set_matrix_precision("bf16")
    assert _plan_points_into_the_packs(g) is not plan and stubs["pack"] == 1 + 6
    with pytest.raises(ValueError):
        g.set_matrix_precision("fp16")


def test_bf16_shadow_follows_version_and_raw_counter():
    """Existing behaviour of the TransUNet shadow copies, pinned on the shared stamp: a write autograd sees, a fused optimizer's
    counter bump (``sis_hip.mark_written``), and no refresh without either."""
    import sis_hip
    from networks.trans_u_net.vit_encoder import _Bf16Shadow
    gen = torch.Generator().manual_seed(0)
    a, b = torch.nn.Parameter(torch.randn(4, 3, generator=gen)), torch.nn.Parameter(torch.randn(2, 3, generator=gen))
    shadow = _Bf16Shadow([a, b])
    want = lambda: torch.cat([a.detach(), b.detach()]).bfloat16()   # noqa: E731
    assert torch.equal(shadow.tensor(), want())
    key = shadow.key
    assert shadow.tensor() is shadow.buf and shadow.key == key
    with torch.no_grad():
        a.mul_(3.0)
    assert torch.equal(shadow.tensor(), want()) and shadow.key != key
    b.detach().numpy()[:] *= -2.0   # a kernel-style write: ``_version`` stays
    stale = shadow.key
    sis_hip.mark_written(b)
    assert sis_hip.weight_stamp(b)[2] == 1 and sis_hip.weight_stamp(b, raw=False)[2] == 0
    assert torch.equal(shadow.tensor(), want()) and shadow.key != stale
    from training.fused_adam import GradientClipAdam   # the optimizer's own bump is this mark (host path: ``_version`` moves instead)
    a.grad, b.grad = torch.ones_like(a), torch.ones_like(b)
    GradientClipAdam([a, b], lr=0.5).step()
    assert torch.equal(shadow.tensor(), want())


def test_mark_written_takes_tensors_modules_and_iterables():
    import sis_hip
    lin, p = torch.nn.BatchNorm1d(3), torch.nn.Parameter(torch.zeros(2))
    before = [sis_hip.weight_stamp(t) for t in list(lin.parameters()) + list(lin.buffers()) + [p]]
    sis_hip.mark_written(lin, [p])
    after = [sis_hip.weight_stamp(t) for t in list(lin.parameters()) + list(lin.buffers()) + [p]]
    assert all(x[:2] == y[:2] and y[2] == x[2] + 1 for x, y in zip(before, after))


# ---------------------------------------------------------------------------------------------------------------- the encoder
ENCODER = (32, 32, 3, {32: 8, 16: 16, 8: 24, 4: 32})   # the smallest map the encoder's tests use (tests/golden/make_golden_encoder.py)


def _encoder(seed):
    from networks.encoder.u_net_like_encoder import WPlusEncoder
    enc = W.seeded(lambda: WPlusEncoder(*ENCODER, stylegan_variant=2), seed)
    with torch.no_grad():
        gen = torch.Generator().manual_seed(seed)
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.3 * torch.randn(m.running_mean.shape, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))
    return enc.eval()


def _packs_are_current(enc, real_fold):
    """``_packs()`` (the whole of what the inference path derives from the tensors, reachable without a device) against the live
    tensors; the stride-2 images are built at first use, so they are asked for as the forward does."""
    state = enc._packs()
    for block, p in zip(enc._blocks(), state["packs"]):
        for fold, bn in ((p["bn1"], block.bn1), (p["bn2"], block.bn2)):
            assert all(torch.equal(a, b) for a, b in zip(fold, real_fold(bn)))
        assert torch.equal(p["invstd1"], torch.rsqrt(block.bn1.running_var + block.bn1.eps))
        assert torch.equal(p["u2"], block.conv2.weight)
        if block.stride == 1 and block.conv1.in_channels % 8 == 0:
            assert torch.equal(p["u1"], block.conv1.weight)
        if block.stride == 2:
            assert torch.equal(enc._stride2_image(block, p, "u1"), block.conv1.weight)
            s2 = enc._stride2_image(block, p, "s2")
            assert torch.equal(s2[0], block.conv1.weight) and torch.equal(s2[1], block.downsample[0].weight)
            assert all(torch.equal(a, b) for a, b in zip(p["bnd"], real_fold(block.downsample[1], block.downsample[0].bias)))
    return state


@pytest.mark.parametrize("name", W.HOST_WRITERS + ["running_statistics"])
def test_encoder_packs_follow_every_writer(stubs, name):
    enc, other = _encoder(1), _encoder(2)
    state = _packs_are_current(enc, stubs.real_fold)
    built = sum(stubs.values())
    assert enc._packs() is state and _packs_are_current(enc, stubs.real_fold) is state and sum(stubs.values()) == built
    if name == "running_statistics":   # buffers: a train-mode forward moves them (a control: ``_version`` sees it)
        enc.train()
        enc._forward_aten(torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(3)))
        enc.eval()
    else:
        W.writer(name)(enc, other)
    after = _packs_are_current(enc, stubs.real_fold)
    assert after is not state and sum(stubs.values()) == 2 * built
    assert _packs_are_current(enc, stubs.real_fold) is after and sum(stubs.values()) == 2 * built
