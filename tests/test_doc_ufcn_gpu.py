"""DocUFCN on the HIP kernels of csrc/doc_ufcn.hip against float64 torch.nn.functional oracles on the device."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "synthesis-in-style_amd"))

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# every 3x3 layer shape of DocUFCN at 64^2 input (levels 64, 32, 16, 8) plus the config-scale d = H/2 and d >= H cases
CONV_SHAPES = [
    (3, 32, 64, 1), (32, 32, 64, 2), (32, 32, 64, 16), (32, 64, 32, 1), (64, 64, 32, 8), (64, 64, 32, 16),
    (64, 128, 16, 1), (128, 128, 16, 8), (128, 256, 8, 1), (256, 256, 8, 4), (256, 256, 8, 8), (256, 256, 8, 16),
    (256, 128, 8, 1), (256, 64, 16, 1), (128, 32, 32, 1), (64, 3, 64, 1), (256, 256, 32, 16),
]


@pytest.mark.parametrize("cin,cout,size,d", CONV_SHAPES)
def test_dconv3x3_matches_conv2d(cin, cout, size, d):
    import sis_hip
    g = torch.Generator().manual_seed(cin * 1000 + cout + d)
    x = torch.randn(2, cin, size, size, generator=g).to(DEV)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)).to(DEV)
    b = torch.randn(cout, generator=g).to(DEV)
    gy = torch.randn(2, cout, size, size, generator=g).to(DEV)
    xd, wd, bd = (t.double().requires_grad_() for t in (x, w, b))
    ref = F.conv2d(xd, wd, bd, padding=d, dilation=d)
    ref.backward(gy.double())
    y = sis_hip.dconv3x3(x, w, b, d)
    assert _rel(y, ref) < 1e-5
    dx = sis_hip.dconv3x3(gy, sis_hip.dconv3x3_adjoint(w), None, d)
    assert _rel(dx, xd.grad) < 1e-5
    dw = sis_hip.dconv3x3_wgrad(gy, x, d)
    assert _rel(dw, wd.grad) < 1e-5
    assert _rel(sis_hip.channel_sum(gy), bd.grad) < 1e-5
    # deterministic: a second run gives the same bits
    assert torch.equal(dw, sis_hip.dconv3x3_wgrad(gy, x, d))


@pytest.mark.parametrize("batch,cin,cout,size,d", [(8, 64, 64, 112, 1), (8, 32, 32, 160, 4), (2, 64, 64, 10, 2), (3, 16, 8, 9, 1)])
def test_dconv3x3_wgrad_slice_plans(batch, cin, cout, size, d):
    """Weight gradient on shapes whose pixel count does not split evenly into the slice plan (B = 8 at 112^2 used to need
    one slice more than its workspace held) and on maps whose pixel count is not a multiple of the 16-pixel stage."""
    import sis_hip
    g = torch.Generator().manual_seed(batch * size + cin)
    x = torch.randn(batch, cin, size, size, generator=g).to(DEV)
    gy = torch.randn(batch, cout, size, size, generator=g).to(DEV)
    n_ws = int(sis_hip.lib().sis_dconv3x3_wgrad_workspace_floats(batch, cin, cout, size, size, 9))
    assert n_ws > 0
    xd = x.double()
    wd = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, device=DEV, requires_grad=True)
    F.conv2d(xd, wd, padding=d, dilation=d).backward(gy.double())
    dw = sis_hip.dconv3x3_wgrad(gy, x, d)
    assert _rel(dw, wd.grad) < 1e-5
    assert torch.equal(dw, sis_hip.dconv3x3_wgrad(gy, x, d))


@pytest.mark.parametrize("cin,cout,size", [(128, 128, 8), (64, 64, 16), (32, 32, 32)])
def test_conv_transpose_into_concatenation(cin, cout, size):
    from networks.doc_ufcn.doc_ufcn import _ConvT2Fn
    g = torch.Generator().manual_seed(cin + size)
    x = torch.randn(2, cin, size, size, generator=g).to(DEV).requires_grad_()
    w = (torch.randn(cin, cout, 2, 2, generator=g) / cin ** 0.5).to(DEV).requires_grad_()
    b = torch.randn(cout, generator=g).to(DEV).requires_grad_()
    gz = torch.randn(2, cout, 2 * size, 2 * size, generator=g).to(DEV)
    z = _ConvT2Fn.apply(x, w, b)
    z.backward(gz)
    xd, wd, bd = (t.detach().double().requires_grad_() for t in (x, w, b))
    ref = F.conv_transpose2d(xd, wd, bd, stride=2)
    ref.backward(gz.double())
    assert _rel(z, ref) < 1e-5
    for got, want in ((x.grad, xd.grad), (w.grad, wd.grad), (b.grad, bd.grad)):
        assert _rel(got, want) < 1e-5


def _mask_host(seed, site, n, p):
    """numpy restatement of sis_drop_key + sis_drop_quad (csrc/vit_common.h): keep flags of elements 0 .. n-1."""
    M = np.uint64(0xFFFFFFFF)
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    s0 = np.uint64(((s & 0xFFFFFFFF) ^ ((site * 0x632BE5AB) & 0xFFFFFFFF)) & 0xFFFFFFFF)
    s1 = np.uint64(((s >> 32) + site * 0x9E3779B9 + 0x7F4A7C15) & 0xFFFFFFFF)
    q = np.arange(n // 4, dtype=np.uint64)

    def fin(h, a, b, c, m1, m2):
        h = h ^ (h >> np.uint64(a)); h = (h * np.uint64(m1)) & M
        h = h ^ (h >> np.uint64(b)); h = (h * np.uint64(m2)) & M
        return h ^ (h >> np.uint64(c))
    h = fin((q * np.uint64(0x9E3779B1) + s0) & M, 16, 13, 16, 0x85EBCA6B, 0xC2B2AE35)
    h2 = fin((q * np.uint64(0xC2B2AE3D) + s1) & M, 15, 12, 15, 0x2C1B3C6D, 0x297A2D39)
    thr = np.uint64(int(p * 65536.0 + 0.5))
    u = np.stack([h & np.uint64(0xFFFF), h >> np.uint64(16), h2 & np.uint64(0xFFFF), h2 >> np.uint64(16)], axis=1).reshape(-1)
    return u >= thr


def test_bn_relu_dropout_matches_host_masks():
    import sis_hip
    g = torch.Generator().manual_seed(5)
    b, c, h, w, p = 2, 32, 32, 32, 0.4
    z = (torch.randn(b, c, h, w, generator=g) * 2 + 0.3).to(DEV)
    gamma = (torch.rand(c, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(c, generator=g) * 0.1).to(DEV)
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    seed = torch.tensor([0x123456789ABCDEF], dtype=torch.int64, device=DEV)
    site = 0x0D0C0007
    mean, invstd = sis_hip.bn_stats(z, rm, rv, 1e-5, 0.1)
    y, mask = sis_hip.bn_drop_fwd(z, mean, invstd, gamma, beta, seed=seed, site=site, drop_p=p)
    keep = torch.from_numpy(_mask_host(seed.item(), site, z.numel(), p).reshape(z.shape)).to(DEV)
    assert torch.equal(keep, _keep_dev(seed.item(), site, z.shape, p))
    rate = keep.double().mean().item()
    sigma = (0.6 * 0.4 / z.numel()) ** 0.5
    assert abs(rate - 0.6) < 4 * sigma
    scale = 65536.0 / (65536 - int(p * 65536 + 0.5))
    zd = z.double().requires_grad_()
    gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    ref = F.relu(F.batch_norm(zd, None, None, gd, bd, training=True, eps=1e-5)) * keep.double() * scale
    assert _rel(y, ref) < 1e-5
    # running statistics as torch's BatchNorm2d(momentum=0.1) updates them
    assert _rel(rm, 0.1 * z.double().mean((0, 2, 3))) < 1e-5
    gy = torch.randn(b, c, h, w, generator=g).to(DEV)
    ref.backward(gy.double())
    dz, dgamma, dbeta = sis_hip.bn_drop_bwd(gy, z, mean, invstd, gamma, mask, p)
    assert _rel(dz, zd.grad) < 1e-4
    assert _rel(dgamma, gd.grad) < 1e-5 and _rel(dbeta, bd.grad) < 1e-5


def test_weighted_cross_entropy():
    from updater.segmentation_updater import weighted_cross_entropy
    g = torch.Generator().manual_seed(9)
    logits = torch.randn(2, 3, 64, 64, generator=g).to(DEV).requires_grad_()
    labels = torch.randint(0, 3, (2, 64, 64), generator=g).to(DEV)
    wts = torch.tensor([1.0, 2.0, 0.5], device=DEV)
    loss = weighted_cross_entropy(logits, labels, wts)
    loss.backward()
    ld = logits.detach().double().requires_grad_()
    ref = F.cross_entropy(ld, labels, weight=wts.double())
    ref.backward()
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    assert _rel(logits.grad, ld.grad) < 1e-5


def _adam_reference(params, grads_per_step, groups, max_norm):
    ps = [p.detach().double().clone().requires_grad_() for p in params]
    opt = torch.optim.Adam([{'params': [ps[i] for i in idx], **hp} for idx, hp in groups])
    for grads in grads_per_step:
        for p, gr in zip(ps, grads):
            p.grad = gr.double().clone()
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
    return ps


@pytest.mark.parametrize("scale", [0.01, 10.0])   # clipping inactive / active
def test_gradient_clip_adam_device(scale):
    from training.fused_adam import GradientClipAdam
    g = torch.Generator().manual_seed(3)
    shapes = [(64, 32, 3, 3), (64,), (70000,), (3, 64, 3, 3)]
    params = [torch.randn(s, generator=g).to(DEV) for s in shapes]
    groups = [([0, 1], dict(lr=5e-3, betas=(0.5, 0.999), weight_decay=1e-4, eps=1e-8)),
              ([2, 3], dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.0, eps=1e-6))]
    grads = [[torch.randn(s, generator=g).to(DEV) * scale for s in shapes] for _ in range(3)]
    mine = [p.clone().requires_grad_() for p in params]
    opt = GradientClipAdam([{'params': [mine[i] for i in idx], **hp} for idx, hp in groups], max_norm=1.0)
    for step in grads:
        for p, gr in zip(mine, step):
            p.grad = gr.clone()
        opt.step()
    ref = _adam_reference(params, grads, groups, 1.0)
    for a, b in zip(mine, ref):
        assert _rel(a.detach(), b.detach()) < 1e-5


def _net(cls, **kw):
    from networks.doc_ufcn import get_doc_ufcn
    torch.manual_seed(0)
    net = get_doc_ufcn(cls)(3, 3, min_confidence=0.0, min_contour_area=0, **kw)
    with torch.no_grad():   # non-trivial BN affine parameters and running stats
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
    return net


def _keep_dev(seed, site, shape, p):
    """``_mask_host`` on the device (int64 arithmetic; products wrap, the low 32 bits are exact) -> bool tensor of ``shape``."""
    M = 0xFFFFFFFF
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    s0 = ((s & M) ^ ((site * 0x632BE5AB) & M)) & M
    s1 = ((s >> 32) + site * 0x9E3779B9 + 0x7F4A7C15) & M
    n = int(np.prod(shape))
    q = torch.arange(n // 4, dtype=torch.int64, device=DEV)

    def fin(h, a, b, c, m1, m2):
        h = h ^ (h >> a); h = (h * m1) & M
        h = h ^ (h >> b); h = (h * m2) & M
        return h ^ (h >> c)
    h = fin((q * 0x9E3779B1 + s0) & M, 16, 13, 16, 0x85EBCA6B, 0xC2B2AE35)
    h2 = fin((q * 0xC2B2AE3D + s1) & M, 15, 12, 15, 0x2C1B3C6D, 0x297A2D39)
    u = torch.stack([h & 0xFFFF, h >> 16, h2 & 0xFFFF, h2 >> 16], dim=1).reshape(shape)
    return u >= int(p * 65536.0 + 0.5)


def _replay_masks(net, seed):
    """Forward hooks on every nn.Dropout of ``net`` (a copy of the network under test): the output becomes
    input * keep * scale with the keep flags the HIP path drew (seed word of the step, site of the layer's BatchNorm)."""
    for layer in net.modules():
        drop, bn = getattr(layer, 'dropout', None), getattr(layer, 'bn', None)
        if isinstance(drop, torch.nn.Dropout) and drop.p > 0 and bn is not None:
            p, site = drop.p, bn._sis_site
            scale = 65536.0 / (65536 - int(p * 65536 + 0.5))
            drop.register_forward_hook(
                lambda m, inp, out, p=p, site=site, scale=scale: inp[0] * (_keep_dev(seed, site, inp[0].shape, p).to(inp[0].dtype) * scale))


def _step_parity(cls, batch, size, tol_logits=1e-4, median_check=True, **kw):
    """One training step (forward, weighted CE, backward) of the HIP path against float64 torch on the device, and the same
    comparison for the fp32 step on the ROCm libraries (the rounding floor of fp32 for this network)."""
    import sis_hip
    from updater.segmentation_updater import weighted_cross_entropy
    net = _net(cls, **kw)
    ref = copy.deepcopy(net).double().to(DEV).train()
    f32 = copy.deepcopy(net).to(DEV).train()
    net = net.to(DEV).train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(batch, 3, size, size, generator=g).to(DEV)
    labels = torch.randint(0, 3, (batch, size, size), generator=g).to(DEV)
    wts = torch.tensor([1.0, 2.0, 0.5], device=DEV)
    logits = net(x)
    loss = weighted_cross_entropy(logits, labels, wts)
    loss.backward()
    seed = sis_hip.dropout_seed(DEV).item()   # the word this step's masks were drawn from (advanced at the forward's start)
    _replay_masks(ref, seed)
    _replay_masks(f32, seed)
    ref_logits = ref._forward_torch(x.double())
    ref_loss = F.cross_entropy(ref_logits, labels, weight=wts.double())
    ref_loss.backward()
    F.cross_entropy(f32._forward_torch(x), labels, weight=wts).backward()
    assert _rel(logits, ref_logits) < tol_logits
    assert abs(loss.item() - ref_loss.item()) < 1e-5 * abs(ref_loss.item())
    own, lib = [], []
    for (name, p), (_, q), (_, r) in zip(net.named_parameters(), ref.named_parameters(), f32.named_parameters()):
        if name.endswith("conv.bias") and not name.startswith("classifier"):
            # bias in front of a train-mode BatchNorm: its gradient is zero in exact arithmetic (absolute bound)
            assert p.grad.abs().max().item() < 1e-3, name
            continue
        own.append(_rel(p.grad, q.grad))
        lib.append(_rel(r.grad, q.grad))
        # single parameters: a max-pool argmax or ReLU gate that flips under fp32 rounding (either fp32 path, data-dependent)
        # moves one element's gradient by O(1); 3e-2 caps such an outlier
        assert own[-1] < max(3e-2, 8 * lib[-1]), (name, own[-1], lib[-1])
    # systematic precision: the own path's typical error is that of the fp32 library step (each kernel alone is at ~1e-7).
    # Held at the configuration shape.  At B = 2, 64^2 it is not asserted (median_check=False; DESIGN.md §7,
    # profiles/doc_ufcn_small_shape_localisation.txt): of the step's 3 031 040 ReLU gates, up to four in the own step and up to
    # two in the library step fall on the other side of zero than in float64 (pre-activations within fp32 rounding of zero), each
    # turns one element's gradient on or off, and every layer upstream inherits ~1 / sqrt(elements): without dropout medians of
    # 1.0e-2 (own) and 4.5e-3 - 9.0e-3 (library, by machine), in the own step 9.7e-6 once the float64 model's gates are forced on
    # its kernels; with dropout 3e-6 when no gate flips and 2e-3 when one does, by seed word.  Which gates flip differs between two
    # correct fp32 implementations, so 2x the library's median is not a property of the kernels at this shape; they are pinned
    # call by call, on the step's own tensors, by tests/test_doc_ufcn_layouts_gpu.py::test_step_kernels_at_their_in_step_inputs.
    if median_check:
        assert np.median(own) < max(1e-3, 2.0 * np.median(lib)), (np.median(own), np.median(lib))
    for (name, b), (_, c) in zip(net.named_buffers(), ref.named_buffers()):
        if "running" in name:
            assert _rel(b, c) < 1e-5, name
    return net


@pytest.mark.parametrize("cls", ["base", "no_dropout", "pixelshuffle"])
def test_variants_forward_backward_parity(cls):
    kw = dict(encoder_dropout_prob=0.0, decoder_dropout_prob=0.0) if cls != "no_dropout" else {}
    _step_parity(cls, 2, 64, median_check=False, **kw)


def test_dropout_step_parity_small():
    """DocUFCN('base') with its dropout 0.4 at B = 2, 64^2: float64 oracle with the masks regenerated per layer site."""
    _step_parity("base", 2, 64, median_check=False)


def test_config_shape_step_with_dropout():
    """The trained configuration: DocUFCN('base'), dropout 0.4, B = 8, 256^2, against float64 with the regenerated masks."""
    _step_parity("base", 8, 256)


def test_config_shape_step_without_dropout():
    _step_parity("no_dropout", 8, 256)


def test_eval_mode_predict_classes():
    net = _net("no_dropout")
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 2.0)
    ref = copy.deepcopy(net).double().to(DEV).eval()
    net = net.to(DEV).eval()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        got = net.predict_classes(x)
        logits = ref._forward_torch(x.double())
    top2 = logits.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    want = torch.argmax(logits, dim=1, keepdim=True)
    assert torch.equal(got[:, 0][clear], want[:, 0][clear])


def _updater(net, hip_graph, batches):
    from training.fused_adam import GradientClipAdam
    from updater.segmentation_updater import StandardUpdater
    opt = GradientClipAdam(net.parameters(), lr=5e-3, betas=(0.5, 0.999), weight_decay=1e-4)
    return StandardUpdater(iterators={'images': batches}, networks={'segmentation': net}, optimizers={'main': opt},
                           device=DEV, class_weights=[1.0, 2.0, 0.5], hip_graph=hip_graph)


def _batches(n, b=2, size=64):
    g = torch.Generator().manual_seed(11)
    return [{'images': torch.randn(b, 3, size, size, generator=g).to(DEV),
             'segmented': torch.randint(0, 3, (b, 1, size, size), generator=g).to(DEV)} for _ in range(n)]


def test_graph_replay_equals_eager_and_masks_change():
    """Six iterations eager and graphed (two eager warm-ups, a capture, replays) with the LR changed before every iteration:
    bit-identical parameters; the captured step advances the dropout seed word on every replay."""
    import sis_hip
    batches = _batches(4)
    nets = [_net("base").to(DEV).train() for _ in range(2)]
    seed = sis_hip.dropout_seed(DEV)
    start = seed.clone()
    outs, seeds, ups = [], [], []
    for net, graphed in zip(nets, (False, True)):
        seed.copy_(start)
        up = _updater(net, graphed, batches)
        words = []
        for it in range(6):
            up.optimizers['main'].param_groups[0]['lr'] = 5e-3 * (1.0 - 0.1 * it)
            up.update()
            words.append(seed.item())
        torch.cuda.synchronize()
        outs.append([p.detach().clone() for p in net.parameters()])
        seeds.append(words)
        ups.append(up)
    graph = ups[1]._step_graph
    assert graph.graph is not None and graph.capture_error is None, graph.capture_error
    assert ups[0]._step_graph.graph is None
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert seeds[0] == seeds[1]
    assert len(set(seeds[1][3:])) == 3   # every replay drew from a fresh seed word


def test_own_kernels_only_and_no_library_fallback():
    """The kernels of one training step (profiled eagerly: the tracer does not see inside a graph replay, and the captured
    step launches the same kernels)."""
    import sis_hip
    net = _net("base").to(DEV).train()
    up = _updater(net, False, _batches(3))
    up.update()
    torch.cuda.synchronize()
    sis_hip.library_calls(reset=True)
    strict = sis_hip._LIBRARY_STRICT
    sis_hip._LIBRARY_STRICT = True   # as under SIS_NO_LIBRARY_FALLBACK=1: any library fallback raises
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            up.update()
            torch.cuda.synchronize()
    finally:
        sis_hip._LIBRARY_STRICT = strict
    # allow-list: memory copies and sets (the pinned pointer-table / hyper-parameter uploads)
    allow = ("Memcpy", "Memset", "memcpy", "memset")
    names = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    assert any("dconv3x3_kernel" in n for n in names), names
    foreign = {n for n in names if not sis_hip.is_own_kernel(n) and not any(a in n for a in allow)}
    assert not foreign, foreign
    assert not sis_hip.library_calls()["fallback"]


def _free_port():
    import socket
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def _dp_worker(rank, out):
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    import torch.distributed as dist
    from training.grad_exchange import BucketedDataParallel
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1, device_id=DEV)
    try:
        batches = _batches(2)
        bare = _net("no_dropout").to(DEV).train()
        wrapped = BucketedDataParallel(_net("no_dropout").to(DEV).train())
        for net in (bare, wrapped):
            up = _updater(net, False, batches)
            up.update()
            up.update()
        torch.cuda.synchronize()
        out[rank] = max((a - b).abs().max().item() for a, b in zip(bare.parameters(), wrapped.module.parameters()))
    finally:
        dist.destroy_process_group()


def test_data_parallel_world_size_one_equals_bare_step():
    import torch.multiprocessing as mp
    out = mp.Manager().dict()
    mp.spawn(_dp_worker, args=(out,), nprocs=1, join=True)
    assert out[0] < 1e-6, out[0]


def test_step_matches_reference_fixture():
    """The fixture's step (p = 0, B = 2, 64^2) on the HIP path against the unmodified reference's CPU run
    (tests/golden/doc_ufcn_step.npz, tests/golden/make_golden_doc_ufcn.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_doc_ufcn as G
    from networks.doc_ufcn import DocUFCN
    from training.fused_adam import GradientClipAdam
    from updater.segmentation_updater import weighted_cross_entropy
    fx = np.load(os.path.join(ROOT, "tests", "golden", "doc_ufcn_step.npz"))
    net = DocUFCN(3, 3, encoder_dropout_prob=0.0, decoder_dropout_prob=0.0)
    schema = [(k, tuple(t.shape)) for k, t in net.state_dict().items()]
    net.load_state_dict(G.seeded_state_dict(schema), strict=True)
    net = net.to(DEV).train()
    x, y = (t.to(DEV) for t in G.seeded_batch())
    w = torch.tensor(G.CONFIG['class_weights'], device=DEV)
    opt = GradientClipAdam(net.parameters(), lr=G.CONFIG['lr'], betas=G.CONFIG['betas'], weight_decay=G.CONFIG['weight_decay'],
                           max_norm=G.CONFIG['max_norm'])
    # Only the first iteration is compared element by element: Adam's first update maps every gradient element to about +-lr
    # whatever its size, so elements whose gradient is at the fp32 noise level (both runs are fp32) move by lr in either
    # direction and the second forward differs by percents.  The second iteration's loss is compared loosely.
    for it in range(G.CONFIG['iterations']):
        opt.zero_grad()
        logits = net(x)
        if it > 0:
            loss = weighted_cross_entropy(logits, y, w)
            assert abs(loss.item() - fx[f'loss{it}']) <= 0.05 * abs(fx[f'loss{it}'])
            break
        loss = weighted_cross_entropy(logits, y, w)
        loss.backward()
        # the fixture is itself an fp32 run (CPU): the bounds cover two fp32 roundings through 24 train-mode BatchNorms, whose
        # backward amplifies rounding (ReLU gates flip near zero) -- the float64 oracle tests above pin the kernels tighter
        ref = fx[f'logits{it}']
        got = logits.detach().cpu().numpy()
        assert np.linalg.norm(got - ref) <= 1e-4 * np.linalg.norm(ref)
        assert abs(loss.item() - fx[f'loss{it}']) <= 1e-4 * abs(fx[f'loss{it}'])
        norms = np.array([p.grad.norm().item() for p in net.parameters()])
        names = list(fx['param_names'])
        for n, a, b in zip(names, norms, fx[f'grad_norms{it}']):
            if n.endswith("conv.bias") and not n.startswith("classifier"):
                continue   # rounding noise in both runs (bias in front of a train-mode BatchNorm)
            assert abs(a - b) <= 1e-2 * b + 1e-6, n
        opt.step()
        running = torch.cat([b.reshape(-1) for n, b in net.named_buffers() if 'running' in n]).cpu().numpy()
        np.testing.assert_allclose(running, fx[f'running{it}'], rtol=1e-4, atol=1e-5)
