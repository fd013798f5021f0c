"""Shared by tests/test_weight_state_cpu.py and tests/test_weight_state_gpu.py: does state derived from the weights (packed
weight images, the modulation plan, the encoder's folded BatchNorms) follow every way this project writes weights?

Three pieces (torch only, no fixtures):

* ``WRITERS``: name -> function ``(module, other)`` that changes ``module``'s parameters in place, given a second, differently
  seeded module of the same shape.  The project's own invisible writers (the weight average through a real
  ``Stylegan2Updater``, the fused optimizers, whose device steps write from a kernel), the visible controls (``torch.optim.Adam``,
  ``load_state_dict``, ``copy_``) and the documented notification for foreign raw writers (``sis_hip.mark_written``).
* ``fresh_like(module)``: a newly constructed module of the same configuration with the same state: the reference.  It runs
  the same kernels on the same weights, so every comparison is ``torch.equal``: there is no tolerance anywhere in this family.
* ``assert_follows(run, module, writer, other, builds)``: the output after the write is the fresh module's, in every
  activation; the write mattered for every layer that holds packed state; a forward with no write in between builds nothing.
"""
import torch

LR = 1e-2   # Adam's first step moves every weight by lr, about 1 % of the scale of N(0, 1) weights


# ---------------------------------------------------------------------------------------------------------------- writers
def _updater(g_ema):
    from updater.stylegan_2_updater import Stylegan2Updater
    return Stylegan2Updater(iterators={}, networks={}, optimizers={}, device=next(g_ema.parameters()).device, g_ema=g_ema, latent_size=8)


def _random_grads(module, seed=1234):
    gen = torch.Generator().manual_seed(seed)
    for p in module.parameters():
        p.grad = torch.randn(p.shape, generator=gen).to(p.device)


def _step(module, optimizer):
    _random_grads(module)
    optimizer.step()
    for p in module.parameters():
        p.grad = None


def accumulate_half(module, other):
    _updater(module).accumulate(other, 0.5)


def accumulate_zero(module, other):
    """What train_stylegan_2.py calls right after a resume: the average becomes the trained generator."""
    _updater(module).accumulate(other, 0)


def clip_adam_step(module, other):
    from training.fused_adam import GradientClipAdam
    _step(module, GradientClipAdam(module.parameters(), lr=LR))


def fused_sgd_step(module, other):
    from training.fused_sgd import FusedSGD
    _step(module, FusedSGD(module.parameters(), lr=LR, momentum=0.9))


def torch_adam_step(module, other):
    _step(module, torch.optim.Adam(module.parameters(), lr=LR))


def load_state(module, other):
    module.load_state_dict(other.state_dict())


def copy_under_no_grad(module, other):
    with torch.no_grad():
        for p, q in zip(module.parameters(), other.parameters()):
            p.copy_(q)


def raw_write_then_mark(module, other):
    """A foreign raw writer and the documented notification.  The write itself is one nothing can see: through a NumPy view on
    the host, through ``.data`` on the device (neither moves the parameter's ``_version``)."""
    import sis_hip
    for p, q in zip(module.parameters(), other.parameters()):
        version = p._version
        if p.is_cuda:
            p.data.mul_(0.5).add_(q.data, alpha=0.5)
        else:
            view = p.detach().numpy()
            view *= 0.5
            view += 0.5 * q.detach().numpy()
        assert p._version == version, "the raw write was meant to be invisible to autograd"
    sis_hip.mark_written(module)


# name -> (writer, needs a device).  The first four are the writers the stamp exists for; the next three are controls that worked
# before it; the last is the public call for everybody else's raw writes.
WRITERS = {
    "accumulate_half": (accumulate_half, False),
    "accumulate_zero": (accumulate_zero, False),
    "clip_adam_step": (clip_adam_step, False),     # host tensors: a plain torch path; device tensors: sis_adam_clip_step
    "fused_sgd_step": (fused_sgd_step, True),      # no host path
    "torch_adam_step": (torch_adam_step, False),
    "load_state_dict": (load_state, False),
    "copy_under_no_grad": (copy_under_no_grad, False),
    "raw_write_then_mark": (raw_write_then_mark, False),
}
HOST_WRITERS = [name for name, (_, device_only) in WRITERS.items() if not device_only]


def writer(name):
    return WRITERS[name][0]


# ---------------------------------------------------------------------------------------------------------------- the reference
def _construct_like(module):
    from networks.encoder.u_net_like_encoder import UNetLikeEncoder
    from networks.stylegan2.model import Generator, ModulatedConv2d
    if isinstance(module, ModulatedConv2d):
        new = ModulatedConv2d(module.in_channel, module.out_channel, module.kernel_size, module.modulation.weight.shape[1],
                              demodulate=module.demodulate, upsample=module.upsample, downsample=module.downsample)
        new.set_matrix_precision(module.matrix_precision)
        return new
    if isinstance(module, Generator):
        new = Generator(module.size, module.style_dim, len(module.style) - 1, channel_multiplier=module.channels[64] // 256)
        return new.set_matrix_precision(module.conv1.conv.matrix_precision)
    if isinstance(module, UNetLikeEncoder):
        return type(module)(module.image_size, module.latent_size, module.start_block.conv1.in_channels, dict(module.size_channel_map),
                            target_size=2 ** module.log_target_size, stylegan_variant=module.stylegan_variant)
    raise TypeError(f"fresh_like: no recipe for {type(module).__name__}")


def fresh_like(module):
    """A newly constructed module of ``module``'s configuration, its state loaded, on its device, in its mode: nothing derived
    from the weights exists in it yet."""
    new = _construct_like(module)
    new.load_state_dict(module.state_dict())
    new = new.to(next(module.parameters()).device)
    return new.train(module.training)


def packed_layers(module):
    """[(name, convolution weight)] of every layer that keeps state derived from that weight and is run by a forward."""
    from networks.encoder.u_net_like_encoder import UNetLikeEncoder
    from networks.stylegan2.model import Generator, ModulatedConv2d, StyledConv
    if isinstance(module, ModulatedConv2d):
        return [("weight", module.weight)]
    if isinstance(module, Generator):
        return [(f"{name}.conv.weight", m.conv.weight) for name, m in module.named_modules() if isinstance(m, StyledConv)]
    if isinstance(module, UNetLikeEncoder):
        out = []
        for j, block in enumerate(module._blocks()):
            out += [(f"block{j}.conv1.weight", block.conv1.weight), (f"block{j}.conv2.weight", block.conv2.weight)]
        return out
    raise TypeError(f"packed_layers: no recipe for {type(module).__name__}")


# ---------------------------------------------------------------------------------------------------------------- the check
def first_difference(got, want):
    """Name of the first tensor of ``got`` (a dict in execution order) that is not bit-equal to ``want``'s, or None."""
    assert list(got) == list(want), (list(got), list(want))
    for name in got:
        if got[name].shape != want[name].shape or not torch.equal(got[name], want[name]):
            return name
    return None


def assert_follows(run, module, write, other, builds, final=None, layers=None):
    """``run(module)`` -> {name: tensor} in execution order, the last entry (or ``final``) being the result; ``builds()`` -> how
    many pieces of derived state have been built so far (pack calls on the host, prepack launches on the device); ``layers(module)``
    -> [(name, tensor)] the write is about (default ``packed_layers``: the convolution weights that images are packed from).

    1. after ``write(module, other)`` the module's output equals a fresh module's, in every activation;
    2. sensitivity, from the reference alone: with only one layer's convolution weight put back to its value before the write
       the reference's result changes -- for every layer that holds packed state.  (The probe is a second fresh module whose
       weight is put back and restored with ``copy_`` under ``no_grad``, the oldest of the visible writers: were the probe to
       keep a stale pack its result would EQUAL the reference's and this check would fail, so it cannot pass by staleness.)
    3. the write changed the result at all;
    4. a second forward with no write in between builds nothing."""
    layers = layers or packed_layers
    before = {name: w.detach().clone() for name, w in layers(module)}
    y0 = run(module)
    y0 = {k: v.clone() for k, v in y0.items()}
    write(module, other)
    y1 = run(module)
    y1 = {k: v.clone() for k, v in y1.items()}
    built = builds()
    y2 = run(module)
    rebuilt = builds() - built
    reference = fresh_like(module)
    y_ref = run(reference)
    final = final or list(y_ref)[-1]
    stale = first_difference(y1, y_ref)
    assert stale is None, f"after the write, '{stale}' is the first activation that is not the fresh module's: derived state of that layer is stale"
    # 2.
    probe = fresh_like(module)
    for name, w in layers(probe):
        assert not torch.equal(before[name], w.detach()), f"the writer left {name} unchanged: it cannot show a stale pack"
        new = w.detach().clone()
        with torch.no_grad():
            w.copy_(before[name])
        y_old = run(probe)[final].clone()
        with torch.no_grad():
            w.copy_(new)
        assert not torch.equal(y_old, y_ref[final]), f"the result does not depend on the write to {name}: this writer / seed cannot show a stale pack there"
    assert first_difference(run(probe), y_ref) is None   # the probe is the reference again
    # 3.
    assert not torch.equal(y0[final], y_ref[final]), "the write did not change the result"
    # 4.
    assert rebuilt == 0, f"{rebuilt} pieces of derived state were rebuilt by a forward with no write in front of it"
    assert first_difference(y2, y_ref) is None
    return y_ref


def seeded(make, seed):
    """``make()`` under a fixed seed of the global generator (constructors draw their initial weights from it)."""
    state = torch.random.get_rng_state()
    try:
        torch.manual_seed(seed)
        return make()
    finally:
        torch.random.set_rng_state(state)
