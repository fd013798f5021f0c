"""Float64 restatements of the DocUFCN kernel calls (csrc/doc_ufcn.hip, csrc/pool_ops.hip) and the per-plane / per-channel metrics
they are held to.  Shared by tests/test_doc_ufcn_layouts_gpu.py (stand-alone calls in their slice / offset forms, and every call of
a real training step on the tensors the step gave it) and tools/localise_doc_ufcn_grad.py.

Metrics (a Frobenius norm over a whole tensor hides one wrong channel of a 32-channel vector or one wrong border row of a map):

* maps and weights, ``plane_figure``: per plane (sample, channel) -- per output row for a weight gradient -- max |err| against
  ``tol`` x the plane's max |ref|;
* per-channel sums (dgamma, dbeta, bias gradients), ``channel_sum_figure``: |err_c| <= 1e-5 x sum |terms_c| (the kernel bound on the
  sum's condition-free scale), and |err_c| <= max(1e-5 x |ref_c|, 8 x the fp32 ATen formulation's error on the same inputs);
* layout operators (shuffle, pooling, slices of a wider buffer): equality.

A Figure's ``worst`` is the largest error / bound over its planes or channels: <= 1 passes.

The ReLU gate of the BatchNorm references: an element whose float64 pre-activation lies within 1e-5 of the magnitude of its terms
around zero has no determined sign under fp32 rounding; there (and only there) the reference takes the gate the kernel took, and the
figure's note counts these elements.
"""
import inspect

import numpy as np
import torch
import torch.nn.functional as F

from test_doc_ufcn_gpu import DEV, _keep_dev, _net

KERNEL_TOL = 1e-5   # the project's bound of one fp32 kernel against float64
BN_DX_TOL = 1e-4    # BatchNorm data gradient (tests/test_doc_ufcn_gpu.py)
ATEN_FACTOR = 8.0   # as _step_parity: within 8x the fp32 library formulation


def keep_scale(p):
    return 65536.0 / (65536 - int(p * 65536.0 + 0.5)) if p > 0 else 1.0


def unpack_mask(mask, shape):
    """The 1-bit-per-element mask of bn_drop_fwd -> bool tensor: element 4 i + q is bit i % 64 of word (i / 64) * 4 + q."""
    n4 = int(np.prod(shape)) // 4
    i = torch.arange(n4, dtype=torch.int64, device=mask.device)
    words = mask.view(-1, 4)[i >> 6]
    return ((words >> (i & 63).unsqueeze(1)) & 1).bool().reshape(shape)


class Figure:
    def __init__(self, quantity, got, ref, worst, where="", aten=None, note=""):
        self.quantity, self.got, self.ref, self.worst, self.where, self.aten, self.note = quantity, got, ref, worst, where, aten, note

    @property
    def ok(self):
        return self.worst <= 1.0

    def rel(self):
        """Frobenius error of the whole tensor (the figure DESIGN.md quotes)."""
        a, b = self.got.double(), self.ref.double()
        return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()

    def __str__(self):
        aten = "" if self.aten is None else f"  ATen {self.aten:.2e}"
        return f"{self.quantity:<13s} err/bound {self.worst:.2e} at {self.where}{aten}  {self.note}"


def _ratio(err, bound):
    """err / bound elementwise; 0 where both are 0, inf where only the bound is."""
    zero_bound = torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))
    return torch.where(bound > 0, err / bound.clamp_min(1e-300), zero_bound)


def _worst(ratio):
    k = int(ratio.reshape(-1).argmax())
    return ratio.reshape(-1)[k].item(), k


def plane_figure(quantity, got, ref, tol, lead=2, aten=None, note=""):
    """Planes = the first ``lead`` axes; per plane max |got - ref| <= tol * max |ref|."""
    planes = int(np.prod(ref.shape[:lead]))
    g, r = got.double().reshape(planes, -1), ref.double().reshape(planes, -1)
    scale = r.abs().amax(1)
    worst, k = _worst(_ratio((g - r).abs().amax(1), tol * scale))
    fig_aten = None
    if aten is not None:
        fig_aten = _worst(_ratio((aten.double().reshape(planes, -1) - r).abs().amax(1), tol * scale))[0]
    return Figure(quantity, got, ref, worst, f"plane {tuple(int(v) for v in np.unravel_index(k, ref.shape[:lead]))}", fig_aten, note)


def bounded_figure(quantity, got, ref, bound, note=""):
    """|got - ref| <= bound, elementwise."""
    worst, k = _worst(_ratio((got.double() - ref).abs(), bound))
    return Figure(quantity, got, ref, worst, f"element {k}", None, note)


def channel_sum_figure(quantity, got, terms, aten=None, relative=True, note=""):
    """got [C] against the float64 sum of terms [C, N]: the two per-channel bounds of the module docstring.  ``relative=False``
    keeps only the first one (sums that cancel to zero in exact arithmetic: a bias gradient in front of a train-mode BatchNorm)."""
    ref, scale = terms.sum(1), terms.abs().sum(1)
    err = (got.double() - ref).abs()
    ratio = _ratio(err, KERNEL_TOL * scale)
    fig_aten = None
    if aten is not None:
        err_aten = (aten.double() - ref).abs()
        fig_aten = _worst(_ratio(err_aten, KERNEL_TOL * scale))[0]
        if relative:
            ratio = torch.maximum(ratio, _ratio(err, torch.maximum(KERNEL_TOL * ref.abs(), ATEN_FACTOR * err_aten)))
    worst, k = _worst(ratio)
    note = f"|err| = {err[k] / scale[k].clamp_min(1e-300):.1e} sum|terms| = {err[k] / ref[k].abs().clamp_min(1e-300):.1e} |ref|" \
        + (f" (ATen {err_aten[k] / scale[k].clamp_min(1e-300):.1e}, {err_aten[k] / ref[k].abs().clamp_min(1e-300):.1e})" if aten is not None else "") \
        + (" " + note if note else "")
    return Figure(quantity, got, ref, worst, f"channel {k}", fig_aten, note)


def exact_figure(quantity, got, ref, note=""):
    bad = int((got != ref).sum()) if got.shape == ref.shape else -1
    return Figure(quantity, got, ref, 0.0 if bad == 0 else float("inf"), f"{bad} elements differ", None, note)


# ---------------------------------------------------------------------------------------------------- one check per entry point


def check_dconv3x3(x, weight, bias, dilation, out):
    d = int(dilation)
    ref = F.conv2d(x.double(), weight.double(), None if bias is None else bias.double(), padding=d, dilation=d)
    return [plane_figure("y", out, ref, KERNEL_TOL, aten=F.conv2d(x, weight, bias, padding=d, dilation=d))]


def check_dconv3x3_adjoint(weight, out):
    return [exact_figure("adjoint", out, weight.transpose(0, 1).flip(2, 3).contiguous())]


def check_transpose2d(x, out):
    return [exact_figure("transpose", out, x.t().contiguous())]


def wgrad_reference(gy, x, dilation, taps):
    """float64 (or the dtype of its inputs) weight gradient: the einsum over samples and pixels."""
    if taps == 1:
        return torch.einsum("bohw,bihw->oi", gy, x)[:, :, None, None]
    d = int(dilation)
    shape = (gy.shape[1], x.shape[1], 3, 3)
    return torch.nn.grad.conv2d_weight(x, shape, gy, padding=d, dilation=d)


def check_dconv3x3_wgrad(gy, x, dilation, taps, out):
    ref = wgrad_reference(gy.double(), x.double(), dilation, taps)
    return [plane_figure("dw", out, ref, KERNEL_TOL, lead=1, aten=wgrad_reference(gy, x, dilation, taps))]


def check_channel_sum(x, out):
    terms = x.double().transpose(0, 1).reshape(x.shape[1], -1)
    return [channel_sum_figure("db", out, terms, aten=x.sum((0, 2, 3)), relative=False)]


def check_bn_stats(x, rm0, rv0, eps, momentum, mean, invstd, rm1, rv1):
    """mean on the scale mean |x_c| (a mean is a sum that may cancel), invstd relative; the running buffers as
    BatchNorm2d(momentum) updates them (unbiased variance)."""
    xd = x.double()
    n = xd.numel() // xd.shape[1]
    m, var = xd.mean((0, 2, 3)), xd.var((0, 2, 3), unbiased=False)
    mabs = xd.abs().mean((0, 2, 3))
    istd = (var + eps).rsqrt()
    rm = (1 - momentum) * rm0.double() + momentum * m
    rv = (1 - momentum) * rv0.double() + momentum * var * (n / max(n - 1, 1))
    return [bounded_figure("mean", mean, m, KERNEL_TOL * mabs),
            bounded_figure("invstd", invstd, istd, KERNEL_TOL * istd),
            bounded_figure("running_mean", rm1, rm, KERNEL_TOL * ((1 - momentum) * rm0.double().abs() + momentum * mabs)),
            bounded_figure("running_var", rv1, rv, KERNEL_TOL * rv)]


def _bcast(v):
    return v.double().view(1, -1, 1, 1)


def _ambiguous(a, x, m, gis, beta):
    """Elements whose pre-activation a = gis * (x - m) + beta is within 1e-5 of its terms' magnitude of zero."""
    return a.abs() <= KERNEL_TOL * (gis.abs() * (x.abs() + m.abs()) + beta.abs())


def check_bn_drop_fwd(x, mean, scale_src, gamma, beta, eval_mode, eps, keep, p, y, mask):
    """y (the written channel slice, [B, C, H, W]) and the mask against float64 from the call's own statistics.  Eval mode:
    F.batch_norm(training=False) + ReLU."""
    xd = x.double()
    if eval_mode:
        a = F.batch_norm(xd, mean.double(), scale_src.double(), gamma.double(), beta.double(), False, 0.0, eps)
        gis = _bcast(gamma) * (_bcast(scale_src) + eps).rsqrt()
    else:
        gis = _bcast(gamma) * _bcast(scale_src)
        a = gis * (xd - _bcast(mean)) + _bcast(beta)
    ref = F.relu(a)
    if keep is not None:
        ref = ref * (keep.double() * keep_scale(p))
    figs = [plane_figure("y", y, ref, KERNEL_TOL)]
    if mask is not None:
        want = (a > 0) if keep is None else (a > 0) & keep
        amb = _ambiguous(a, xd, _bcast(mean), gis, _bcast(beta))
        bad = int(((unpack_mask(mask, x.shape) != want) & ~amb).sum())
        figs.append(Figure("mask", mask, mask, 0.0 if bad == 0 else float("inf"), f"{bad} bits differ", None,
                           f"{int(amb.sum())} gates within rounding of zero"))
    return figs


def bn_drop_autograd(z, gamma, beta, keep, p, eps, g, own_gate=None):
    """autograd of y = relu(batch_norm(z)) * keep * scale in the dtype of ``z`` under ``g``: the output gradient, or a function
    y -> scalar loss (what follows y in the network) -> (dz, dgamma, dbeta, gate * keep * scale, xhat, number of ambiguous gates,
    dL/dy).  With ``own_gate`` the ambiguous elements (module docstring) take it."""
    zd, gd, bd = (t.detach().clone().requires_grad_() for t in (z, gamma, beta))
    a = F.batch_norm(zd, None, None, gd, bd, True, 0.0, eps)
    with torch.no_grad():
        m, var = z.mean((0, 2, 3), keepdim=True), z.var((0, 2, 3), unbiased=False, keepdim=True)
        istd = (var + eps).rsqrt()
        xhat = (z - m) * istd
        gate, n_amb = a > 0, 0
        if own_gate is not None:
            amb = _ambiguous(a, z, m, gamma.view(1, -1, 1, 1) * istd, beta.view(1, -1, 1, 1))
            if keep is not None:
                amb = amb & keep
            gate, n_amb = torch.where(amb, own_gate, gate), int(amb.sum())
        factor = gate.to(z.dtype)
        if keep is not None:
            factor = factor * (keep.to(z.dtype) * keep_scale(p))
    y = a * factor   # relu(a) = a * (a > 0): the same gradients as F.relu's wherever the gate is the reference's own
    y.retain_grad()
    if callable(g):
        g(y).backward()
    else:
        y.backward(g.to(z.dtype))
    return zd.grad, gd.grad, bd.grad, factor, xhat, n_amb, y.grad


def check_bn_drop_bwd(g, x, gamma, beta, keep, p, eps, mask, dx, dgamma, dbeta):
    """The backward (g: the gradient of y [B, C, H, W], or a function y -> loss) against float64 autograd with the masks
    regenerated on the device, beside the fp32 ATen formulation of the same expression."""
    own_gate = unpack_mask(mask, x.shape)
    rdx, rdg, rdb, factor, xhat, n_amb, gy = bn_drop_autograd(x.double(), gamma.double(), beta.double(), keep, p, eps, g, own_gate)
    adx, adg, adb = bn_drop_autograd(x, gamma, beta, keep, p, eps, g)[:3]
    c = x.shape[1]
    t_beta = (factor * gy).transpose(0, 1).reshape(c, -1)
    t_gamma = (factor * gy * xhat).transpose(0, 1).reshape(c, -1)
    note = f"{n_amb} gates within rounding of zero"
    return [plane_figure("dx", dx, rdx, BN_DX_TOL, aten=adx, note=note),
            channel_sum_figure("dgamma", dgamma, t_gamma, aten=adg),
            channel_sum_figure("dbeta", dbeta, t_beta, aten=adb)]


def check_conv1x1_f32(x, weight, bias, data_gradient, out):
    def run(x, w, b):
        return F.conv_transpose2d(x, w) if data_gradient else F.conv2d(x, w, b)
    ref = run(x.double(), weight.double(), None if bias is None else bias.double())
    return [plane_figure("dx" if data_gradient else "y", out, ref, KERNEL_TOL, aten=run(x, weight, bias))]


def check_pixel_shuffle2(x, bias, y):
    ref = F.pixel_shuffle(x, 2)
    if bias is not None:
        ref = ref + bias.view(1, -1, 1, 1)
    return [exact_figure("shuffle", y, ref)]


def check_pixel_shuffle2_grad(g, out):
    return [exact_figure("unshuffle", out, F.pixel_unshuffle(g, 2))]


def check_max_pool2x2(src, out, arg):
    """src: the pooled channel slice [B, C, H, W]; values and the argmax byte (kh * 2 + kw, first maximum) as F.max_pool2d."""
    ref, idx = F.max_pool2d(src, 2, return_indices=True)
    w = src.shape[3]
    k = ((idx // w) % 2) * 2 + idx % 2
    return [exact_figure("pooled", out, ref), exact_figure("argmax", arg.long(), k)]


def check_max_pool2d_backward(src, grad_out, dx):
    s = src.double().requires_grad_()
    F.max_pool2d(s, 2).backward(grad_out.double())
    return [exact_figure("dpool", dx.double(), s.grad)]


def check_weighted_ce_fwd(logits, labels, weight, loss, stats):
    wd = None if weight is None else weight.double()
    ref = F.cross_entropy(logits.double(), labels, weight=wd).reshape(1)
    wsum = (wd[labels].sum() if wd is not None else torch.tensor(float(labels.numel()), device=logits.device)).reshape(1)
    return [bounded_figure("loss", loss, ref, KERNEL_TOL * ref.abs()), bounded_figure("weight_sum", stats, wsum, KERNEL_TOL * wsum)]


def check_weighted_ce_bwd(grad_loss, logits, labels, weight, out):
    def run(lg, w):
        lg = lg.detach().clone().requires_grad_()
        F.cross_entropy(lg, labels, weight=w).backward(grad_loss.reshape(()).to(lg.dtype))
        return lg.grad
    ref = run(logits.double(), None if weight is None else weight.double())
    return [plane_figure("dlogits", out, ref, KERNEL_TOL, aten=run(logits, weight))]


# ---------------------------------------------------------------------------------------------------- recording a real step

ENTRY_POINTS = ("dconv3x3", "dconv3x3_adjoint", "dconv3x3_wgrad", "channel_sum", "bn_stats", "bn_drop_fwd", "bn_drop_bwd",
                "conv1x1_f32", "transpose2d", "pixel_shuffle2", "pixel_shuffle2_grad", "max_pool2x2_slice", "max_pool2d_backward",
                "weighted_ce_fwd", "weighted_ce_bwd")


def _clone(v):
    if isinstance(v, torch.Tensor):
        return v.detach().clone()
    if isinstance(v, (tuple, list)):
        return type(v)(_clone(u) for u in v)
    return v


class Call:
    """One call of a sis_hip entry point: ``args`` (by parameter name, tensors cloned before the call), ``after`` (the tensor
    arguments cloned after it: buffers written in place), ``out`` (cloned), and the call's own tensors (``live`` / ``live_out``,
    kept so that no address is reused while the step runs: calls are paired by data pointer)."""

    def __init__(self, name, phase, args, live):
        self.name, self.phase, self.args, self.live = name, phase, args, live
        self.after, self.out, self.live_out, self.label = {}, None, None, ""

    def ptr(self, arg):
        return self.live[arg].data_ptr()


class Recorder:
    def __init__(self):
        self.calls, self.phase, self._undo = [], "forward", []

    def install(self, setattr_fn=setattr):
        import sis_hip
        for name in ENTRY_POINTS:
            real = getattr(sis_hip, name)
            self._undo.append((setattr_fn, sis_hip, name, real))
            setattr_fn(sis_hip, name, self._wrap(name, real))
        return self

    def remove(self):
        for setattr_fn, mod, name, real in reversed(self._undo):
            setattr_fn(mod, name, real)
        self._undo = []

    def _wrap(self, name, real):
        sig = inspect.signature(real)

        def wrapper(*a, **k):
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            live = dict(bound.arguments)
            call = Call(name, self.phase, {n: _clone(v) for n, v in live.items()}, live)
            out = real(*a, **k)
            call.after = {n: _clone(v) for n, v in live.items() if isinstance(v, torch.Tensor) and n in ("out", "running_mean", "running_var")}
            call.out, call.live_out = _clone(out), out
            self.calls.append(call)
            return out
        return wrapper


STEP_SEED_WORD = 0x5EED0D0C0FFEE   # the dropout seed word record_step starts from: the same masks in every process


def record_step(cls, batch, size, setattr_fn=setattr, **kw):
    """One training step of the seeded network of ``_step_parity`` (same input, labels and class weights) with every kernel call
    recorded -> (net, x, labels, class weights, calls in execution order, labelled with the layer they belong to)."""
    import sis_hip
    from updater.segmentation_updater import weighted_cross_entropy
    sis_hip.dropout_seed(DEV).fill_(STEP_SEED_WORD)
    net = _net(cls, **kw).to(DEV).train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(batch, 3, size, size, generator=g).to(DEV)
    labels = torch.randint(0, 3, (batch, size, size), generator=g).to(DEV)
    wts = torch.tensor([1.0, 2.0, 0.5], device=DEV)
    rec = Recorder().install(setattr_fn)
    try:
        loss = weighted_cross_entropy(net(x), labels, wts)
        rec.phase = "backward"
        loss.backward()
        torch.cuda.synchronize()
    finally:
        rec.remove()
    label_calls(rec.calls, net)
    return net, x, labels, wts, rec.calls


def label_calls(calls, net):
    """Layer names from the parameters a call was given (convolution weight, BatchNorm gamma, shuffle bias); a call without one
    belongs to the layer of the call before it -- the backward runs the layers in reverse order, each BatchNorm backward followed by
    its convolution's -- except the per-pixel product of a transposed convolution's forward and a pooling backward, which come in
    front of the call that names their layer."""
    names = {}
    for n, p in net.named_parameters():
        names[p.data_ptr()] = n.rsplit(".", 1)[0]
    current = {"forward": "?", "backward": "loss"}
    for call in calls:
        for arg in ("weight", "gamma", "bias"):
            v = call.live.get(arg)
            if isinstance(v, torch.Tensor) and v.data_ptr() in names:
                layer = names[v.data_ptr()]   # '<layer>.conv', '<layer>.bn' or 'classifier'
                current[call.phase] = layer[:-3] if layer.endswith(".bn") else layer[:-5] if layer.endswith(".conv") else layer
                break
        call.label = current[call.phase]
    for k in range(len(calls) - 2, -1, -1):
        c = calls[k]
        lookahead = c.name == "max_pool2d_backward" or (c.name in ("conv1x1_f32", "transpose2d") and c.phase == "forward")
        if lookahead and calls[k + 1].phase == c.phase:
            c.label = calls[k + 1].label
    for c in calls:
        if c.name in ("weighted_ce_fwd", "weighted_ce_bwd"):
            c.label = "loss"
        elif c.phase == "backward" and c.label == "loss":
            c.label = "classifier"


def verify_calls(calls):
    """Every recorded call recomputed in float64 from its own recorded fp32 inputs -> [(call, [Figure])] in execution order."""
    fwd_of_x, stats_of_x, pool_of_arg = {}, {}, {}
    for c in calls:
        if c.name == "bn_drop_fwd":
            fwd_of_x[c.ptr("x")] = c
        elif c.name == "bn_stats":
            stats_of_x[c.ptr("x")] = c
        elif c.name == "max_pool2x2_slice":
            pool_of_arg[c.live_out[1].data_ptr()] = c
    rows = []
    for c in calls:
        a = c.args
        if c.name == "dconv3x3":
            figs = check_dconv3x3(a["x"], a["weight"], a["bias"], a["dilation"], c.out)
        elif c.name == "dconv3x3_adjoint":
            figs = check_dconv3x3_adjoint(a["weight"], c.out)
        elif c.name == "transpose2d":
            figs = check_transpose2d(a["x"], c.out)
        elif c.name == "dconv3x3_wgrad":
            figs = check_dconv3x3_wgrad(a["grad_output"], a["x"], a["dilation"], a["taps"], c.out)
        elif c.name == "channel_sum":
            figs = check_channel_sum(a["x"], c.out)
        elif c.name == "bn_stats":
            figs = check_bn_stats(a["x"], a["running_mean"], a["running_var"], a["eps"], a["momentum"], c.out[0], c.out[1],
                                  c.after["running_mean"], c.after["running_var"])
        elif c.name == "bn_drop_fwd":
            figs = _verify_bn_drop_fwd(c)
        elif c.name == "bn_drop_bwd":
            figs = _verify_bn_drop_bwd(c, fwd_of_x[c.ptr("x")], stats_of_x[c.ptr("x")])
        elif c.name == "conv1x1_f32":
            figs = check_conv1x1_f32(a["x"], a["weight"], a["bias"], a["data_gradient"], c.out)
        elif c.name == "pixel_shuffle2":
            figs = _verify_pixel_shuffle2(c)
        elif c.name == "pixel_shuffle2_grad":
            g = a["g"]
            ch = g.shape[1] - a["channel_offset"] if a["channels"] is None else a["channels"]
            figs = check_pixel_shuffle2_grad(g[:, a["channel_offset"]:a["channel_offset"] + ch], c.out)
        elif c.name == "max_pool2x2_slice":
            off, ch = a["channel_offset"], a["channels"]
            figs = check_max_pool2x2(a["buf"][:, off:off + ch], c.out[0], c.out[1])
        elif c.name == "max_pool2d_backward":
            f = pool_of_arg[c.ptr("argmax")]
            off, ch = f.args["channel_offset"], f.args["channels"]
            figs = check_max_pool2d_backward(f.args["buf"][:, off:off + ch], a["grad_output"], c.out)
        elif c.name == "weighted_ce_fwd":
            figs = check_weighted_ce_fwd(a["logits"], a["labels"], a["weight"], c.out[0], c.out[1])
        elif c.name == "weighted_ce_bwd":
            figs = check_weighted_ce_bwd(a["grad_loss"], a["logits"], a["labels"], a["weight"], c.out)
        else:
            raise AssertionError(c.name)
        rows.append((c, figs))
    return rows


def _untouched(before, after, lo, hi):
    """The channels outside [lo, hi) of a wider buffer, bit for bit as before the call (the buffer may be uninitialised)."""
    keep = [k for k in range(before.shape[1]) if not lo <= k < hi]
    b, a = before[:, keep].contiguous().view(torch.int32), after[:, keep].contiguous().view(torch.int32)
    return exact_figure("other channels", a, b)


def _call_keep(fwd):
    a = fwd.args
    if not a["drop_p"] > 0:
        return None
    return _keep_dev(a["seed"].item(), a["site"], a["x"].shape, a["drop_p"])


def _verify_bn_drop_fwd(c):
    a = c.args
    ch, off = a["x"].shape[1], a["channel_offset"] if a["out"] is not None else 0
    out = c.out[0]
    figs = check_bn_drop_fwd(a["x"], a["mean"], a["invstd_or_var"], a["gamma"], a["beta"], a["eval_mode"], a["eps"], _call_keep(c),
                             a["drop_p"], out[:, off:off + ch], c.out[1])
    if a["out"] is not None:
        figs.append(_untouched(a["out"], c.after["out"], off, off + ch))
    return figs


def _verify_bn_drop_bwd(c, fwd, stats):
    a = c.args
    ch = a["x"].shape[1]
    if a["dy"] is None:
        g = a["dy2"].double()
    else:
        g = a["dy"][:, a["channel_offset"]:a["channel_offset"] + ch].double()
        if a["dy2"] is not None:
            g = g + a["dy2"].double()
    return check_bn_drop_bwd(g, a["x"], a["gamma"], fwd.args["beta"], _call_keep(fwd), a["drop_p"], stats.args["eps"], a["mask"], *c.out)


def _verify_pixel_shuffle2(c):
    a = c.args
    ch = a["x"].shape[1] // 4
    off = a["channel_offset"] if a["out"] is not None else 0
    figs = check_pixel_shuffle2(a["x"], a["bias"], c.out[:, off:off + ch])
    if a["out"] is not None:
        figs.append(_untouched(a["out"], c.after["out"], off, off + ch))
    return figs


def report(rows, out=print):
    """One line per figure; returns the failing ones as (label, call name, Figure)."""
    failed = []
    for c, figs in rows:
        for f in figs:
            out(f"{c.phase:<8s} {c.label:<30s} {c.name:<20s} {f}")
            if not f.ok:
                failed.append((c.label, c.name, f))
    return failed
