#!/usr/bin/env python
"""Where does the small-shape gradient error of the own DocUFCN step enter?  

One training step of DocUFCN('base') at B = 2, 64^2 -- the seeded network, input and loss of
tests/test_doc_ufcn_gpu.py::_step_parity -- once with dropout 0.4 and once with p = 0.  For each it prints

1. one row per kernel call of the backward, in execution order, with
     local        the call's outputs against float64 recomputed from the call's OWN recorded fp32 inputs (teacher-forced:
                  tests/doc_ufcn_checks.py), Frobenius error and the worst error / bound over planes or channels;
     propagated   the same tensor against the float64 model's gradient at that point (full-backward hooks on the float64 copy);
     lib local / lib propagated   the same two figures for the fp32 library step: the module's backward recomputed in float64 from
                  the input and output gradient the fp32 module saw (for a BatchNorm module this is the normalisation alone; ReLU
                  and dropout are modules of their own there), and the module's gradients against the float64 model's;
2. the discrete decisions that differ from the float64 model's: ReLU gates and max-pool argmaxes, per layer, own and library;
3. the median weight-gradient error of the step with one kernel family at a time replaced by its fp32 torch equivalent, and with
   the own kernels kept but the gates / argmaxes of the float64 model forced on them.

    python tools/localise_doc_ufcn_grad.py [--out profiles/doc_ufcn_small_shape_localisation.txt]
"""
import argparse
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "synthesis-in-style_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import doc_ufcn_checks as K   # noqa: E402
from test_doc_ufcn_gpu import DEV, _net, _rel, _replay_masks   # noqa: E402

LINES = []


def emit(line=""):
    print(line, flush=True)
    LINES.append(line)


def _batch():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 64, 64, generator=g).to(DEV)
    labels = torch.randint(0, 3, (2, 64, 64), generator=g).to(DEV)
    return x, labels, torch.tensor([1.0, 2.0, 0.5], device=DEV)


class Hooked:
    """A torch copy of the network (float64 oracle or fp32 library step) run with the step's masks; keeps, per convolution /
    BatchNorm module, its input, output gradient and input gradient, and per layer the final activation (gate and argmax)."""

    def __init__(self, net, dtype, seed, x, labels, wts):
        self.net = copy.deepcopy(net).to(dtype).to(DEV).train()
        _replay_masks(self.net, seed)
        self.inp, self.gout, self.gin, self.act = {}, {}, {}, {}
        self.modules = dict(self.net.named_modules())
        for name, m in self.modules.items():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d, torch.nn.BatchNorm2d)):
                m.register_forward_pre_hook(lambda mod, inp, name=name: self.inp.__setitem__(name, inp[0].detach()))
                m.register_full_backward_hook(lambda mod, gi, go, name=name: self._keep_grads(name, gi[0], go[0]))
            if isinstance(m, torch.nn.Sequential) and hasattr(m, "bn"):
                m.register_forward_hook(lambda mod, inp, out, name=name: self.act.__setitem__(name, out.detach()))
        self.logits = self.net._forward_torch(x.to(dtype))
        F.cross_entropy(self.logits, labels, weight=wts.to(dtype)).backward()

    def _keep_grads(self, name, grad_input, grad_output):
        self.gin[name], self.gout[name] = grad_input, grad_output

    def grad(self, name):
        return dict(self.net.named_parameters())[name].grad


def _module_local(h, name):
    """The fp32 module's backward against a float64 copy of the module on the same input and output gradient."""
    m = h.modules[name]
    m64 = copy.deepcopy(m).double()
    for hooks in (m64._forward_pre_hooks, m64._backward_hooks, m64._forward_hooks):
        hooks.clear()
    m64.zero_grad(set_to_none=True)
    x = h.inp[name].double().requires_grad_()
    m64(x).backward(h.gout[name].double())
    return x.grad, m64.weight.grad, (m64.bias.grad if m64.bias is not None else None)


def _fmt(v):
    return "    -    " if v is None else f"{v:9.2e}"


def _targets(call, fig):
    """(module name, which) of the float64 / library model that the figure's tensor is the gradient of."""
    layer = call.label
    conv = layer if layer == "classifier" else layer + ".conv"
    if call.name == "weighted_ce_bwd":
        return "classifier", "gout"
    if call.name == "dconv3x3" or (call.name == "conv1x1_f32" and call.args["data_gradient"]):
        return conv, "gin"
    if call.name == "dconv3x3_wgrad":
        return conv, "weight1" if call.args["taps"] == 1 else "weight"
    if call.name == "channel_sum":
        return conv, "bias"
    if call.name == "bn_drop_bwd":
        return layer + ".bn", {"dx": "gin", "dgamma": "weight", "dbeta": "bias"}[fig.quantity]
    return None, None


def _model_tensor(h, module, which, local=None):
    if which == "gout":
        return h.gout[module]
    if which == "gin":
        return h.gin.get(module) if local is None else local[0]
    if which in ("weight", "weight1"):
        w = h.grad(module + ".weight") if local is None else local[1]
        if which == "weight1":   # ConvTranspose2d [Cin, Cout, 2, 2] -> the per-pixel product's [4 Cout, Cin, 1, 1]
            w = w.reshape(w.shape[0], -1).t().reshape(-1, w.shape[0], 1, 1)
        return w
    return h.grad(module + ".bias") if local is None else local[2]


def localisation_table(calls, ref, lib):
    emit(f"{'layer':<28s} {'call':<20s} {'quantity':<9s} {'local':>9s} {'(err/bound)':>11s} {'propagated':>10s} | {'lib local':>9s} {'lib propag.':>11s}")
    rows = K.verify_calls(calls)
    local_cache = {}
    failed = []
    for call, figs in rows:
        if call.phase != "backward":
            failed += [(call, f) for f in figs if not f.ok]
            continue
        for f in figs:
            if not f.ok:
                failed.append((call, f))
            module, which = _targets(call, f)
            prop = lib_local = lib_prop = None
            if module is not None:
                want = _model_tensor(ref, module, which)
                if want is not None:
                    prop = _rel(f.got.reshape(want.shape), want)
                    got_lib = _model_tensor(lib, module, which)
                    lib_prop = _rel(got_lib, want)
                    if which != "gout":
                        if module not in local_cache:
                            local_cache[module] = _module_local(lib, module)
                        lib_local = _rel(got_lib, _model_tensor(lib, module, which, local_cache[module]))
            emit(f"{call.label:<28s} {call.name:<20s} {f.quantity:<9s} {_fmt(f.rel())} {f.worst:11.2e} {_fmt(prop):>10s} | {_fmt(lib_local)} {_fmt(lib_prop):>11s}")
    emit()
    emit(f"local checks (forward and backward calls, {sum(len(f) for _, f in rows)} figures): "
         + ("all within their bounds" if not failed else "OUTSIDE: " + "; ".join(f"{c.label} {c.name} {f}" for c, f in failed)))


def _argmax_bytes(y):
    _, idx = F.max_pool2d(y, 2, return_indices=True)
    return ((idx // y.shape[3]) % 2) * 2 + idx % 2


def decisions(calls, ref, lib):
    """ReLU gates (with the dropout keep flag) and pooling argmaxes of the own step and of the library step that differ from the
    float64 model's."""
    emit(f"{'layer':<28s} {'elements':>9s} {'own gates':>10s} {'lib gates':>10s} {'own argmax':>11s} {'lib argmax':>11s}   (decisions unlike the float64 model's)")
    own_gate, own_arg = {}, {}
    for c in calls:
        if c.name == "bn_drop_fwd":
            own_gate[c.label] = K.unpack_mask(c.out[1], c.args["x"].shape)
        elif c.name == "max_pool2x2_slice":
            own_arg[c.label] = c.out[1].long()
    total = [0, 0, 0, 0]
    for layer, gate in own_gate.items():
        y64, y32 = ref.act[layer], lib.act[layer]
        n = [int((gate != (y64 > 0)).sum()), int(((y32 > 0) != (y64 > 0)).sum()), None, None]
        if layer in own_arg:
            k64 = _argmax_bytes(y64)
            n[2], n[3] = int((own_arg[layer] != k64).sum()), int((_argmax_bytes(y32) != k64).sum())
        for k in range(4):
            total[k] += n[k] or 0
        if any(n):
            emit(f"{layer:<28s} {gate.numel():>9d} {n[0]:>10d} {n[1]:>10d} {str(n[2] if n[2] is not None else '-'):>11s} {str(n[3] if n[3] is not None else '-'):>11s}")
    emit(f"{'all layers':<28s} {sum(g.numel() for g in own_gate.values()):>9d} {total[0]:>10d} {total[1]:>10d} {total[2]:>11d} {total[3]:>11d}")


def _medians(net, ref, lib):
    own, libs = [], []
    for (name, p), (_, q), (_, r) in zip(net.named_parameters(), ref.net.named_parameters(), lib.net.named_parameters()):
        if name.endswith("conv.bias") and not name.startswith("classifier"):
            continue
        own.append(_rel(p.grad, q.grad))
        libs.append(_rel(r.grad, q.grad))
    return float(np.median(own)), float(np.median(libs)), float(np.max(own)), float(np.max(libs))


# ---------------------------------------------------------------------------------------------------- substitutions


def _pack_gate(gate):
    """bool [B, C, H, W] -> the mask words of bn_drop_fwd (inverse of doc_ufcn_checks.unpack_mask)."""
    bits = gate.reshape(-1, 4).long()
    pad = (-bits.shape[0]) % 64
    bits = torch.cat([bits, bits.new_zeros(pad, 4)]).reshape(-1, 64, 4)
    shift = torch.arange(64, dtype=torch.int64, device=gate.device).view(1, 64, 1)
    return (bits << shift).sum(1).reshape(-1).contiguous()


def _families(real, ref):
    """name -> {entry point: replacement}.  The fp32 torch equivalents keep the entry points' signatures."""
    def conv(x, weight, bias=None, dilation=1):
        return F.conv2d(x, weight, bias, padding=dilation, dilation=dilation)

    def wgrad(grad_output, x, dilation=1, taps=9):
        return K.wgrad_reference(grad_output, x, dilation, taps).contiguous()

    def conv1x1(x, weight, bias=None, data_gradient=False):
        return F.conv_transpose2d(x, weight) if data_gradient else F.conv2d(x, weight, bias)

    def bn_stats(x, running_mean, running_var, eps, momentum):
        var, mean = torch.var_mean(x, (0, 2, 3), unbiased=False)
        n = x.numel() // x.shape[1]
        running_mean.mul_(1 - momentum).add_(momentum * mean)
        running_var.mul_(1 - momentum).add_(momentum * var * (n / (n - 1)))
        return mean, (var + eps).rsqrt()

    def bn_drop_fwd(x, mean, invstd_or_var, gamma, beta, eval_mode=False, eps=1e-5, seed=None, site=0, drop_p=0.0, out=None,
                    channel_offset=0, want_mask=True):
        v = lambda t: t.view(1, -1, 1, 1)
        a = (x - v(mean)) * v(invstd_or_var) * v(gamma) + v(beta)
        factor = (a > 0).float()
        if drop_p > 0:
            factor = factor * (K._keep_dev(seed.item(), site, x.shape, drop_p).float() * K.keep_scale(drop_p))
        y = a * factor
        if out is None:
            return y, factor
        out[:, channel_offset:channel_offset + x.shape[1]] = y
        return out, factor

    def bn_drop_bwd(dy, x, mean, invstd, gamma, mask, drop_p, channel_offset=0, dy2=None):
        c = x.shape[1]
        g = dy2 if dy is None else dy[:, channel_offset:channel_offset + c] + (0 if dy2 is None else dy2)
        g = g * mask
        v = lambda t: t.view(1, -1, 1, 1)
        n = x.numel() // c
        xhat = (x - v(mean)) * v(invstd)
        dbeta, dgamma = g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))
        dx = v(gamma * invstd) * (g - v(dbeta) / n - xhat * v(dgamma) / n)
        return dx.contiguous(), dgamma, dbeta

    def pool(buf, channel_offset, channels):
        src = buf[:, channel_offset:channel_offset + channels]
        return F.max_pool2d(src, 2).contiguous(), _argmax_bytes(src).to(torch.uint8).contiguous()

    def ce_fwd(logits, labels, weight=None):
        return F.cross_entropy(logits, labels, weight=weight).reshape(1), weight[labels].sum().reshape(1)

    def ce_bwd(grad_loss, logits, labels, weight, stats):
        lg = logits.detach().clone().requires_grad_()
        with torch.enable_grad():
            F.cross_entropy(lg, labels, weight=weight).backward(grad_loss.reshape(()))
        return lg.grad

    layer_of_site = {m.bn._sis_site: name for name, m in ref.modules.items() if isinstance(m, torch.nn.Sequential) and hasattr(m, "bn")}

    def own_fwd_float64_gates(x, mean, invstd_or_var, gamma, beta, **kw):
        y, mask = real["bn_drop_fwd"](x, mean, invstd_or_var, gamma, beta, **kw)
        return y, _pack_gate(ref.act[layer_of_site[kw["site"]]] > 0)

    def own_pool_float64_argmax(buf, channel_offset, channels):
        out, arg = real["max_pool2x2_slice"](buf, channel_offset, channels)
        layer = next(n for n, y in ref.act.items() if y.shape == (buf.shape[0], channels) + tuple(buf.shape[2:]) and n.endswith(".4"))
        return out, _argmax_bytes(ref.act[layer]).to(torch.uint8).contiguous()

    bn = {"bn_stats": bn_stats, "bn_drop_fwd": bn_drop_fwd, "bn_drop_bwd": bn_drop_bwd}
    families = {
        "none (the own step)": {},
        "3x3 convolution, forward and data gradient": {"dconv3x3": conv},
        "weight and bias gradients": {"dconv3x3_wgrad": wgrad, "channel_sum": lambda x: x.sum((0, 2, 3))},
        "per-pixel product of the transposed convolution": {"conv1x1_f32": conv1x1},
        "BatchNorm + ReLU + dropout, statistics / forward / backward": bn,
        "max pooling": {"max_pool2x2_slice": pool},
        "weighted cross-entropy": {"weighted_ce_fwd": ce_fwd, "weighted_ce_bwd": ce_bwd},
        "all of the above": {"dconv3x3": conv, "dconv3x3_wgrad": wgrad, "channel_sum": lambda x: x.sum((0, 2, 3)), "conv1x1_f32": conv1x1,
                             "max_pool2x2_slice": pool, "weighted_ce_fwd": ce_fwd, "weighted_ce_bwd": ce_bwd, **bn},
        "own kernels, ReLU gates of the float64 model": {"bn_drop_fwd": own_fwd_float64_gates},
        "own kernels, gates and pooling argmaxes of the float64 model": {"bn_drop_fwd": own_fwd_float64_gates,
                                                                         "max_pool2x2_slice": own_pool_float64_argmax},
    }
    return families


def substitutions(kw, start_word, ref, lib):
    import sis_hip
    from updater.segmentation_updater import weighted_cross_entropy
    x, labels, wts = _batch()
    real = {name: getattr(sis_hip, name) for name in K.ENTRY_POINTS}
    emit(f"{'replaced by its fp32 torch equivalent':<62s} {'median':>9s} {'max':>9s}   (weight-gradient error of the step against float64)")
    for title, patch in _families(real, ref).items():
        sis_hip.dropout_seed(DEV).fill_(start_word)
        net = _net("base", **kw).to(DEV).train()
        try:
            for name, fn in patch.items():
                setattr(sis_hip, name, fn)
            weighted_cross_entropy(net(x), labels, wts).backward()
            torch.cuda.synchronize()
        finally:
            for name, fn in real.items():
                setattr(sis_hip, name, fn)
        med, lib_med, worst, lib_worst = _medians(net, ref, lib)
        emit(f"{title:<62s} {med:9.2e} {worst:9.2e}")
    emit(f"{'the fp32 library step (plain torch modules)':<62s} {lib_med:9.2e} {lib_worst:9.2e}")


def run(p):
    import sis_hip
    kw = {} if p > 0 else dict(encoder_dropout_prob=0.0, decoder_dropout_prob=0.0)
    emit("=" * 130)
    emit(f"DocUFCN('base'), B = 2, 64^2, dropout p = {p}")
    emit("=" * 130)
    net, x, labels, wts, calls = K.record_step("base", 2, 64, **kw)
    start_word = K.STEP_SEED_WORD
    seed = sis_hip.dropout_seed(DEV).item()
    fresh = _net("base", **kw)
    ref = Hooked(fresh, torch.float64, seed, x, labels, wts)
    lib = Hooked(fresh, torch.float32, seed, x, labels, wts)
    med, lib_med, worst, lib_worst = _medians(net, ref, lib)
    emit(f"logits: own {_rel(calls[[c.name for c in calls].index('weighted_ce_fwd')].args['logits'], ref.logits):.2e}, "
         f"library {_rel(lib.logits, ref.logits):.2e};  weight-gradient error, median (max): own {med:.2e} ({worst:.2e}), "
         f"library {lib_med:.2e} ({lib_worst:.2e})")
    emit()
    localisation_table(calls, ref, lib)
    emit()
    decisions(calls, ref, lib)
    emit()
    substitutions(kw, start_word, ref, lib)
    emit()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    for p in (0.4, 0.0):
        run(p)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
