"""float64 torch restatements for the GAN-training tests (tests/test_train_stylegan2_*.py, tests/test_gan_train_guard_bands_gpu.py):
the phase split, the composed downsampling weight and its adjoint, the two formulations of a discriminator downsampling layer, and
the error bound the polyphase route is held to."""
import torch
import torch.nn.functional as F

BLUR_1331 = [1.0, 3.0, 3.0, 1.0]


def fir_taps(k=BLUR_1331, dtype=torch.float64):
    """Normalised 2-D taps as ``networks.stylegan2.model.make_kernel`` builds them."""
    t = torch.tensor(k, dtype=dtype)
    t = torch.outer(t, t) if t.ndim == 1 else t
    return t / t.sum()


def ref_image_batch(images_u8, ids):
    """ToTensor + Normalize(0.5, 0.5) of the listed samples in float32: true divisions by 255 and by 0.5 (divisors as tensors, so
    that no reciprocal multiplication is substituted)."""
    x = images_u8[ids.long()].to(torch.float32)
    return x.div(torch.tensor(255.0)).sub(0.5).div(torch.tensor(0.5))


def ref_split(x):
    return F.pixel_unshuffle(x, 2)


def ref_merge(p):
    return F.pixel_shuffle(p, 2)


def ref_kernel6(w, f, scale):
    """K [Cout, Cin, 6, 6]: blur (a true convolution with f) followed by a correlation with scale * w, as one stride-2 kernel."""
    w, f = w.double(), f.double()
    k = w.new_zeros(w.shape[0], w.shape[1], 6, 6)
    for i in range(3):
        for j in range(3):
            for u in range(4):
                for v in range(4):
                    k[:, :, i + u, j + v] += w[:, :, i, j] * f[3 - u, 3 - v]
    return k * scale


def ref_compose(w, f, scale):
    """W' [Cout, 4 Cin, 3, 3]: W'[co, 4 ci + 2 py + px, a, b] = K[co, ci, 2 a + py, 2 b + px]."""
    co, ci = w.shape[:2]
    k = ref_kernel6(w, f, scale).view(co, ci, 3, 2, 3, 2)   # [co, ci, a, py, b, px]
    return k.permute(0, 1, 3, 5, 2, 4).reshape(co, 4 * ci, 3, 3)


def ref_compose_adjoint(g, f, scale):
    """dW [Cout, Cin, 3, 3] from dW' [Cout, 4 Cin, 3, 3]: the transpose of ``ref_compose``, written out (not by autograd)."""
    g, f = g.double(), f.double()
    co, ci = g.shape[0], g.shape[1] // 4
    k = g.view(co, ci, 2, 2, 3, 3).permute(0, 1, 4, 2, 5, 3).reshape(co, ci, 6, 6)   # [co, ci, (a, py), (b, px)]
    dw = g.new_zeros(co, ci, 3, 3)
    for i in range(3):
        for j in range(3):
            for u in range(4):
                for v in range(4):
                    dw[:, :, i, j] += k[:, :, i + u, j + v] * f[3 - u, 3 - v]
    return dw * scale


def blur_pad2(x, f):
    """``upfirdn2d(x, f, pad=(2, 2))`` restated: zero padding by 2, then a true convolution with f per channel."""
    c = x.shape[1]
    taps = torch.flip(f.to(x.dtype), [0, 1])[None, None].expand(c, 1, *f.shape).contiguous()
    return F.conv2d(F.pad(x, (2, 2, 2, 2)), taps, groups=c)


def library_down(x, w, f, scale):
    """The two-operator formulation every discriminator downsampling layer runs today: blur, then stride-2 conv2d."""
    return F.conv2d(blur_pad2(x, f), w * scale, stride=2)


def polyphase_down(x, w, f, scale, compose=ref_compose):
    return F.conv2d(ref_split(x), compose(w, f, scale).to(x.dtype), padding=1)


def first_and_second_order(fn, x, w, gy, probe_w):
    """(y, dx, dW, d2/dx, d2/dW, d2/dgy) of y = fn(x, w): first-order gradients against ``gy``; second-order gradients of
    |dx|^2 + <dW, probe_w> with respect to (x, w, gy) -- |dx|^2 is the R1 penalty's form, and it reaches W and gy only through the
    gradient-of-gradient path; <dW, probe_w> reaches x the same way."""
    x, w, gy = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True), gy.detach().clone().requires_grad_(True)
    y = fn(x, w)
    dx, dw = torch.autograd.grad(y, (x, w), gy, create_graph=True)
    second = torch.autograd.grad(dx.pow(2).sum() + (dw * probe_w).sum(), (x, w, gy))
    return (y.detach(), dx.detach(), dw.detach()) + tuple(t.detach() for t in second)


ORDER_NAMES = ("y", "dx", "dW", "d2/dx", "d2/dW", "d2/dgy")
CAP = 1e-4   # the project's cap for a Winograd result against float64: never allow more than CAP * max|ref|


def max_abs(a, b):
    d = (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()
    return d if d == d else float("inf")   # NaN never passes a bound


def winograd_bound(library_fp32, ref64):
    """What a Winograd result may differ from float64 by: 4 x the error the library's direct fp32 formulation makes on the same
    operands (the Winograd-over-direct factor of DESIGN.md §13.3), never above ``CAP * max|ref|``.  Returns (bound, library
    error)."""
    lib_err = max_abs(library_fp32, ref64)
    return min(4.0 * lib_err, CAP * ref64.detach().abs().max().item()), lib_err
