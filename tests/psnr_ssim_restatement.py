"""float64 numpy / scipy restatement of the definitions of DESIGN.md §15 (``sis_psnr_ssim``, ``sis_autoencoder_batch``), the same
metric as an ATen formulation (the way the reference's kornia call computes it: a 2-D Gaussian by grouped ``conv2d`` on a
reflect-padded input), and the inputs the tests share.  A restatement of the project's own statement, not of kornia or imgaug."""
import functools

import numpy as np

SIGMA = 1.5


# ------------------------------------------------------------------------------------------------------------ PSNR / SSIM

def gaussian_taps(window, sigma=SIGMA):
    k = np.arange(window, dtype=np.float64) - window // 2
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return g / g.sum()


def unnormalize(x, mode=0):
    """One sample, float64.  mode 0: by its minimum; 1: always; 2: never."""
    if mode == 1 or (mode == 0 and x.min() < 0):
        return (np.clip(x, -1.0, 1.0) + 1.0) / 2.0
    return x


def _filter(plane, taps):
    from scipy.ndimage import correlate1d
    return correlate1d(correlate1d(plane, taps, axis=-1, mode="mirror"), taps, axis=-2, mode="mirror")


def ssim_map(x, y, window, max_val=1.0):
    """[..., H, W] float64 twice (already unnormalised) -> the unclamped s."""
    taps = gaussian_taps(window)
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    mu_x, mu_y = _filter(x, taps), _filter(y, taps)
    var_x, var_y = _filter(x * x, taps) - mu_x * mu_x, _filter(y * y, taps) - mu_y * mu_y
    cov = _filter(x * y, taps) - mu_x * mu_y
    return ((2.0 * mu_x * mu_y + c1) * (2.0 * cov + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (var_x + var_y + c2))


def psnr_ssim(image, target, window=5, max_val=1.0, mode=0):
    """float32 / float64 [B, C, H, W] twice -> (psnr [B] in dB, ssim [B], s [B, C, H, W]), all float64."""
    image, target = np.asarray(image, dtype=np.float64), np.asarray(target, dtype=np.float64)
    psnr, ssim, maps = [], [], []
    for x, y in zip(image, target):
        x, y = unnormalize(x, mode), unnormalize(y, mode)
        mse = np.mean((x - y) ** 2)
        with np.errstate(divide="ignore"):
            psnr.append(10.0 * np.log10(max_val * max_val / mse) if mse > 0 else np.inf)
        s = ssim_map(x, y, window, max_val)
        maps.append(s)
        ssim.append(np.mean(np.clip(s, 0.0, 1.0)))
    return np.array(psnr), np.array(ssim), np.stack(maps)


def aten_psnr_ssim(image, target, window=5, max_val=1.0, mode=0):
    """The same metric in torch, in the tensors' dtype and on their device, every sample on its own as the reference scores it:
    reflect padding, ONE grouped conv2d per moment with the 2-D kernel outer(g, g), element-wise ops.  No host sync (the
    unnormalise decision is a ``where``).  -> (psnr [B], ssim [B], s [B, C, H, W])."""
    import torch
    import torch.nn.functional as F
    b, c, h, w = image.shape
    r = window // 2
    g = torch.from_numpy(gaussian_taps(window)).to(device=image.device, dtype=image.dtype)
    kernel = torch.outer(g, g).expand(c, 1, window, window).contiguous()

    def prepare(x):
        if mode == 2:
            return x
        mapped = (x.clamp(-1, 1) + 1) / 2
        return mapped if mode == 1 else torch.where(x.amin(dim=(1, 2, 3), keepdim=True) < 0, mapped, x)

    def blur(t):
        return F.conv2d(F.pad(t, (r, r, r, r), mode="reflect"), kernel, groups=c)

    x, y = prepare(image), prepare(target)
    c1, c2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    mu_x, mu_y = blur(x), blur(y)
    var_x, var_y, cov = blur(x * x) - mu_x * mu_x, blur(y * y) - mu_y * mu_y, blur(x * y) - mu_x * mu_y
    s = ((2 * mu_x * mu_y + c1) * (2 * cov + c2)) / ((mu_x * mu_x + mu_y * mu_y + c1) * (var_x + var_y + c2))
    mse = ((x - y) ** 2).mean(dim=(1, 2, 3))
    return 10 * torch.log10(max_val * max_val / mse), s.clamp(0, 1).mean(dim=(1, 2, 3)), s


# ---- inputs.  T stands for the kernel's tile edge (sis_hip.psnr_ssim_tile()).
SHAPES = [(1, 3, 3, 3, 5), (2, 1, 2, 2, 3), (2, 3, 7, 5, 5), (1, 3, 6, 9, 11), (3, 3, 33, 65, 5), (2, 3, "T+1", "2T+3", 11)]
CONTENTS = ["noisy", "smooth", "independent", "inverted", "identical", "constant_target", "mixed_range", "target_negative"]


def resolve_shape(shape, tile):
    sizes = {"T+1": tile + 1, "2T+3": 2 * tile + 3}
    return tuple(sizes.get(v, v) for v in shape)


@functools.lru_cache(maxsize=None)
def case(shape, content):
    """(image, target) float32 [B, C, H, W] numpy arrays of one (resolved) shape and content; seeded by both."""
    b, c, h, w, window = shape
    rng = np.random.default_rng([b, c, h, w, window, CONTENTS.index(content)])
    uniform = lambda: rng.random((b, c, h, w), dtype=np.float32)   # noqa: E731
    if content == "noisy":
        y = uniform()
        x = np.clip(y + 0.05 * rng.standard_normal(y.shape).astype(np.float32), 0, 1)
    elif content == "smooth":   # sigma^2 of a few 1e-4 from two means near 0.5: the cancellation-heavy case
        yy, xx = np.mgrid[0:h, 0:w]
        y = np.broadcast_to(0.5 + 0.3 * np.sin(0.23 * xx + 0.1) * np.cos(0.17 * yy), (b, c, h, w)).astype(np.float32)
        x = (y + 1e-3 * rng.standard_normal(y.shape)).astype(np.float32)
    elif content == "independent":   # the first draw with 10 % .. 90 % of its s negative (a 3 x 3 plane has ONE sign more often than not)
        while True:
            x, y = uniform(), uniform()
            if 0.10 <= (psnr_ssim(x, y, window=window)[2] < 0).mean() <= 0.90:
                break
    elif content == "inverted":
        x = uniform()
        y = 1 - x
    elif content == "identical":
        x = uniform()
        y = x.copy()
    elif content == "constant_target":
        x, y = uniform(), np.full((b, c, h, w), 0.3, dtype=np.float32)
    elif content == "mixed_range":   # even samples in [-1.2, 1.2] (both unnormalised, the clamp works), odd samples in [0, 1]
        x, y = uniform(), uniform()
        x[0::2], y[0::2] = 2.4 * x[0::2] - 1.2, 2.4 * y[0::2] - 1.2
        for sample in range(0, b, 2):
            x[sample].flat[0], y[sample].flat[0] = -1.2, -1.0   # negative, and x past the clamp, whatever the draw
    elif content == "target_negative":
        x, y = uniform(), 2 * uniform() - 1
        y.reshape(b, -1)[:, 0] = -0.5
    else:
        raise KeyError(content)
    return np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def reference(shape, content):
    """(psnr, ssim, s) of ``case`` by the restatement, computed once."""
    x, y = case(shape, content)
    return psnr_ssim(x, y, window=shape[4])


FLOOR, MARGIN = 2.0 ** -19, 4   # bound of a device result: max(MARGIN * E, FLOOR)


@functools.lru_cache(maxsize=None)
def aten_error(shape, content):
    """(E map, E ssim, E psnr in dB): max |float32 ATen formulation on the CPU - ref64| over the case."""
    import torch
    x, y = case(shape, content)
    psnr, ssim, s = reference(shape, content)
    a_psnr, a_ssim, a_s = aten_psnr_ssim(torch.from_numpy(x), torch.from_numpy(y), window=shape[4])
    finite = np.isfinite(psnr)
    e_psnr = np.abs(a_psnr.double().numpy()[finite] - psnr[finite]).max() if finite.any() else 0.0
    return float(np.abs(a_s.double().numpy() - s).max()), float(np.abs(a_ssim.double().numpy() - ssim).max()), float(e_psnr)


def bound(e):
    return max(MARGIN * e, FLOOR)


# ------------------------------------------------------------------------------------------------- denoising loader batch

def hash32(seed, component, pixel):
    """uint32 array: murmur3's finaliser on pixel * 0x9E3779B1 + (seed ^ component * 0x85EBCA77), all modulo 2^32."""
    with np.errstate(over="ignore"):
        key = np.uint32(int(seed) & 0xFFFFFFFF) ^ np.uint32((int(component) * 0x85EBCA77) & 0xFFFFFFFF)
        h = np.asarray(pixel, dtype=np.uint32) * np.uint32(0x9E3779B1) + key
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return h


def normal(seed, channel, n_pixels):
    """float64 [n_pixels]: Box-Muller on u1 = ((h(2 ch) >> 8) + 1) / 2^24 and u2 = (h(2 ch + 1) >> 8) / 2^24."""
    pixel = np.arange(n_pixels, dtype=np.uint32)
    u1 = ((hash32(seed, 2 * channel, pixel) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (hash32(seed, 2 * channel + 1, pixel) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def grey_levels(q):
    """[..., 3, H, W] integer levels -> L [..., H, W] = (19595 R + 38470 G + 7471 B + 32768) >> 16."""
    q = np.asarray(q, dtype=np.int64)
    return (19595 * q[..., 0, :, :] + 38470 * q[..., 1, :, :] + 7471 * q[..., 2, :, :] + 32768) >> 16


def encode(levels):
    """0..255 levels -> float32 (v / 255 - 0.5) / 0.5 with true float32 divisions (ToTensor, Normalize)."""
    v = np.asarray(levels, dtype=np.float32)
    return (v / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)


def decode(images):
    """float32 encodings -> integer levels."""
    return np.rint((np.asarray(images, dtype=np.float64) * 0.5 + 0.5) * 255.0).astype(np.int64)


def autoencoder_batch(images, ids, scale, per_channel, seed, grey, eps=2.0 ** -8):
    """images uint8 [N, 3, S, S]; ids, scale, per_channel, seed, grey sequences of length B ->
    (input levels int64 [B, 3, S, S], output levels, ambiguous bool [B, 3, S, S]).  ``ambiguous``: where an error of ``eps`` in
    the value before rounding could change the level (the value lies within eps of a half-integer; with grey, where the two
    candidate roundings of the pixel's channels give different L)."""
    images = np.asarray(images)
    size = images.shape[-1]
    levels, outputs, ambiguous = [], [], []
    for b, i in enumerate(ids):
        p = images[int(i)].astype(np.float64)
        z = np.stack([normal(seed[b], c if per_channel[b] else 0, size * size).reshape(size, size) for c in range(3)])
        v = p + float(scale[b]) * z
        q = np.clip(np.rint(v), 0, 255).astype(np.int64)
        lo = np.clip(np.rint(v - eps), 0, 255).astype(np.int64)
        hi = np.clip(np.rint(v + eps), 0, 255).astype(np.int64)
        if grey[b]:
            q = np.broadcast_to(grey_levels(q), q.shape)
            amb = np.broadcast_to(grey_levels(lo) != grey_levels(hi), q.shape)
        else:
            amb = lo != hi
        levels.append(q)
        outputs.append(images[int(i)].astype(np.int64))
        ambiguous.append(amb)
    return np.stack(levels), np.stack(outputs), np.stack(ambiguous)


# ---- inputs of the loader tests: (per_channel, grey) pairs at both sizes, every scale of the dataset once
NOISE_SIZES = (5, 8)
NOISE_FLAGS = [(0, 0), (1, 0), (0, 1), (1, 1)]
NOISE_IDS = [3, 0, 3]
NOISE_SCALES = [[5.0, 10.0, 15.0], [25.0, 35.0, 50.0]]


@functools.lru_cache(maxsize=None)
def noise_images(size):
    """uint8 [4, 3, S, S]: random images; image 3 has plateaux of 0 and 255 (the clip)."""
    rng = np.random.default_rng([size, 7])
    images = rng.integers(0, 256, (4, 3, size, size), dtype=np.uint8)
    images[3, :, : size // 2] = 0
    images[3, :, size // 2:, : size // 2] = 255
    return images


def noise_cases():
    """(size, per_channel, grey, scales [3], seeds [3]) for every case of the noise comparison."""
    out = []
    for size in NOISE_SIZES:
        for k, (per_channel, grey) in enumerate(NOISE_FLAGS):
            for j, scales in enumerate(NOISE_SCALES):
                seeds = [(0x9E3779B9 * (size + 13 * k + 101 * j + 7 * n + 1)) & 0xFFFFFFFF for n in range(3)]
                out.append((size, per_channel, grey, tuple(scales), tuple(seeds)))
    return out


STATISTICS_SEED = 0x5EED1234   # the statistics test: mid-grey 64 x 64, scale 50, per channel
