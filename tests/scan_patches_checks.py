"""What tests/test_scan_patches_gpu.py and tests/test_scan_patches_guard_bands_gpu.py share: the device calls of one case, run
through a ``run`` / ``put`` pair (direct, or between guard bands), compared byte for byte with Pillow itself."""
import numpy as np
import torch
from PIL import Image

import scan_patches_restatement as R


def pil_resize(a, size):
    return np.asarray(Image.fromarray(a).resize(size, Image.BICUBIC, reducing_gap=None))


def pil_thumbnail(a, s):
    image = Image.fromarray(a)
    image.thumbnail((s, s))
    return np.asarray(image)


def pil_patches(a, size):
    """The reference's crop_patches, restated on Pillow's crop with the float boxes."""
    import math
    image = Image.fromarray(a)
    nx, ny = math.ceil(image.width / size), math.ceil(image.height / size)
    ox, oy = (nx * size - image.width) / nx, (ny * size - image.height) / ny
    out = []
    for yi in range(ny):
        sy = yi * (size - oy)
        for xi in range(nx):
            sx = xi * (size - ox)
            out.append(np.asarray(image.crop((sx, sy, sx + size, sy + size))))
    return np.stack(out)


def same_bytes(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    differing = int((got != want).sum())
    assert differing == 0, f"{what}: {differing} of {want.size} bytes differ from Pillow"


def check_resample(run, put, shape, size, kind):
    import sis_hip
    a = R.page(shape[0], shape[1], kind)
    same_bytes(run(sis_hip.scan_resample, put(torch.from_numpy(a)), size), pil_resize(a, size), f"resample {shape} -> {size} {kind}")


def check_thumbnail(run, put, shape, s, kind):
    import sis_hip
    a = R.page(shape[0], shape[1], kind)
    same_bytes(run(sis_hip.scan_thumbnail, put(torch.from_numpy(a)), s), pil_thumbnail(a, s), f"thumbnail {shape} {s} {kind}")


def check_patches(run, put, shape, size):
    import sis_hip
    from utils.scan_patches import patch_origins
    a = R.page(shape[0], shape[1], "random")
    origins = patch_origins(shape[0], shape[1], size)
    same_bytes(run(sis_hip.scan_patches, put(torch.from_numpy(a)), origins, size), pil_patches(a, size), f"patches {shape} {size}")
