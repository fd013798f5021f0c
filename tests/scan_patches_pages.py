"""Three synthetic pages for the end-to-end runs of scripts/create_stylegan_train_dataset.py: 700 x 500 (shrunk to --max-size
first), 300 x 1200 (tall) and 130 x 97 (smaller than --max-size; one side below two windows), in two directories."""
import numpy as np
from PIL import Image

TOOL_OPTIONS = ["--image-size", "64", "--min-size", "100", "--max-size", "300"]
PAGES = [("a/wide.png", 700, 500), ("a/b/tall.png", 300, 1200), ("small.png", 130, 97)]


def synthetic_page(width, height, seed):
    """Text-like dark strokes on a light, slowly varying ground."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    ground = 215 + 25 * np.sin(x / 37.0) * np.cos(y / 53.0)
    a = np.repeat(ground[:, :, None], 3, axis=2) + rng.normal(0, 4, (height, width, 3))
    for _ in range(max(4, width * height // 2500)):
        x0, y0 = int(rng.integers(0, width)), int(rng.integers(0, height))
        a[y0:y0 + int(rng.integers(1, 4)), x0:x0 + int(rng.integers(3, 40))] = rng.integers(0, 70)
    return np.clip(a, 0, 255).astype(np.uint8)


def write_pages(root):
    for seed, (name, width, height) in enumerate(PAGES):
        path = root / name
        path.parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(synthetic_page(width, height, seed)).save(path)
    (root / "notes.txt").write_text("not an image")
    return root
