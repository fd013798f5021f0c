"""Generates tests/golden/reference_checks.npz: what the UNMODIFIED reference computes in the four CPU checks that used to
import it live (build container only; oracle/load_reference.py):

gen16_*        reference Generator(16, 64, 3, cm=1): state_dict names / shapes, and of the image and every activation on
               seeded state 99 / inputs 98, run under PINNED_ENV, the SHA-256 of the bytes plus a strided slice
               (tests/test_oracle_cpu.py::test_oracle_bit_identical_to_imported_reference)
k2_want<i>     the reference's own ``upfirdn2d_native`` (op/upfirdn2d.py:152-186, lifted with ``ast``) on K2_CASES, fp64
d<size>_<cm>_* reference Discriminator(size, cm): state_dict names / shapes (tests/test_gan_oracle_cpu.py)
cosine_lrs     the reference ``ClampedCosineAnnealingLR`` (utils/clamped_cosine.py:8-19, lifted with ``ast``) over 25
               steps of two parameter groups (tests/test_training_entry_cpu.py)

Before writing, the oracle is asserted bit-identical to the reference on gen16 under PINNED_ENV.

    python tests/golden/make_golden_reference_checks.py
"""
import ast
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "reference_checks.npz")

# Float kernels that round alike on every x86-64 host: oneDNN and ATen at their baseline ISA, MKL in its conditional
# numerical reproducibility mode, one thread.  Natively the generator's image moves by ~2e-6 between instruction sets and
# thread counts, so a bit-for-bit comparison with a stored result only means something under these settings.
PINNED_ENV = {"ONEDNN_MAX_CPU_ISA": "SSE41", "ATEN_CPU_CAPABILITY": "default", "MKL_CBWR": "COMPATIBLE", "OMP_NUM_THREADS": "1",
              "MKL_NUM_THREADS": "1"}
GEN16 = (16, 64, 3, 1)     # size, style_dim, n_mlp, channel_multiplier
GEN16_SEEDS = (99, 98)     # state, inputs
GEN16_BATCH = 3
K2_CASES = [(3, 9, 7, 1, 4, 4, 1, 1, 1, 1), (2, 5, 6, 2, 4, 4, 2, 1, 2, 1), (2, 8, 9, 1, 4, 4, 1, 2, 1, 1),
            (1, 6, 5, 3, 3, 2, 2, 2, 1, -1), (2, 4, 4, 1, 2, 2, 2, 1, 1, 0)]
DISCRIMINATORS = [(32, 1), (128, 2)]
SHAPE_WIDTH = 6
COSINE = dict(lrs=(0.009, 0.018), t_max=15, eta_min=1e-8, steps=25)


def k2_inputs():
    """Inputs of K2_CASES from one frozen RandomState stream, in order."""
    rng = np.random.RandomState(77)
    return [(rng.standard_normal((major, ih, iw, minor)), rng.standard_normal((kh, kw)))
            for major, ih, iw, minor, kh, kw, *_ in K2_CASES]


def gen16_forward(use_reference):
    """(image, {index: activation}) of Generator GEN16 on GEN16_SEEDS: the reference module or the functional oracle."""
    from oracle import stylegan2_ref as R
    torch.set_num_threads(1)
    size, sdim, n_mlp, cm = GEN16
    sd = R.seeded_state_dict(size, sdim, n_mlp, cm, seed=GEN16_SEEDS[0])
    z, noise = R.seeded_inputs(size, GEN16_BATCH, sdim, seed=GEN16_SEEDS[1])
    with torch.no_grad():
        if use_reference:
            from oracle import load_reference
            g = load_reference.load_reference_stylegan2().Generator(size, sdim, n_mlp, channel_multiplier=cm).eval()
            g.load_state_dict(sd, strict=True)
            return g([z], noise=noise, return_intermediate_activations=True)
        return R.generator_forward(sd, [z], noise=noise, return_intermediate_activations=True)


def pinned_gen16(use_reference):
    """gen16_forward in a child process under PINNED_ENV, as {"image": ..., "act<k>": ...} numpy arrays."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "gen16.npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--gen16", "reference" if use_reference else "oracle", path],
                       env=dict(os.environ, **PINNED_ENV), check=True, timeout=600)
        with np.load(path) as f:
            return {k: f[k] for k in f.files}


def _write_gen16(which, path):
    img, acts = gen16_forward(which == "reference")
    np.savez(path, image=img.numpy(), **{f"act{k}": v.numpy() for k, v in acts.items()})


def digest(a):
    """SHA-256 of an array's dtype, shape and bytes (C order)."""
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()


def strided_slice(a):
    """A few hundred elements of an NCHW array, for a readable message when the digests differ."""
    return a[:, ::max(1, a.shape[1] // 8), ::4, ::4]


def names_and_shapes(module):
    """state_dict names, and shapes as rows padded with -1 to SHAPE_WIDTH."""
    sd = module.state_dict()
    return np.array(list(sd.keys())), np.array([list(v.shape) + [-1] * (SHAPE_WIDTH - v.dim()) for v in sd.values()], dtype=np.int64)


def reference_cosine_lrs():
    from oracle.load_reference import REFERENCE_ROOT
    from torch import nn
    from torch.optim.lr_scheduler import CosineAnnealingLR
    path = os.path.join(REFERENCE_ROOT, "utils", "clamped_cosine.py")
    node = next(n for n in ast.parse(open(path).read()).body if isinstance(n, ast.ClassDef) and n.name == "ClampedCosineAnnealingLR")

    class Base(CosineAnnealingLR):  # the reference forwards ``verbose`` (torch 1.9); torch >= 2.7 dropped the argument
        def __init__(self, optimizer, T_max, eta_min=0, last_epoch=-1, verbose=False):
            super().__init__(optimizer, T_max, eta_min, last_epoch)

    scope = {"CosineAnnealingLR": Base}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), scope)
    opt = torch.optim.SGD([{"params": [nn.Parameter(torch.zeros(1))], "lr": lr} for lr in COSINE["lrs"]], lr=0.1, momentum=0.9)
    sched = scope["ClampedCosineAnnealingLR"](opt, COSINE["t_max"], eta_min=COSINE["eta_min"])
    lrs = []
    for _ in range(COSINE["steps"]):
        opt.step(), sched.step()
        lrs.append([g["lr"] for g in opt.param_groups])
    return np.array(lrs, dtype=np.float64)


def main():
    from oracle import load_reference
    assert load_reference.reference_available(), "run in the build container (needs the reference tree)"
    ref = load_reference.load_reference_stylegan2()
    out = {}
    names, shapes = names_and_shapes(ref.Generator(*GEN16[:3], channel_multiplier=GEN16[3]))
    out["gen16_names"], out["gen16_shapes"] = names, shapes
    want, mine = pinned_gen16(True), pinned_gen16(False)
    assert sorted(want) == sorted(mine) and all(np.array_equal(want[k], mine[k]) for k in want), "oracle != reference"
    for k, v in want.items():
        out[f"gen16_{k}_sha256"], out[f"gen16_{k}_slice"] = np.array(digest(v)), strided_slice(v)
    native = load_reference.load_reference_upfirdn2d_native()
    for i, ((x, k), (_, _, _, _, _, _, up, down, p0, p1)) in enumerate(zip(k2_inputs(), K2_CASES)):
        out[f"k2_want{i}"] = native(torch.from_numpy(x), torch.from_numpy(k), up, up, down, down, p0, p1, p0, p1).numpy()
    for size, cm in DISCRIMINATORS:
        out[f"d{size}_{cm}_names"], out[f"d{size}_{cm}_shapes"] = names_and_shapes(ref.Discriminator(size, channel_multiplier=cm))
    out["cosine_lrs"] = reference_cosine_lrs()
    np.savez_compressed(OUT, **out)
    print(f"wrote {os.path.relpath(OUT, ROOT)}: {sorted(out)}")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--gen16":
        _write_gen16(sys.argv[2], sys.argv[3])
    else:
        main()
