"""GPU: ``sis_hip.seg_eval`` (csrc/seg_eval.h) against the float64 restatement tests/seg_eval_restatement.py.

Launch geometry the shapes are chosen from: a workgroup is 256 lanes, a lane takes four consecutive pixels of one image at a time,
so a workgroup covers 1024 pixels per round; a launch has at most 512 workgroups, beyond 512 x 1024 pixels they walk with the
grid's stride.  Planes whose size is a multiple of 4 take 16-byte loads, all others element loads.
  * 2 x 33 x 37: 1221 pixels per image (odd: element loads, label rows off 16-byte alignment), 612 lanes of work = two full
    workgroups and a third with 100 lanes;  3 x 20 x 36: the same with 16-byte loads (540 lanes);
  * 3 x 419 x 419 and 2 x 512 x 520: more than 524 288 pixels, the grid-stride rounds, on either load path.

``N_THREAD`` = 0: a lane adds every term in double (the kernel keeps no float32 partial sum), so the bound on ``sums`` is
8 * 2^-24 * sum |term| per entry: expf, log1pf, the division and the subtractions at 2 ulp each (the device library documents
expf and log1pf at 1 ulp; the kernel uses these, not the fast intrinsics).  The same bound holds on the interpolated route with
general scales, although the float64 reference does not round the interpolated values to float32 as the device does.
"""
import ctypes

import numpy as np
import pytest
import torch

import seg_eval_restatement as R

pytestmark = pytest.mark.gpu

N_THREAD = 0
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}
MULTI_WORKGROUP = [(2, 33, 37), (3, 20, 36)]
GRID_STRIDE = [(3, 419, 419), (2, 512, 520)]


def _device_state(dev, logits, labels, dtype="f32", size=None, counts=None, sums=None):
    import sis_hip
    x = torch.from_numpy(np.ascontiguousarray(logits)).to(dev).to(TORCH_DTYPE[dtype])
    lab = torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    counts, sums = sis_hip.seg_eval(x, lab, size=size, counts=counts, sums=sums)
    return counts, sums


def _check(dev, logits, labels, dtype="f32", size=None, exact=True):
    """``exact``: the values the device sees are exact in float32 (full size, or a power-of-two scale on small integers): no
    pixel is undecided.  The bound on the sums is the same either way."""
    ref = R.reference(logits, labels, size)
    counts, sums = _device_state(dev, logits, labels, dtype, size)
    counts, sums = counts.cpu().numpy(), sums.cpu().numpy()
    undecided = R.check_counts(counts, ref, labels, exact=exact)
    err, bound = np.abs(sums - ref.sums), R.sums_bound(ref, N_THREAD)
    print(f"{dtype} {tuple(logits.shape)} -> {tuple(labels.shape)}: undecided {undecided}, max err / bound "
          f"{np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.isfinite(sums).all() and (err <= bound).all(), (err, bound)
    return ref, counts, sums


def _full_case(rng, shape, classes, dtype):
    b, h, w = shape
    logits = R.tie_logits(rng, (b, classes, h, w))   # small integers: exact in bf16 as well
    return logits, R.labels_with_ignored(rng, shape, classes)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("classes", R.CLASS_COUNTS)
def test_full_resolution_counts_are_exact(device, classes, dtype):
    rng = np.random.default_rng(100 * classes + (dtype == "bf16"))
    ignored = 0
    for shape in R.FULL_SHAPES + MULTI_WORKGROUP:
        logits, labels = _full_case(rng, shape, classes, dtype)
        ref, counts, _ = _check(device, logits, labels, dtype)
        ties = (np.sort(ref.values, axis=1)[:, -1] == np.sort(ref.values, axis=1)[:, -2]).mean()
        assert shape[1] * shape[2] < 64 or ties > 0.05        # the first maximal class is decided by ties, not by luck
        ignored += counts[-1]
    assert ignored > 0


@pytest.mark.parametrize("shape,dtype", [(GRID_STRIDE[0], "bf16"), (GRID_STRIDE[1], "f32")], ids=["odd-bf16", "aligned-f32"])
def test_full_resolution_grid_stride(device, shape, dtype):
    rng = np.random.default_rng(7)
    assert shape[0] * shape[1] * shape[2] > 512 * 1024
    logits, labels = _full_case(rng, shape, 2, dtype)
    _check(device, logits, labels, dtype)


def test_full_resolution_standard_normal_sums(device):
    """General float logits (no ties to speak of): the sums against float64, both dtypes, 4 and 16 classes."""
    rng = np.random.default_rng(3)
    for classes in (4, 16):
        for dtype in ("f32", "bf16"):
            logits = rng.standard_normal((2, classes, 33, 37)).astype(np.float32)
            if dtype == "bf16":
                logits = R.to_bf16_values(logits)
            _check(device, logits, R.labels_with_ignored(rng, (2, 33, 37), classes), dtype)


def test_accumulation_and_determinism(device):
    rng = np.random.default_rng(11)
    a = (rng.standard_normal((2, 5, 33, 37)).astype(np.float32), R.labels_with_ignored(rng, (2, 33, 37), 5))
    b = (rng.standard_normal((3, 5, 5, 7)).astype(np.float32), R.labels_with_ignored(rng, (3, 5, 7), 5))
    ca, sa = _device_state(device, *a)
    cb, sb = _device_state(device, *b)
    counts, sums = _device_state(device, *a)
    assert torch.equal(counts, ca) and torch.equal(sums, sa)                    # the same call twice: the same bits
    c2, s2 = _device_state(device, *b, counts=counts, sums=sums)                # ... and a second call on that state
    assert c2 is counts and s2 is sums
    assert torch.equal(counts, ca + cb) and torch.equal(sums, sa + sb)


@pytest.mark.parametrize("classes", [2, 3, 4, 7, 16])
@pytest.mark.parametrize("scale", R.EXACT_SCALES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_low_resolution_exact_scales(device, scale, classes):
    """Power-of-two scales and small-integer logits: every interpolated value is exact in float32, so nothing is undecided and
    ties that only arise BETWEEN source pixels go to the first class on the device as in float64."""
    (h, w), (oh, ow) = scale
    rng = np.random.default_rng(classes * 1000 + h * 10 + oh)
    logits = R.tie_logits(rng, (3, classes, h, w))
    labels = R.labels_with_ignored(rng, (3, oh, ow), classes)
    ref, _, _ = _check(device, logits, labels, size=(oh, ow), exact=True)
    between = np.zeros((oh, ow), dtype=bool)
    between[[y for y in range(oh) if (y * (h - 1)) % (oh - 1)], :] = True
    top = np.sort(ref.values, axis=1)
    assert ((top[:, -1] == top[:, -2]) & between[None]).any()


@pytest.mark.parametrize("scale", R.GENERAL_SCALES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_low_resolution_general_scales(device, scale):
    (h, w), (oh, ow) = scale
    rng = np.random.default_rng(0)
    batch = 1 if oh * ow > 4096 else 2
    logits = rng.standard_normal((batch, 4, h, w)).astype(np.float32)
    labels = R.labels_with_ignored(rng, (batch, oh, ow), 4)
    ref = R.reference(logits, labels, (oh, ow))
    assert ref.undecided.sum() * 1000 <= ref.undecided.size      # a condition on the input, not a measurement
    _check(device, logits, labels, size=(oh, ow), exact=False)


def test_saturated_softmax(device):
    """Logits of magnitude 30: the softmax saturates, -log p[label] is either ~60 or ~1e-26, and nothing cancels."""
    rng = np.random.default_rng(5)
    winner = rng.integers(0, 4, size=(2, 1, 17, 9))
    logits = (np.where(np.arange(4).reshape(1, 4, 1, 1) == winner, 30.0, -30.0) + rng.standard_normal((2, 4, 17, 9))).astype(np.float32)
    labels = R.labels_with_ignored(rng, (2, 17, 9), 4)
    ref, _, sums = _check(device, logits, labels)
    assert ref.sums[0] > 30 and np.isfinite(sums).all()
    agree = np.where((labels >= 0) & (labels < 4), winner[:, 0], labels)         # every label the argmax: ce is tiny, not 0 - 0
    ref, _, sums = _check(device, logits, agree)
    assert 0 < ref.sums[0] < 1e-20 and sums[0] > 0
    low = (30 * rng.choice([-1.0, 1.0], size=(2, 4, 3, 5))).astype(np.float32)   # exact at the power-of-two scale 3x5 -> 9x9
    _check(device, low, R.labels_with_ignored(rng, (2, 9, 9), 4), size=(9, 9), exact=True)


def test_every_label_ignored(device):
    from training.validation import scores_from_state
    rng = np.random.default_rng(9)
    logits = rng.standard_normal((3, 4, 5, 7)).astype(np.float32)
    labels = np.array(R.ODD_LABELS + (4,), dtype=np.int64)[rng.integers(0, 4, size=(3, 5, 7))]
    ref, counts, sums = _check(device, logits, labels)
    assert counts[:16].sum() == 0 and counts[16] == 0 and counts[17] == 105 and sums[0] == 0
    assert all(sums[3 + 3 * c] == 0 and sums[1 + 3 * c] == 0 and sums[2 + 3 * c] > 0 for c in range(4))
    scores = scores_from_state(counts, sums, ["background", "printed_text", "handwritten_text", "stamp"])
    assert scores["ce"] == 0.0 and scores["counted"] == 0 and scores["ignored"] == 105
    assert all(np.isfinite(v) for v in scores.values())


def test_wrapper_refuses_with_the_offending_value(device):
    import sis_hip
    x = torch.zeros((2, 4, 8, 8), device=device)
    lab = torch.zeros((2, 8, 8), dtype=torch.int64, device=device)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        sis_hip.seg_eval(x.cpu(), lab)
    with pytest.raises(RuntimeError, match="torch.float16"):
        sis_hip.seg_eval(x.half(), lab)
    with pytest.raises(RuntimeError, match="torch.int32"):
        sis_hip.seg_eval(x, lab.int())
    with pytest.raises(RuntimeError, match=r"\(2, 8, 9\)"):
        sis_hip.seg_eval(x, torch.zeros((2, 8, 9), dtype=torch.int64, device=device), size=(8, 8))
    with pytest.raises(RuntimeError, match=r"\(17,\)"):
        sis_hip.seg_eval(x, lab, counts=torch.zeros(17, dtype=torch.int64, device=device))
    with pytest.raises(RuntimeError, match="2..16"):
        sis_hip.seg_eval(torch.zeros((2, 17, 8, 8), device=device), lab)
    with pytest.raises(RuntimeError, match="bfloat16 at the size of the labels"):
        sis_hip.seg_eval(x[:, :, :4, :4].bfloat16(), lab)
    counts, sums = sis_hip.seg_eval(x, lab[:, None])          # [B, 1, H, W] labels
    assert counts[0].item() == 128 and counts[16].item() == 128


def test_entry_declines_and_touches_nothing(device):
    """classes 1 and 17, bf16 on the interpolated route, h > out_h, each null pointer: an error code, no launch -- state and
    workspace keep the 0xA5 bytes they were filled with."""
    import sis_hip
    L = sis_hip.lib()
    fill = lambda n, dtype: torch.full((n * torch.empty((), dtype=dtype).element_size(),), 0xA5, dtype=torch.uint8,   # noqa: E731
                                       device=device).view(dtype)
    counts, sums, ws = fill(16 * 16 + 2, torch.int64), fill(1 + 3 * 16, torch.float64), fill(4096, torch.float64)
    x = torch.zeros((2, 17, 8, 8), device=device)
    xb = x.bfloat16()
    lab = torch.zeros((2, 8, 8), dtype=torch.int64, device=device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    good = dict(counts=p(counts), sums=p(sums), ws=p(ws), logits=p(x), dtype=sis_hip.F32, labels=p(lab), b=2, c=4, h=8, w=8, oh=8, ow=8)

    def call(**changes):
        a = {**good, **changes}
        return L.sis_seg_eval(a["counts"], a["sums"], a["ws"], a["logits"], a["dtype"], a["labels"], a["b"], a["c"], a["h"], a["w"],
                              a["oh"], a["ow"], None)

    declined = [dict(c=1), dict(c=17), dict(logits=p(xb), dtype=sis_hip.BF16, h=4, w=4), dict(h=9), dict(w=9), dict(dtype=sis_hip.F16),
                dict(counts=None), dict(sums=None), dict(ws=None), dict(logits=None), dict(labels=None), dict(oh=0), dict(b=0)]
    for changes in declined:
        assert call(**changes) != 0, changes
        assert L.sis_last_error().decode().startswith("sis_seg_eval"), changes
    assert L.sis_seg_eval_workspace_bytes(2, 1, 8, 8) == 0 and L.sis_seg_eval_workspace_bytes(2, 17, 8, 8) == 0
    assert L.sis_seg_eval_workspace_bytes(2, 4, 8, 8) == 13 * 8
    torch.cuda.synchronize()
    for t in (counts, sums, ws):
        assert bool((t.view(torch.uint8) == 0xA5).all())
    assert call() == 0        # the same arguments unchanged are accepted
    torch.cuda.synchronize()
    assert not bool((counts.view(torch.uint8)[:18 * 8] == 0xA5).all())
