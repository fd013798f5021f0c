"""Python restatement of the launch plans of the fp32 matrix-core convolutions, for tests that must know which kernel form,
tile and K split a shape reaches.  Nothing of the package is imported; each function names the lines it restates
(paths below synthesis-in-style_amd/csrc).  tests/test_conv_f32_exact_cpu.py holds every case of
tests/conv_f32_exact_cases.py to the route it claims, tests/test_conv_f32_exact_gpu.py holds this file to what the library
lets one observe (kernel names, eligibility, workspace sizes).

Route values of the plain Winograd forward (``sis_conv3x3``) that no shape reaches, and why:

* ``XI`` in {4, 8} (xt > 512) on the pipelined kernel: its LDS image ``lds2`` = 132 352 + 64 xt + 256 nb bytes must stay within
  160 KB, i.e. xt <= 492 - 4 nb.  The tile shapes whose xt = nb (th + 2)(tw + 8) lies in [256, 488] are 16 x 16 x 1 sample
  (432), 8 x 16 x 2 samples (480) and the tiles that a small batch cuts short (e.g. 2 x 8 x 4 samples: 256); larger xt run on
  the first kernel, which takes xt as a run-time argument.
* ``tpw`` in {8, 16}: the pipelined kernel's smallest tile that is eligible (10 x 12 pixels of a 16 x 16 tile, 16 channels)
  needs 8 192 / 16 384 tiles, 63 / 126 MB of input; the cases stop at ``tpw`` = 4 (31 MB).
* ``xcd_group`` = 1 with ``tpw`` > 1: not excluded by the plan, but it needs >= 2048 workgroups of two or more output-channel
  blocks: outputs of 128+ channels on 1024+ tiles (>= 80 MB).
"""

WORKSPACE_BYTES = 128 << 20      # sis_hip.WORKSPACE_BYTES (SIS_WORKSPACE_MB unset)
JOBS_MAX = 16                    # sis_common.h:52 SIS_JOBS_MAX


def cdiv(a, b):
    return -(-a // b)


def ilog2_ceil(v):               # modconv_common.h:49
    l = 0
    while (1 << l) < v:
        l += 1
    return l


def run_jobs(n_jobs, fits):
    """sis_common.h:58 sis_run_jobs: the launches [(first, n)] of ``n_jobs`` queued layers."""
    out, first = [], 0
    while first < n_jobs:
        n = min(n_jobs - first, JOBS_MAX)
        while n > 1 and not fits(n):
            n = (n + 1) // 2
        out.append((first, n))
        first += n
    return out


# ------------------------------------------------------------------------------------------ Winograd F(2x2,3x3) forward

WCC, WMBLK, WTILES, WNTHR = 8, 64, 64, 512     # modconv_wino.hip:36,41,42,201
LDS_LIMIT = 160 * 1024


def wino_forward_plan(batch, cin, cout, h, w, workspace_bytes=WORKSPACE_BYTES):
    """None when ``sis_conv3x3`` declines the shape, else the plan as a dict.  Restates conv3x3_plan (modconv_entries.hip:55-62),
    mc_wino_tiles / mc_add_class (modconv_common.h:70-91,107-112), mc_plan_splitk (modconv_common.h:117-131) and
    modconv_wino_launch (modconv_wino.hip:993-1046) for p.s == nullptr."""
    if min(batch, cin, cout, h, w) <= 0 or batch * max(cin, cout) * h * w >= 1 << 31:
        return None
    if w % 4 or h % 2 or cin % 8 or cout % 4:
        return None
    # mc_add_class(p, 256, 2, B, 0, H, 0, W, 16, 16)
    twl = min(ilog2_ceil(w), ilog2_ceil(16))
    thl = min(ilog2_ceil(h), 8 - twl)
    nb = min(256 >> (thl + twl), 16, batch)
    th, tw = 1 << thl, 1 << twl
    nth, ntw = cdiv(h, th), cdiv(w, tw)
    npos_tiles = nth * ntw * cdiv(batch, nb)
    xt = nb * (th + 2) * (tw + 8)                                   # mc_wino_tiles: rows padded by 4 left and right
    if thl < 1 or twl < 2 or xt > WNTHR * 4:                        # modconv_wino.hip:998
        return None
    # mc_plan_splitk(p, WMBLK, WCC, 256, 384, ...)
    blocks = npos_tiles * cdiv(cout, WMBLK)
    ksplit, kchunk = 1, cin
    if not (blocks >= 256 or cin < 4 * WCC or not workspace_bytes):
        want = min(cdiv(384, blocks), cin // (2 * WCC))
        out_bytes = batch * cout * h * w * 4
        if want * out_bytes > workspace_bytes:
            want = workspace_bytes // out_bytes
        if want >= 2:
            kchunk = cdiv(cdiv(cin, want), WCC) * WCC
            ksplit = cdiv(cin, kchunk)
    lds = (2 * WCC * 16 * WMBLK + 2 * WCC * xt) * 4
    lds2 = lds + (2 * 16 * WCC * WTILES + nb * WMBLK + WMBLK + WTILES * 4) * 4
    if lds > LDS_LIMIT:
        return None
    plan = dict(th=th, tw=tw, nb=nb, xt=xt, npos_tiles=npos_tiles, blocks=blocks, ksplit=ksplit, kchunk=kchunk, lds=lds, lds2=lds2)
    if lds2 <= LDS_LIMIT and xt >= 256:                             # modconv_wino.hip:1014
        tpw = 1
        while kchunk % (2 * WCC) == 0 and tpw * 2 <= 16 and npos_tiles % (tpw * 2) == 0 and blocks // (tpw * 2) >= 1024:
            tpw *= 2
        grid = blocks // tpw
        n_co = cdiv(cout, WMBLK)
        xcd_group = int(cin * cout * 16 * 4 <= 5 * 1048576 and n_co > 1 and grid % (8 * n_co) == 0)
        xi = 1 if xt <= 256 else 2 if xt <= 512 else 4 if xt <= 1024 else 8
        plan.update(kernel="modconv_wino2_kernel", xi=xi, tpw=tpw, xcd_group=xcd_group, grid=grid)
    else:
        plan.update(kernel="modconv_wino_kernel", xi=None, tpw=1, xcd_group=0, grid=blocks)
    return plan


def wino_forward_eligible(batch, cin, cout, h, w):
    """sis_conv3x3_eligible (modconv_entries.hip:86-90): the plan without a workspace (the K split rejects nothing)."""
    return wino_forward_plan(batch, cin, cout, h, w, 0) is not None


def wino_forward_route(batch, cin, cout, h, w):
    """What a case claims: the kernel form and every plan property that selects other code in it."""
    p = wino_forward_plan(batch, cin, cout, h, w)
    if p is None:
        return None
    if p["ksplit"] == 1:
        split = "none"
    else:
        split = "even" if cin % p["kchunk"] == 0 else "uneven"
    return dict(kernel=p["kernel"], xi=p["xi"], ksplit=p["ksplit"], split=split, tpw=p["tpw"], xcd_group=p["xcd_group"],
                partial_rows=h % p["th"] != 0, partial_cols=w % p["tw"] != 0, short_batch_tile=batch % p["nb"] != 0,
                partial_co=cout % WMBLK != 0, co_blocks=min(cdiv(cout, WMBLK), 2), tile=(p["th"], p["tw"]))


# ------------------------------------------------------------------------------------------ Winograd weight gradient

GK, GBLK = 8, 64                 # conv_wgrad_wino.hip:31,32
WGRAD_TARGET_WGS = 256           # conv_wgrad_wino.hip:333 (SIS_WGRAD_WGS unset)


def wino_wgrad_plan(batch, cin, cout, h, w, workspace_bytes=WORKSPACE_BYTES, jobs=1):
    """wgrad_plan (conv_wgrad_wino.hip:317-343) and the reduce rule of gw_jobs (:384): None when not eligible."""
    workspace_bytes //= jobs
    if min(batch, cin, cout, h, w) <= 0 or h % 2 or w % 2 or cin % GBLK or cout % GBLK:
        return None
    tiles = batch * (h // 2) * (w // 2)
    if tiles % GK or batch * max(cin, cout) * h * w >= 1 << 29 or tiles >= 1 << 24:
        return None
    chunks_total = tiles // GK
    blocks = (cin // GBLK) * (cout // GBLK) * jobs
    slab_bytes = 16 * cin * cout * 4
    want = cdiv(WGRAD_TARGET_WGS, blocks)
    while want > 1 and want * blocks > WGRAD_TARGET_WGS:
        want -= 1
    want = max(min(want, chunks_total // 4), 1)
    if want * slab_bytes > workspace_bytes:
        want = workspace_bytes // slab_bytes
    if want < 1:
        return None
    cps = cdiv(chunks_total, want)
    ksplit = cdiv(chunks_total, cps)
    slices = [min(cps, chunks_total - s * cps) for s in range(ksplit)]
    return dict(chunks_total=chunks_total, chunks_per_slice=cps, ksplit=ksplit, slices=slices, reduce=ksplit > 4,
                tiles_per_row=w // 2, tiles_per_sample=(h // 2) * (w // 2), tiles=tiles, ci_blocks=cin // GBLK, co_blocks=cout // GBLK)


def wino_wgrad_launches(n_jobs, batch, cin, cout, h, w, workspace_bytes=WORKSPACE_BYTES):
    """sis_conv3x3_wgrad_multi (conv_wgrad_wino.hip:399-408): [(first, n, plan of that launch)]; every layer of a launch has
    workspace_bytes / n for its slabs."""
    fits = lambda n: wino_wgrad_plan(batch, cin, cout, h, w, workspace_bytes, n) is not None
    return [(first, n, wino_wgrad_plan(batch, cin, cout, h, w, workspace_bytes, n)) for first, n in run_jobs(n_jobs, fits)]


def _is_pow2(v):
    return v & (v - 1) == 0


def wino_wgrad_route(batch, cin, cout, h, w):
    p = wino_wgrad_plan(batch, cin, cout, h, w)
    if p is None:
        return None
    return dict(chunks=min(p["chunks_total"], 4), slices=p["slices"], last_slice=min(p["slices"][-1], 4), reduce=p["reduce"],
                ksplit=p["ksplit"], tiles_per_row=p["tiles_per_row"], tiles_per_sample=p["tiles_per_sample"],
                odd_divisors=(not _is_pow2(p["tiles_per_row"]), not _is_pow2(p["tiles_per_sample"])),
                w2=w == 2, h2=h == 2, chunk_crosses_samples=p["tiles_per_sample"] % GK != 0 and batch > 1,
                ci_blocks=min(p["ci_blocks"], 2), co_blocks=min(p["co_blocks"], 2))


def tile_split(t, tiles_per_sample, tiles_per_row, correct=True, quotient=None):
    """The kernel's split of a flat tile index into (sample, tile row, tile column) (conv_wgrad_wino.hip:69,81-84): float
    reciprocals in fp32, truncation, ONE correction step each.  ``quotient``: what stands in for the truncation of the float
    quotient (the sensitivity check rounds it up); ``correct`` = False leaves the correction steps out."""
    import numpy as np
    f = np.float32
    trunc = quotient or (lambda q: int(q))
    inv_tps, inv_tpr = f(1) / f(tiles_per_sample), f(1) / f(tiles_per_row)
    b = trunc(f(t) * inv_tps)
    rem = t - b * tiles_per_sample
    if correct:
        if rem < 0:
            b, rem = b - 1, rem + tiles_per_sample
        elif rem >= tiles_per_sample:
            b, rem = b + 1, rem - tiles_per_sample
    ty = trunc(f(rem) * inv_tpr)
    tx = rem - ty * tiles_per_row
    if correct:
        if tx < 0:
            ty, tx = ty - 1, tx + tiles_per_row
        elif tx >= tiles_per_row:
            ty, tx = ty + 1, tx - tiles_per_row
    return b, ty, tx


# ------------------------------------------------------------------------------------------ pointwise forward / data gradient

PW_MIN_TILES = 256               # conv1x1_f32.hip:245 (SIS_PW_MIN_TILES unset)
PW_KC = 16                       # conv1x1_f32.hip:278 (SIS_PW_KC unset)
PW_TILES = [(128, 256), (128, 128), (64, 256), (64, 128)]


def pw_ok(k, m, hw):             # conv1x1_f32.hip:235
    return k > 0 and m > 0 and hw > 0 and k % 32 == 0 and m % 4 == 0 and hw % 4 == 0


def pointwise_supported(cin, cout, hw):     # conv1x1_f32.hip:259: both directions
    return pw_ok(cin, cout, hw) and pw_ok(cout, cin, hw)


def pointwise_plan(batch, cin, cout, hw, data_gradient=False):
    """dispatch_pw (conv1x1_f32.hip:238-255) behind conv1x1_impl (:261-280): M = output channels of the launch, K = its
    contraction; the first tile of 128x256, 128x128, 64x256, 64x128 (channels x pixels) that gives >= 256 tiles, 128-channel
    tiles only for M > 64, else 64x128.  ``checked``: the last output-channel tile is partial (store_tile, :208-209)."""
    k, m = (cout, cin) if data_gradient else (cin, cout)
    if not pw_ok(k, m, hw):
        return None
    pick = 3
    for i, (mt, npix) in enumerate(PW_TILES):
        if mt == 128 and m <= 64:
            continue
        if batch * cdiv(hw, npix) * cdiv(m, mt) >= PW_MIN_TILES:
            pick = i
            break
    mt, npix = PW_TILES[pick]
    return dict(mt=mt, npix=npix, kernel=f"conv1x1_f32_kernel<{mt},{npix},{PW_KC}>", checked=m % mt != 0, partial_pixels=hw % npix != 0,
                px_tiles=cdiv(hw, npix), live_pixels_last=hw - (cdiv(hw, npix) - 1) * npix)


# ------------------------------------------------------------------------------------------ pointwise weight gradient

PK = 64                          # conv1x1_wgrad_f32.hip:20
PWG_TARGET = 768                 # conv1x1_wgrad_f32.hip:188 (SIS_PWG_TARGET unset)


def pwg_tile(cout, cin):
    """pwg_tile (conv1x1_wgrad_f32.hip:175-181): (id, tm, tn) or None."""
    if cout % 128 == 0 and cin % 128 == 0 and (cout // 128) * (cin // 128) >= 8:
        return 3, 128, 128
    if cout % 128 == 0 and cin % 64 == 0:
        return 0, 128, 64
    if cout % 64 == 0 and cin % 128 == 0:
        return 1, 64, 128
    if cout % 256 == 0 and cin % 32 == 0:
        return 2, 256, 32
    return None


def pwg_supported(batch, cin, cout, hw):      # conv1x1_wgrad_f32.hip:199-203
    return (batch > 0 and hw > 0 and hw % PK == 0 and pwg_tile(cout, cin) is not None and batch * cout * hw < 1 << 30
            and batch * cin * hw < 1 << 30)


def pwg_slices(batch, cin, cout, hw, jobs=1):
    """pwg_slices (conv1x1_wgrad_f32.hip:184-195): the K slices a launch is planned for."""
    _, tm, tn = pwg_tile(cout, cin)
    tiles, chunks = (cout // tm) * (cin // tn) * jobs, batch * (hw // PK)
    slices = min(cdiv(PWG_TARGET, tiles), chunks // 2, (32 << 20) // (cout * cin * 4), 256)
    return max(slices, 1)


def pwg_workspace(batch, cin, cout, hw):      # sis_conv1x1_wgrad_f32_workspace (conv1x1_wgrad_f32.hip:205-209)
    if not pwg_supported(batch, cin, cout, hw):
        return 0
    slices = pwg_slices(batch, cin, cout, hw)
    return slices * cout * cin * 4 if slices > 1 else 0


def pwg_plan(batch, cin, cout, hw, jobs=1, workspace_bytes=None):
    """pwg_jobs (conv1x1_wgrad_f32.hip:211-251).  ``workspace_bytes`` None: the single-layer binding, which brings exactly
    ``pwg_workspace`` (none for one slice); the queue brings the shared workspace."""
    if not pwg_supported(batch, cin, cout, hw):
        return None
    tile_id, tm, tn = pwg_tile(cout, cin)
    chunks = batch * (hw // PK)
    slices = pwg_slices(batch, cin, cout, hw, jobs)
    if workspace_bytes is None:
        workspace_bytes = pwg_workspace(batch, cin, cout, hw)
    n = cout * cin
    if not workspace_bytes or slices * n * 4 * jobs > workspace_bytes:
        slices = workspace_bytes // (n * 4 * jobs) if workspace_bytes else 1
    slices = max(slices, 1)
    cps = cdiv(chunks, slices)
    slices = cdiv(chunks, cps)
    return dict(tile_id=tile_id, tm=tm, tn=tn, chunks=chunks, chunks_per_slice=cps, ksplit=slices,
                slices=[min(cps, chunks - s * cps) for s in range(slices)], tiles=(cout // tm) * (cin // tn))


def pwg_launches(n_jobs, batch, cin, cout, hw, workspace_bytes=WORKSPACE_BYTES):
    """sis_conv1x1_wgrad_f32_multi (conv1x1_wgrad_f32.hip:256-265): any count fits, 16 layers per launch."""
    return [(first, n, pwg_plan(batch, cin, cout, hw, n, workspace_bytes)) for first, n in run_jobs(n_jobs, lambda n: True)]
