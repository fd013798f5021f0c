// What the Winograd F(2x4,3x3) and F(4x4,3x3) kernels (modconv_wino24.h, modconv_wino44.h) have in common.  Both walk one-sample
// tiles of 512 pixels (8 x 64 or 16 x 32) with 8 waves and 64 output channels per workgroup, stage the same raw input tile, use
// the 6-point transform (points 0, +-1, +-2, inf) on the column axis -- F(4x4) on the row axis too -- and end in the same layer
// tail.  Included by modconv_wino.hip in front of the two form headers (one translation unit: the helpers above are used here).
//
// Here: the 6-point transforms, the layer tail of one value, the opaque thread index and the tail-operand staging of the tile
// start, the ToRGB operands, the tile constants, and the host side: one plan and one launch, driven by a Wino512Form.
// Per form: the plane order and prepack addressing, the LDS images, the MFMA shape and chunk schedule with its slot tables, the
// lane / wave maps of the transform, the partner exchange and the RGB sum order, the noise staging.
// Still twice, marked "twin" in both kernels: workgroup order, input-piece plan, TileState / tile_setup / stage_x_piece and the
// style-row loop: behind shared functions they compiled to other scalar code (profiles/wino_tile512_refactor.txt).
//
// The bit-exact tests pin the association and FMA placement of every expression below, and the generated code is held to that of
// the former separate copies: the transforms take pointers / arrays because the compiler orders a commutative add's operands by the
// order in which they are read, not by the arithmetic as written.

namespace {

constexpr int W512_CC = 4;    // input channels per chunk
constexpr int W512_XT = 720;  // floats per channel of the staged input tile: 10 x 72 or 18 x 40
constexpr int W512_XP = 3;    // 64-lane float4 pieces of a channel (the last one shifted back to end with the tile)

// ---- 6-point transforms

// o = G4 g: 3 taps (GS floats apart) -> 6 points (OS floats apart), i.e. along either axis of a row-major array
template <int GS, int OS>
__device__ __forceinline__ void wino_g6(const float* g, float* o) {
    const float a = g[0], b = g[GS], c = g[2 * GS];
    o[0] = 0.25f * a;
    o[OS] = (-1.f / 6.f) * (a + b + c);
    o[2 * OS] = (-1.f / 6.f) * (a - b + c);
    o[3 * OS] = (1.f / 24.f) * a + (1.f / 12.f) * b + (1.f / 6.f) * c;
    o[4 * OS] = (1.f / 24.f) * a - (1.f / 12.f) * b + (1.f / 6.f) * c;
    o[5 * OS] = c;
}

// Half of the input transform: o = scale * (rows 3 HALF .. 3 HALF + 2 of B6^T d), from the five samples p those rows read: d0..d4
// (HALF = 0) or d1..d5 (HALF = 1).  scale: the style in the pass that finishes V, a literal 1 (which folds away) in the other.
template <int HALF>
__device__ __forceinline__ void wino_b6_half(const float (&p)[5], float scale, float (&o)[3]) {
    if (HALF == 0) {
        const float u = fmaf(-4.f, p[2], p[4]), v = fmaf(-4.f, p[1], p[3]);
        o[0] = fmaf(4.f, p[0], fmaf(-5.f, p[2], p[4])) * scale;
        o[1] = (u + v) * scale;
        o[2] = (u - v) * scale;
    } else {
        const float u = p[3] - p[1], v = p[2] - p[0];
        o[0] = fmaf(2.f, v, u) * scale;
        o[1] = fmaf(-2.f, v, u) * scale;
        o[2] = fmaf(4.f, p[0], fmaf(-5.f, p[2], p[4])) * scale;
    }
}

// y = A4^T m: 6 points -> 4 outputs; lo: points 0..2, hi: points 3..5 (in the kernels' epilogues the two come from two waves)
__device__ __forceinline__ void wino_a4(const float* lo, const float* hi, float (&y)[4]) {
    const float s12 = lo[1] + lo[2], d12 = lo[1] - lo[2], s34 = hi[0] + hi[1], d34 = hi[0] - hi[1];
    y[0] = (lo[0] + s12) + s34;
    y[1] = fmaf(2.f, d34, d12);
    y[2] = fmaf(4.f, s34, s12);
    y[3] = fmaf(8.f, d34, d12) + hi[2];
}

// ---- layer tail of one value: scale * demodulation, noise, bias, leaky ReLU * sqrt(2) (slope = gain = 1: tail off)
__device__ __forceinline__ float wino_layer_tail(float y, float dd, float nz, float bb, float slope, float gain) {
    float val = y * dd;
    val += nz;
    val += bb;
    return fmaxf(val, val * slope) * gain;  // = (val > 0 ? val : 0.2 val) * sqrt(2) when the tail is on
}

// ---- tile start

// A copy of the thread index that the compiler cannot see through.  Lane-derived values of the tile start and of the epilogue come
// from such copies: the compiler would otherwise compute them once and hold (spill) them across the chunk loop, whose registers
// are all taken.
__device__ __forceinline__ int wino_opaque_tid() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

// Tile start, thread tp: the layer-tail operands of sample b and the channel block at o0, to LDS
template <bool RGB, class Rgb>
__device__ __forceinline__ void wino512_stage_tail_operands(const ConvParams& p, const Rgb& rgb, int b, int o0, int tp, float* Dl, float* Bl,
                                                            float* Wl) {
    if (tp < WMBLK) {
        Dl[tp] = p.dscale[(int64_t)b * p.Cout + o0 + tp];
        Bl[tp] = (p.fuse && p.bias) ? p.bias[o0 + tp] : 0.f;
    }
    if constexpr (RGB) {
        if (tp < 3 * WMBLK) {
            const int co = o0 + (tp & (WMBLK - 1));
            Wl[tp] = rgb.scale * rgb.w[(tp / WMBLK) * p.Cout + co] * rgb.s[(int64_t)b * p.Cout + co];
        }
    }
}

// ---- ToRGB operands of the instantiations that also emit RGB partial sums (RGB = true; the others take an empty struct)
struct WinoRgb {
    const float* w;   // [3][Cout]  ToRGB weight
    const float* s;   // [B][Cout]  ToRGB style
    float* part;      // [Cout / 64][B][3][H][W]  partial sums of the workgroup's channel block
    float scale;
};
struct WinoNoRgb {};

// ---- host side: what the plan and the launch need to know of a form
struct Wino512Form {
    int h_mult;            // H is a multiple of this (whole output tiles); W of 4
    int u_floats;          // floats of U per (ci, co)
    int uf, vf, nf;        // LDS floats: a weight chunk, a V chunk, the noise of a tile's pixels
    const char* kernel;    // name of both instantiations in the per-kernel records
    const char* eligible;  // the form's eligibility entry, for the error text
    void (*with_rgb)(const ConvParams, const int, const int, const WinoRgb);   // (first: the kernels' order in the code object)
    void (*plain)(const ConvParams, const int, const int, const WinoNoRgb);
};

}  // namespace

// Both kernels take a layer by (Cin, Cout, H, W) alone: 64-channel output blocks, 8-channel input steps, whole output tiles, and a
// map that one-sample tiles of 512 pixels (8 x 64 or 16 x 32) cover -- W > 16, H * W >= 512 after rounding up to powers of two.
// Returns the bytes of dynamic LDS, or -1 where the form does not take the layer.
static int wino512_plan(const Wino512Form& f, ConvParams& p, int cin, int cout, int h, int w, bool rgb = false) {
    if (cin <= 0 || cout <= 0 || h <= 0 || w <= 0) return -1;
    if (cin % 8 || cout % WMBLK || h % f.h_mult || w % 4) return -1;
    if ((int64_t)cin * h * w * 4 >= ((int64_t)1 << 31) || (int64_t)cin * cout * (f.u_floats * 4) >= ((int64_t)1 << 31)) return -1;  // 32-bit DMA offsets
    p.Cin = cin;
    mc_reset_splitk(p);
    mc_reset_tiles(p);
    mc_add_class(p, 512, 2, 1, 0, h, 0, w, 64, 1);
    const TileClass& tc = p.cls[0];
    if (tc.nb != 1 || tc.th_log2 + tc.tw_log2 != 9 || tc.tw_log2 < 5) return -1;
    if (((1 << tc.th_log2) + 2) * ((1 << tc.tw_log2) + 8) != W512_XT) return -1;
    const size_t lds = (size_t)(2 * f.uf + 2 * f.vf + 2 * W512_CC * W512_XT + cin + (rgb ? 5 : 2) * WMBLK + f.nf) * sizeof(float);
    if (lds > 160 * 1024) return -1;
    return (int)lds;
}

// name: the C entry (sis_modconv2d_wino24 / wino44 document out); rgb (or null) selects the instantiation with the RGB partial sums.
template <const Wino512Form& FORM>
static int wino512_launch(const char* name, float* out, const float* x, const float* u, const float* s, const float* dscale,
                          const float* noise, int64_t noise_batch_stride, const float* noise_weight, const float* bias, int batch,
                          int cin, int cout, int h, int w, int fuse_act, int tiles_per_wg, const WinoRgb* rgb, void* stream) {
    SIS_REQUIRE(out && x && u && s && dscale, "%s: null pointer", name);
    SIS_REQUIRE(batch > 0, "%s: non-positive size", name);
    if (noise) SIS_REQUIRE(noise_weight, "%s: noise given without noise_weight", name);
    ConvParams p = mc_params(out, x, u, s, dscale, noise, noise_batch_stride, noise_weight, bias, batch, cin, cout, h, w, h, w, w,
                             fuse_act != 0);
    const int lds = wino512_plan(FORM, p, cin, cout, h, w, rgb != nullptr);
    SIS_REQUIRE(lds > 0, "%s: shape %dx%d, %d -> %d not eligible (%s)", name, h, w, cin, cout, FORM.eligible);
    SIS_REQUIRE((int64_t)batch * (cin > cout ? cin : cout) * h * w < ((int64_t)1 << 31), "%s: tensor too large", name);
    SIS_REQUIRE(((((uintptr_t)x | (uintptr_t)u | (uintptr_t)out) & 15) == 0) && (!noise || ((uintptr_t)noise & 3) == 0),
                "%s: pointers must be 16-byte aligned", name);
    const TileClass& tc = p.cls[0];
    const int64_t tiles = (int64_t)batch * tc.nth * tc.ntw;  // one-sample tiles
    p.npos_tiles = (int)tiles;
    const int n_co = cout / WMBLK;
    const int64_t blocks = tiles * n_co;
    SIS_REQUIRE(blocks < ((int64_t)1 << 31), "%s: bad grid", name);
    // pixel tiles per workgroup: as many as keep >= 1024 workgroups in flight (scheduling only: every tile is computed the same
    // way whichever workgroup walks it); tiles_per_wg > 0 is the tests' override
    int tpw = 1;
    if (tiles_per_wg > 0) {
        SIS_REQUIRE(tiles % tiles_per_wg == 0, "%s: %d tiles per workgroup do not divide %lld tiles", name, tiles_per_wg, (long long)tiles);
        tpw = tiles_per_wg;
    } else {
        while (tpw * 2 <= 16 && tiles % (tpw * 2) == 0 && blocks / (tpw * 2) >= 1024) tpw *= 2;
    }
    const int64_t grid = blocks / tpw;
    // all co-blocks of a pixel tile on one XCD when the whole transformed weight tensor (<= 5 MB) stays L2-resident there
    const int xcd_group = (double)cin * cout * FORM.u_floats * sizeof(float) <= 5.0 * 1048576.0 && n_co > 1 && grid % (8 * n_co) == 0;
    static bool have_attr[2] = {false, false};  // of this form: the function is instantiated once per form
    const void* fn = rgb ? reinterpret_cast<const void*>(FORM.with_rgb) : reinterpret_cast<const void*>(FORM.plain);
    if (!have_attr[rgb != nullptr]) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return sis_fail("modconv: cannot raise the dynamic LDS limit: %s", hipGetErrorString(e));
        have_attr[rgb != nullptr] = true;
    }
    sis_kernel_name = FORM.kernel;  // both instantiations: one kernel to the per-kernel records
    if (rgb) {
        hipLaunchKernelGGL(FORM.with_rgb, dim3((unsigned)grid), dim3(WNTHR), (size_t)lds, (hipStream_t)stream, p, tpw, xcd_group, *rgb);
    } else {
        hipLaunchKernelGGL(FORM.plain, dim3((unsigned)grid), dim3(WNTHR), (size_t)lds, (hipStream_t)stream, p, tpw, xcd_group, WinoNoRgb{});
    }
    SIS_CHECK_LAUNCH(name);
    return 0;
}
