// C entries of the modulated-convolution family and the order in which its kernels are tried.  Host code only: every
// kernel lives in the file of its launcher (modconv_common.h lists them), this file decides who is asked first.
//
//   stride-1 (sis_modconv2d):   Winograd F(2x2,3x3) where the caller passes transformed weights and H % 2 == 0, W % 4 == 0;
//                               then the LDS-DMA kernel; then the register-staged kernel, which takes any shape
//   transposed (sis_modconv2d_up): LDS-DMA kernel; then register-staged
//   plain 3x3 (sis_conv3x3):    Winograd F(2x2,3x3) or an error
#include "modconv_common.h"

namespace {

int check_common(const char* name, const void* out, const void* x, const void* wpk, const void* s, const void* dscale,
                 int batch, int cin, int cout, int h, int w, int oh, int ow) {
    SIS_REQUIRE(out && x && wpk && s && dscale, "%s: null pointer", name);
    SIS_REQUIRE(batch > 0 && cin > 0 && cout > 0 && h > 0 && w > 0, "%s: non-positive size", name);
    SIS_REQUIRE((int64_t)batch * cin * h * w < ((int64_t)1 << 31) && (int64_t)batch * cout * oh * ow < ((int64_t)1 << 31),
                "%s: tensor too large for 32-bit plane offsets", name);
    return 0;
}

// Exact-halo tiles of the direct kernels.  mode 0: one class of up to 256 pixels.  mode 1: positions run over
// (H+1) x (W+1), tiles of up to 128 positions in four classes.
void direct_tiles(ConvParams& p, int mode, int ks) {
    const int batch = p.B, h = p.H, w = p.W;
    mc_reset_tiles(p);
    if (mode == 0) {
        mc_add_class(p, 256, ks - 1, batch, 0, h, 0, w, 32, 16);
        return;
    }
    mc_add_class(p, 128, 1, batch, 0, h, 0, w, 32, 8);          // interior positions
    mc_add_class(p, 128, 1, batch, h, h + 1, 0, w, 128, h >= 16 ? 4 : 8);  // last row (T[2H, 0..2W-1]); 16 x 16: 8 style rows here made the grid's LDS 86 KB, one workgroup per CU
    // last col (T[0..2H-1, 2W]): one position per row, each staged as a padded 8-float row, and the corner: capped at
    // 64 rows / 4 samples per tile.  The grid's LDS size follows its LARGEST class: uncapped, the last column's staging
    // area (2 x 65 x 8 floats per channel) and the corner's 8 style rows made it 120 KB -- one workgroup per CU for
    // every tile of the layer (measured with hipOccupancyMaxActiveBlocksPerMultiprocessor; 74-80 KB now: two per CU).
    // (4x4 and 8x8 layers keep 8 samples per edge tile: they are split-K / launch bound, more tiles cost them 30-50 %.)
    const int edge_nb = h >= 16 ? 4 : 8;
    mc_add_class(p, 64, 1, batch, 0, h, w, w + 1, 1, edge_nb);
    mc_add_class(p, 128, 1, batch, h, h + 1, w, w + 1, 1, edge_nb);   // corner    (T[2H, 2W])
}

// LDS-DMA kernel, then the register-staged one.  The first rewrites every class's xt to its padded-row form (and may plan a
// split) before it can still decline, and the second needs exact-halo tiles: they are built again in between.
int launch_direct(ConvParams& p, int mode, int ks, hipStream_t st, void* workspace, int64_t workspace_bytes) {
    direct_tiles(p, mode, ks);
    const int rc = modconv_v2_launch(p, mode, ks, st, workspace, workspace_bytes);
    if (rc >= 0) return rc;
    direct_tiles(p, mode, ks);
    mc_reset_splitk(p);
    return modconv_v1_launch(p, mode, ks, st);
}

// Plain (unmodulated) 3x3 convolution, stride 1, padding 1, on the Winograd kernel: unit style, unit demodulation,
// no epilogue.  Used for the segmentation networks' 3x3 layers (forward, and data gradient with adjoint weights).
int conv3x3_plan(ConvParams& p, float* out, const float* x, const float* u, int batch, int cin, int cout, int h, int w) {
    if (batch <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0) return -1;
    if ((int64_t)batch * (cin > cout ? cin : cout) * h * w >= ((int64_t)1 << 31)) return -1;
    if (w % 4 != 0 || h % 2 != 0 || cin % 8 != 0 || cout % 4 != 0) return -1;
    p = mc_params(out, x, u, nullptr, nullptr, nullptr, 0, nullptr, nullptr, batch, cin, cout, h, w, h, w, w, false);
    mc_wino_tiles(p);
    return 0;
}

}  // namespace

extern "C" int sis_modconv2d(float* out, const float* x, const float* wpk, const float* s, const float* dscale,
                             const float* noise, int64_t noise_batch_stride, const float* noise_weight,
                             const float* bias, int batch, int cin, int cout, int h, int w, int ksize, int fuse_act,
                             const float* wino_u, void* workspace, int64_t workspace_bytes, void* stream) {
    if (batch == 0) return 0;
    if (check_common("sis_modconv2d", out, x, wpk, s, dscale, batch, cin, cout, h, w, h, w)) return 1;
    SIS_REQUIRE(ksize == 1 || ksize == 3, "sis_modconv2d: kernel size %d not supported (1 or 3)", ksize);
    if (noise) SIS_REQUIRE(noise_weight, "sis_modconv2d: noise given without noise_weight");
    ConvParams p = mc_params(out, x, wpk, s, dscale, noise, noise_batch_stride, noise_weight, bias, batch, cin, cout, h, w, h, w,
                             w, fuse_act != 0);
    if (wino_u && ksize == 3 && w % 4 == 0 && h % 2 == 0) {
        ConvParams pw = p;
        pw.wpk = wino_u;
        mc_wino_tiles(pw);
        const int rcw = modconv_wino_launch(pw, (hipStream_t)stream, workspace, workspace_bytes);
        if (rcw >= 0) return rcw;
    }
    return launch_direct(p, 0, ksize, (hipStream_t)stream, workspace, workspace_bytes);
}

extern "C" int sis_conv3x3_eligible(int batch, int cin, int cout, int h, int w) {
    ConvParams p;
    if (conv3x3_plan(p, nullptr, nullptr, nullptr, batch, cin, cout, h, w) < 0) return 0;
    return modconv_wino_launch(p, nullptr, nullptr, 0, true) == 0 ? 1 : 0;
}

extern "C" int sis_conv3x3(float* out, const float* x, const float* u, int batch, int cin, int cout, int h, int w,
                           void* workspace, int64_t workspace_bytes, void* stream) {
    if (batch == 0) return 0;
    SIS_REQUIRE(out && x && u, "sis_conv3x3: null pointer");
    ConvParams p;
    SIS_REQUIRE(conv3x3_plan(p, out, x, u, batch, cin, cout, h, w) == 0,
                "sis_conv3x3: needs W %% 4 == 0, H %% 2 == 0, Cin %% 8 == 0, Cout %% 4 == 0 and < 2^31 elements "
                "(got %d x %dx%d, %d -> %d)", batch, h, w, cin, cout);
    const int rc = modconv_wino_launch(p, (hipStream_t)stream, workspace, workspace_bytes);
    SIS_REQUIRE(rc >= 0, "sis_conv3x3: shape %dx%d, %d -> %d not eligible for the Winograd kernel", h, w, cin, cout);
    return rc;
}

extern "C" int sis_modconv2d_up(float* t, const float* x, const float* wpk, const float* s, const float* dscale,
                                int batch, int cin, int cout, int h, int w, int t_row_stride, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    if (batch == 0) return 0;
    const int oh = 2 * h + 1, ow = 2 * w + 1;
    if (t_row_stride <= 0) t_row_stride = ow;
    SIS_REQUIRE(t_row_stride >= ow, "sis_modconv2d_up: row stride %d smaller than 2W+1 = %d", t_row_stride, ow);
    if (check_common("sis_modconv2d_up", t, x, wpk, s, dscale, batch, cin, cout, h, w, oh, t_row_stride)) return 1;
    ConvParams p = mc_params(t, x, wpk, s, dscale, nullptr, 0, nullptr, nullptr, batch, cin, cout, h, w, oh, ow, t_row_stride,
                             false);
    return launch_direct(p, 1, 3, (hipStream_t)stream, workspace, workspace_bytes);
}
