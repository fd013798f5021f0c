// Shared by the modulated-convolution kernels (modconv_mfma.hip: register-staged, any shape; modconv_mfma2.hip: LDS-DMA
// double-buffered; modconv_wino.hip / modconv_wino24.h: Winograd) and their C entries (modconv_entries.hip): the kernel
// argument, the tile and split-K planning, and one launcher per kernel file.
#pragma once
#include "sis_device.h"

constexpr int MC_MAX_CLS = 4;
constexpr int MC_XI = 3;  // staged x elements per lane per channel (covers xt <= 768)

// A "tile class" is a family of equally shaped position tiles.  The stride-1 conv needs one; the
// transposed conv needs four because its positions run over (H+1) x (W+1): interior, last row,
// last column and corner get their own tile shapes instead of padding every tile.
struct TileClass {
    int th_log2, tw_log2, nb;  // tile = nb samples x 2^th_log2 rows x 2^tw_log2 cols
    int h0, w0, h1, w1;        // region of positions this class owns: [h0,h1) x [w0,w1)
    int nth, ntw;              // tiles per sample
    int first_block;           // first position-tile index of this class
    int xt;                    // floats per channel of the staged input tile
};

struct ConvParams {
    const float* x; const float* wpk; const float* s; const float* dscale;
    const float* noise; const float* noise_w; const float* bias;
    float* out;
    float* slab;               // split-K partial sums [ksplit][B][Cout][OH][OW] or nullptr
    int64_t noise_bstride;
    int B, Cin, Cout, H, W, OH, OW;
    int ORS;                   // output row stride in floats (>= OW)
    int fuse;
    int npos_tiles, ncls;
    int cout_vec4;
    int ksplit, kchunk;        // split-K: blockIdx.y = k slice, kchunk input channels per slice
    int nb_max;
    TileClass cls[MC_MAX_CLS];
};

template <int MODE, int KS>
struct ConvCfg {
    static constexpr int NTAPS = KS * KS;
    static constexpr int MBLK = MODE == 0 ? 128 : 64;
    static constexpr int NPOS = MODE == 0 ? 256 : 128;
    static constexpr int MT = 2;
    static constexpr int NT = MODE == 0 ? 4 : 1;
    static constexpr int NACC = 4;
    static constexpr int PAD_LO = MODE == 0 ? KS / 2 : 1;
    static constexpr int EXT = MODE == 0 ? KS - 1 : 1;
};

static inline int mc_ilog2_ceil(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// "No tile classes yet" and "no split-K": what a plan starts from, and what a launcher that declined leaves to be redone.
static inline void mc_reset_tiles(ConvParams& p) { p.npos_tiles = 0; p.ncls = 0; p.nb_max = 0; }
static inline void mc_reset_splitk(ConvParams& p) { p.ksplit = 1; p.kchunk = p.Cin; p.slab = nullptr; }

// Everything of a launch that the tile plan does not decide.  A plain convolution passes null s / dscale / noise / bias.
static inline ConvParams mc_params(float* out, const float* x, const float* wpk, const float* s, const float* dscale,
                                   const float* noise, int64_t noise_bstride, const float* noise_w, const float* bias,
                                   int batch, int cin, int cout, int h, int w, int oh, int ow, int ors, bool fuse) {
    ConvParams p;
    p.x = x; p.wpk = wpk; p.s = s; p.dscale = dscale; p.noise = noise; p.noise_w = noise_w; p.bias = bias;
    p.out = out; p.noise_bstride = noise_bstride;
    p.B = batch; p.Cin = cin; p.Cout = cout; p.H = h; p.W = w; p.OH = oh; p.OW = ow; p.ORS = ors; p.fuse = fuse;
    p.cout_vec4 = (cout % 4 == 0) && (((uintptr_t)wpk & 15) == 0);
    mc_reset_tiles(p);
    mc_reset_splitk(p);
    return p;
}

// Adds a tile class covering positions [h0,h1) x [w0,w1) with tiles of at most npos positions.
static inline void mc_add_class(ConvParams& p, int npos, int ext, int batch, int h0, int h1, int w0, int w1,
                                int tw_cap, int nb_cap) {
    const int hh = h1 - h0, ww = w1 - w0;
    if (hh <= 0 || ww <= 0) return;
    TileClass& c = p.cls[p.ncls];
    int twl = mc_ilog2_ceil(ww);
    const int capl = mc_ilog2_ceil(tw_cap);
    if (twl > capl) twl = capl;
    const int npl = mc_ilog2_ceil(npos);
    int thl = mc_ilog2_ceil(hh);
    if (thl > npl - twl) thl = npl - twl;
    c.th_log2 = thl; c.tw_log2 = twl; c.nb = npos >> (thl + twl);
    if (c.nb > nb_cap) c.nb = nb_cap;
    if (c.nb > batch) c.nb = batch;
    c.h0 = h0; c.w0 = w0; c.h1 = h1; c.w1 = w1;
    c.nth = sis_cdiv(hh, 1 << thl); c.ntw = sis_cdiv(ww, 1 << twl);
    c.first_block = p.npos_tiles;
    c.xt = c.nb * ((1 << thl) + ext) * ((1 << twl) + ext);
    p.npos_tiles += c.nth * c.ntw * sis_cdiv(batch, c.nb);
    if (c.nb > p.nb_max) p.nb_max = c.nb;
    p.ncls++;
}

// Fast paths stage the input tile with 16-byte LDS-DMA: rows become the 16-byte aligned superset of the halo'd
// tile columns (left pad 4 instead of 1, right edge rounded up to a multiple of 4).  W % 4 == 0 makes every
// aligned float4 lie entirely inside or entirely outside the image.
static inline int mc_padded_ew(int tw, int pad_lo, int ext) { return (pad_lo ? 4 : 0) + ((tw + ext - pad_lo + 3) & ~3); }
static inline void mc_set_padded_xt(ConvParams& p, int pad_lo, int ext) {
    for (int c = 0; c < p.ncls; ++c) {
        TileClass& tc = p.cls[c];
        tc.xt = tc.nb * ((1 << tc.th_log2) + ext) * mc_padded_ew(1 << tc.tw_log2, pad_lo, ext);
    }
}


// Tile plan of the Winograd F(2x2,3x3) kernels: one class of 16 x 16-pixel regions (conflict-free patch reads), rows staged
// as the 16-byte aligned superset of the halo (left pad 4, right pad 4).
static inline void mc_wino_tiles(ConvParams& p) {
    mc_reset_tiles(p);
    mc_add_class(p, 256, 2, p.B, 0, p.H, 0, p.W, 16, 16);
    TileClass& tc = p.cls[0];
    tc.xt = tc.nb * ((1 << tc.th_log2) + 2) * ((1 << tc.tw_log2) + 8);
}

// Chooses the K split of a kernel with `mblk` output channels per workgroup and `cc` input channels per chunk: below
// `min_blocks` (tile x oc-block) workgroups, enough slices to reach `target`, slices a multiple of the chunk size and at
// least two chunks long, and the slabs [ksplit][B][Cout][OH][ORS] must fit the caller's workspace (none: no split).
static inline void mc_plan_splitk(ConvParams& p, int mblk, int cc, int min_blocks, int target, void* workspace,
                                  int64_t workspace_bytes) {
    mc_reset_splitk(p);
    const int64_t blocks = (int64_t)p.npos_tiles * sis_cdiv(p.Cout, mblk);
    if (blocks >= min_blocks || p.Cin < 4 * cc || !workspace) return;
    int want = (int)((target + blocks - 1) / blocks);
    const int max_split = p.Cin / (2 * cc);
    if (want > max_split) want = max_split;
    const int64_t out_bytes = (int64_t)p.B * p.Cout * p.OH * p.ORS * 4;
    if ((int64_t)want * out_bytes > workspace_bytes) want = (int)(workspace_bytes / out_bytes);
    if (want < 2) return;
    p.kchunk = sis_cdiv(sis_cdiv(p.Cin, want), cc) * cc;
    p.ksplit = sis_cdiv(p.Cin, p.kchunk);
    p.slab = (float*)workspace;
}

// One launcher per kernel file.  Each returns 0 on success, 1 on error (sis_last_error), -1 when the shape is not the
// kernel's: the caller (modconv_entries.hip) then tries the next one.
// modconv_wino.hip: Winograd F(2x2,3x3), stride-1 3x3 layers; p.wpk holds the transformed weights, tiles from mc_wino_tiles.
int modconv_wino_launch(ConvParams& p, hipStream_t st, void* workspace, int64_t workspace_bytes, bool plan_only = false);
// modconv_mfma2.hip: LDS-DMA kernel.  Rewrites every class's xt to the padded-row form BEFORE it can still decline.
int modconv_v2_launch(ConvParams& p, int mode, int ks, hipStream_t st, void* workspace, int64_t workspace_bytes);
// modconv_mfma.hip: register-staged kernel, any shape; wants exact-halo xt and no split-K.
int modconv_v1_launch(ConvParams& p, int mode, int ks, hipStream_t st);
// modconv_mfma2.hip: adds the K slices of p.slab in slice order and applies the epilogue.
int modconv_splitk_finish_launch(const ConvParams& p, hipStream_t st);
