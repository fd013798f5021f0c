// The projection encoders' own kernels (networks/encoder/u_net_like_encoder.py, inference path): what a U-Net-like W+ encoder
// needs beyond the stride-1 Winograd convolution (sis_conv3x3) and the fused batch norm (sis_bn_act_fwd).  Included from
// stem_conv.hip (kernels of a header live in the including translation unit, as modconv_wino24.h and pixel_ensemble_train.h).
// Eval-mode BatchNorm enters every kernel folded: scale = gamma / sqrt(var + eps), shift = beta - mean * scale.
//
//   K1 enc_conv3x3_s2_kernel    3x3, stride 2, padding 1, fp32 NCHW as an implicit GEMM on v_mfma_f32_32x32x2_f32:
//                               y_main = relu(scale1 * conv + shift1) and, from the SAME centre-tap operand in LDS, the block's
//                               projection shortcut y_short = scale_d * conv1x1_s2(x, wd) + shift_d.
//   K2 enc_stem_kernel          3x3 stride 1 from <= 4 input channels plus the 1x1 shortcut of the start block (VALU).
//   K3 enc_block_tail_kernel    y = relu(scale2 * c + shift2 + residual); optionally the to_noise 1x1 convolution to one channel
//                               and per-(sample, channel, tile) partial sums of y for the average pool, from the same registers.
//   K4 enc_latent_heads_kernel  every to_latent head of an encode in one launch: pool = sum of the tile partials / HW, then
//                               [latent, C] x pool + bias into row `slot` of the W+ tensor (or the sum over the heads).
// No atomics; every sum has a fixed order (stated at the sum).
#pragma once
#include <atomic>
#include "sis_device.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- K1
// GEMM view: M = output channels (tile 64), N = output pixels of one sample, flattened oy * Wo + ox (tile 128: wave w takes
// pixels 32 w .. 32 w + 31 and both 32-channel halves), K = (input channel, tap) in chunks of 8 channels.  Per chunk the
// workgroup stages (a) the 8 x T x 64 weights of its channel tile, T = 9 taps (+ 1: the shortcut's 1x1 weight), from the packed
// image [Cin][T][Cout padded to 64], and (b) for each of the 8 channels the input rows 2 oy0 - 1 .. 2 oy1 + 1 of the tile's
// output rows oy0 .. oy1, W + 1 columns (column 0 = the left padding, row 2 oy0 - 1 = -1 for the first tile: zeros).  With
// even H and W nothing is padded on the right or at the bottom.  B operand of tap (ky, kx) for pixel (oy, ox): LDS element
// [channel][2 (oy - oy0) + ky][2 ox + kx] -- a stride-2 ds_read_b32 (2-way bank conflict).  The centre tap (1, 1) is input
// pixel (2 oy, 2 ox): the sample of the 1x1 stride-2 shortcut, so its B value feeds two more MFMAs with the shortcut weights.
// ORDER of the sum for one output: channel chunks ascending; inside a chunk taps 0..8 (ky major); inside a tap channel pairs
// ascending; an MFMA adds k = 0 then k = 1 (the f32 MFMA is a k-ordered fmaf chain).
constexpr int ES_MT = 64, ES_NT = 128, ES_KC = 8;

struct EncS2Params {
    const float* x;        // [B][Cin][H][W]
    const float* wp;       // packed [Cin][T][cout_pad]
    float* y_main;         // [B][Cout][Ho][Wo]
    float* y_short;        // same, or null (T = 9)
    const float *scale1, *shift1, *scale_d, *shift_d;   // [Cout]
    int cin, cout, cout_pad, H, W, Ho, Wo;
};

// rows of the output a 128-pixel tile can span, and the floats of one staged input channel
__host__ __device__ inline int enc_s2_rows_max(int ho, int wo) {
    const int rows = (ES_NT % wo == 0) ? ES_NT / wo : ES_NT / wo + 2;
    return rows < ho ? rows : ho;
}
inline int64_t enc_s2_lds_bytes(int h, int w, int taps) {
    const int64_t chan = (int64_t)(2 * enc_s2_rows_max(h / 2, w / 2) + 1) * (w + 1);
    return ((int64_t)ES_KC * taps * ES_MT + ES_KC * chan) * 4;
}

template <bool SHORT>
__global__ __launch_bounds__(256) void enc_conv3x3_s2_kernel(EncS2Params p) {
    extern __shared__ __attribute__((aligned(16))) float es_lds[];
    constexpr int T = SHORT ? 10 : 9;
    float* wl = es_lds;                      // [8][T][64]
    float* xl = es_lds + ES_KC * T * ES_MT;  // [8][nr][W + 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z, m0 = blockIdx.y * ES_MT, p0 = blockIdx.x * ES_NT;
    const int npix = p.Ho * p.Wo;
    const int plast = min(p0 + ES_NT, npix) - 1;
    const int oy0 = p0 / p.Wo, oy1 = plast / p.Wo;
    const int nr = 2 * (oy1 - oy0 + 1) + 1, rowlen = p.W + 1, chan = nr * rowlen;
    // this lane's pixel (a lane past the end computes the last pixel again and stores nothing)
    const int pix = min(p0 + wave * 32 + r, npix - 1);
    const int oy = pix / p.Wo, ox = pix - oy * p.Wo;
    const int boff = 2 * (oy - oy0) * rowlen + 2 * ox;

    sis_f32x16 acc[2], accs[SHORT ? 2 : 1];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        acc[0][i] = 0.f; acc[1][i] = 0.f; accs[0][i] = 0.f;
        if constexpr (SHORT) accs[1][i] = 0.f;
    }

    for (int c0 = 0; c0 < p.cin; c0 += ES_KC) {
        __syncthreads();   // the previous chunk's fragments are read
        for (int e = tid; e < ES_KC * T * (ES_MT / 4); e += 256) {
            const int row = e >> 4, q = e & 15;
            *reinterpret_cast<float4*>(wl + row * ES_MT + 4 * q) =
                *reinterpret_cast<const float4*>(p.wp + ((int64_t)c0 * T + row) * p.cout_pad + m0 + 4 * q);
        }
        const float* xb = p.x + ((int64_t)b * p.cin + c0) * p.H * p.W;
        for (int row = wave; row < ES_KC * nr; row += 4) {
            const int k = row / nr, rr = row - k * nr, iy = 2 * oy0 - 1 + rr;
            const bool rowok = iy >= 0 && iy < p.H;
            const float* src = xb + ((int64_t)k * p.H + (rowok ? iy : 0)) * p.W;
            float* dst = xl + k * chan + rr * rowlen;
            for (int c = lane; c < rowlen; c += 64) dst[c] = (rowok && c >= 1) ? src[c - 1] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int toff = (tap / 3) * rowlen + (tap % 3);
#pragma unroll
            for (int kp = 0; kp < ES_KC / 2; ++kp) {
                const int k = 2 * kp + h;
                const float bv = xl[k * chan + boff + toff];
                const float* wr = wl + (k * T + tap) * ES_MT + r;
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[0], bv, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[32], bv, acc[1], 0, 0, 0);
                if constexpr (SHORT) {
                    if (tap == 4) {
                        const float* ws = wl + (k * T + 9) * ES_MT + r;
                        accs[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[0], bv, accs[0], 0, 0, 0);
                        accs[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[32], bv, accs[1], 0, 0, 0);
                    }
                }
            }
        }
    }

    const int px = p0 + wave * 32 + r;
    if (px >= npix) return;
    const int64_t obase = (int64_t)b * p.cout * npix + px;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = m0 + mb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (co < p.cout) {
                p.y_main[obase + (int64_t)co * npix] = fmaxf(p.scale1[co] * acc[mb][i] + p.shift1[co], 0.f);
                if constexpr (SHORT) p.y_short[obase + (int64_t)co * npix] = p.scale_d[co] * accs[mb][i] + p.shift_d[co];
            }
        }
}

// packed[(ci * T + tap) * cout_pad + co] = w1[co][ci][tap] (tap < 9), wd[co][ci] (tap 9), 0 for co >= cout
__global__ __launch_bounds__(256) void enc_s2_pack_kernel(float* __restrict__ packed, const float* __restrict__ w1, const float* __restrict__ wd,
                                                          int cin, int cout, int cout_pad, int taps) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)cin * taps * cout_pad) return;
    const int co = (int)(i % cout_pad), tap = (int)((i / cout_pad) % taps), ci = (int)(i / ((int64_t)cout_pad * taps));
    float v = 0.f;
    if (co < cout) v = tap < 9 ? w1[((int64_t)co * cin + ci) * 9 + tap] : wd[(int64_t)co * cin + ci];
    packed[i] = v;
}

bool enc_s2_ok(int cin, int cout, int h, int w) {
    if (cin <= 0 || cout <= 0 || cin % ES_KC || h < 2 || w < 2 || (h & 1) || (w & 1)) return false;
    if ((int64_t)cin * h * w >= (1LL << 31) || (int64_t)cout * (h / 2) * (w / 2) >= (1LL << 31)) return false;
    return enc_s2_lds_bytes(h, w, 10) <= 64 * 1024;
}

// ---------------------------------------------------------------------------------------------------------------- K2
// One thread per pixel, 32 output channels per workgroup (their weights in LDS, read as broadcasts); the 3x3 x Cin patch is in
// registers.  ORDER of a sum: input channels ascending, taps 0..8 inside; the shortcut: input channels ascending, then + bias.
struct EncStemParams {
    const float *x, *w1, *wd, *bias_d, *scale1, *shift1, *scale_d, *shift_d;
    float *y_main, *y_short;
    int cin, cout, H, W;
};
constexpr int EST_CO = 32;

__global__ __launch_bounds__(256) void enc_stem_kernel(EncStemParams p) {
    __shared__ float w1l[EST_CO * 4 * 9];
    __shared__ float wdl[EST_CO * 4];
    const int tid = threadIdx.x, b = blockIdx.z, co0 = blockIdx.y * EST_CO;
    const int nco = min(EST_CO, p.cout - co0);
    for (int e = tid; e < nco * p.cin * 9; e += 256) w1l[e] = p.w1[(int64_t)co0 * p.cin * 9 + e];
    for (int e = tid; e < nco * p.cin; e += 256) wdl[e] = p.wd[(int64_t)co0 * p.cin + e];
    __syncthreads();
    const int hw = p.H * p.W, pix = blockIdx.x * 256 + tid;
    if (pix >= hw) return;
    const int y = pix / p.W, x = pix - y * p.W;
    float v[4][9];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int iy = y - 1 + t / 3, ix = x - 1 + t % 3;
            v[ci][t] = (ci < p.cin && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) ? p.x[((int64_t)b * p.cin + ci) * hw + iy * p.W + ix] : 0.f;
        }
    for (int c = 0; c < nco; ++c) {
        float s = 0.f, d = 0.f;
#pragma unroll
        for (int ci = 0; ci < 4; ++ci)
            if (ci < p.cin) {
#pragma unroll
                for (int t = 0; t < 9; ++t) s += w1l[(c * p.cin + ci) * 9 + t] * v[ci][t];
                d += wdl[c * p.cin + ci] * v[ci][4];
            }
        const int co = co0 + c;
        const int64_t o = ((int64_t)b * p.cout + co) * hw + pix;
        p.y_main[o] = fmaxf(p.scale1[co] * s + p.shift1[co], 0.f);
        if (p.bias_d) d += p.bias_d[co];
        p.y_short[o] = p.scale_d[co] * d + p.shift_d[co];
    }
}

// ---------------------------------------------------------------------------------------------------------------- K3
// Workgroup = one tile of 256 pixels x one slice of the channels of one sample: lane = 4 consecutive pixels, wave w takes the
// slice's channels w, w + 4, ...  The number of slices depends on (channels, pixels) only -- never on the batch -- so that a
// sample's bits do not depend on what it is batched with: enough slices for about 512 workgroups per sample, at least 8
// channels each (enc_tail_slices).  With one workgroup per tile (the first form) the small maps ran on one to four workgroups
// that walked up to 512 channels one after the other.
// ORDER.  pool partial of (sample, channel, tile): (v0 + v1) + (v2 + v3) per lane, then the butterfly of sis_wave_sum.
// noise: each wave adds its channels ascending, then ((wave 0 + wave 1) + wave 2) + wave 3 = the slice's sum; one slice: + bias
// and done; several: the slice sums go to the workspace [B][slices][HW] and enc_noise_finish_kernel adds them, slices
// ascending from 0, then + bias.
constexpr int ET_PIX = 256;

struct EncTailParams {
    const float *c, *res, *scale, *shift, *wn, *bn;
    float *y, *noise, *partial, *nws;
    int C, HW, tiles, slices, cps;   // cps: channels per slice (a multiple of 4)
};

inline int enc_tail_cps(int channels, int hw) {
    const int tiles = sis_cdiv(hw, ET_PIX);
    int want = sis_cdiv(512, tiles);                 // slices for about 512 workgroups per sample
    const int most = sis_cdiv(channels, 8);          // at least 8 channels per slice
    if (want > most) want = most;
    if (want < 1) want = 1;
    return sis_cdiv(sis_cdiv(channels, want), 4) * 4;
}
inline int enc_tail_slices(int channels, int hw) { return sis_cdiv(channels, enc_tail_cps(channels, hw)); }

__global__ __launch_bounds__(256) void enc_block_tail_kernel(EncTailParams p) {
    __shared__ sis_f32x4 nred[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, t = blockIdx.x, slice = blockIdx.y, b = blockIdx.z;
    const int q = t * ET_PIX + lane * 4;
    const bool valid = q < p.HW;   // HW % 4 == 0: the whole quad is inside
    const int c_end = min(p.C, (slice + 1) * p.cps);
    sis_f32x4 nacc = {0.f, 0.f, 0.f, 0.f};
    for (int c = slice * p.cps + wave; c < c_end; c += 4) {
        sis_f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (valid) {
            const int64_t idx = ((int64_t)b * p.C + c) * p.HW + q;
            const sis_f32x4 cv = *reinterpret_cast<const sis_f32x4*>(p.c + idx);
            const float sc = p.scale[c], sh = p.shift[c];
            v = cv * sc + sh;
            if (p.res) v += *reinterpret_cast<const sis_f32x4*>(p.res + idx);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            *reinterpret_cast<sis_f32x4*>(p.y + idx) = v;
        }
        if (p.partial) {
            const float s = sis_wave_sum((v[0] + v[1]) + (v[2] + v[3]));
            if (lane == 0) p.partial[((int64_t)b * p.C + c) * p.tiles + t] = s;
        }
        if (p.noise) nacc += v * p.wn[c];
    }
    if (p.noise) {
        nred[wave][lane] = nacc;
        __syncthreads();
        if (wave == 0 && valid) {
            sis_f32x4 s = ((nred[0][lane] + nred[1][lane]) + nred[2][lane]) + nred[3][lane];
            if (p.slices == 1) {
                s += p.bn[0];
                *reinterpret_cast<sis_f32x4*>(p.noise + (int64_t)b * p.HW + q) = s;
            } else {
                *reinterpret_cast<sis_f32x4*>(p.nws + ((int64_t)b * p.slices + slice) * p.HW + q) = s;
            }
        }
    }
}

// noise[b][q .. q + 3] = nws[b][0] + nws[b][1] + ... (slices ascending) + bias; grid (quads / 256, B)
__global__ __launch_bounds__(256) void enc_noise_finish_kernel(float* __restrict__ noise, const float* __restrict__ nws, const float* __restrict__ bn,
                                                               int HW, int slices) {
    const int q = (blockIdx.x * 256 + threadIdx.x) * 4, b = blockIdx.y;
    if (q >= HW) return;
    sis_f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < slices; ++i) s += *reinterpret_cast<const sis_f32x4*>(nws + ((int64_t)b * slices + i) * HW + q);
    s += bn[0];
    *reinterpret_cast<sis_f32x4*>(noise + (int64_t)b * HW + q) = s;
}

// ---------------------------------------------------------------------------------------------------------------- K4
// table: n_heads rows of 8 int64 {partial pointer, weight pointer [latent][C], bias pointer [latent], C, tiles, HW, slot, 0}.
// grid (n_heads, latent / 32, B), or (1, latent / 32, B) with sum_heads: the workgroup then adds the heads in table order into
// out[b][0][:].  A workgroup computes 32 outputs, 8 per wave, whose weight rows are read together (independent loads); every
// workgroup of a head recomputes the head's pool (the partials are a few KB up to 128 KB, from L2).  The first form (one
// workgroup per head walking all outputs four at a time) took 0.5 ms for 14 heads.
// ORDER.  pool of a channel: up to 4 tiles: tiles ascending; more: lanes take tiles lane, lane + 64, ... ascending, then the
// butterfly of sis_wave_sum; then / HW.  A head's output l: lanes take channels lane, lane + 64, ... ascending, then the
// butterfly, then + bias; with sum_heads the heads are added one after the other in table order, from 0.
constexpr int EH_COLS = 8, EH_OUT = 32, EH_PER_WAVE = 8;

__global__ __launch_bounds__(256) void enc_latent_heads_kernel(float* __restrict__ out, const int64_t* __restrict__ table, int n_heads, int latent,
                                                               int n_slots, int sum_heads, int max_channels) {
    extern __shared__ __attribute__((aligned(16))) float eh_lds[];
    float* pooled = eh_lds;                  // [max_channels]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.z;
    const int l0 = blockIdx.y * EH_OUT + wave * EH_PER_WAVE;
    const int first = sum_heads ? 0 : blockIdx.x, last = sum_heads ? n_heads : first + 1;
    float total[EH_PER_WAVE];
#pragma unroll
    for (int j = 0; j < EH_PER_WAVE; ++j) total[j] = 0.f;
    int slot = 0;
    for (int hd = first; hd < last; ++hd) {
        const int64_t* row = table + (int64_t)hd * EH_COLS;
        const float* partial = reinterpret_cast<const float*>(row[0]);
        const float* w = reinterpret_cast<const float*>(row[1]);
        const float* bias = reinterpret_cast<const float*>(row[2]);
        const int C = min((int)row[3], max_channels), tiles = (int)row[4], HW = (int)row[5];   // (C <= max_channels: the caller's contract)
        slot = (int)row[6];
        __syncthreads();                  // the previous head's pool is read
        if (tiles <= 4) {
            for (int c = tid; c < C; c += 256) {
                const float* pp = partial + ((int64_t)b * C + c) * tiles;
                float s = 0.f;
                for (int t = 0; t < tiles; ++t) s += pp[t];
                pooled[c] = s / (float)HW;
            }
        } else {
            for (int c = wave; c < C; c += 4) {
                const float* pp = partial + ((int64_t)b * C + c) * tiles;
                float s = 0.f;
                for (int t = lane; t < tiles; t += 64) s += pp[t];
                s = sis_wave_sum(s);
                if (lane == 0) pooled[c] = s / (float)HW;
            }
        }
        __syncthreads();
        float d[EH_PER_WAVE];
#pragma unroll
        for (int j = 0; j < EH_PER_WAVE; ++j) d[j] = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float pv = pooled[c];
#pragma unroll
            for (int j = 0; j < EH_PER_WAVE; ++j) {
                const int l = min(l0 + j, latent - 1);   // (outputs past the end are computed again and not stored)
                d[j] += w[(int64_t)l * C + c] * pv;
            }
        }
#pragma unroll
        for (int j = 0; j < EH_PER_WAVE; ++j) total[j] += sis_wave_sum(d[j]) + bias[min(l0 + j, latent - 1)];
    }
    if (sum_heads) slot = 0;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < EH_PER_WAVE; ++j)
            if (l0 + j < latent) out[((int64_t)b * n_slots + slot) * latent + l0 + j] = total[j];
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- C ABI

extern "C" int sis_enc_conv3x3_s2_supported(int cin, int cout, int h, int w) { return enc_s2_ok(cin, cout, h, w) ? 1 : 0; }

extern "C" int64_t sis_enc_conv3x3_s2_packed_floats(int cin, int cout, int with_shortcut) {
    if (cin <= 0 || cout <= 0) return -1;
    return (int64_t)cin * (with_shortcut ? 10 : 9) * (sis_cdiv(cout, ES_MT) * ES_MT);
}

extern "C" int sis_enc_conv3x3_s2_pack(float* packed, const float* w1, const float* wd, int cin, int cout, void* stream) {
    SIS_REQUIRE(packed && w1, "sis_enc_conv3x3_s2_pack: null pointer");
    SIS_REQUIRE(cin > 0 && cout > 0, "sis_enc_conv3x3_s2_pack: %d -> %d channels", cin, cout);
    const int taps = wd ? 10 : 9, cout_pad = sis_cdiv(cout, ES_MT) * ES_MT;
    const int64_t total = (int64_t)cin * taps * cout_pad;
    SIS_REQUIRE(total < (1LL << 31), "sis_enc_conv3x3_s2_pack: weight image too large");
    hipLaunchKernelGGL(enc_s2_pack_kernel, dim3(sis_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, packed, w1, wd, cin, cout, cout_pad, taps);
    SIS_CHECK_LAUNCH("enc_s2_pack_kernel");
    return 0;
}

extern "C" int sis_enc_conv3x3_s2(float* y_main, float* y_short, const float* x, const float* packed, const float* scale1, const float* shift1,
                                  const float* scale_d, const float* shift_d, int batch, int cin, int cout, int h, int w, void* stream) {
    if (batch <= 0) return 0;
    SIS_REQUIRE(y_main && x && packed && scale1 && shift1, "sis_enc_conv3x3_s2: null pointer");
    SIS_REQUIRE(!y_short || (scale_d && shift_d), "sis_enc_conv3x3_s2: the shortcut output needs its scale and shift");
    SIS_REQUIRE(enc_s2_ok(cin, cout, h, w), "sis_enc_conv3x3_s2: %d -> %d channels on %d x %d not supported (Cin %% 8, even H and W, staged rows within 64 KiB of LDS)", cin, cout, h, w);
    SIS_REQUIRE((((uintptr_t)packed) & 15) == 0, "sis_enc_conv3x3_s2: the packed weights must be 16-byte aligned");
    SIS_REQUIRE(batch <= 65535, "sis_enc_conv3x3_s2: more than 65 535 samples");
    EncS2Params p;
    p.x = x; p.wp = packed; p.y_main = y_main; p.y_short = y_short;
    p.scale1 = scale1; p.shift1 = shift1; p.scale_d = scale_d; p.shift_d = shift_d;
    p.cin = cin; p.cout = cout; p.cout_pad = sis_cdiv(cout, ES_MT) * ES_MT; p.H = h; p.W = w; p.Ho = h / 2; p.Wo = w / 2;
    const int taps = y_short ? 10 : 9;
    const size_t lds = (size_t)enc_s2_lds_bytes(h, w, taps);
    const dim3 grid(sis_cdiv((int64_t)p.Ho * p.Wo, ES_NT), p.cout_pad / ES_MT, batch);
    SIS_REQUIRE(grid.y <= 65535, "sis_enc_conv3x3_s2: too many output channels");
    // the LDS limit is a per-device attribute of the kernel; setting it twice is harmless, so a flag per device needs no lock
    static std::atomic<bool> attr_set[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return sis_fail("sis_enc_conv3x3_s2: cannot tell the current device");
    if (!attr_set[dev].load(std::memory_order_acquire)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&enc_conv3x3_s2_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(&enc_conv3x3_s2_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
        if (e != hipSuccess) return sis_fail("sis_enc_conv3x3_s2: cannot raise the LDS limit: %s", hipGetErrorString(e));
        attr_set[dev].store(true, std::memory_order_release);
    }
    if (y_short) hipLaunchKernelGGL(enc_conv3x3_s2_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(enc_conv3x3_s2_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, p);
    SIS_CHECK_LAUNCH("enc_conv3x3_s2_kernel");
    sis_kernel_name = "enc_conv3x3_s2_kernel";
    return 0;
}

extern "C" int sis_enc_stem_supported(int cin, int cout, int h, int w) {
    return cin >= 1 && cin <= 4 && cout >= 1 && cout <= 65535 * EST_CO && h >= 1 && w >= 1 && (int64_t)h * w * (cout > cin ? cout : cin) < (1LL << 31) ? 1 : 0;
}

extern "C" int sis_enc_stem(float* y_main, float* y_short, const float* x, const float* w1, const float* wd, const float* bias_d, const float* scale1,
                            const float* shift1, const float* scale_d, const float* shift_d, int batch, int cin, int cout, int h, int w, void* stream) {
    if (batch <= 0) return 0;
    SIS_REQUIRE(y_main && y_short && x && w1 && wd && scale1 && shift1 && scale_d && shift_d, "sis_enc_stem: null pointer");
    SIS_REQUIRE(sis_enc_stem_supported(cin, cout, h, w), "sis_enc_stem: %d -> %d channels on %d x %d not supported (1 .. 4 input channels)", cin, cout, h, w);
    SIS_REQUIRE(batch <= 65535, "sis_enc_stem: more than 65 535 samples");
    EncStemParams p;
    p.x = x; p.w1 = w1; p.wd = wd; p.bias_d = bias_d; p.scale1 = scale1; p.shift1 = shift1; p.scale_d = scale_d; p.shift_d = shift_d;
    p.y_main = y_main; p.y_short = y_short; p.cin = cin; p.cout = cout; p.H = h; p.W = w;
    const dim3 grid(sis_cdiv((int64_t)h * w, 256), sis_cdiv(cout, EST_CO), batch);
    hipLaunchKernelGGL(enc_stem_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    SIS_CHECK_LAUNCH("enc_stem_kernel");
    sis_kernel_name = "enc_stem_kernel";
    return 0;
}

extern "C" int sis_enc_block_tail_supported(int channels, int hw) {
    return channels >= 1 && hw >= 4 && hw % 4 == 0 && (int64_t)channels * hw < (1LL << 31) ? 1 : 0;
}

extern "C" int sis_enc_block_tail_tiles(int hw) { return hw > 0 ? sis_cdiv(hw, ET_PIX) : 0; }

extern "C" int64_t sis_enc_block_tail_workspace_floats(int batch, int channels, int hw) {
    if (batch <= 0 || channels <= 0 || hw <= 0) return 0;
    const int slices = enc_tail_slices(channels, hw);
    return slices > 1 ? (int64_t)batch * slices * hw : 0;
}

extern "C" int sis_enc_block_tail(float* y, float* noise, float* partial, const float* c, const float* residual, const float* scale, const float* shift,
                                  const float* noise_w, const float* noise_b, float* noise_workspace, int batch, int channels, int hw, void* stream) {
    if (batch <= 0) return 0;
    SIS_REQUIRE(y && c && scale && shift, "sis_enc_block_tail: null pointer");
    SIS_REQUIRE(!noise || (noise_w && noise_b), "sis_enc_block_tail: the noise output needs its weight and bias");
    SIS_REQUIRE(sis_enc_block_tail_supported(channels, hw), "sis_enc_block_tail: %d channels on %d pixels not supported (pixels %% 4 must be 0)", channels, hw);
    SIS_REQUIRE((((uintptr_t)y | (uintptr_t)c | (uintptr_t)residual | (uintptr_t)noise | (uintptr_t)noise_workspace) & 15) == 0,
                "sis_enc_block_tail: pointers must be 16-byte aligned");
    SIS_REQUIRE(batch <= 65535, "sis_enc_block_tail: more than 65 535 samples");
    EncTailParams p;
    p.c = c; p.res = residual; p.scale = scale; p.shift = shift; p.wn = noise_w; p.bn = noise_b; p.y = y; p.noise = noise; p.partial = partial;
    p.nws = noise_workspace;
    p.C = channels; p.HW = hw; p.tiles = sis_cdiv(hw, ET_PIX); p.cps = enc_tail_cps(channels, hw); p.slices = sis_cdiv(channels, p.cps);
    SIS_REQUIRE(!noise || p.slices == 1 || noise_workspace, "sis_enc_block_tail: the noise output needs a workspace of sis_enc_block_tail_workspace_floats floats");
    hipLaunchKernelGGL(enc_block_tail_kernel, dim3(p.tiles, p.slices, batch), dim3(256), 0, (hipStream_t)stream, p);
    SIS_CHECK_LAUNCH("enc_block_tail_kernel");
    if (noise && p.slices > 1) {
        hipLaunchKernelGGL(enc_noise_finish_kernel, dim3(sis_cdiv(hw / 4, 256), batch), dim3(256), 0, (hipStream_t)stream, noise, (const float*)noise_workspace,
                           noise_b, hw, p.slices);
        SIS_CHECK_LAUNCH("enc_noise_finish_kernel");
    }
    sis_kernel_name = "enc_block_tail_kernel";
    return 0;
}

extern "C" int sis_enc_latent_heads_supported(int max_channels, int latent) {
    return max_channels >= 1 && latent >= 1 && ((int64_t)max_channels + latent) * 4 <= 48 * 1024 ? 1 : 0;
}

extern "C" int sis_enc_latent_heads(float* out, const int64_t* table, int n_heads, int batch, int latent, int n_slots, int sum_heads, int max_channels,
                                    void* stream) {
    if (batch <= 0 || n_heads <= 0) return 0;
    SIS_REQUIRE(out && table, "sis_enc_latent_heads: null pointer");
    SIS_REQUIRE(sis_enc_latent_heads_supported(max_channels, latent), "sis_enc_latent_heads: %d channels, latent size %d not supported", max_channels, latent);
    SIS_REQUIRE(sum_heads ? n_slots == 1 : n_slots >= 1, "sis_enc_latent_heads: the summed form writes one row");
    SIS_REQUIRE(batch <= 65535, "sis_enc_latent_heads: more than 65 535 samples");
    SIS_REQUIRE(n_heads <= 65535 && sis_cdiv(latent, EH_OUT) <= 65535, "sis_enc_latent_heads: too many heads or outputs");
    const size_t lds = (size_t)max_channels * 4;
    hipLaunchKernelGGL(enc_latent_heads_kernel, dim3(sum_heads ? 1 : n_heads, sis_cdiv(latent, EH_OUT), batch), dim3(256), lds, (hipStream_t)stream, out, table,
                       n_heads, latent, n_slots, sum_heads, max_channels);
    SIS_CHECK_LAUNCH("enc_latent_heads_kernel");
    sis_kernel_name = "enc_latent_heads_kernel";
    return 0;
}
