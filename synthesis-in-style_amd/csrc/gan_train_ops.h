// GAN training from an image list (train_stylegan_2.py): the batch gather of the device-resident image loader and the two linear
// maps that turn a discriminator downsampling layer -- Blur(pad 2, 4 x 4 FIR) + 3 x 3 stride-2 convolution -- into ONE 3 x 3
// stride-1 padding-1 convolution over the four pixel phases of its input (networks/hip_conv.py ``down_conv3x3``), which then runs
// on the Winograd kernels of modconv_wino.hip / conv_wgrad_wino.hip in both directions and for the second-order terms.  Included
// from stem_conv.hip (kernels of a header live in the including translation unit, as encoder_ops.h).
//
//   K1 gan_image_batch_kernel      uint8 [N][3][S][S], int32 ids [B] -> float32 [B][3][S][S], (v / 255 - 0.5) / 0.5
//   K2 phase_split_kernel<MERGE>   [B][C][H][W] <-> [B][4C][H/2][W/2], channel (c, py, px): pixel_unshuffle / pixel_shuffle by 2
//   K3 down_weight_compose_kernel  W [Cout][Cin][3][3], f [4][4], scale -> W' [Cout][4 Cin][3][3]
//   K4 down_weight_adjoint_kernel  dW' -> dW, the transpose of K3 (scale included)
// The blur is a true convolution with f (upfirdn2d), the strided layer a correlation with W, so the 6 x 6 stride-2 kernel is
//   K[m][n] = scale * sum_{i, j} W[i][j] * f[3 - (m - i)][3 - (n - j)]      (terms with 0 <= m - i, n - j <= 3)
// and W'[co][4 ci + 2 py + px][a][b] = K[co][ci][2 a + py][2 b + px]: the 36 values of one (co, ci) pair are CONTIGUOUS in W'.
// No atomics, no cross-thread sums; every sum has a fixed order (stated at the sum).
#pragma once
#include "sis_device.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- K1
// One thread = 4 consecutive bytes of a sample (one dword load) -> one 16-byte store; per4 = 3 S S / 4 dwords per sample.
// An id outside 0 .. n_images - 1 reads nothing and writes NaN (the ids are device memory the entry cannot check).
__device__ __forceinline__ float gan_norm(unsigned v) { return ((float)v / 255.0f - 0.5f) / 0.5f; }   // ToTensor, then Normalize(0.5, 0.5)

__global__ __launch_bounds__(256) void gan_image_batch_kernel(float* __restrict__ out, const uint8_t* __restrict__ src, const int* __restrict__ ids,
                                                              int n_images, int64_t per4, int64_t total4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int64_t b = i / per4, e = i - b * per4;
    const int id = ids[b];
    sis_f32x4 v;
    if (id >= 0 && id < n_images) {
        const unsigned q = *reinterpret_cast<const unsigned*>(src + ((int64_t)id * per4 + e) * 4);
        v = sis_f32x4{gan_norm(q & 255u), gan_norm((q >> 8) & 255u), gan_norm((q >> 16) & 255u), gan_norm(q >> 24)};
    } else {
        const float nan = __builtin_nanf("");
        v = sis_f32x4{nan, nan, nan, nan};
    }
    *reinterpret_cast<sis_f32x4*>(out + i * 4) = v;
}

// sample sizes that are no multiple of 4 bytes (odd S): one element per thread
__global__ __launch_bounds__(256) void gan_image_batch_scalar_kernel(float* __restrict__ out, const uint8_t* __restrict__ src,
                                                                     const int* __restrict__ ids, int n_images, int64_t per, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / per, e = i - b * per;
    const int id = ids[b];
    out[i] = (id >= 0 && id < n_images) ? gan_norm(src[(int64_t)id * per + e]) : __builtin_nanf("");
}

// ---------------------------------------------------------------------------------------------------------------- K2
// full [B][C][H][W], phases [B][4C][H/2][W/2]: phases[b][4 c + 2 py + px][i][j] = full[b][c][2 i + py][2 j + px].
// Vector form (W % 8 == 0): one thread = 8 consecutive pixels of a full row (two 16-byte accesses) = 4 consecutive pixels of
// the two phase rows (2 (r & 1) + px, r >> 1), px = 0, 1 (one 16-byte access each).  MERGE copies the other way.
template <bool MERGE>
__global__ __launch_bounds__(256) void phase_split_kernel(float* __restrict__ dst, const float* __restrict__ src, int H, int W, int64_t total8) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total8) return;
    const int w8 = W >> 3, hw = H * W, qhw = hw >> 2, w2 = W >> 1;
    const int j8 = (int)(i % w8);
    const int64_t t = i / w8;
    const int r = (int)(t % H);
    const int64_t bc = t / H;
    const int64_t full = bc * hw + (int64_t)r * W + 8 * j8;
    const int64_t ph0 = (bc * 4 + 2 * (r & 1)) * qhw + (int64_t)(r >> 1) * w2 + 4 * j8;   // px = 0; px = 1 is one plane further
    if constexpr (MERGE) {
        const sis_f32x4 e = *reinterpret_cast<const sis_f32x4*>(src + ph0), o = *reinterpret_cast<const sis_f32x4*>(src + ph0 + qhw);
        *reinterpret_cast<sis_f32x4*>(dst + full) = sis_f32x4{e[0], o[0], e[1], o[1]};
        *reinterpret_cast<sis_f32x4*>(dst + full + 4) = sis_f32x4{e[2], o[2], e[3], o[3]};
    } else {
        const sis_f32x4 a = *reinterpret_cast<const sis_f32x4*>(src + full), c = *reinterpret_cast<const sis_f32x4*>(src + full + 4);
        *reinterpret_cast<sis_f32x4*>(dst + ph0) = sis_f32x4{a[0], a[2], c[0], c[2]};
        *reinterpret_cast<sis_f32x4*>(dst + ph0 + qhw) = sis_f32x4{a[1], a[3], c[1], c[3]};
    }
}

// any even H and W: one element per thread, indexed on the phase side
template <bool MERGE>
__global__ __launch_bounds__(256) void phase_split_scalar_kernel(float* __restrict__ dst, const float* __restrict__ src, int H, int W, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int w2 = W >> 1, h2 = H >> 1;
    const int j = (int)(i % w2);
    int64_t t = i / w2;
    const int r = (int)(t % h2);
    t /= h2;
    const int ph = (int)(t & 3);
    const int64_t bc = t >> 2;
    const int64_t full = bc * H * W + (int64_t)(2 * r + (ph >> 1)) * W + 2 * j + (ph & 1);
    if constexpr (MERGE) dst[full] = src[i];
    else dst[i] = src[full];
}

// ---------------------------------------------------------------------------------------------------------------- K3 / K4
// One thread = one (co, ci) pair: 9 weights in, 36 contiguous values out (nine 16-byte stores), or the reverse.
// ORDER of K[m][n]: i = 0, 1, 2 outer, j = 0, 1, 2 inner, terms outside the FIR skipped; the scale multiplies the finished sum.
__global__ __launch_bounds__(256) void down_weight_compose_kernel(float* __restrict__ wp, const float* __restrict__ w, const float* __restrict__ fir,
                                                                  float scale, int64_t pairs) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= pairs) return;
    float f[16], k3[9], o[36];
#pragma unroll
    for (int e = 0; e < 16; ++e) f[e] = fir[e];
#pragma unroll
    for (int e = 0; e < 9; ++e) k3[e] = w[p * 9 + e];
#pragma unroll
    for (int m = 0; m < 6; ++m)
#pragma unroll
        for (int n = 0; n < 6; ++n) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int u = m - i, v = n - j;
                    if (u >= 0 && u <= 3 && v >= 0 && v <= 3) s += k3[i * 3 + j] * f[(3 - u) * 4 + (3 - v)];
                }
            o[(2 * (m & 1) + (n & 1)) * 9 + (m >> 1) * 3 + (n >> 1)] = scale * s;
        }
    float* dst = wp + p * 36;
#pragma unroll
    for (int q = 0; q < 9; ++q) *reinterpret_cast<sis_f32x4*>(dst + 4 * q) = sis_f32x4{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
}

// dW[i][j] = scale * sum_{u, v} dW'[(i + u) & 1, (j + v) & 1][(i + u) >> 1][(j + v) >> 1] * f[3 - u][3 - v].
// ORDER: u = 0 .. 3 outer, v = 0 .. 3 inner; the scale multiplies the finished sum.
__global__ __launch_bounds__(256) void down_weight_adjoint_kernel(float* __restrict__ dw, const float* __restrict__ dwp, const float* __restrict__ fir,
                                                                  float scale, int64_t pairs) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= pairs) return;
    float f[16], g[36];
#pragma unroll
    for (int e = 0; e < 16; ++e) f[e] = fir[e];
    const float* src = dwp + p * 36;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const sis_f32x4 t = *reinterpret_cast<const sis_f32x4*>(src + 4 * q);
        g[4 * q] = t[0]; g[4 * q + 1] = t[1]; g[4 * q + 2] = t[2]; g[4 * q + 3] = t[3];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float s = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int m = i + u, n = j + v;
                    s += g[(2 * (m & 1) + (n & 1)) * 9 + (m >> 1) * 3 + (n >> 1)] * f[(3 - u) * 4 + (3 - v)];
                }
            dw[p * 9 + i * 3 + j] = scale * s;
        }
}

inline bool gan_aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

template <bool MERGE>
int gan_phase_launch(const char* name, float* dst, const float* src, int batch, int channels, int h, int w, void* stream) {
    SIS_REQUIRE(dst && src, "%s: null pointer", name);
    SIS_REQUIRE(batch > 0 && channels > 0 && h > 0 && w > 0, "%s: empty tensor", name);
    SIS_REQUIRE(sis_phase_split_supported(h, w), "%s: %d x %d not supported (H and W must be even)", name, h, w);
    const int64_t total = (int64_t)batch * channels * h * w;
    hipStream_t st = (hipStream_t)stream;
    if (w % 8 == 0 && gan_aligned16(dst) && gan_aligned16(src)) {
        const int64_t blocks = (total / 8 + 255) / 256;
        SIS_REQUIRE(blocks < (1LL << 31), "%s: tensor too large", name);
        phase_split_kernel<MERGE><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(dst, src, h, w, total / 8);
    } else {
        const int64_t blocks = (total + 255) / 256;
        SIS_REQUIRE(blocks < (1LL << 31), "%s: tensor too large", name);
        phase_split_scalar_kernel<MERGE><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(dst, src, h, w, total);
    }
    SIS_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace

extern "C" int sis_gan_image_batch(float* out, const uint8_t* images, const int* ids, int64_t n_images, int batch, int size, void* stream) {
    SIS_REQUIRE(out && images && ids, "sis_gan_image_batch: null pointer");
    SIS_REQUIRE(n_images > 0 && n_images < (1LL << 31) && batch > 0 && size > 0 && size <= 16384, "sis_gan_image_batch: %lld images, batch %d, size %d",
                (long long)n_images, batch, size);
    const int64_t per = 3LL * size * size, total = per * batch;
    hipStream_t st = (hipStream_t)stream;
    if (per % 4 == 0 && gan_aligned16(out) && (((uintptr_t)images) & 3) == 0) {
        const int64_t blocks = (total / 4 + 255) / 256;
        SIS_REQUIRE(blocks < (1LL << 31), "sis_gan_image_batch: batch too large");
        gan_image_batch_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(out, images, ids, (int)n_images, per / 4, total / 4);
    } else {
        const int64_t blocks = (total + 255) / 256;
        SIS_REQUIRE(blocks < (1LL << 31), "sis_gan_image_batch: batch too large");
        gan_image_batch_scalar_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(out, images, ids, (int)n_images, per, total);
    }
    SIS_CHECK_LAUNCH("sis_gan_image_batch");
    return 0;
}

extern "C" int sis_phase_split_supported(int h, int w) { return (h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0) ? 1 : 0; }

extern "C" int sis_phase_split(float* phases, const float* x, int batch, int channels, int h, int w, void* stream) {
    return gan_phase_launch<false>("sis_phase_split", phases, x, batch, channels, h, w, stream);
}

extern "C" int sis_phase_merge(float* x, const float* phases, int batch, int channels, int h, int w, void* stream) {
    return gan_phase_launch<true>("sis_phase_merge", x, phases, batch, channels, h, w, stream);
}

extern "C" int sis_down_weight_compose_supported(int fir_h, int fir_w) { return (fir_h == 4 && fir_w == 4) ? 1 : 0; }

extern "C" int sis_down_weight_compose(float* w_phases, const float* w, const float* fir, int fir_h, int fir_w, float scale, int cout, int cin,
                                       void* stream) {
    SIS_REQUIRE(w_phases && w && fir, "sis_down_weight_compose: null pointer");
    SIS_REQUIRE(sis_down_weight_compose_supported(fir_h, fir_w), "sis_down_weight_compose: a %d x %d FIR is not supported (4 x 4 only)", fir_h, fir_w);
    SIS_REQUIRE(cout > 0 && cin > 0, "sis_down_weight_compose: %d -> %d channels", cin, cout);
    SIS_REQUIRE(gan_aligned16(w_phases), "sis_down_weight_compose: the composed weight must be 16-byte aligned");
    const int64_t pairs = (int64_t)cout * cin;
    SIS_REQUIRE(pairs < (1LL << 31), "sis_down_weight_compose: weight too large");
    down_weight_compose_kernel<<<dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(w_phases, w, fir, scale, pairs);
    SIS_CHECK_LAUNCH("sis_down_weight_compose");
    return 0;
}

extern "C" int sis_down_weight_compose_adjoint(float* dw, const float* dw_phases, const float* fir, int fir_h, int fir_w, float scale, int cout,
                                               int cin, void* stream) {
    SIS_REQUIRE(dw && dw_phases && fir, "sis_down_weight_compose_adjoint: null pointer");
    SIS_REQUIRE(sis_down_weight_compose_supported(fir_h, fir_w), "sis_down_weight_compose_adjoint: a %d x %d FIR is not supported (4 x 4 only)", fir_h,
                fir_w);
    SIS_REQUIRE(cout > 0 && cin > 0, "sis_down_weight_compose_adjoint: %d -> %d channels", cin, cout);
    SIS_REQUIRE(gan_aligned16(dw_phases), "sis_down_weight_compose_adjoint: the composed gradient must be 16-byte aligned");
    const int64_t pairs = (int64_t)cout * cin;
    SIS_REQUIRE(pairs < (1LL << 31), "sis_down_weight_compose_adjoint: weight too large");
    down_weight_adjoint_kernel<<<dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(dw, dw_phases, fir, scale, pairs);
    SIS_CHECK_LAUNCH("sis_down_weight_compose_adjoint");
    return 0;
}
