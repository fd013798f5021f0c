// DocUFCN segmenter (reference: networks/doc_ufcn/doc_ufcn.py), fp32 NCHW: the kernels its training step needs beyond the rest
// of the library.
//
//   sis_dconv3x3            3x3 stride-1 convolution, dilation d, padding d (doc_ufcn.py:51-59), any Cin / Cout >= 1: an
//                           implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products).  M = output channels, N = pixels of
//                           one sample, K = (tap, input channel).  A tap whose shifted window lies wholly in the zero padding
//                           for the workgroup's pixel rows / columns is skipped (with d >= H only the centre tap is left).
//                           Optional per-channel bias.  The data gradient is the same kernel on adjoint weights
//                           (sis_dconv3x3_adjoint: channel axes swapped, taps rotated by 180 degrees).
//   sis_dconv3x3_wgrad      dW [Cout][Cin*taps] = sum over pixels of dY x shifted X (taps 9: the dilated 3x3, taps 1: a 1x1
//                           product, the transposed 2x2 convolution's weight gradient); pixels split in fixed slices, one
//                           partial per slice, summed in slice order by a second launch: deterministic, no float atomics.
//   sis_channel_sum         db[c] = sum over (b, pixels) of dY, fixed-order tree per channel (bias gradients).
//   sis_pixel_shuffle2      out[b][c][2y+i][2x+j] = in[b][4c+2i+j][y][x] (+ bias[c]): ConvTranspose2d(k=2, s=2) after its
//                           per-pixel [Cin] -> [4*Cout] product, and nn.PixelShuffle(2) straight into the decoder's
//                           concatenation buffer; backward = the inverse gather.
//   sis_transpose2d         out[c][r] = in[r][c] (ConvTranspose2d weights [Cin][4*Cout] <-> the 1x1 product's [4*Cout][Cin]).
//   sis_bn_drop_fwd/bwd     train-mode BatchNorm (statistics from sis_bn_stats) + ReLU + Dropout; y may be written into a
//                           channel slice of a wider buffer (the decoder's concatenation).  Dropout draws from the counter
//                           stream of vit_common.h (sis_drop_quad, device seed word), one bit per element kept for the
//                           backward: (relu output > 0) & keep.  Eval mode: running statistics, no dropout.
//   sis_weighted_ce_fwd/bwd nn.CrossEntropyLoss(weight=w) (mean reduction: sum w_y nll / sum w_y) on [B, K, H, W] logits.
//   sis_adam_clip_norm/step GradientClipAdam: a partial-norm launch over every gradient chunk, then one launch that clips,
//                           adds L2 weight decay, updates exp_avg / exp_avg_sq and the parameter with the bias correction of a
//                           device-side step counter; hyper-parameters from device memory (graph-capturable).
#include "vit_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ dilated 3x3 convolution

constexpr int DC_KC = 16;    // K rows (input channels of one tap, or pixels for the weight gradient) per LDS stage
constexpr int DC_PAD = 4;    // LDS row padding (floats)

// acc[j] of lane l holds C[row = 8 * (j / 4) + 4 * (l / 32) + j % 4][col = l % 32]; A operand A[m = l % 32][k = l / 32],
// B operand B[k = l / 32][n = l % 32].
template <int WM>   // waves along M (2: 64 x 64 tile, 1: 32 x 128 tile)
__global__ __launch_bounds__(256) void dconv3x3_kernel(float* __restrict__ out, const float* __restrict__ x,
                                                       const float* __restrict__ w, const float* __restrict__ bias, int Cin,
                                                       int Cout, int H, int W, int d) {
    constexpr int TM = 32 * WM, TN = 32 * (4 / WM);
    __shared__ float As[DC_KC][TM + DC_PAD];
    __shared__ float Bs[DC_KC][TN + DC_PAD];
    const int HW = H * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int p0 = blockIdx.x * TN, co0 = blockIdx.y * TM, b = blockIdx.z;
    const float* xb = x + (int64_t)b * Cin * HW;

    // rows / columns this tile touches (a tile of whole rows spans every column)
    const int plast = min(p0 + TN, HW) - 1;
    const int ya = p0 / W, yb = plast / W;
    const int xa = ya == yb ? p0 % W : 0, xb_ = ya == yb ? plast % W : W - 1;

    sis_f32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;

    for (int t = 0; t < 9; ++t) {
        const int dy = d * (t / 3 - 1), dx = d * (t % 3 - 1);
        if (ya + dy > H - 1 || yb + dy < 0 || xa + dx > W - 1 || xb_ + dx < 0) continue;   // wholly in the zero padding
        for (int ci0 = 0; ci0 < Cin; ci0 += DC_KC) {
            __syncthreads();
            for (int e = tid; e < DC_KC * TM; e += 256) {
                const int k = e / TM, m = e % TM;
                const int ci = ci0 + k, co = co0 + m;
                As[k][m] = (ci < Cin && co < Cout) ? w[((int64_t)co * Cin + ci) * 9 + t] : 0.f;
            }
            for (int e = tid; e < DC_KC * TN; e += 256) {
                const int k = e / TN, n = e % TN;
                const int ci = ci0 + k, p = p0 + n;
                float v = 0.f;
                if (ci < Cin && p < HW) {
                    const int ys = p / W + dy, xs = p % W + dx;
                    if (ys >= 0 && ys < H && xs >= 0 && xs < W) v = xb[(int64_t)ci * HW + ys * W + xs];
                }
                Bs[k][n] = v;
            }
            __syncthreads();
            const int kn = min(DC_KC, Cin - ci0);
            for (int kk = 0; kk < kn; kk += 2) {
                const float a = As[kk + (lane >> 5)][wm * 32 + (lane & 31)];
                const float bv = Bs[kk + (lane >> 5)][wn * 32 + (lane & 31)];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc, 0, 0, 0);
            }
        }
    }
    const int p = p0 + wn * 32 + (lane & 31);
    if (p >= HW) return;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int co = co0 + wm * 32 + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3);
        if (co < Cout) out[((int64_t)b * Cout + co) * HW + p] = acc[j] + (bias ? bias[co] : 0.f);
    }
}

// wa[ci][co][t] = w[co][ci][8 - t]
__global__ void dconv3x3_adjoint_kernel(float* __restrict__ wa, const float* __restrict__ w, int Cin, int Cout) {
    const int64_t n = (int64_t)Cin * Cout * 9;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int t = (int)(i % 9);
        const int64_t r = i / 9;
        const int co = (int)(r % Cout), ci = (int)(r / Cout);
        wa[i] = w[((int64_t)co * Cin + ci) * 9 + (8 - t)];
    }
}

// Weight gradient, one pixel slice per blockIdx.z: ws[z][co][n] = sum over the slice's pixels of dY[co][p] * X[ci][p + off(t)],
// n = ci * taps + t.  64 x 64 tile, K = DC_KC pixels per stage.
__global__ __launch_bounds__(256) void dconv3x3_wgrad_kernel(float* __restrict__ ws, const float* __restrict__ gy,
                                                             const float* __restrict__ x, int B, int Cin, int Cout, int H, int W,
                                                             int d, int taps, int64_t per_slice) {
    __shared__ float As[DC_KC][64 + DC_PAD];
    __shared__ float Bs[DC_KC][64 + DC_PAD];
    const int HW = H * W, N = Cin * taps;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int n0 = blockIdx.x * 64, co0 = blockIdx.y * 64;
    const int64_t P = (int64_t)B * HW;
    const int64_t lo = blockIdx.z * per_slice, hi = min(P, lo + per_slice);
    sis_f32x16 acc;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    for (int64_t q0 = lo; q0 < hi; q0 += DC_KC) {
        __syncthreads();
        // pixel q0 + k of the slice: sample q / HW, pixel q % HW (a stage may straddle two samples; pixels >= hi load 0)
        for (int e = tid; e < DC_KC * 64; e += 256) {
            const int m = e / DC_KC, k = e % DC_KC;
            const int co = co0 + m;
            const int64_t q = q0 + k;
            As[k][m] = (co < Cout && q < hi) ? gy[((q / HW) * Cout + co) * HW + q % HW] : 0.f;
        }
        for (int e = tid; e < DC_KC * 64; e += 256) {
            const int nl = e / DC_KC, k = e % DC_KC;
            const int n = n0 + nl;
            const int64_t q = q0 + k;
            float v = 0.f;
            if (n < N && q < hi) {
                const int ci = n / taps, t = n % taps;
                const int64_t b = q / HW;
                const int p = (int)(q - b * HW);
                const int ys = p / W + (taps == 9 ? d * (t / 3 - 1) : 0), xs = p % W + (taps == 9 ? d * (t % 3 - 1) : 0);
                if (ys >= 0 && ys < H && xs >= 0 && xs < W) v = x[(b * Cin + ci) * HW + ys * W + xs];
            }
            Bs[k][nl] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < DC_KC; kk += 2) {
            const float a = As[kk + (lane >> 5)][wm * 32 + (lane & 31)];
            const float bv = Bs[kk + (lane >> 5)][wn * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc, 0, 0, 0);
        }
    }
    const int n = n0 + wn * 32 + (lane & 31);
    if (n >= N) return;
    float* wz = ws + (int64_t)blockIdx.z * Cout * N;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int co = co0 + wm * 32 + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3);
        if (co < Cout) wz[(int64_t)co * N + n] = acc[j];
    }
}

__global__ void slice_sum_kernel(float* __restrict__ out, const float* __restrict__ ws, int64_t n, int slices) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float s = 0.f;
        for (int z = 0; z < slices; ++z) s += ws[(int64_t)z * n + i];
        out[i] = s;
    }
}

// db[c] = sum over b, p of dy[b][c][p] (rows of dy are `bstride` floats apart per sample)
__global__ __launch_bounds__(256) void channel_sum_kernel(float* __restrict__ db, const float* __restrict__ dy, int B, int C,
                                                          int HW) {
    __shared__ float red[4];
    const int c = blockIdx.x;
    float s = 0.f;
    for (int b = 0; b < B; ++b) {
        const float* row = dy + ((int64_t)b * C + c) * HW;
        for (int p = threadIdx.x; p < HW; p += 256) s += row[p];
    }
    s = sis_block_sum4(s, red);
    if (threadIdx.x == 0) db[c] = s;
}

// ------------------------------------------------------------------------------------------------ shuffle / transpose

// forward: out[b][c][2y+i][2x+j] = in[b][4c+2i+j][y][x] + bias[c]; backward (inverse = 1): in <- out, a gather as well
// (the wide map's samples are `wide_bstride` floats apart: it may be a channel slice of the decoder's concatenation buffer)
__global__ void shuffle2_kernel(float* __restrict__ dst, const float* __restrict__ src, const float* __restrict__ bias, int C, int H,
                                int W, int64_t wide_bstride, int64_t total, int inverse) {
    const int W2 = 2 * W, H2 = 2 * H;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        // i enumerates the wide map [B][C][2H][2W]
        const int X = (int)(i % W2);
        const int64_t r = i / W2;
        const int Y = (int)(r % H2);
        const int64_t bc = r / H2;
        const int c = (int)(bc % C);
        const int64_t b = bc / C;
        const int64_t wi = b * wide_bstride + ((int64_t)c * H2 + Y) * W2 + X;
        const int64_t j = ((b * 4 * C + 4 * c + 2 * (Y & 1) + (X & 1)) * H + (Y >> 1)) * W + (X >> 1);
        if (inverse) dst[j] = src[wi];
        else dst[wi] = src[j] + (bias ? bias[c] : 0.f);
    }
}

__global__ void transpose2d_kernel(float* __restrict__ out, const float* __restrict__ in, int rows, int cols) {
    const int64_t n = (int64_t)rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i / rows), r = (int)(i % rows);   // out[c][r]
        out[i] = in[(int64_t)r * cols + c];
    }
}

// ------------------------------------------------------------------------------------------------ BN + ReLU + Dropout

// Element e of the [B][C][HW] map (row-major) belongs to float4 i = e / 4.  Dropout: quad i of the site, sis_drop_quad.
// Mask: bit i % 64 of 64-bit word (i / 64) * 4 + e % 4 (one ballot per float4 component and wave).
__global__ __launch_bounds__(256) void bn_drop_fwd_kernel(float* __restrict__ y, int64_t y_bstride, const float* __restrict__ x,
                                                          const float* __restrict__ mean, const float* __restrict__ scale_src,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, int C,
                                                          int HW4, int64_t total4, int eval, float eps,
                                                          const unsigned long long* __restrict__ seed, unsigned site,
                                                          unsigned thr16, float keep_scale, unsigned long long* __restrict__ mask) {
    const SisDropKey key = sis_drop_key(thr16 ? seed : nullptr, site);
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t rounded = (total4 + 63) / 64 * 64;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rounded; i += stride) {   // wave-uniform trip count
        bool on[4] = {false, false, false, false};
        if (i < total4) {
            const int64_t plane = i / HW4;
            const int r4 = (int)(i - plane * HW4);
            const int c = (int)(plane % C);
            const int64_t b = plane / C;
            const float m = mean[c];
            const float is = eval ? 1.f / sqrtf(scale_src[c] + eps) : scale_src[c];
            const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
            const float4 v = reinterpret_cast<const float4*>(x)[i];
            float f[4] = {1.f, 1.f, 1.f, 1.f};
            if (thr16) sis_drop_quad(key, (unsigned)i, thr16, keep_scale, f);
            const float in[4] = {v.x, v.y, v.z, v.w};
            float o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float a = fmaxf(__builtin_fmaf(g * is, in[q] - m, bt), 0.f);
                on[q] = a > 0.f && f[q] != 0.f;
                o[q] = a * f[q];
            }
            *reinterpret_cast<float4*>(y + b * y_bstride + (int64_t)c * HW4 * 4 + (int64_t)r4 * 4) = make_float4(o[0], o[1], o[2], o[3]);
        }
        if (mask) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned long long bits = __ballot(on[q]);
                if ((threadIdx.x & 63) == 0 && i - (threadIdx.x & 63) < total4) mask[((i >> 6) << 2) + q] = bits;
            }
        }
    }
}

constexpr int BD_SLICE4 = 4096;   // float4s of one channel per backward-reduction workgroup

struct BnDropBwdArgs {
    const float* dy1; int64_t dy1_bstride;   // gradient of y (may be a channel slice of a wider buffer)
    const float* dy2;                        // NULL or a second, contiguous [B][C][HW] gradient added to it
    const float* x; const float* mean; const float* invstd;
    const unsigned long long* mask; float keep_scale;
    int B, C, HW4;
};

__device__ __forceinline__ void bn_drop_grad4(const BnDropBwdArgs& a, int b, int c, int r4, float gate_out[4], float xh[4]) {
    const int64_t i = ((int64_t)b * a.C + c) * a.HW4 + r4;   // float4 index in the [B][C][HW] map
    const float4 g1 = *reinterpret_cast<const float4*>(a.dy1 + b * a.dy1_bstride + ((int64_t)c * a.HW4 + r4) * 4);
    float g[4] = {g1.x, g1.y, g1.z, g1.w};
    if (a.dy2) {
        const float4 g2 = reinterpret_cast<const float4*>(a.dy2)[i];
        g[0] += g2.x; g[1] += g2.y; g[2] += g2.z; g[3] += g2.w;
    }
    const float4 xv = reinterpret_cast<const float4*>(a.x)[i];
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
    const float m = a.mean[c], is = a.invstd[c];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool on = (a.mask[((i >> 6) << 2) + q] >> (i & 63)) & 1ull;
        gate_out[q] = on ? g[q] * a.keep_scale : 0.f;
        xh[q] = (xs[q] - m) * is;
    }
}

// partial[c][s] = (sum g', sum g' * xhat) over slice s of channel c, in double: sum of the gated g, and of g * (x - mean), with
// exact products, scaled by keep_scale (and invstd) once at the end.  dgamma[c] and dbeta[c] are sums of gradients of both signs
// that cancel to a small part of sum |terms|: an fp32 running sum over fp32-rounded terms left ~1e-8 - 6e-8 sum |terms|, which is
// more than 1e-5 of the result on the channels that cancel to 1e-3 (a few per thousand).  Summed this way dbeta is exact up to its
// final rounding, and dgamma up to the fp32 statistics it is given.  The kernel is bound by its loads.
__global__ __launch_bounds__(256) void bn_drop_bwd_reduce_kernel(double* __restrict__ partial, BnDropBwdArgs a, int S) {
    __shared__ double red[4];
    const int c = blockIdx.x / S, s = blockIdx.x % S;
    const int64_t n4 = (int64_t)a.B * a.HW4, lo = (int64_t)s * BD_SLICE4, hi = min(n4, lo + BD_SLICE4);
    const double m = a.mean[c];
    double s0 = 0., s1 = 0.;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 256) {
        const int b = (int)(j / a.HW4), r4 = (int)(j % a.HW4);
        const int64_t i = ((int64_t)b * a.C + c) * a.HW4 + r4;
        const float4 g1 = *reinterpret_cast<const float4*>(a.dy1 + b * a.dy1_bstride + ((int64_t)c * a.HW4 + r4) * 4);
        float g[4] = {g1.x, g1.y, g1.z, g1.w};
        if (a.dy2) {   // the same fp32 sum as bn_drop_grad4: the gradient the apply kernel uses
            const float4 g2 = reinterpret_cast<const float4*>(a.dy2)[i];
            g[0] += g2.x; g[1] += g2.y; g[2] += g2.z; g[3] += g2.w;
        }
        const float4 xv = reinterpret_cast<const float4*>(a.x)[i];
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool on = (a.mask[((i >> 6) << 2) + q] >> (i & 63)) & 1ull;
            const double gq = on ? (double)g[q] : 0.;
            s0 += gq;
            s1 += gq * ((double)xs[q] - m);
        }
    }
    s0 = sis_block_sum4(s0, red);
    s1 = sis_block_sum4(s1, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = s0 * (double)a.keep_scale;
        partial[2 * blockIdx.x + 1] = s1 * (double)a.keep_scale * (double)a.invstd[c];
    }
}

__global__ void bn_drop_bwd_finish_kernel(float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ coef,
                                          const double* __restrict__ partial, int C, int S, float inv_n) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double d0 = 0., d1 = 0.;
    for (int s = 0; s < S; ++s) { d0 += partial[2 * (c * S + s)]; d1 += partial[2 * (c * S + s) + 1]; }
    const float s0 = (float)d0, s1 = (float)d1;
    dbeta[c] = s0;
    dgamma[c] = s1;
    coef[2 * c] = s0 * inv_n;
    coef[2 * c + 1] = s1 * inv_n;
}

__global__ __launch_bounds__(256) void bn_drop_bwd_apply_kernel(float* __restrict__ dx, BnDropBwdArgs a,
                                                                const float* __restrict__ gamma, const float* __restrict__ coef,
                                                                int64_t total4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        const int64_t plane = i / a.HW4;
        const int r4 = (int)(i - plane * a.HW4);
        const int c = (int)(plane % a.C), b = (int)(plane / a.C);
        float g[4], xh[4];
        bn_drop_grad4(a, b, c, r4, g, xh);
        const float k = (gamma ? gamma[c] : 1.f) * a.invstd[c], c0 = coef[2 * c], c1 = coef[2 * c + 1];
        float o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = k * (g[q] - c0 - xh[q] * c1);
        reinterpret_cast<float4*>(dx)[i] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ------------------------------------------------------------------------------------------------ weighted cross-entropy

constexpr int CE_BLOCKS = 256;
constexpr int CE_MAX_K = 32;

__device__ __forceinline__ int ce_label(const int64_t* labels, int64_t i, int K) {
    const int64_t y = labels[i];
    return (y >= 0 && y < K) ? (int)y : -1;   // (out-of-range labels carry no weight)
}

// partial[blk] = (sum w_y * nll, sum w_y) over a fixed pixel range
__global__ __launch_bounds__(256) void wce_fwd_kernel(float* __restrict__ partial, const float* __restrict__ logits,
                                                      const int64_t* __restrict__ labels, const float* __restrict__ weight, int K,
                                                      int HW, int64_t P) {
    __shared__ float red[4];
    const int64_t per = (P + CE_BLOCKS - 1) / CE_BLOCKS, lo = blockIdx.x * per, hi = min(P, lo + per);
    float sl = 0.f, sw = 0.f;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const int64_t b = i / HW;
        const int p = (int)(i % HW);
        const int y = ce_label(labels, i, K);
        if (y < 0) continue;
        const float* l = logits + b * K * HW + p;
        float mx = -INFINITY;
        for (int k = 0; k < K; ++k) mx = fmaxf(mx, l[(int64_t)k * HW]);
        float se = 0.f;
        for (int k = 0; k < K; ++k) se += expf(l[(int64_t)k * HW] - mx);
        const float nll = logf(se) + mx - l[(int64_t)y * HW];
        const float w = weight ? weight[y] : 1.f;
        sl = __builtin_fmaf(w, nll, sl);
        sw += w;
    }
    sl = sis_block_sum4(sl, red);
    sw = sis_block_sum4(sw, red);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = sl; partial[2 * blockIdx.x + 1] = sw; }
}

// loss[0] = sum w nll / sum w; stats[0] = sum w
__global__ void wce_finish_kernel(float* __restrict__ loss, float* __restrict__ stats, const float* __restrict__ partial) {
    if (threadIdx.x != 0) return;
    float sl = 0.f, sw = 0.f;
    for (int i = 0; i < CE_BLOCKS; ++i) { sl += partial[2 * i]; sw += partial[2 * i + 1]; }
    loss[0] = sl / sw;
    stats[0] = sw;
}

__global__ __launch_bounds__(256) void wce_bwd_kernel(float* __restrict__ grad, const float* __restrict__ logits,
                                                      const int64_t* __restrict__ labels, const float* __restrict__ weight,
                                                      const float* __restrict__ stats, const float* __restrict__ grad_loss, int K,
                                                      int HW, int64_t P) {
    const float g = grad_loss[0] / stats[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / HW;
        const int p = (int)(i % HW);
        const int y = ce_label(labels, i, K);
        const float* l = logits + b * K * HW + p;
        float* o = grad + b * K * HW + p;
        if (y < 0) {
            for (int k = 0; k < K; ++k) o[(int64_t)k * HW] = 0.f;
            continue;
        }
        float mx = -INFINITY;
        for (int k = 0; k < K; ++k) mx = fmaxf(mx, l[(int64_t)k * HW]);
        float se = 0.f;
        for (int k = 0; k < K; ++k) se += expf(l[(int64_t)k * HW] - mx);
        const float gw = g * (weight ? weight[y] : 1.f), inv = 1.f / se;
        for (int k = 0; k < K; ++k) o[(int64_t)k * HW] = gw * (expf(l[(int64_t)k * HW] - mx) * inv - (k == y ? 1.f : 0.f));
    }
}

// ------------------------------------------------------------------------------------------------ GradientClipAdam

constexpr int ADAM_CHUNK = 65536;
// table row: param, grad, exp_avg, exp_avg_sq, count | group << 48
// hyper: per group g (< 4) {lr, beta1, beta2, eps, weight_decay} at 5 g, then max_norm at 20

__global__ __launch_bounds__(256) void adam_clip_norm_kernel(float* __restrict__ partial, const int64_t* __restrict__ table,
                                                             int* __restrict__ step) {
    __shared__ float red[4];
    const int64_t* row = table + (int64_t)blockIdx.x * 5;
    const float* __restrict__ gr = reinterpret_cast<const float*>(row[1]);
    const int n = (int)(row[4] & 0xffffffffll);
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s = __builtin_fmaf(gr[i], gr[i], s);
    s = sis_block_sum4(s, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = s;
        if (blockIdx.x == 0) step[0] += 1;   // read by the update launch that follows (stream order)
    }
}

__global__ __launch_bounds__(256) void adam_step_kernel(const int64_t* __restrict__ table, const float* __restrict__ partial,
                                                        int n_chunks, const float* __restrict__ hyper,
                                                        const int* __restrict__ step) {
    __shared__ float red[4];
    // the total norm: every workgroup sums the same partials in the same order
    float s = 0.f;
    for (int i = threadIdx.x; i < n_chunks; i += 256) s += partial[i];
    s = sis_block_sum4(s, red);
    const float max_norm = hyper[20];
    const float coef = fminf(max_norm / (sqrtf(s) + 1e-6f), 1.f);

    const int64_t* row = table + (int64_t)blockIdx.x * 5;
    float* __restrict__ p = reinterpret_cast<float*>(row[0]);
    const float* __restrict__ gr = reinterpret_cast<const float*>(row[1]);
    float* __restrict__ m = reinterpret_cast<float*>(row[2]);
    float* __restrict__ v = reinterpret_cast<float*>(row[3]);
    const int n = (int)(row[4] & 0xffffffffll), grp = (int)(row[4] >> 48);
    const float* h = hyper + 5 * grp;
    const float lr = h[0], b1 = h[1], b2 = h[2], eps = h[3], wd = h[4];
    const float t = (float)step[0];
    const float bc1 = 1.f - powf(b1, t), bc2 = 1.f - powf(b2, t);
    const float step_size = lr / bc1, bc2_sqrt = sqrtf(bc2);
    for (int i = threadIdx.x; i < n; i += 256) {
        const float pv = p[i];
        const float g = __builtin_fmaf(wd, pv, gr[i] * coef);
        const float mv = m[i] + (1.f - b1) * (g - m[i]);
        const float vv = __builtin_fmaf(b2, v[i], (1.f - b2) * g * g);
        m[i] = mv;
        v[i] = vv;
        p[i] = pv - step_size * mv / (sqrtf(vv) / bc2_sqrt + eps);
    }
}

int ew_grid(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (int)(b < 8192 ? (b > 0 ? b : 1) : 8192);
}

int dconv_slices(int64_t P, int tiles) {
    // about 1024 workgroups in all, slices of at least 8 stages
    int64_t s = (1024 + tiles - 1) / tiles;
    const int64_t max_s = P / (8 * DC_KC);
    if (s > max_s) s = max_s;
    if (s > 256) s = 256;
    return s < 1 ? 1 : (int)s;
}

}  // namespace

extern "C" int sis_dconv3x3(float* out, const float* x, const float* weight, const float* bias, int batch, int cin, int cout, int h,
                            int w, int dilation, void* stream) {
    if (batch <= 0) return 0;
    SIS_REQUIRE(out && x && weight, "sis_dconv3x3: null pointer");
    SIS_REQUIRE(cin > 0 && cout > 0 && h > 0 && w > 0 && dilation >= 1, "sis_dconv3x3: bad shape %d -> %d, %d x %d, d %d", cin,
                cout, h, w, dilation);
    SIS_REQUIRE((int64_t)cin * h * w < (1LL << 31) && (int64_t)cout * h * w < (1LL << 31) && batch < 65536,
                "sis_dconv3x3: planes exceed 2^31 elements");
    hipStream_t st = (hipStream_t)stream;
    const int hw = h * w;
    if (cout <= 32) {
        hipLaunchKernelGGL(dconv3x3_kernel<1>, dim3(sis_cdiv(hw, 128), sis_cdiv(cout, 32), batch), dim3(256), 0, st, out, x, weight,
                           bias, cin, cout, h, w, dilation);
    } else {
        hipLaunchKernelGGL(dconv3x3_kernel<2>, dim3(sis_cdiv(hw, 64), sis_cdiv(cout, 64), batch), dim3(256), 0, st, out, x, weight,
                           bias, cin, cout, h, w, dilation);
    }
    SIS_CHECK_LAUNCH("dconv3x3_kernel");
    return 0;
}

extern "C" int sis_dconv3x3_adjoint(float* wa, const float* weight, int cin, int cout, void* stream) {
    SIS_REQUIRE(wa && weight && cin > 0 && cout > 0, "sis_dconv3x3_adjoint: bad arguments");
    const int64_t n = (int64_t)cin * cout * 9;
    hipLaunchKernelGGL(dconv3x3_adjoint_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, wa, weight, cin, cout);
    SIS_CHECK_LAUNCH("dconv3x3_adjoint_kernel");
    return 0;
}

namespace {

// The pixel slices of the weight gradient: `per` pixels each (a multiple of DC_KC, rounded up from P / S so that at most S
// slices are needed), `used` of them cover the P pixels.  The workspace and the launch both take their count from here.
struct WgradSlices { int64_t per; int used; };
WgradSlices wgrad_slices(int batch, int cin, int cout, int h, int w, int taps) {
    const int64_t P = (int64_t)batch * h * w;
    const int tiles = sis_cdiv((int64_t)cin * taps, 64) * sis_cdiv(cout, 64);
    const int S = dconv_slices(P, tiles);
    WgradSlices r;
    r.per = ((P + S - 1) / S + DC_KC - 1) / DC_KC * DC_KC;
    r.used = (int)((P + r.per - 1) / r.per);   // <= S: per >= P / S
    return r;
}

}  // namespace

extern "C" int64_t sis_dconv3x3_wgrad_workspace_floats(int batch, int cin, int cout, int h, int w, int taps) {
    return (int64_t)wgrad_slices(batch, cin, cout, h, w, taps).used * cout * cin * taps;
}

extern "C" int sis_dconv3x3_wgrad(float* dw, const float* grad_output, const float* x, float* workspace, int64_t workspace_floats,
                                  int batch, int cin, int cout, int h, int w, int dilation, int taps, void* stream) {
    if (batch <= 0) return 0;
    SIS_REQUIRE(dw && grad_output && x && workspace, "sis_dconv3x3_wgrad: null pointer");
    SIS_REQUIRE(taps == 9 || taps == 1, "sis_dconv3x3_wgrad: taps must be 9 or 1");
    SIS_REQUIRE(workspace_floats >= sis_dconv3x3_wgrad_workspace_floats(batch, cin, cout, h, w, taps),
                "sis_dconv3x3_wgrad: workspace too small");
    const int tn = sis_cdiv((int64_t)cin * taps, 64), tm = sis_cdiv(cout, 64);
    const WgradSlices sl = wgrad_slices(batch, cin, cout, h, w, taps);
    const int64_t per = sl.per;
    const int S_used = sl.used;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(dconv3x3_wgrad_kernel, dim3(tn, tm, S_used), dim3(256), 0, st, workspace, grad_output, x, batch, cin, cout, h,
                       w, dilation, taps, per);
    SIS_CHECK_LAUNCH("dconv3x3_wgrad_kernel");
    const int64_t n = (int64_t)cout * cin * taps;
    hipLaunchKernelGGL(slice_sum_kernel, dim3(ew_grid(n)), dim3(256), 0, st, dw, workspace, n, S_used);
    SIS_CHECK_LAUNCH("slice_sum_kernel");
    return 0;
}

extern "C" int sis_channel_sum(float* out, const float* x, int batch, int channels, int hw, void* stream) {
    if (channels <= 0) return 0;
    SIS_REQUIRE(out && x, "sis_channel_sum: null pointer");
    hipLaunchKernelGGL(channel_sum_kernel, dim3(channels), dim3(256), 0, (hipStream_t)stream, out, x, batch, channels, hw);
    SIS_CHECK_LAUNCH("channel_sum_kernel");
    return 0;
}

extern "C" int sis_pixel_shuffle2(float* out, const float* in, const float* bias, int batch, int channels, int h, int w,
                                  int64_t wide_batch_stride, int inverse, void* stream) {
    if (batch <= 0) return 0;
    SIS_REQUIRE(out && in, "sis_pixel_shuffle2: null pointer");
    SIS_REQUIRE(!(inverse && bias), "sis_pixel_shuffle2: the inverse gather takes no bias");
    SIS_REQUIRE(wide_batch_stride >= (int64_t)channels * 4 * h * w, "sis_pixel_shuffle2: batch stride below C * 2H * 2W");
    const int64_t total = (int64_t)batch * channels * 4 * h * w;
    hipLaunchKernelGGL(shuffle2_kernel, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, out, in, bias, channels, h, w,
                       wide_batch_stride, total, inverse);
    SIS_CHECK_LAUNCH("shuffle2_kernel");
    return 0;
}

extern "C" int sis_transpose2d(float* out, const float* in, int rows, int cols, void* stream) {
    SIS_REQUIRE(out && in && rows > 0 && cols > 0, "sis_transpose2d: bad arguments");
    hipLaunchKernelGGL(transpose2d_kernel, dim3(ew_grid((int64_t)rows * cols)), dim3(256), 0, (hipStream_t)stream, out, in, rows, cols);
    SIS_CHECK_LAUNCH("transpose2d_kernel");
    return 0;
}

extern "C" int64_t sis_bn_drop_bwd_workspace_floats(int batch, int channels, int hw) {
    // [C][S][2] double partials (4 floats each pair), then [C][2] float coefficients
    return (int64_t)channels * sis_cdiv((int64_t)batch * hw / 4, BD_SLICE4) * 4 + 2 * (int64_t)channels;
}

extern "C" int sis_bn_drop_fwd(float* y, int64_t y_batch_stride, const float* x, const float* mean, const float* invstd_or_var,
                               const float* gamma, const float* beta, int batch, int channels, int hw, int eval, float eps,
                               const void* seed, int site, float drop_p, void* mask, void* stream) {
    if (batch <= 0) return 0;
    SIS_REQUIRE(y && x && mean && invstd_or_var, "sis_bn_drop_fwd: null pointer");
    SIS_REQUIRE(hw % 4 == 0 && y_batch_stride % 4 == 0 && y_batch_stride >= (int64_t)channels * hw, "sis_bn_drop_fwd: H*W and the batch stride must be multiples of 4");
    SIS_REQUIRE((((uintptr_t)y | (uintptr_t)x) & 15) == 0, "sis_bn_drop_fwd: 16-byte alignment");
    SIS_REQUIRE(drop_p >= 0.f && drop_p < 1.f && (drop_p == 0.f || (seed && !eval)), "sis_bn_drop_fwd: dropout %f needs a seed word in train mode", drop_p);
    SIS_REQUIRE((int64_t)batch * channels * hw / 4 < (1LL << 32), "sis_bn_drop_fwd: too many elements");
    const unsigned thr = eval ? 0u : sis_drop_thr16(drop_p);
    const int64_t total4 = (int64_t)batch * channels * hw / 4;
    hipLaunchKernelGGL(bn_drop_fwd_kernel, dim3(ew_grid(total4)), dim3(256), 0, (hipStream_t)stream, y, y_batch_stride, x, mean,
                       invstd_or_var, gamma, beta, channels, hw / 4, total4, eval, eps, (const unsigned long long*)seed, (unsigned)site, thr,
                       sis_drop_scale(thr), (unsigned long long*)mask);
    SIS_CHECK_LAUNCH("bn_drop_fwd_kernel");
    return 0;
}

extern "C" int sis_bn_drop_bwd(float* dx, float* dgamma, float* dbeta, const float* dy, int64_t dy_batch_stride, const float* dy2,
                               const float* x, const float* mean, const float* invstd, const float* gamma, const void* mask,
                               float drop_p, float* workspace, int batch, int channels, int hw, void* stream) {
    if (batch <= 0) return 0;
    SIS_REQUIRE(dx && dgamma && dbeta && dy && x && mean && invstd && mask && workspace, "sis_bn_drop_bwd: null pointer");
    SIS_REQUIRE(hw % 4 == 0 && dy_batch_stride % 4 == 0, "sis_bn_drop_bwd: H*W and the batch stride must be multiples of 4");
    SIS_REQUIRE((((uintptr_t)dx | (uintptr_t)dy | (uintptr_t)dy2 | (uintptr_t)x | (uintptr_t)workspace) & 15) == 0, "sis_bn_drop_bwd: 16-byte alignment");
    SIS_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "sis_bn_drop_bwd: dropout probability %f", drop_p);
    BnDropBwdArgs a;
    a.dy1 = dy; a.dy1_bstride = dy_batch_stride; a.dy2 = dy2; a.x = x; a.mean = mean; a.invstd = invstd;
    a.mask = (const unsigned long long*)mask; a.keep_scale = sis_drop_scale(sis_drop_thr16(drop_p));
    a.B = batch; a.C = channels; a.HW4 = hw / 4;
    const int S = sis_cdiv((int64_t)batch * hw / 4, BD_SLICE4);
    double* partial = reinterpret_cast<double*>(workspace);
    float* coef = workspace + (int64_t)channels * S * 4;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_drop_bwd_reduce_kernel, dim3(channels * S), dim3(256), 0, st, partial, a, S);
    SIS_CHECK_LAUNCH("bn_drop_bwd_reduce_kernel");
    hipLaunchKernelGGL(bn_drop_bwd_finish_kernel, dim3(sis_cdiv(channels, 64)), dim3(64), 0, st, dgamma, dbeta, coef, partial,
                       channels, S, 1.f / (float)((int64_t)batch * hw));
    SIS_CHECK_LAUNCH("bn_drop_bwd_finish_kernel");
    const int64_t total4 = (int64_t)batch * channels * hw / 4;
    hipLaunchKernelGGL(bn_drop_bwd_apply_kernel, dim3(ew_grid(total4)), dim3(256), 0, st, dx, a, gamma, coef, total4);
    SIS_CHECK_LAUNCH("bn_drop_bwd_apply_kernel");
    return 0;
}

extern "C" int sis_weighted_ce_workspace_floats(void) { return 2 * CE_BLOCKS; }

extern "C" int sis_weighted_ce_fwd(float* loss, float* stats, float* workspace, const float* logits, const int64_t* labels,
                                   const float* weight, int batch, int classes, int hw, void* stream) {
    SIS_REQUIRE(loss && stats && workspace && logits && labels, "sis_weighted_ce_fwd: null pointer");
    SIS_REQUIRE(classes >= 1 && classes <= CE_MAX_K && batch > 0 && hw > 0, "sis_weighted_ce_fwd: %d classes (1..%d)", classes, CE_MAX_K);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(wce_fwd_kernel, dim3(CE_BLOCKS), dim3(256), 0, st, workspace, logits, labels, weight, classes, hw,
                       (int64_t)batch * hw);
    SIS_CHECK_LAUNCH("wce_fwd_kernel");
    hipLaunchKernelGGL(wce_finish_kernel, dim3(1), dim3(64), 0, st, loss, stats, workspace);
    SIS_CHECK_LAUNCH("wce_finish_kernel");
    return 0;
}

extern "C" int sis_weighted_ce_bwd(float* grad_logits, const float* grad_loss, const float* logits, const int64_t* labels,
                                   const float* weight, const float* stats, int batch, int classes, int hw, void* stream) {
    SIS_REQUIRE(grad_logits && grad_loss && logits && labels && stats, "sis_weighted_ce_bwd: null pointer");
    SIS_REQUIRE(classes >= 1 && classes <= CE_MAX_K && batch > 0 && hw > 0, "sis_weighted_ce_bwd: %d classes (1..%d)", classes, CE_MAX_K);
    const int64_t P = (int64_t)batch * hw;
    hipLaunchKernelGGL(wce_bwd_kernel, dim3(ew_grid(P)), dim3(256), 0, (hipStream_t)stream, grad_logits, logits, labels, weight, stats,
                       grad_loss, classes, hw, P);
    SIS_CHECK_LAUNCH("wce_bwd_kernel");
    return 0;
}

extern "C" int sis_adam_chunk_elems(void) { return ADAM_CHUNK; }

extern "C" int sis_adam_clip_step(const int64_t* table, int n_chunks, float* partial, const float* hyper, int* step, void* stream) {
    if (n_chunks <= 0) return 0;
    SIS_REQUIRE(table && partial && hyper && step, "sis_adam_clip_step: null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(adam_clip_norm_kernel, dim3(n_chunks), dim3(256), 0, st, partial, table, step);
    SIS_CHECK_LAUNCH("adam_clip_norm_kernel");
    hipLaunchKernelGGL(adam_step_kernel, dim3(n_chunks), dim3(256), 0, st, table, partial, n_chunks, hyper, step);
    SIS_CHECK_LAUNCH("adam_step_kernel");
    return 0;
}
