// Reconstruction metrics and the denoising loader.  Included from stem_conv.hip after gan_train_ops.h, whose
// gan_norm it shares (kernels of a header live in the including translation unit, as encoder_ops.h).
//
//   sis_psnr_ssim          evaluation/psnr_ssim.py of the reference (one kornia call per image: five grouped convolutions, a dozen
//                          element-wise passes, two host syncs) for a whole batch in three launches that read both tensors once
//                          (twice with the automatic unnormalise decision):
//     K1 eval_min_kernel        per-sample partial minima of image and target (the `image.min() < 0` of `unnormalize`)
//     K2 psnr_ssim_tile_kernel  one workgroup = one 32 x 32 tile of one (b, c) plane: tile + mirror halo of both tensors into LDS,
//                               row pass then column pass of the five Gaussian moments out of LDS, the SSIM value s, and two tile
//                               partials (sum of clamp(s, 0, 1), sum of squared error)
//     K3 psnr_ssim_finish_kernel  the partials of a sample -> psnr[b], ssim[b]
//   sis_autoencoder_batch  data/autoencoder_dataset.py (the three datasets' __getitem__ + collate): gather, additive Gaussian noise
//                          from a counter hash, optional grey conversion, ToTensor + Normalize for input and output in ONE launch.
//
// Precision of K2.  The moments are ACCUMULATED IN DOUBLE from the fp32 pixels (products of two floats are exact in double) and the
// row pass' results stay double in LDS: sigma^2 = G(x^2) - mu^2 cancels up to 1 / C2 = 1100 times its operands' rounding (the
// float32 formulation is off by up to 5e-4 in s on a smooth image).  The price is measured: the double arithmetic and its LDS
// traffic, not HBM, bound the kernel (0.1 ms per 32 images of 3 x 256 x 256).
// The unnormalisation x' = (clamp(x, -1, 1) + 1) / 2 is not applied to the pixels (x' is no float): the clamp is (exact), and the
// affine map a x + b is applied to the FINISHED moments, G(x') = a G(x) + b, var(x') = a^2 var(x), cov(x', y') = ax ay cov(x, y)
// (the taps sum to 1 to double rounding).
// No atomics; every sum has a fixed order, stated at the sum; caller's stream, no host sync: capturable.
#pragma once
#include "sis_device.h"

namespace {

constexpr int EV_TILE = 32;          // tile edge of K2 (sis_psnr_ssim_tile)
constexpr int EV_MAX_R = 5;          // window <= 11
constexpr int EV_MIN_CHUNKS = 64;    // K1: at most this many workgroups per sample

struct EvalTaps { double w[EV_MAX_R + 1]; };   // w[k] = exp(-k^2 / (2 sigma^2)) / sum over -r..r, k = 0..r

__device__ __forceinline__ int eval_mirror(int i, int n) {   // scipy's "mirror" / torch's "reflect", one reflection: |overhang| < n
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

// ---------------------------------------------------------------------------------------------------------------- K1
// pmin[(b * chunks + chunk) * 2 + {0, 1}] = min over the chunk's elements of image / target.  A minimum does not depend on the
// order of its terms.  fminf drops a NaN operand (torch's min would return it; `nan < 0` is false there, here the other elements decide).
template <bool VEC>
__global__ __launch_bounds__(256) void eval_min_kernel(float* __restrict__ pmin, const float* __restrict__ image, const float* __restrict__ target,
                                                       int64_t per) {
    __shared__ float red[2][4];
    const int b = blockIdx.y, chunks = gridDim.x;
    const float* x = image + (int64_t)b * per;
    const float* y = target + (int64_t)b * per;
    float mx = __builtin_inff(), my = __builtin_inff();
    if constexpr (VEC) {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per / 4; i += (int64_t)chunks * 256) {
            const sis_f32x4 a = *reinterpret_cast<const sis_f32x4*>(x + 4 * i), c = *reinterpret_cast<const sis_f32x4*>(y + 4 * i);
            mx = fminf(mx, fminf(fminf(a[0], a[1]), fminf(a[2], a[3])));
            my = fminf(my, fminf(fminf(c[0], c[1]), fminf(c[2], c[3])));
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)chunks * 256) {
            mx = fminf(mx, x[i]);
            my = fminf(my, y[i]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = fminf(mx, __shfl_xor(mx, o, 64));
        my = fminf(my, __shfl_xor(my, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = mx;
        red[1][threadIdx.x >> 6] = my;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const float* r = red[threadIdx.x];
        pmin[((int64_t)b * chunks + blockIdx.x) * 2 + threadIdx.x] = fminf(fminf(r[0], r[1]), fminf(r[2], r[3]));
    }
}

// ---------------------------------------------------------------------------------------------------------------- K2
struct SsimArgs {
    double* partial;          // [B][tiles per sample][2]: sum of clamp(s, 0, 1), sum of squared error
    float* map;               // [B][C][H][W] unclamped s, or null
    const float* image; const float* target;
    const float* pmin;        // K1's partial minima (mode 0)
    int chunks, mode;         // mode 0: per sample and tensor by its minimum; 1: unnormalise both; 2: neither
    int channels, height, width, tiles_x, tiles_y;
    double c1, c2;
    EvalTaps taps;
};

// LDS: the two staged tiles as float, row stride TH + 1 (odd); the row pass' five moments as double [5][TH][32]: lanes run along x in
// every access, 32 consecutive floats or doubles per half wave, so no access has a bank conflict.  68 KiB at window 11: two
// workgroups per CU.
template <int R>
__global__ __launch_bounds__(256) void psnr_ssim_tile_kernel(SsimArgs a) {
    constexpr int T = EV_TILE, TH = T + 2 * R, LD = TH + 1;
    __shared__ float tile_x[TH * LD];
    __shared__ float tile_y[TH * LD];
    __shared__ double rows[5][TH][T];
    __shared__ double red[4];
    __shared__ int unnorm[2];

    const int b = blockIdx.y;
    int t = blockIdx.x;
    const int tx = t % a.tiles_x;
    t /= a.tiles_x;
    const int ty = t % a.tiles_y, c = t / a.tiles_y;
    const int x_first = tx * T, y_first = ty * T, H = a.height, W = a.width;
    const int64_t plane = ((int64_t)b * a.channels + c) * H * W;

    if (a.mode == 0) {
        if (threadIdx.x < 64) {   // the sample's minima from K1's partials (chunks <= 64)
            float mx = __builtin_inff(), my = __builtin_inff();
            if ((int)threadIdx.x < a.chunks) {
                mx = a.pmin[((int64_t)b * a.chunks + threadIdx.x) * 2];
                my = a.pmin[((int64_t)b * a.chunks + threadIdx.x) * 2 + 1];
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                mx = fminf(mx, __shfl_xor(mx, o, 64));
                my = fminf(my, __shfl_xor(my, o, 64));
            }
            if (threadIdx.x == 0) {
                unnorm[0] = mx < 0.f;
                unnorm[1] = my < 0.f;
            }
        }
        __syncthreads();
    }
    const bool ux = a.mode == 0 ? unnorm[0] != 0 : a.mode == 1;
    const bool uy = a.mode == 0 ? unnorm[1] != 0 : a.mode == 1;

    // tile + halo.  Rows / columns from H + R / W + R on feed no pixel of the image and are not read (their mirror index would
    // leave the plane); x_first - R >= -R and R < H, W keep every other index inside after one reflection.
    for (int e = threadIdx.x; e < TH * TH; e += 256) {
        const int r = e / TH, col = e - r * TH;
        const int gy = y_first - R + r, gx = x_first - R + col;
        float vx = 0.f, vy = 0.f;
        if (gy < H + R && gx < W + R) {
            const int64_t at = plane + (int64_t)eval_mirror(gy, H) * W + eval_mirror(gx, W);
            vx = a.image[at];
            vy = a.target[at];
            if (ux) vx = fminf(fmaxf(vx, -1.f), 1.f);
            if (uy) vy = fminf(fmaxf(vy, -1.f), 1.f);
        }
        tile_x[r * LD + col] = vx;
        tile_y[r * LD + col] = vy;
    }
    __syncthreads();

    // row pass.  ORDER of each of the five sums: the centre tap, then k = 1 .. R, each adding w[k] * (left term + right term) by FMA.
    for (int e = threadIdx.x; e < TH * T; e += 256) {
        const int r = e / T, col = e % T;
        const float* px = tile_x + r * LD + col + R;
        const float* py = tile_y + r * LD + col + R;
        const double x0 = px[0], y0 = py[0], w0 = a.taps.w[0];
        double gx = w0 * x0, gy = w0 * y0, gxx = w0 * (x0 * x0), gyy = w0 * (y0 * y0), gxy = w0 * (x0 * y0);
#pragma unroll
        for (int k = 1; k <= R; ++k) {
            const double xl = px[-k], xr = px[k], yl = py[-k], yr = py[k], wk = a.taps.w[k];
            gx = fma(wk, xl + xr, gx);
            gy = fma(wk, yl + yr, gy);
            gxx = fma(wk, xl * xl + xr * xr, gxx);
            gyy = fma(wk, yl * yl + yr * yr, gyy);
            gxy = fma(wk, xl * yl + xr * yr, gxy);
        }
        rows[0][r][col] = gx;
        rows[1][r][col] = gy;
        rows[2][r][col] = gxx;
        rows[3][r][col] = gyy;
        rows[4][r][col] = gxy;
    }
    __syncthreads();

    // column pass and s: a thread owns column (threadIdx.x & 31) of the 4 consecutive rows from 4 (threadIdx.x >> 5) on, so the
    // 4 + 2 R row-pass values of a moment are read once into registers and serve all four pixels.
    const double ax = ux ? 0.5 : 1.0, bx = ux ? 0.5 : 0.0, ay = uy ? 0.5 : 1.0, by = uy ? 0.5 : 0.0;
    const int col = threadIdx.x & 31, gxp = x_first + col, row0 = (threadIdx.x >> 5) * 4;
    const bool strip_inside = gxp < W && y_first + row0 < H;
    double m[4][5];
    if (strip_inside) {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double v[4 + 2 * R];
#pragma unroll
            for (int j = 0; j < 4 + 2 * R; ++j) v[j] = rows[q][row0 + j][col];
#pragma unroll
            for (int i = 0; i < 4; ++i) {   // ORDER: as the row pass, (upper + lower)
                double acc = a.taps.w[0] * v[i + R];
#pragma unroll
                for (int k = 1; k <= R; ++k) acc = fma(a.taps.w[k], v[i + R - k] + v[i + R + k], acc);
                m[i][q] = acc;
            }
        }
    }
    double sum_s = 0.0, sum_e = 0.0;   // ORDER: i = 0 .. 3 (pixels outside the image add nothing)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = row0 + i, gyp = y_first + r;
        if (strip_inside && gyp < H) {
            const double mux = ax * m[i][0] + bx, muy = ay * m[i][1] + by;
            const double sxx = (ax * ax) * (m[i][2] - m[i][0] * m[i][0]), syy = (ay * ay) * (m[i][3] - m[i][1] * m[i][1]);
            const double sxy = (ax * ay) * (m[i][4] - m[i][0] * m[i][1]);
            const double s = ((2.0 * mux * muy + a.c1) * (2.0 * sxy + a.c2)) / ((mux * mux + muy * muy + a.c1) * (sxx + syy + a.c2));
            if (a.map) a.map[plane + (int64_t)gyp * W + gxp] = (float)s;
            sum_s += fmin(fmax(s, 0.0), 1.0);
            const double d = (ax * (double)tile_x[(r + R) * LD + col + R] + bx) - (ay * (double)tile_y[(r + R) * LD + col + R] + by);
            sum_e += d * d;
        }
    }
    // ORDER: sis_block_sum4 (each wave's butterfly, then (r0 + r1) + (r2 + r3))
    sum_s = sis_block_sum4(sum_s, red);
    sum_e = sis_block_sum4(sum_e, red);
    if (threadIdx.x == 0) {
        double* p = a.partial + ((int64_t)b * gridDim.x + blockIdx.x) * 2;
        p[0] = sum_s;
        p[1] = sum_e;
    }
}

// ---------------------------------------------------------------------------------------------------------------- K3
// One wave per sample.  ORDER: lane l adds tiles l, l + 64, ... in that order; then the butterfly of sis_wave_sum.
__global__ __launch_bounds__(64) void psnr_ssim_finish_kernel(float* __restrict__ psnr, float* __restrict__ ssim, const double* __restrict__ partial,
                                                              int tiles, double count, double max_val) {
    const int b = blockIdx.x;
    const double* p = partial + (int64_t)b * tiles * 2;
    double s = 0.0, e = 0.0;
    for (int t = threadIdx.x; t < tiles; t += 64) {
        s += p[2 * t];
        e += p[2 * t + 1];
    }
    s = sis_wave_sum(s);
    e = sis_wave_sum(e);
    if (threadIdx.x == 0) {
        ssim[b] = (float)(s / count);
        psnr[b] = (float)(10.0 * log10(max_val * max_val / (e / count)));   // mse == 0: +inf
    }
}

// ------------------------------------------------------------------------------------------------- sis_autoencoder_batch
// uniform bits from (seed word, component, pixel number): the generator of augment.hip's elastic_noise (murmur3's 32-bit finaliser
// on an affine image of the pixel number); DESIGN.md §15 states the recipe for the numpy restatement.
__device__ __forceinline__ unsigned eval_hash(unsigned seed, unsigned component, unsigned pixel) {
    unsigned h = pixel * 0x9E3779B1u + (seed ^ (component * 0x85EBCA77u));
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// standard normal of noise channel `ch`: Box-Muller on u1 = ((h(2 ch) >> 8) + 1) * 2^-24 in (0, 1] and u2 = (h(2 ch + 1) >> 8) * 2^-24
// in [0, 1), both exact in fp32; z = sqrtf(-2 logf(u1)) * cospif(2 u2), |z| <= 5.77.
__device__ __forceinline__ float eval_normal(unsigned seed, unsigned ch, unsigned pixel) {
    const float u1 = (float)((eval_hash(seed, 2u * ch, pixel) >> 8) + 1u) * 5.9604644775390625e-08f;
    const float u2 = (float)(eval_hash(seed, 2u * ch + 1u, pixel) >> 8) * 5.9604644775390625e-08f;
    return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

// one pixel: p[3] bytes -> q[3] noisy levels.  rintf rounds half to even, as numpy.rint; scale == 0 gives p (z is finite).
__device__ __forceinline__ void eval_noisy_pixel(const unsigned* p, unsigned* q, float scale, bool per_channel, bool grey, unsigned seed, unsigned pixel) {
    float z = eval_normal(seed, 0u, pixel);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (per_channel && c > 0) z = eval_normal(seed, (unsigned)c, pixel);
        q[c] = (unsigned)fminf(fmaxf(rintf(__fmaf_rn(scale, z, (float)p[c])), 0.f), 255.f);
    }
    if (grey) q[0] = q[1] = q[2] = (19595u * q[0] + 38470u * q[1] + 7471u * q[2] + 32768u) >> 16;   // PIL's convert('L')
}

struct AeArgs {
    float* input; float* output;
    const uint8_t* images; const int* ids;
    const float* scale; const int* per_channel; const unsigned* seed; const int* grey;
    int n_images, plane;   // plane = S * S
};

// VEC (S * S % 4 == 0): one thread = 4 consecutive pixels of a sample in all three planes: three dword loads, six 16-byte stores.
// Otherwise one pixel per thread.  An id outside 0 .. n_images - 1 reads nothing and writes NaN to both outputs.
template <bool VEC>
__global__ __launch_bounds__(256) void autoencoder_batch_kernel(AeArgs a) {
    constexpr int N = VEC ? 4 : 1;
    const int b = blockIdx.y;
    const int first = (blockIdx.x * 256 + threadIdx.x) * N;
    if (first >= a.plane) return;
    const int id = a.ids[b];
    const int64_t out_at = (int64_t)b * 3 * a.plane + first;
    float vin[3][N], vout[3][N];
    if (id >= 0 && id < a.n_images) {
        const float scale = a.scale[b];
        const bool per_channel = a.per_channel[b] != 0, grey = a.grey[b] != 0;
        const unsigned seed = a.seed[b];
        const uint8_t* src = a.images + (int64_t)id * 3 * a.plane + first;
        unsigned p[3][N];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if constexpr (VEC) {
                const unsigned w = *reinterpret_cast<const unsigned*>(src + (int64_t)c * a.plane);
#pragma unroll
                for (int k = 0; k < 4; ++k) p[c][k] = (w >> (8 * k)) & 255u;
            } else {
                p[c][0] = src[(int64_t)c * a.plane];
            }
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const unsigned pk[3] = {p[0][k], p[1][k], p[2][k]};
            unsigned q[3];
            eval_noisy_pixel(pk, q, scale, per_channel, grey, seed, (unsigned)(first + k));
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                vin[c][k] = gan_norm(q[c]);
                vout[c][k] = gan_norm(pk[c]);
            }
        }
    } else {
        const float nan = __builtin_nanf("");
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < N; ++k) vin[c][k] = vout[c][k] = nan;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* pi = a.input + out_at + (int64_t)c * a.plane;
        float* po = a.output + out_at + (int64_t)c * a.plane;
        if constexpr (VEC) {
            *reinterpret_cast<sis_f32x4*>(pi) = sis_f32x4{vin[c][0], vin[c][1], vin[c][2], vin[c][3]};
            *reinterpret_cast<sis_f32x4*>(po) = sis_f32x4{vout[c][0], vout[c][1], vout[c][2], vout[c][3]};
        } else {
            *pi = vin[c][0];
            *po = vout[c][0];
        }
    }
}

inline int eval_tiles(int n) { return (n + EV_TILE - 1) / EV_TILE; }
inline int eval_chunks(int64_t per) { return (int)(per >= 4096LL * EV_MIN_CHUNKS ? EV_MIN_CHUNKS : (per + 4095) / 4096); }   // 1 .. 64

template <int R>
void psnr_ssim_tile_launch(const SsimArgs& a, dim3 grid, hipStream_t st) {
    psnr_ssim_tile_kernel<R><<<grid, dim3(256), 0, st>>>(a);
}

}  // namespace

extern "C" int sis_psnr_ssim_tile(void) { return EV_TILE; }

extern "C" int64_t sis_psnr_ssim_workspace_bytes(int batch, int channels, int height, int width) {
    if (batch < 1 || channels < 1 || height < 1 || width < 1) return 0;
    const int64_t tiles = (int64_t)channels * eval_tiles(height) * eval_tiles(width);
    return (int64_t)batch * (tiles * 2 * (int64_t)sizeof(double) + (int64_t)EV_MIN_CHUNKS * 2 * (int64_t)sizeof(float));
}

extern "C" int sis_psnr_ssim(float* psnr, float* ssim, float* ssim_map, const float* image, const float* target, int batch, int channels,
                             int height, int width, int window, float max_val, int mode, void* workspace, int64_t workspace_bytes,
                             void* stream) {
    SIS_REQUIRE(psnr && ssim && image && target && workspace, "sis_psnr_ssim: null pointer");
    SIS_REQUIRE(batch > 0 && batch <= 65535 && channels > 0 && height > 0 && width > 0 && height <= 16384 && width <= 16384,
                "sis_psnr_ssim: batch %d (1..65535), %d channels, %d x %d (1..16384)", batch, channels, height, width);
    SIS_REQUIRE(window >= 3 && window <= 2 * EV_MAX_R + 1 && window % 2 == 1, "sis_psnr_ssim: window %d is not odd in 3..11", window);
    const int radius = window / 2;
    SIS_REQUIRE(height > radius && width > radius, "sis_psnr_ssim: a %d x %d image is not larger than the window's radius %d (one reflection)",
                height, width, radius);
    SIS_REQUIRE(mode >= 0 && mode <= 2, "sis_psnr_ssim: mode %d (0 by the minimum, 1 unnormalise, 2 leave)", mode);
    SIS_REQUIRE(max_val > 0.f, "sis_psnr_ssim: max_val %g", (double)max_val);
    const int64_t per = (int64_t)channels * height * width;
    const int tiles_x = eval_tiles(width), tiles_y = eval_tiles(height);
    const int64_t tiles = (int64_t)channels * tiles_x * tiles_y;
    SIS_REQUIRE(per < (1LL << 31) && tiles < (1LL << 31), "sis_psnr_ssim: sample too large");
    SIS_REQUIRE(workspace_bytes >= sis_psnr_ssim_workspace_bytes(batch, channels, height, width) && (((uintptr_t)workspace) & 7) == 0,
                "sis_psnr_ssim: workspace of %lld bytes is too small or not 8-byte aligned", (long long)workspace_bytes);
    double* partial = (double*)workspace;
    float* pmin = (float*)(partial + (int64_t)batch * tiles * 2);
    hipStream_t st = (hipStream_t)stream;
    const int chunks = eval_chunks(per);
    if (mode == 0) {
        const dim3 grid(chunks, batch);
        if (per % 4 == 0 && gan_aligned16(image) && gan_aligned16(target))
            eval_min_kernel<true><<<grid, dim3(256), 0, st>>>(pmin, image, target, per);
        else
            eval_min_kernel<false><<<grid, dim3(256), 0, st>>>(pmin, image, target, per);
        SIS_CHECK_LAUNCH("eval_min_kernel");
    }
    SsimArgs a{partial, ssim_map, image, target, pmin, chunks, mode, channels, height, width, tiles_x, tiles_y, 0.0, 0.0, {}};
    a.c1 = (0.01 * (double)max_val) * (0.01 * (double)max_val);
    a.c2 = (0.03 * (double)max_val) * (0.03 * (double)max_val);
    double sum = 0.0;   // kornia's get_gaussian_kernel1d(window, 1.5), in double
    for (int k = -radius; k <= radius; ++k) sum += exp(-(double)(k * k) / (2.0 * 1.5 * 1.5));
    for (int k = 0; k <= EV_MAX_R; ++k) a.taps.w[k] = k <= radius ? exp(-(double)(k * k) / (2.0 * 1.5 * 1.5)) / sum : 0.0;
    const dim3 grid((unsigned)tiles, batch);
    switch (radius) {
        case 1: psnr_ssim_tile_launch<1>(a, grid, st); break;
        case 2: psnr_ssim_tile_launch<2>(a, grid, st); break;
        case 3: psnr_ssim_tile_launch<3>(a, grid, st); break;
        case 4: psnr_ssim_tile_launch<4>(a, grid, st); break;
        default: psnr_ssim_tile_launch<5>(a, grid, st); break;
    }
    SIS_CHECK_LAUNCH("psnr_ssim_tile_kernel");
    psnr_ssim_finish_kernel<<<dim3(batch), dim3(64), 0, st>>>(psnr, ssim, partial, (int)tiles, (double)per, (double)max_val);
    SIS_CHECK_LAUNCH("psnr_ssim_finish_kernel");
    return 0;
}

extern "C" int sis_autoencoder_batch(float* input_image, float* output_image, const uint8_t* images, const int* ids, const float* scale,
                                     const int* per_channel, const uint32_t* seed, const int* grey, int64_t n_images, int batch, int size,
                                     void* stream) {
    SIS_REQUIRE(input_image && output_image && images && ids && scale && per_channel && seed && grey, "sis_autoencoder_batch: null pointer");
    SIS_REQUIRE(n_images > 0 && n_images < (1LL << 31) && batch > 0 && batch <= 65535 && size > 0 && size <= 16384,
                "sis_autoencoder_batch: %lld images, batch %d (1..65535), size %d", (long long)n_images, batch, size);
    const int plane = size * size;
    AeArgs a{input_image, output_image, images, ids, scale, per_channel, seed, grey, (int)n_images, plane};
    hipStream_t st = (hipStream_t)stream;
    if (plane % 4 == 0 && gan_aligned16(input_image) && gan_aligned16(output_image) && (((uintptr_t)images) & 3) == 0)
        autoencoder_batch_kernel<true><<<dim3((plane / 4 + 255) / 256, batch), dim3(256), 0, st>>>(a);
    else
        autoencoder_batch_kernel<false><<<dim3((plane + 255) / 256, batch), dim3(256), 0, st>>>(a);
    SIS_CHECK_LAUNCH("autoencoder_batch_kernel");
    return 0;
}
