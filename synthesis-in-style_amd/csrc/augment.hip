// Training-time augmentation of a device-resident [image | label] dataset, instead of imgaug on the host:
//  * sis_augment_warp    utils/augment_dataset.py:33-59 (geometric + colour augmenters) and data/segmentation_dataset.py:80-107
//                        (AugmentedSegmentationDataset.__getitem__: augment, ToTensor, Normalize, colours -> classes, resize) for a
//                        whole batch in one launch: gather by sample id, colour LUT, one bilinear resampling through the composed
//                        inverse affine map (+ elastic displacement), optional rounding to a byte, encode; nearest-neighbour class map.
//  * sis_elastic_field   the displacement fields of iaa.ElasticTransformation (augment_dataset.py:35): alpha * (Gaussian of sigma,
//                        mirror boundary, truncated at 4 sigma) * uniform noise, noise from a counter hash; two separable passes.
// Tiling.  The warp's output side is what can be made regular: a lane owns 4 consecutive output pixels of a row, so the three
// image planes leave as one 16-byte store each and the int64 labels as two, fully coalesced along the row (rows whose width is
// no multiple of 4 take the scalar stores).  The source side is a data-dependent gather of 3-byte pixels, 4 taps per output
// pixel; neighbouring lanes read neighbouring (or, under rotation, nearby) source bytes, so the taps are served by the vector L1
// / L2 and no staging of source tiles is attempted: the footprint of an output tile under shear + rotation + elastic is not a
// rectangle known before the coordinates are.  A workgroup belongs to ONE sample, so its 256-byte colour LUT sits in LDS.
// The field's row pass generates (or loads) a row tile with its mirror halo of up to 36 columns into LDS and every lane reads
// its 2r+1 taps from there; the column pass reads its taps from the row pass' result directly: lanes run along x, so every tap
// is one coalesced row segment, re-read from L1 / L2 by the 2r neighbouring rows.
#include "sis_common.h"

namespace {

constexpr int AW_THREADS = 256;
constexpr int EF_MAX_FIELDS = 64;
constexpr int EF_MAX_RADIUS = 36;   // floor(4 * 9 + 0.5): sigma <= 9
constexpr int EF_TILE = 256;

struct WarpArgs {
    float* images; int64_t* segmented;
    const uint8_t* pixels; const uint8_t* classes;
    const int* index; const float* minv; const uint8_t* lut; const int* field_slot; const float* field;
    int64_t n_samples;
    int height, width, num_fields, background_id, out_h, out_w, quantize;
};

__device__ __forceinline__ float bilinear_clamped(const float* __restrict__ f, int height, int width, float qx, float qy) {
    // edge clamp: the displacement outside the image is the one of the nearest border pixel
    qx = fminf(fmaxf(qx, 0.f), (float)(width - 1));
    qy = fminf(fmaxf(qy, 0.f), (float)(height - 1));
    const int x0 = (int)qx, y0 = (int)qy;
    const int x1 = min(x0 + 1, width - 1), y1 = min(y0 + 1, height - 1);
    const float fx = qx - (float)x0, fy = qy - (float)y0;
    const float a = f[(int64_t)y0 * width + x0], b = f[(int64_t)y0 * width + x1];
    const float c = f[(int64_t)y1 * width + x0], d = f[(int64_t)y1 * width + x1];
    const float top = a + fx * (b - a), bottom = c + fx * (d - c);
    return top + fy * (bottom - top);
}

// VEC: out_w % 4 == 0, every quad of a lane is 16-byte aligned in all three outputs.
template <bool VEC>
__global__ __launch_bounds__(AW_THREADS) void augment_warp_kernel(WarpArgs a) {
    __shared__ uint8_t lut[256];
    const int b = blockIdx.y;
    lut[threadIdx.x] = a.lut[(int64_t)b * 256 + threadIdx.x];
    __syncthreads();
    const int quads_per_row = (a.out_w + 3) >> 2;
    const int q = blockIdx.x * AW_THREADS + threadIdx.x;
    if (q >= quads_per_row * a.out_h) return;
    const int y = q / quads_per_row, x_first = (q - y * quads_per_row) * 4;

    const int sample = a.index[b];
    const bool sample_ok = sample >= 0 && (int64_t)sample < a.n_samples;   // an id outside the dataset reads nothing
    const int64_t plane_in = (int64_t)a.height * a.width;
    const uint8_t* px = a.pixels + (sample_ok ? (int64_t)sample : 0) * plane_in * 3;
    const uint8_t* cl = a.classes + (sample_ok ? (int64_t)sample : 0) * plane_in;
    const float* m = a.minv + b * 6;
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
    const int slot = a.field_slot[b];
    const float* field = (slot >= 0 && slot < a.num_fields) ? a.field + (int64_t)slot * 2 * plane_in : nullptr;
    const float fw = (float)a.width, fh = (float)a.height;

    float v[3][4];
    int64_t lab[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float xo = (float)(x_first + k), yo = (float)y;
        float sx = m00 * xo + m01 * yo + m02;
        float sy = m10 * xo + m11 * yo + m12;
        if (field) {
            const float dx = bilinear_clamped(field, a.height, a.width, sx, sy);
            const float dy = bilinear_clamped(field + plane_in, a.height, a.width, sx, sy);
            sx += dx;
            sy += dy;
        }
        float r = 0.f, g = 0.f, bl = 0.f;
        int id = a.background_id;
        // every tap of a coordinate outside (-1, W) x (-1, H) lies outside the image (also catches NaN and values no int holds)
        if (sample_ok && sx > -1.f && sx < fw && sy > -1.f && sy < fh) {
            const float x0f = floorf(sx), y0f = floorf(sy);
            const int x0 = (int)x0f, y0 = (int)y0f;
            const float fx = sx - x0f, fy = sy - y0f;
            const float wx[2] = {1.f - fx, fx}, wy[2] = {1.f - fy, fy};
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int xi = x0 + i, yi = y0 + j;
                    if (xi >= 0 && xi < a.width && yi >= 0 && yi < a.height) {   // a tap outside contributes 0, not lut[0]
                        const uint8_t* p = px + ((int64_t)yi * a.width + xi) * 3;
                        const float w = wx[i] * wy[j];
                        r += w * (float)lut[p[0]];
                        g += w * (float)lut[p[1]];
                        bl += w * (float)lut[p[2]];
                    }
                }
            const float nx = floorf(sx + 0.5f), ny = floorf(sy + 0.5f);
            if (nx >= 0.f && nx < fw && ny >= 0.f && ny < fh) id = cl[(int64_t)(int)ny * a.width + (int)nx];
        }
        if (a.quantize) {   // rintf: half to even, as numpy.rint; the weights sum to 1, the clamp only guards round-off
            r = fminf(fmaxf(rintf(r), 0.f), 255.f);
            g = fminf(fmaxf(rintf(g), 0.f), 255.f);
            bl = fminf(fmaxf(rintf(bl), 0.f), 255.f);
        }
        // ToTensor (true division by 255) and Normalize(0.5, 0.5), as crop_patches_kernel and encode_batch
        v[0][k] = (r / 255.0f - 0.5f) / 0.5f;
        v[1][k] = (g / 255.0f - 0.5f) / 0.5f;
        v[2][k] = (bl / 255.0f - 0.5f) / 0.5f;
        lab[k] = id;
    }

    const int64_t plane_out = (int64_t)a.out_h * a.out_w;
    const int64_t at = (int64_t)y * a.out_w + x_first;
    float* img = a.images + (int64_t)b * 3 * plane_out + at;
    int64_t* seg = a.segmented + (int64_t)b * plane_out + at;
    if (VEC) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *reinterpret_cast<float4*>(img + c * plane_out) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        *reinterpret_cast<longlong2*>(seg) = make_longlong2(lab[0], lab[1]);
        *reinterpret_cast<longlong2*>(seg + 2) = make_longlong2(lab[2], lab[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x_first + k < a.out_w) {
#pragma unroll
                for (int c = 0; c < 3; ++c) img[c * plane_out + k] = v[c][k];
                seg[k] = lab[k];
            }
    }
}

// ---------------------------------------------------------------------------------------------- elastic displacement fields

struct FieldParams {
    float alpha[EF_MAX_FIELDS];
    float sigma[EF_MAX_FIELDS];
    unsigned seed[EF_MAX_FIELDS];
    int radius[EF_MAX_FIELDS];
};

// uniform in [-1, 1) from (seed word, component, pixel number): murmur3's 32-bit finaliser (as sis_drop_quad, vit_common.h) on an
// affine image of the pixel number; (h >> 8) * 2^-23 - 1 is exact in fp32.  DESIGN.md §12 states it for the numpy restatement.
__device__ __forceinline__ float elastic_noise(unsigned seed, unsigned component, unsigned pixel) {
    unsigned h = pixel * 0x9E3779B1u + (seed ^ (component * 0x85EBCA77u));
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return (float)(h >> 8) * 1.1920928955078125e-07f - 1.0f;
}

__device__ __forceinline__ int mirror(int i, int n) {   // scipy's "mirror": d c b | a b c d | c b a; one reflection: radius < n
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

// w[k] = exp(-k^2 / (2 sigma^2)) / sum over -r..r, k = 0..r, in LDS; every lane leaves with the weights visible
__device__ __forceinline__ void gaussian_weights(float* w, float sigma, int radius) {
    if ((int)threadIdx.x <= radius) {
        const float k = (float)threadIdx.x;
        w[threadIdx.x] = expf(-0.5f * k * k / (sigma * sigma));
    }
    __syncthreads();
    float sum = w[0];
    for (int k = 1; k <= radius; ++k) sum += 2.f * w[k];
    __syncthreads();
    if ((int)threadIdx.x <= radius) w[threadIdx.x] /= sum;
    __syncthreads();
}

// tmp[f][c][y][x] = sum_k w[|k|] noise[f][c][y][mirror(x + k)]
__global__ __launch_bounds__(EF_TILE) void elastic_rows_kernel(float* __restrict__ tmp, float* __restrict__ noise_out,
                                                               const float* __restrict__ noise_in, FieldParams p, int height,
                                                               int width) {
    __shared__ float w[EF_MAX_RADIUS + 1];
    __shared__ float tile[EF_TILE + 2 * EF_MAX_RADIUS];
    const int plane = blockIdx.z, f = plane >> 1, c = plane & 1, y = blockIdx.y;
    const int radius = p.radius[f];
    const int x_first = blockIdx.x * EF_TILE;
    const int64_t row = ((int64_t)plane * height + y) * width;
    gaussian_weights(w, p.sigma[f], radius);
    for (int i = threadIdx.x; i < EF_TILE + 2 * radius; i += EF_TILE) {
        const int col = x_first - radius + i;
        float v = 0.f;
        if (col < width + radius) {   // columns further right feed no output of this row
            const int mc = mirror(col, width);
            v = noise_in ? noise_in[row + mc] : elastic_noise(p.seed[f], (unsigned)c, (unsigned)(y * width + mc));
            if (noise_out && col >= 0 && col < width && i >= radius && i < radius + EF_TILE) noise_out[row + col] = v;
        }
        tile[i] = v;
    }
    __syncthreads();
    const int x = x_first + threadIdx.x;
    if (x >= width) return;
    const float* t = tile + threadIdx.x + radius;
    float acc = w[0] * t[0];
    for (int k = 1; k <= radius; ++k) acc += w[k] * (t[-k] + t[k]);
    tmp[row + x] = acc;
}

// field[f][c][y][x] = alpha[f] * sum_k w[|k|] tmp[f][c][mirror(y + k)][x]
__global__ __launch_bounds__(EF_TILE) void elastic_cols_kernel(float* __restrict__ field, const float* __restrict__ tmp,
                                                               FieldParams p, int height, int width) {
    __shared__ float w[EF_MAX_RADIUS + 1];
    const int plane = blockIdx.z, f = plane >> 1, y = blockIdx.y;
    const int radius = p.radius[f];
    gaussian_weights(w, p.sigma[f], radius);
    const int x = blockIdx.x * EF_TILE + threadIdx.x;
    if (x >= width) return;
    const float* t = tmp + (int64_t)plane * height * width + x;
    float acc = w[0] * t[(int64_t)y * width];
    for (int k = 1; k <= radius; ++k)
        acc += w[k] * (t[(int64_t)mirror(y - k, height) * width] + t[(int64_t)mirror(y + k, height) * width]);
    field[((int64_t)plane * height + y) * width + x] = p.alpha[f] * acc;
}

int elastic_radius(float sigma) { return (int)(4.0f * sigma + 0.5f); }   // scipy: int(truncate * sigma + 0.5)

}  // namespace

extern "C" int sis_augment_warp(float* images, int64_t* segmented, const uint8_t* pixels, const uint8_t* classes, const int* index,
                                const float* minv, const uint8_t* lut, const int* field_slot, const float* field,
                                int64_t n_samples, int batch, int height, int width, int num_fields, int background_id, int out_h,
                                int out_w, int quantize, void* stream) {
    SIS_REQUIRE(images && segmented && pixels && classes && index && minv && lut && field_slot,
                "sis_augment_warp: null pointer");
    SIS_REQUIRE(num_fields == 0 || field, "sis_augment_warp: %d fields but no field array", num_fields);
    SIS_REQUIRE(n_samples > 0 && batch > 0 && batch <= 65535, "sis_augment_warp: batch %d / %lld samples out of range", batch,
                (long long)n_samples);
    SIS_REQUIRE(height > 0 && width > 0 && height <= 16384 && width <= 16384, "sis_augment_warp: source %dx%d outside 1..16384",
                height, width);
    SIS_REQUIRE(out_h > 0 && out_w > 0 && out_h <= 16384 && out_w <= 16384, "sis_augment_warp: output %dx%d outside 1..16384",
                out_h, out_w);
    SIS_REQUIRE(num_fields >= 0 && background_id >= 0 && background_id <= 255, "sis_augment_warp: bad field count or background id");
    WarpArgs a{images, segmented, pixels, classes, index, minv, lut, field_slot, field, n_samples,
               height, width, num_fields, background_id, out_h, out_w, quantize ? 1 : 0};
    const dim3 grid(sis_cdiv((int64_t)((out_w + 3) / 4) * out_h, AW_THREADS), batch);
    const bool vec = out_w % 4 == 0 && (uintptr_t)images % 16 == 0 && (uintptr_t)segmented % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(augment_warp_kernel<true>, grid, dim3(AW_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(augment_warp_kernel<false>, grid, dim3(AW_THREADS), 0, (hipStream_t)stream, a);
    SIS_CHECK_LAUNCH("augment_warp_kernel");
    return 0;
}

extern "C" int sis_elastic_field(float* field, float* workspace, float* noise_out, const float* noise, const float* alpha,
                                 const float* sigma, const uint32_t* seeds, int num_fields, int height, int width, void* stream) {
    SIS_REQUIRE(field && workspace && alpha && sigma && (noise || seeds), "sis_elastic_field: null pointer");
    SIS_REQUIRE(num_fields >= 1 && num_fields <= EF_MAX_FIELDS, "sis_elastic_field: %d fields outside 1..%d", num_fields,
                EF_MAX_FIELDS);
    SIS_REQUIRE(height > 0 && width > 0 && height <= 65535 && (int64_t)height * width < ((int64_t)1 << 31),
                "sis_elastic_field: image %dx%d out of range", height, width);
    FieldParams p;
    for (int f = 0; f < num_fields; ++f) {   // HOST arrays
        SIS_REQUIRE(sigma[f] > 0.f && sigma[f] <= 9.0f, "sis_elastic_field: sigma %g outside (0, 9]", (double)sigma[f]);
        p.alpha[f] = alpha[f];
        p.sigma[f] = sigma[f];
        p.seed[f] = seeds ? seeds[f] : 0u;
        p.radius[f] = elastic_radius(sigma[f]);
        SIS_REQUIRE(p.radius[f] <= EF_MAX_RADIUS && height > p.radius[f] && width > p.radius[f],
                    "sis_elastic_field: image %dx%d is not larger than the filter radius %d", height, width, p.radius[f]);
    }
    const dim3 grid(sis_cdiv(width, EF_TILE), height, num_fields * 2);
    hipLaunchKernelGGL(elastic_rows_kernel, grid, dim3(EF_TILE), 0, (hipStream_t)stream, workspace, noise_out, noise, p, height,
                       width);
    SIS_CHECK_LAUNCH("elastic_rows_kernel");
    hipLaunchKernelGGL(elastic_cols_kernel, grid, dim3(EF_TILE), 0, (hipStream_t)stream, field, workspace, p, height, width);
    SIS_CHECK_LAUNCH("elastic_cols_kernel");
    return 0;
}
