// Patch-wise inference of a page image, device-resident:
//  * sis_crop_patches_u8   segmentation/analysis_segmenter.py:115-130 -- PIL crop (zero padding outside the image),
//                          ToTensor (u8 / 255) and Normalize(0.5, 0.5) for a whole grid of patches in one pass;
//  * sis_assemble_max      :147-167 -- element-wise maximum over the patches that cover a pixel, as a gather (one
//                          lane per page pixel walks the patch grid: deterministic, no atomics, no -inf fill pass),
//                          optionally with the label map of networks/base_segmenter.py:59-62 (first maximal class).
//  * sis_assemble_vote     :198-223 (VotingAssemblySegmenter) -- the same gather, adding the confidences of the covering patches
//                          in the reference's row-major patch order and dividing by their sum over the classes (0 where
//                          that sum is 0, torch.nan_to_num);
//  * sis_confusion_matrix   evaluation/segmentation_metric_calculation.py:71-94 -- rows ground truth, columns prediction (first
//                          maximal class when given confidences), per-workgroup histogram in LDS, one integer atomic per
//                          non-empty cell and workgroup, accumulated into the caller's int64 matrix;
//  * sis_color_to_class     utils/segmentation_utils.py:137-157 -- RGB ground-truth image -> class ids by exact colour match.
// All are HBM-bound single passes: 1 byte read + 4 bytes written per element / 4 bytes read per covering patch
// element + 4 written.
#include "sis_common.h"

namespace {

constexpr int PG_MAXC = 16;

struct PatchGrid {
    const int* xs; const int* ys;  // left / top of the patch columns / rows (device arrays, ascending)
    int nx, ny, patch, height, width, channels;
};

__global__ __launch_bounds__(256) void crop_patches_kernel(float* __restrict__ out, const uint8_t* __restrict__ image,
                                                           PatchGrid g) {
    const int n = blockIdx.z, py = blockIdx.y;
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (px >= g.patch) return;
    const int top = g.ys[n / g.nx], left = g.xs[n % g.nx];
    const int y = top + py, x = left + px;
    const bool inside = y < g.height && x < g.width;
    const uint8_t* src = image + ((int64_t)y * g.width + x) * g.channels;
    float* dst = out + (int64_t)n * g.channels * g.patch * g.patch + (int64_t)py * g.patch + px;
    for (int c = 0; c < g.channels; ++c) {
        const float t = (inside ? (float)src[c] : 0.f) / 255.0f;  // ToTensor
        dst[(int64_t)c * g.patch * g.patch] = (t - 0.5f) / 0.5f;  // Normalize(0.5, 0.5)
    }
}

__global__ __launch_bounds__(256) void assemble_max_kernel(float* __restrict__ out, uint8_t* __restrict__ labels,
                                                           const float* __restrict__ pred, PatchGrid g) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= g.width) return;
    float m[PG_MAXC];
#pragma unroll
    for (int c = 0; c < PG_MAXC; ++c) m[c] = -INFINITY;
    const int64_t plane = (int64_t)g.patch * g.patch;
    for (int yi = 0; yi < g.ny; ++yi) {
        const int top = g.ys[yi];
        if (y < top || y >= top + g.patch) continue;
        for (int xi = 0; xi < g.nx; ++xi) {
            const int left = g.xs[xi];
            if (x < left || x >= left + g.patch) continue;
            const float* p = pred + (int64_t)(yi * g.nx + xi) * g.channels * plane + (int64_t)(y - top) * g.patch + (x - left);
#pragma unroll
            for (int c = 0; c < PG_MAXC; ++c)
                if (c < g.channels) m[c] = fmaxf(m[c], p[c * plane]);
        }
    }
    int best = 0;
#pragma unroll
    for (int c = 0; c < PG_MAXC; ++c)
        if (c < g.channels) {
            out[((int64_t)c * g.height + y) * g.width + x] = m[c];
            if (m[c] > m[best]) best = c;
        }
    if (labels) labels[(int64_t)y * g.width + x] = (uint8_t)best;
}

__global__ __launch_bounds__(256) void assemble_vote_kernel(float* __restrict__ out, uint8_t* __restrict__ labels,
                                                            const float* __restrict__ pred, PatchGrid g) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= g.width) return;
    float s[PG_MAXC];
#pragma unroll
    for (int c = 0; c < PG_MAXC; ++c) s[c] = 0.0f;
    const int64_t plane = (int64_t)g.patch * g.patch;
    for (int yi = 0; yi < g.ny; ++yi) {   // row-major over the patches: the order of the reference's `+=` loop
        const int top = g.ys[yi];
        if (y < top || y >= top + g.patch) continue;
        for (int xi = 0; xi < g.nx; ++xi) {
            const int left = g.xs[xi];
            if (x < left || x >= left + g.patch) continue;
            const float* p = pred + (int64_t)(yi * g.nx + xi) * g.channels * plane + (int64_t)(y - top) * g.patch + (x - left);
#pragma unroll
            for (int c = 0; c < PG_MAXC; ++c)
                if (c < g.channels) s[c] += p[c * plane];
        }
    }
    float total = 0.0f;
#pragma unroll
    for (int c = 0; c < PG_MAXC; ++c)
        if (c < g.channels) total += s[c];
    int best = 0;
    float best_v = 0.0f;
#pragma unroll
    for (int c = 0; c < PG_MAXC; ++c)
        if (c < g.channels) {
            float v = s[c] / total;
            if (v != v) v = 0.0f;                                  // torch.nan_to_num: nan -> 0,
            else if (fabsf(v) == INFINITY) v = copysignf(3.4028234663852886e38f, v);   // +-inf -> +-FLT_MAX
            out[((int64_t)c * g.height + y) * g.width + x] = v;
            if (c == 0 || v > best_v) { best = c; best_v = v; }
        }
    if (labels) labels[(int64_t)y * g.width + x] = (uint8_t)best;
}

constexpr int CM_PIXELS_PER_LANE = 16;

// prediction: confidences [classes][n] (first maximal class is taken here) or null; labels: uint8 [n] class ids, used when
// prediction is null.  Pixels whose ground truth or label is not a class id count nowhere, as in the reference's double loop.
__global__ __launch_bounds__(256) void confusion_matrix_kernel(unsigned long long* __restrict__ matrix,
                                                               const float* __restrict__ prediction,
                                                               const uint8_t* __restrict__ labels,
                                                               const uint8_t* __restrict__ truth, int64_t n, int classes) {
    __shared__ int hist[PG_MAXC * PG_MAXC];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * 256 * CM_PIXELS_PER_LANE + threadIdx.x;
    for (int k = 0; k < CM_PIXELS_PER_LANE; ++k) {
        const int64_t i = first + (int64_t)k * 256;
        if (i >= n) break;
        int best = 0;
        if (prediction) {
            float best_v = prediction[i];
            for (int c = 1; c < classes; ++c) {
                const float v = prediction[(int64_t)c * n + i];
                if (v > best_v) { best = c; best_v = v; }
            }
        } else {
            best = labels[i];
        }
        const int t = truth[i];
        if (t < classes && best < classes) atomicAdd(&hist[t * classes + best], 1);
    }
    __syncthreads();
    if ((int)threadIdx.x < classes * classes && hist[threadIdx.x] != 0)
        atomicAdd(&matrix[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

constexpr int CC_MAX = 64;
struct ColorTable {
    int count;
    uint32_t rgb[CC_MAX];   // r | g << 8 | b << 16
    uint8_t id[CC_MAX];
};

__global__ __launch_bounds__(256) void color_to_class_kernel(uint8_t* __restrict__ out, const uint8_t* __restrict__ image,
                                                             int64_t n, int background_id, ColorTable t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t px = image[3 * i] | (uint32_t)image[3 * i + 1] << 8 | (uint32_t)image[3 * i + 2] << 16;
    int id = background_id;
    for (int k = 0; k < t.count; ++k)   // a later entry of the map wins, as in the reference's chain of numpy.where
        if (t.rgb[k] == px) id = t.id[k];
    out[i] = (uint8_t)id;
}

int check_grid(const char* who, const PatchGrid& g) {
    SIS_REQUIRE(g.xs && g.ys, "%s: null patch grid", who);
    SIS_REQUIRE(g.nx > 0 && g.ny > 0 && g.patch > 0 && g.height > 0 && g.width > 0, "%s: non-positive size", who);
    SIS_REQUIRE(g.channels >= 1 && g.channels <= PG_MAXC, "%s: %d channels outside 1..%d", who, g.channels, PG_MAXC);
    SIS_REQUIRE((int64_t)g.nx * g.ny <= 65535, "%s: more than 65535 patches", who);
    return 0;
}

}  // namespace

extern "C" int sis_crop_patches_u8(float* out, const uint8_t* image, const int* xs, const int* ys, int nx, int ny,
                                   int height, int width, int channels, int patch, void* stream) {
    PatchGrid g{xs, ys, nx, ny, patch, height, width, channels};
    if (check_grid("sis_crop_patches_u8", g)) return 1;
    SIS_REQUIRE(out && image, "sis_crop_patches_u8: null pointer");
    SIS_REQUIRE(patch <= 65535, "sis_crop_patches_u8: patch too large");
    hipLaunchKernelGGL(crop_patches_kernel, dim3(sis_cdiv(patch, 256), patch, nx * ny), dim3(256), 0, (hipStream_t)stream,
                       out, image, g);
    SIS_CHECK_LAUNCH("crop_patches_kernel");
    return 0;
}

extern "C" int sis_assemble_max(float* out, uint8_t* labels, const float* pred, const int* xs, const int* ys, int nx,
                                int ny, int classes, int height, int width, int patch, void* stream) {
    PatchGrid g{xs, ys, nx, ny, patch, height, width, classes};
    if (check_grid("sis_assemble_max", g)) return 1;
    SIS_REQUIRE(out && pred, "sis_assemble_max: null pointer");
    SIS_REQUIRE(height <= 65535, "sis_assemble_max: image too tall");
    hipLaunchKernelGGL(assemble_max_kernel, dim3(sis_cdiv(width, 256), height), dim3(256), 0, (hipStream_t)stream, out,
                       labels, pred, g);
    SIS_CHECK_LAUNCH("assemble_max_kernel");
    return 0;
}

extern "C" int sis_assemble_vote(float* out, uint8_t* labels, const float* pred, const int* xs, const int* ys, int nx,
                                 int ny, int classes, int height, int width, int patch, void* stream) {
    PatchGrid g{xs, ys, nx, ny, patch, height, width, classes};
    if (check_grid("sis_assemble_vote", g)) return 1;
    SIS_REQUIRE(out && pred, "sis_assemble_vote: null pointer");
    SIS_REQUIRE(height <= 65535, "sis_assemble_vote: image too tall");
    hipLaunchKernelGGL(assemble_vote_kernel, dim3(sis_cdiv(width, 256), height), dim3(256), 0, (hipStream_t)stream, out,
                       labels, pred, g);
    SIS_CHECK_LAUNCH("assemble_vote_kernel");
    return 0;
}

extern "C" int sis_confusion_matrix(int64_t* matrix, const float* prediction, const uint8_t* labels, const uint8_t* ground_truth,
                                    int64_t pixels, int classes, void* stream) {
    SIS_REQUIRE(matrix && ground_truth && (prediction || labels), "sis_confusion_matrix: null pointer");
    SIS_REQUIRE(classes >= 1 && classes <= PG_MAXC, "sis_confusion_matrix: %d classes outside 1..%d", classes, PG_MAXC);
    SIS_REQUIRE(pixels > 0 && pixels < ((int64_t)1 << 40), "sis_confusion_matrix: pixel count out of range");
    hipLaunchKernelGGL(confusion_matrix_kernel, dim3(sis_cdiv(pixels, 256 * CM_PIXELS_PER_LANE)), dim3(256), 0,
                       (hipStream_t)stream, (unsigned long long*)matrix, prediction, labels, ground_truth, pixels, classes);
    SIS_CHECK_LAUNCH("confusion_matrix_kernel");
    return 0;
}

extern "C" int sis_color_to_class(uint8_t* out, const uint8_t* image, int64_t pixels, int background_id, const uint8_t* colors,
                                  const uint8_t* ids, int count, void* stream) {
    SIS_REQUIRE(out && image && (count == 0 || (colors && ids)), "sis_color_to_class: null pointer");
    SIS_REQUIRE(count >= 0 && count <= CC_MAX, "sis_color_to_class: %d colours outside 0..%d", count, CC_MAX);
    SIS_REQUIRE(pixels > 0 && background_id >= 0 && background_id <= 255, "sis_color_to_class: bad size or background id");
    ColorTable t;
    t.count = count;
    for (int k = 0; k < count; ++k) {   // HOST arrays: colours [count][3] (r, g, b) and the class id of each
        t.rgb[k] = colors[3 * k] | (uint32_t)colors[3 * k + 1] << 8 | (uint32_t)colors[3 * k + 2] << 16;
        t.id[k] = ids[k];
    }
    hipLaunchKernelGGL(color_to_class_kernel, dim3(sis_cdiv(pixels, 256)), dim3(256), 0, (hipStream_t)stream, out, image, pixels,
                       background_id, t);
    SIS_CHECK_LAUNCH("color_to_class_kernel");
    return 0;
}
