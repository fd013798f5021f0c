// Small-contour removal of the segmenters' post-processing (reference networks/base_segmenter.py:25-52,
// utils/segmentation_utils.py:88-102), device-resident and fused with the confidence threshold.  DESIGN.md §10 states the
// definition; in short, per non-background plane of pred [B][C][P][P]:
//   q  = pred < min_confidence ? 0 : pred            M0 = (q * 255.0f) >= 1.0f            M = 5x5 closing of M0
//   O  = background of M that reaches the plane's outside through 4-connected background (every edge pixel touches it)
//   R  = the 8-connected components of (not O): one outermost contour each, holes and islands in holes included
//   2*area(R) = 2 * #(2x2 blocks with 4 pixels in R) + #(2x2 blocks with 3 pixels in R)   (plane padded with zeros)
//   out = q * keep,  keep = 0 on every region with 2*area < 2*min_contour_area, 1 elsewhere
// Connected components are labelled by union-find: a 32x32 tile in LDS, tile borders merged with atomicMin on the global label
// array, then path compression.  Labels are 1-based pixel indices within the plane, a parent is never larger than its child, so
// the root of a set is its smallest member whatever the order the atomics land in; label 0 is "the outside" in the first pass
// and "no region" in the second.  Every decision is an integer one: the output bytes do not depend on timing.
// The launch sequence is fixed (eight launches, no flag read back, no host sync), every find / union loop runs on a step
// budget, and workgroups of one launch only meet through device-scope atomics: a stale plain read of a label yields an older
// parent of the same set, which costs a retry and never a wrong merge.
#include "contour_cc.h"

namespace {

__device__ __forceinline__ float threshold(float v, float min_confidence) { return v < min_confidence ? 0.0f : v; }

// ---- M = closing(M0): dilation sees pixels outside the plane as 0, erosion sees them as 1 -------------------------------------
__global__ __launch_bounds__(CTHREADS) void contour_mask_kernel(uint8_t* __restrict__ mask, const float* __restrict__ pred,
                                                                Plane g, float min_confidence) {
    const int plane = blockIdx.z;
    if (skip_plane(g, plane)) return;
    __shared__ uint8_t m0[CT + 8][CT + 8];
    __shared__ uint8_t dil[CT + 4][CT + 4];
    const int y0 = blockIdx.y * CT, x0 = blockIdx.x * CT;
    const float* src = pred + (int64_t)plane * g.n;
    for (int k = threadIdx.x; k < (CT + 8) * (CT + 8); k += CTHREADS) {
        const int ly = k / (CT + 8), lx = k % (CT + 8);
        const int y = y0 + ly - 4, x = x0 + lx - 4;
        uint8_t v = 0;
        if (y >= 0 && y < g.h && x >= 0 && x < g.w) v = (threshold(src[y * g.w + x], min_confidence) * 255.0f) >= 1.0f;
        m0[ly][lx] = v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < (CT + 4) * (CT + 4); k += CTHREADS) {
        const int ly = k / (CT + 4), lx = k % (CT + 4);
        const int y = y0 + ly - 2, x = x0 + lx - 2;
        uint8_t v = 1;
        if (y >= 0 && y < g.h && x >= 0 && x < g.w) {
            v = 0;
#pragma unroll
            for (int dy = 0; dy < 5; ++dy)
#pragma unroll
                for (int dx = 0; dx < 5; ++dx) v |= m0[ly + dy][lx + dx];
        }
        dil[ly][lx] = v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < CT2; k += CTHREADS) {
        const int ly = k / CT, lx = k % CT;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= g.h || x >= g.w) continue;
        uint8_t v = 1;
#pragma unroll
        for (int dy = 0; dy < 5; ++dy)
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) v &= dil[ly + dy][lx + dx];
        mask[(int64_t)plane * g.n + y * g.w + x] = v;
    }
}

// labels[i] = root; REGION: also clears the area accumulator (the pass-1 label array, no longer read).
template <bool REGION>
__global__ __launch_bounds__(CTHREADS) void contour_compress_kernel(int* __restrict__ labels, int* __restrict__ area2, Plane g) {
    const int plane = blockIdx.y;
    if (skip_plane(g, plane)) return;
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    if (i >= g.n) return;
    int* lab = labels + (int64_t)plane * g.n;
    int budget = g.n + 1;
    const int mine = lab[i];
    if (mine != 0) lab[i] = find_global<false>(lab, mine, budget);
    if (REGION) area2[(int64_t)plane * g.n + i] = 0;
}

// One lane per 2x2 block of the zero-padded plane; lanes of a wave that hold the same region add once.
__global__ __launch_bounds__(CTHREADS) void contour_area_kernel(int* __restrict__ area2, const int* __restrict__ labels,
                                                                const uint8_t* __restrict__ member, Plane g) {
    const int plane = blockIdx.y;
    if (skip_plane(g, plane)) return;
    const int id = blockIdx.x * CTHREADS + threadIdx.x, side = g.w + 1;
    const int64_t base = (int64_t)plane * g.n;
    int add = 0, lab = 0;
    if (id < side * (g.h + 1)) {
        const int by = id / side, bx = id % side;   // pixels (by-1 .. by, bx-1 .. bx)
        int count = 0;
        for (int dy = -1; dy <= 0; ++dy)
            for (int dx = -1; dx <= 0; ++dx) {
                const int y = by + dy, x = bx + dx;
                if (y >= 0 && y < g.h && x >= 0 && x < g.w && member[base + y * g.w + x]) {
                    ++count;
                    lab = labels[base + y * g.w + x];
                }
            }
        add = count == 4 ? 2 : (count == 3 ? 1 : 0);
    }
    if (lab == 0) add = 0;
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(add > 0);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int which = __shfl(lab, leader);
        const bool same = add > 0 && lab == which;
        int sum = same ? add : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == leader) atomicAdd(&area2[base + which - 1], sum);
        pending &= ~__ballot(same);
    }
}

__global__ __launch_bounds__(CTHREADS) void contour_apply_kernel(float* __restrict__ out, const float* __restrict__ pred,
                                                                 const int* __restrict__ labels, const int* __restrict__ area2,
                                                                 Plane g, float min_confidence, int min_area2) {
    const int plane = blockIdx.y;
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    if (i >= g.n) return;
    const int64_t at = (int64_t)plane * g.n + i;
    const float q = threshold(pred[at], min_confidence);
    if (skip_plane(g, plane)) {
        out[at] = q;
        return;
    }
    const int lab = labels[at];
    const bool drop = lab != 0 && area2[(int64_t)plane * g.n + lab - 1] < min_area2;
    out[at] = q * (drop ? 0.0f : 1.0f);
}

}  // namespace

extern "C" int64_t sis_contour_workspace_bytes(int planes, int p) {
    if (planes <= 0 || p <= 0) return 0;
    return (int64_t)planes * p * p * 9;   // two int32 label arrays and one byte mask
}

extern "C" int sis_remove_small_contours(float* out, const float* pred, void* workspace, int64_t workspace_bytes, int batch,
                                         int classes, int p, float min_confidence, int min_contour_area,
                                         int background_class_id, void* stream) {
    SIS_REQUIRE(out && pred && workspace, "sis_remove_small_contours: null pointer");
    SIS_REQUIRE(batch > 0 && classes > 0 && p > 0, "sis_remove_small_contours: non-positive size");
    SIS_REQUIRE(p <= CMAXP, "sis_remove_small_contours: plane edge %d above %d", p, CMAXP);
    SIS_REQUIRE((int64_t)batch * classes <= 65535, "sis_remove_small_contours: more than 65535 planes");
    SIS_REQUIRE(min_contour_area >= 0 && min_contour_area <= (1 << 29), "sis_remove_small_contours: min_contour_area out of range");
    const int planes = batch * classes;
    SIS_REQUIRE(workspace_bytes >= sis_contour_workspace_bytes(planes, p), "sis_remove_small_contours: workspace too small");
    SIS_REQUIRE(((uintptr_t)workspace & 3) == 0, "sis_remove_small_contours: workspace not 4-byte aligned");
    const Plane g{p, p, p * p, classes, background_class_id, 0u};
    const int64_t total = (int64_t)planes * g.n;
    int* outside = (int*)workspace;        // pass-1 labels, later the area accumulator
    int* region = outside + total;         // pass-2 labels
    uint8_t* mask = (uint8_t*)(region + total);
    hipStream_t st = (hipStream_t)stream;
    const dim3 tiles(sis_cdiv(p, CT), sis_cdiv(p, CT), planes), threads(CTHREADS);
    const dim3 pixels(sis_cdiv(g.n, CTHREADS), planes);
    const int lines = (p - 1) / CT;
    const dim3 borders(sis_cdiv((int64_t)2 * lines * p, CTHREADS), planes);

    hipLaunchKernelGGL(contour_mask_kernel, tiles, threads, 0, st, mask, pred, g, min_confidence);
    SIS_CHECK_LAUNCH("contour_mask_kernel");
    hipLaunchKernelGGL(contour_label_tile_kernel<false>, tiles, threads, 0, st, outside, mask, (const int*)nullptr, g);
    SIS_CHECK_LAUNCH("contour_label_tile_kernel<outside>");
    if (lines > 0) {
        hipLaunchKernelGGL(contour_merge_borders_kernel<false>, borders, threads, 0, st, outside, mask, g);
        SIS_CHECK_LAUNCH("contour_merge_borders_kernel<outside>");
    }
    // the pass-2 tile kernel follows pass-1 parents to their roots itself (read only), so pass 1 needs no compression launch
    hipLaunchKernelGGL(contour_label_tile_kernel<true>, tiles, threads, 0, st, region, mask, (const int*)outside, g);
    SIS_CHECK_LAUNCH("contour_label_tile_kernel<region>");
    if (lines > 0) {
        hipLaunchKernelGGL(contour_merge_borders_kernel<true>, borders, threads, 0, st, region, mask, g);
        SIS_CHECK_LAUNCH("contour_merge_borders_kernel<region>");
    }
    hipLaunchKernelGGL(contour_compress_kernel<true>, pixels, threads, 0, st, region, outside, g);
    SIS_CHECK_LAUNCH("contour_compress_kernel");
    hipLaunchKernelGGL(contour_area_kernel, dim3(sis_cdiv((int64_t)(p + 1) * (p + 1), CTHREADS), planes), threads, 0, st, outside,
                       region, mask, g);
    SIS_CHECK_LAUNCH("contour_area_kernel");
    hipLaunchKernelGGL(contour_apply_kernel, pixels, threads, 0, st, out, pred, region, outside, g, min_confidence,
                       2 * min_contour_area);
    SIS_CHECK_LAUNCH("contour_apply_kernel");
    return 0;
}

#include "coco_gt.h"   // the dataset's ground truth: region tables and COCO run lengths on the same labelling kernels
#include "page_visual.h"   // page visualisation: regions of whole pages, colouring, outlines and crops on the same kernels
#include "scan_margin.h"   // scanner-margin removal: Canny front, hysteresis, closing and contour boxes on the same kernels
