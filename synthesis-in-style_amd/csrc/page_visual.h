// Page visualisation on the device (reference segmentation/evaluation/segmentation_visualization.py:22-166,
// visualization/utils.py:9-68, utils/segmentation_utils.py:88-121): the text regions of a whole assembled page with their
// boxes, the colour-coded page and its overlay on the scan, the box outlines and the cut-out regions.  DESIGN.md §17 states the
// contract.  Included at the end of contour_ops.hip, which has the mask, labelling, compression and area kernels in scope; a
// page is a rectangular Plane (contour_cc.h) of up to 8192 x 8192 pixels.
// Every decision is an integer one (the colouring compares floats and converts one to an index, no float is accumulated across
// lanes), every accumulation a min, a max or a sum of integers: the bytes do not depend on timing.  The launch sequences are
// fixed by the arguments, nothing is read back.  Workgroups of one launch meet only through device-scope atomics on the table
// rows, which no kernel reads with a plain load before the launch ends.
#pragma once
#include <limits.h>

namespace {

constexpr int PV_MAX_EDGE = 8192;
constexpr int PV_MAX_CLASSES = 16;
constexpr int PV_STEPS = 100;          // entries of a class's confidence gradient
constexpr int PV_CROP_SLICES = 8;      // workgroups that share one crop (most crops are a few hundred pixels)
constexpr int PV_COORD_LIMIT = 1 << 20;
// a row of the region table
enum { PV_ROOT, PV_X0, PV_Y0, PV_W, PV_H, PV_AREA2, PV_KEPT, PV_ZERO, PV_ROW };

struct PvColours {
    uint8_t rgb[PV_MAX_CLASSES][3];
};

// ---- regions ---------------------------------------------------------------------------------------------------------------------
// One workgroup per plane, as gt_rank_kernel: a root is the pixel whose label names itself, its slot is the number of roots
// before it in raster order.  `area2` holds twice the region's area at the root's pixel (contour_area_kernel); the root's lane
// reads it, counts the region as kept or dropped, writes the row's head and leaves the slot in its place.  Until
// pv_finish_kernel a row holds the box as min x, min y, max x, max y.
__global__ __launch_bounds__(GT_SCAN_THREADS) void pv_rank_kernel(int* __restrict__ area2, int* __restrict__ regions,
                                                                  int* __restrict__ region_count, int* __restrict__ kept_count,
                                                                  const int* __restrict__ labels, Plane g, int max_regions,
                                                                  int min_area2) {
    const int plane = blockIdx.x;
    if (skip_plane(g, plane)) {
        if (threadIdx.x == 0) region_count[plane] = 0, kept_count[plane] = 0;
        return;
    }
    const int* lab = labels + (int64_t)plane * g.n;
    int* slots = area2 + (int64_t)plane * g.n;
    int* rows = regions + (int64_t)plane * max_regions * PV_ROW;
    __shared__ int sums[GT_SCAN_THREADS / 64], kept_sums[GT_SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = GT_SCAN_THREADS / 64;
    const int segment = ((g.n + waves - 1) / waves + 63) / 64 * 64;   // a wave walks one contiguous segment, 64 pixels a step
    const int seg0 = min(wave * segment, g.n), seg1 = min(seg0 + segment, g.n);
    int count = 0, kept = 0;
    for (int i0 = seg0; i0 < seg1; i0 += 64) {
        const int i = i0 + lane;
        const bool root = i < seg1 && lab[i] == i + 1;
        count += __popcll(__ballot(root));
        kept += __popcll(__ballot(root && slots[i] >= min_area2));
    }
    if (lane == 0) sums[wave] = count, kept_sums[wave] = kept;
    __syncthreads();
    int running = 0, total = 0, total_kept = 0;
    for (int w = 0; w < waves; ++w) {
        running += w < wave ? sums[w] : 0;
        total += sums[w];
        total_kept += kept_sums[w];
    }
    for (int i0 = seg0; i0 < seg1; i0 += 64) {
        const int i = i0 + lane;
        const bool root = i < seg1 && lab[i] == i + 1;
        const unsigned long long roots = __ballot(root);
        if (root) {
            const int s = running + __popcll(roots & ((1ull << lane) - 1ull));
            const int twice_area = slots[i];
            slots[i] = s;
            if (s < max_regions) {
                int* row = rows + (int64_t)s * PV_ROW;
                row[PV_ROOT] = i;
                row[PV_X0] = INT_MAX, row[PV_Y0] = INT_MAX, row[PV_W] = INT_MIN, row[PV_H] = INT_MIN;
                row[PV_AREA2] = twice_area, row[PV_KEPT] = twice_area >= min_area2 ? 1 : 0, row[PV_ZERO] = 0;
            }
        }
        running += __popcll(roots);
    }
    if (threadIdx.x == 0) region_count[plane] = total, kept_count[plane] = total_kept;
}

// One lane per pixel: the label map (root + 1, 0 outside any region, 0 on a skipped plane) and the extents of the stored rows.
// Lanes of a wave in the same region combine their extents first, as gt_stats_kernel does.
__global__ __launch_bounds__(CTHREADS) void pv_box_kernel(int* __restrict__ regions, int* __restrict__ region_labels,
                                                          const int* __restrict__ labels, const int* __restrict__ slot_of,
                                                          Plane g, int max_regions) {
    const int plane = blockIdx.y;
    const int i = blockIdx.x * CTHREADS + threadIdx.x, lane = threadIdx.x & 63;
    const bool valid = i < g.n;
    const int64_t base = (int64_t)plane * g.n;
    if (skip_plane(g, plane)) {   // workgroup-uniform
        if (valid && region_labels != nullptr) region_labels[base + i] = 0;
        return;
    }
    const int mine = valid ? labels[base + i] : 0;
    if (valid && region_labels != nullptr) region_labels[base + i] = mine;
    if (regions == nullptr) return;
    const int slot = mine != 0 ? slot_of[base + mine - 1] : 0;
    const int y = valid ? i / g.w : 0, x = valid ? i % g.w : 0;
    const bool own = mine != 0 && slot < max_regions;
    int* rows = regions + (int64_t)plane * max_regions * PV_ROW;
    unsigned long long pending = __ballot(own);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int which = __shfl(mine, leader);
        const bool same = own && mine == which;
        const int min_x = gt_wave_min(same ? x : INT_MAX), max_x = gt_wave_max(same ? x : INT_MIN);
        const int min_y = gt_wave_min(same ? y : INT_MAX), max_y = gt_wave_max(same ? y : INT_MIN);
        if (lane == leader) {
            int* row = rows + (int64_t)slot * PV_ROW;
            gt_lower(&row[PV_X0], min_x), gt_raise(&row[PV_W], max_x);
            gt_lower(&row[PV_Y0], min_y), gt_raise(&row[PV_H], max_y);
        }
        pending &= ~__ballot(same);
    }
}

// One lane per stored row: max x, max y become width and height.
__global__ __launch_bounds__(CTHREADS) void pv_finish_kernel(int* __restrict__ regions, const int* __restrict__ region_count,
                                                             int max_regions) {
    const int plane = blockIdx.y, s = blockIdx.x * CTHREADS + threadIdx.x;
    if (s >= min(region_count[plane], max_regions)) return;
    int* row = regions + ((int64_t)plane * max_regions + s) * PV_ROW;
    row[PV_W] = row[PV_W] - row[PV_X0] + 1;
    row[PV_H] = row[PV_H] - row[PV_Y0] + 1;
}

// ---- colouring and overlay -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pv_store(uint8_t* image, int64_t pixel, uint8_t r, uint8_t g, uint8_t b) {
    if (image == nullptr) return;
    image[3 * pixel] = r, image[3 * pixel + 1] = g, image[3 * pixel + 2] = b;
}

// One lane per pixel.  table == nullptr: the colour of the first maximal class.  Otherwise the confidence mode: where the
// float32 sum of the non-background planes (class order) is > 0, entry (int)(100.0 * (double)max) - 1 of the first maximal
// class's gradient; index -1 is the last entry, as Python's negative list index, and an index past the table (a confidence
// above 1, where the reference raises) is the last entry too.
__global__ __launch_bounds__(CTHREADS) void pv_colour_kernel(uint8_t* __restrict__ segmented, uint8_t* __restrict__ overlay,
                                                             uint8_t* __restrict__ boxes_on_page,
                                                             uint8_t* __restrict__ boxes_on_segmented,
                                                             const float* __restrict__ pred, const uint8_t* __restrict__ page,
                                                             int page_channels, PvColours colours,
                                                             const uint8_t* __restrict__ table, int classes, int n,
                                                             int background) {
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    if (i >= n) return;
    float best = pred[i], others = 0.0f;
    int which = 0;
    for (int k = 0; k < classes; ++k) {
        const float v = pred[(int64_t)k * n + i];
        if (v > best) best = v, which = k;
        if (k != background) others += v;
    }
    uint8_t r = colours.rgb[background][0], g = colours.rgb[background][1], b = colours.rgb[background][2];
    if (table == nullptr) {
        r = colours.rgb[which][0], g = colours.rgb[which][1], b = colours.rgb[which][2];
    } else if (others > 0.0f) {
        int idx = (int)(100.0 * (double)best) - 1;
        if (!(idx >= 0 && idx < PV_STEPS)) idx = PV_STEPS - 1;
        const uint8_t* entry = table + ((int64_t)which * PV_STEPS + idx) * 3;
        r = entry[0], g = entry[1], b = entry[2];
    }
    pv_store(segmented, i, r, g, b);
    pv_store(boxes_on_segmented, i, r, g, b);
    if (page == nullptr) return;
    uint8_t pr, pg, pb;
    if (page_channels == 1) {
        pr = pg = pb = page[i];
    } else {
        pr = page[3 * (int64_t)i], pg = page[3 * (int64_t)i + 1], pb = page[3 * (int64_t)i + 2];
    }
    pv_store(boxes_on_page, i, pr, pg, pb);
    const bool is_background = r == colours.rgb[background][0] && g == colours.rgb[background][1] && b == colours.rgb[background][2];
    if (is_background) pv_store(overlay, i, pr, pg, pb);
    else pv_store(overlay, i, r, g, b);
}

// ---- outlines --------------------------------------------------------------------------------------------------------------------------
// The workgroup paints the pixels of [xa, xb] x [ya, yb] that lie within the image.
__device__ __forceinline__ void pv_fill(uint8_t* a, uint8_t* b, int height, int width, int xa, int ya, int xb, int yb, uint8_t cr,
                                        uint8_t cg, uint8_t cb) {
    xa = max(xa, 0), ya = max(ya, 0), xb = min(xb, width - 1), yb = min(yb, height - 1);
    if (xa > xb || ya > yb) return;
    const int across = xb - xa + 1, count = across * (yb - ya + 1);   // a strip: `stroke` rows or columns, below 2^31
    for (int t = threadIdx.x; t < count; t += blockDim.x) {
        const int64_t pixel = (int64_t)(ya + t / across) * width + xa + t % across;
        pv_store(a, pixel, cr, cg, cb);
        pv_store(b, pixel, cr, cg, cb);
    }
}

// Every pixel of [x0, x1] x [y0, y1] within the image that is nearer than `stroke` to one of the box's four sides: four strips.
__device__ __forceinline__ void pv_outline(uint8_t* a, uint8_t* b, int height, int width, int x0, int y0, int x1, int y1,
                                           int stroke, uint8_t cr, uint8_t cg, uint8_t cb) {
    if (x0 > x1 || y0 > y1) return;
    if (x0 < -PV_COORD_LIMIT || y0 < -PV_COORD_LIMIT || x1 > PV_COORD_LIMIT || y1 > PV_COORD_LIMIT) return;
    pv_fill(a, b, height, width, x0, y0, x1, min(y0 + stroke - 1, y1), cr, cg, cb);
    pv_fill(a, b, height, width, x0, max(y1 - stroke + 1, y0), x1, y1, cr, cg, cb);
    pv_fill(a, b, height, width, x0, y0, min(x0 + stroke - 1, x1), y1, cr, cg, cb);
    pv_fill(a, b, height, width, max(x1 - stroke + 1, x0), y0, x1, y1, cr, cg, cb);
}

// One workgroup per row of the region tables; rows past the plane's count and dropped regions exit.
__global__ __launch_bounds__(CTHREADS) void pv_region_boxes_kernel(uint8_t* __restrict__ a, uint8_t* __restrict__ b,
                                                                   const int* __restrict__ regions,
                                                                   const int* __restrict__ region_count, int max_regions,
                                                                   int height, int width) {
    const int plane = blockIdx.y, s = blockIdx.x;
    if (s >= min(region_count[plane], max_regions)) return;
    const int* row = regions + ((int64_t)plane * max_regions + s) * PV_ROW;
    if (row[PV_KEPT] == 0) return;
    const int x0 = row[PV_X0], y0 = row[PV_Y0], w = row[PV_W], h = row[PV_H];
    if (x0 < 0 || y0 < 0 || x0 >= width || y0 >= height || w < 1 || h < 1 || w > PV_MAX_EDGE || h > PV_MAX_EDGE) return;
    pv_outline(a, b, height, width, x0, y0, x0 + w, y0 + h, 3, 0, 255, 0);
}

// One workgroup per patch box (x0, y0, x1, y1, both ends inclusive).
__global__ __launch_bounds__(CTHREADS) void pv_patch_boxes_kernel(uint8_t* __restrict__ a, uint8_t* __restrict__ b,
                                                                  const int* __restrict__ boxes, int height, int width) {
    const int* box = boxes + (int64_t)blockIdx.x * 4;
    pv_outline(a, b, height, width, box[0], box[1], box[2], box[3], 1, 255, 0, 0);
}

// ---- crops -----------------------------------------------------------------------------------------------------------------------------
// PV_CROP_SLICES workgroups per table row (plane, root, x0, y0, w, h, byte offset).  A row whose box leaves the page, whose
// plane does not exist or whose crop leaves the buffer is not written.
__global__ __launch_bounds__(CTHREADS) void pv_crops_kernel(uint8_t* __restrict__ out, int64_t out_bytes,
                                                            const int64_t* __restrict__ table, const uint8_t* __restrict__ page,
                                                            int page_channels, const int* __restrict__ region_labels, int classes,
                                                            int height, int width, int contour) {
    const int64_t* row = table + (int64_t)blockIdx.x * 7;
    const int64_t plane = row[0], root = row[1], x0 = row[2], y0 = row[3], w = row[4], h = row[5], offset = row[6];
    if (plane < 0 || plane >= classes || x0 < 0 || y0 < 0 || w < 1 || h < 1 || x0 + w > width || y0 + h > height) return;
    if (offset < 0 || offset > out_bytes || w * h * 3 > out_bytes - offset) return;
    const int* lab = region_labels + plane * height * width;   // not dereferenced unless `contour`
    const int64_t count = w * h;
    for (int64_t t = (int64_t)blockIdx.y * CTHREADS + threadIdx.x; t < count; t += (int64_t)PV_CROP_SLICES * CTHREADS) {
        const int64_t pixel = (y0 + t / w) * width + x0 + t % w;
        uint8_t r = 255, g = 255, b = 255;
        if (!contour || lab[pixel] == root + 1) {
            if (page_channels == 1) r = g = b = page[pixel];
            else r = page[3 * pixel], g = page[3 * pixel + 1], b = page[3 * pixel + 2];
        }
        uint8_t* dst = out + offset + 3 * t;
        dst[0] = r, dst[1] = g, dst[2] = b;
    }
}

inline bool pv_page_shape_ok(int classes, int height, int width) {
    return classes >= 2 && classes <= PV_MAX_CLASSES && height >= 1 && height <= PV_MAX_EDGE && width >= 1 && width <= PV_MAX_EDGE;
}

}  // namespace

// At 8192 x 8192: n = 2^26, the union budget 4 * n + 64 and the (h + 1) * (w + 1) blocks of the area kernel are below 2^31,
// 2 * area <= 2^27; offsets across planes are 64-bit.
extern "C" int64_t sis_page_regions_workspace_bytes(int classes, int height, int width) {
    if (!pv_page_shape_ok(classes, height, width)) return 0;
    return (int64_t)classes * height * width * 9;   // two int32 label arrays and one byte mask
}

extern "C" int sis_page_regions(int32_t* regions, int32_t* region_count, int32_t* kept_count, int32_t* region_labels,
                                const float* pred, int classes, int height, int width, int background_class_id,
                                uint32_t filter_classes, int min_contour_area, int max_regions, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    SIS_REQUIRE(region_count && kept_count && pred && workspace, "sis_page_regions: null pointer");
    SIS_REQUIRE(classes >= 2 && classes <= PV_MAX_CLASSES, "sis_page_regions: classes %d outside 2..%d", classes, PV_MAX_CLASSES);
    SIS_REQUIRE(height >= 1 && height <= PV_MAX_EDGE && width >= 1 && width <= PV_MAX_EDGE,
                "sis_page_regions: page %d x %d outside 1..%d a side", height, width, PV_MAX_EDGE);
    SIS_REQUIRE(background_class_id >= 0 && background_class_id < classes, "sis_page_regions: background class %d outside the classes",
                background_class_id);
    SIS_REQUIRE((filter_classes >> classes) == 0, "sis_page_regions: filter_classes names a class past the last");
    SIS_REQUIRE(min_contour_area >= 0 && min_contour_area <= (1 << 29), "sis_page_regions: min_contour_area out of range");
    SIS_REQUIRE(max_regions >= 0 && (int64_t)max_regions * classes * PV_ROW <= INT_MAX, "sis_page_regions: max_regions out of range");
    SIS_REQUIRE(regions != nullptr || max_regions == 0, "sis_page_regions: max_regions without a table");
    SIS_REQUIRE(workspace_bytes >= sis_page_regions_workspace_bytes(classes, height, width), "sis_page_regions: workspace too small");
    SIS_REQUIRE(((uintptr_t)workspace & 3) == 0, "sis_page_regions: workspace not 4-byte aligned");
    const Plane g{width, height, width * height, classes, background_class_id, filter_classes};
    const int64_t total = (int64_t)classes * g.n;
    int* outside = (int*)workspace;        // pass-1 labels, then twice the areas, then the slot of every root
    int* region = outside + total;         // pass-2 labels
    uint8_t* mask = (uint8_t*)(region + total);
    hipStream_t st = (hipStream_t)stream;
    const dim3 tiles(sis_cdiv(width, CT), sis_cdiv(height, CT), classes), threads(CTHREADS);
    const dim3 pixels(sis_cdiv(g.n, CTHREADS), classes);
    const int64_t border_pixels = (int64_t)((width - 1) / CT) * height + (int64_t)((height - 1) / CT) * width;
    const dim3 borders(sis_cdiv(border_pixels, CTHREADS), classes);

    hipLaunchKernelGGL(contour_mask_kernel, tiles, threads, 0, st, mask, pred, g, 0.0f);   // no confidence threshold here
    SIS_CHECK_LAUNCH("contour_mask_kernel");
    hipLaunchKernelGGL(contour_label_tile_kernel<false>, tiles, threads, 0, st, outside, mask, (const int*)nullptr, g);
    SIS_CHECK_LAUNCH("contour_label_tile_kernel<outside>");
    if (border_pixels > 0) {
        hipLaunchKernelGGL(contour_merge_borders_kernel<false>, borders, threads, 0, st, outside, mask, g);
        SIS_CHECK_LAUNCH("contour_merge_borders_kernel<outside>");
    }
    // on a page the pass-1 parent chains cross many tiles: compressed once here, not followed per pixel by the pass-2 kernel
    hipLaunchKernelGGL(contour_compress_kernel<false>, pixels, threads, 0, st, outside, (int*)nullptr, g);
    SIS_CHECK_LAUNCH("contour_compress_kernel<outside>");
    hipLaunchKernelGGL(contour_label_tile_kernel<true>, tiles, threads, 0, st, region, mask, (const int*)outside, g);
    SIS_CHECK_LAUNCH("contour_label_tile_kernel<region>");
    if (border_pixels > 0) {
        hipLaunchKernelGGL(contour_merge_borders_kernel<true>, borders, threads, 0, st, region, mask, g);
        SIS_CHECK_LAUNCH("contour_merge_borders_kernel<region>");
    }
    hipLaunchKernelGGL(contour_compress_kernel<true>, pixels, threads, 0, st, region, outside, g);
    SIS_CHECK_LAUNCH("contour_compress_kernel<region>");
    hipLaunchKernelGGL(contour_area_kernel, dim3(sis_cdiv((int64_t)(height + 1) * (width + 1), CTHREADS), classes), threads, 0, st,
                       outside, region, mask, g);
    SIS_CHECK_LAUNCH("contour_area_kernel");
    hipLaunchKernelGGL(pv_rank_kernel, dim3(classes), dim3(GT_SCAN_THREADS), 0, st, outside, regions, region_count, kept_count, region,
                       g, max_regions, 2 * min_contour_area);
    SIS_CHECK_LAUNCH("pv_rank_kernel");
    if (max_regions > 0 || region_labels != nullptr) {
        hipLaunchKernelGGL(pv_box_kernel, pixels, threads, 0, st, max_regions > 0 ? regions : (int*)nullptr, region_labels, region,
                           outside, g, max_regions);
        SIS_CHECK_LAUNCH("pv_box_kernel");
    }
    if (max_regions > 0) {
        hipLaunchKernelGGL(pv_finish_kernel, dim3(sis_cdiv(max_regions, CTHREADS), classes), threads, 0, st, regions, region_count,
                           max_regions);
        SIS_CHECK_LAUNCH("pv_finish_kernel");
    }
    return 0;
}

extern "C" int sis_page_render(uint8_t* segmented, uint8_t* overlay, uint8_t* boxes_on_page, uint8_t* boxes_on_segmented,
                               const float* pred, const uint8_t* page, int page_channels, const uint8_t* colours,
                               const uint8_t* confidence_table, const int32_t* regions, const int32_t* region_count, int max_regions,
                               const int32_t* patch_boxes, int patches, int classes, int height, int width, int background_class_id,
                               void* stream) {
    SIS_REQUIRE(pred && colours, "sis_page_render: null pointer");
    SIS_REQUIRE(segmented || overlay || boxes_on_page || boxes_on_segmented, "sis_page_render: no output");
    SIS_REQUIRE(page != nullptr || (overlay == nullptr && boxes_on_page == nullptr), "sis_page_render: null page");
    SIS_REQUIRE(page == nullptr || page_channels == 1 || page_channels == 3, "sis_page_render: page of %d channels", page_channels);
    SIS_REQUIRE(classes >= 2 && classes <= PV_MAX_CLASSES, "sis_page_render: classes %d outside 2..%d", classes, PV_MAX_CLASSES);
    SIS_REQUIRE(height >= 1 && height <= PV_MAX_EDGE && width >= 1 && width <= PV_MAX_EDGE,
                "sis_page_render: page %d x %d outside 1..%d a side", height, width, PV_MAX_EDGE);
    SIS_REQUIRE(background_class_id >= 0 && background_class_id < classes, "sis_page_render: background class %d outside the classes",
                background_class_id);
    SIS_REQUIRE(max_regions >= 0 && max_regions <= 65535 * 1024, "sis_page_render: max_regions out of range");
    SIS_REQUIRE(max_regions == 0 || (regions && region_count), "sis_page_render: max_regions without tables");
    SIS_REQUIRE(patches >= 0, "sis_page_render: negative number of patch boxes");
    SIS_REQUIRE(patches == 0 || patch_boxes, "sis_page_render: patch boxes missing");
    PvColours c;
    for (int k = 0; k < PV_MAX_CLASSES; ++k)
        for (int j = 0; j < 3; ++j) c.rgb[k][j] = k < classes ? colours[3 * k + j] : 0;
    hipStream_t st = (hipStream_t)stream;
    const int n = height * width;
    hipLaunchKernelGGL(pv_colour_kernel, dim3(sis_cdiv(n, CTHREADS)), dim3(CTHREADS), 0, st, segmented, overlay, boxes_on_page,
                       boxes_on_segmented, pred, page, page_channels, c, confidence_table, classes, n, background_class_id);
    SIS_CHECK_LAUNCH("pv_colour_kernel");
    if (boxes_on_page == nullptr && boxes_on_segmented == nullptr) return 0;
    if (max_regions > 0) {   // green first, red afterwards: two launches, so the bytes do not depend on the order of the writes
        hipLaunchKernelGGL(pv_region_boxes_kernel, dim3(max_regions, classes), dim3(CTHREADS), 0, st, boxes_on_page, boxes_on_segmented,
                           regions, region_count, max_regions, height, width);
        SIS_CHECK_LAUNCH("pv_region_boxes_kernel");
    }
    if (patches > 0) {
        hipLaunchKernelGGL(pv_patch_boxes_kernel, dim3(patches), dim3(CTHREADS), 0, st, boxes_on_page, boxes_on_segmented, patch_boxes,
                           height, width);
        SIS_CHECK_LAUNCH("pv_patch_boxes_kernel");
    }
    return 0;
}

extern "C" int sis_page_crops(uint8_t* out, int64_t out_bytes, const int64_t* table, int rows, const uint8_t* page, int page_channels,
                              const int32_t* region_labels, int classes, int height, int width, int mode, void* stream) {
    SIS_REQUIRE(out && table && page, "sis_page_crops: null pointer");
    SIS_REQUIRE(mode == 0 || mode == 1, "sis_page_crops: mode %d is neither bbox (0) nor contour (1)", mode);
    SIS_REQUIRE(mode == 0 || region_labels != nullptr, "sis_page_crops: contour mode without region labels");
    SIS_REQUIRE(page_channels == 1 || page_channels == 3, "sis_page_crops: page of %d channels", page_channels);
    SIS_REQUIRE(classes >= 2 && classes <= PV_MAX_CLASSES, "sis_page_crops: classes %d outside 2..%d", classes, PV_MAX_CLASSES);
    SIS_REQUIRE(height >= 1 && height <= PV_MAX_EDGE && width >= 1 && width <= PV_MAX_EDGE,
                "sis_page_crops: page %d x %d outside 1..%d a side", height, width, PV_MAX_EDGE);
    SIS_REQUIRE(rows >= 1 && out_bytes >= 1, "sis_page_crops: non-positive size");
    hipLaunchKernelGGL(pv_crops_kernel, dim3(rows, PV_CROP_SLICES), dim3(CTHREADS), 0, (hipStream_t)stream, out, out_bytes, table,
                       page, page_channels, region_labels, classes, height, width, mode);
    SIS_CHECK_LAUNCH("pv_crops_kernel");
    return 0;
}
