// Cluster-based dataset labeller (reference segmentation/base_cluster_based_dataset_segmenter.py:119-450 and
// segmentation/black_white_handwritten_printed_text_segmenter.py:31-99), device-resident.  DESIGN.md §11 states the
// definition; in short, per image:
//   plane (key, class)  D = 3x3-cross dilation of the nearest-enlarged class mask of the key's cluster map
//                       regions of D as in contour_ops.hip (outside through 4-connected background, 8-connected components)
//   job (class, keys)   groups = transitive closure of "two regions share a pixel" over the job's planes; a gap (4-connected
//                       complement of the union that does not reach the outside) bordering exactly one group joins it
//   jobs 0 .. C-1       the text regions of non-background class c over the class-determination keys
//   job C               the fine regions of the fine-grained class over the fine-grained keys
//   score[f][c] = |f and union of the kept text groups of c|, first maximal class wins, small regions go, label = class of
//   the fine region where the undilated fine-grained mask of the last fine-grained key is set.
// A group is named by the pixel index of its smallest region root: two groups of one job cannot have their roots at the same
// pixel (their regions would share it), so every per-group accumulator is an int array over the pixels of the image.
// Every decision is an integer one, the launch sequence is fixed (one memset, sixteen launches, nothing read back), every
// find / union loop runs on a step budget and accumulators are integer atomics: the output bytes do not depend on timing.
#include "contour_cc.h"

namespace {

constexpr int CS_MAX_KEYS = 8;       // cluster maps, and keys per job
constexpr int CS_MAX_CLASSES = 7;    // non-background classes
constexpr int CS_MAX_JOBS = CS_MAX_CLASSES + 1;
constexpr int CS_MAX_PLANES = CS_MAX_CLASSES * CS_MAX_KEYS + CS_MAX_KEYS;
constexpr int CS_CLUSTERS = 256;

struct Segment {
    int s, n, batch, planes, jobs, classes;            // n = s*s, jobs = classes + 1 (the last one is the fine job)
    int job_first[CS_MAX_JOBS], job_count[CS_MAX_JOBS];  // the job's planes
    uint8_t plane_sources[CS_MAX_PLANES];               // bit k: cluster map k is OR-ed into the plane's mask
    uint8_t plane_bit[CS_MAX_PLANES];                   // class bit of the lookup table the plane tests
    const int64_t* maps[CS_MAX_KEYS];                   // [batch][res][res]
    int res[CS_MAX_KEYS];
    const uint8_t* lut;                                 // [keys][256]: bit c = cluster belongs to non-background class c
    int only_overlapping, min_area2, max_extent;
    int paint_sources, paint_bit;                       // undilated mask of the label step
    uint8_t class_id[CS_MAX_JOBS];                      // [0] background, [1 + c] class c
    uint8_t colour[CS_MAX_JOBS][3];
};

struct Work {
    int *outside, *region;        // [batch*planes][n]; outside is later the group forest of a job, then the gap labels
    uint8_t* member;              // [batch*planes][n]
    int* gid;                     // [batch*jobs][n] root pixel + 1 of the group that covers the pixel
    uint8_t* covered;             // [batch*jobs][n]
    int *members, *area2, *gap_hi, *gap_lo;   // [batch*jobs][n], zeroed per call
    int* score;                   // [batch*classes][n]
    int* box;                     // [batch][4][n]: max of s-1-y, y, s-1-x, x
    int* flags;                   // [batch][2]: classes with a tall / a wide region
    int* has;                     // [batch*planes]
    uint8_t* assigned;            // [batch][n] 1 + class of the fine group rooted here
};

__device__ __forceinline__ bool mask_at(const Segment& g, int image, int sources, int bit, int y, int x) {
    int v = 0;
    for (int k = 0; k < CS_MAX_KEYS; ++k) {
        if (!((sources >> k) & 1)) continue;
        const int r = g.res[k];
        const int64_t id = g.maps[k][((int64_t)image * r + (y * r) / g.s) * r + (x * r) / g.s];
        if ((uint64_t)id < (uint64_t)CS_CLUSTERS) v |= g.lut[k * CS_CLUSTERS + (int)id];
    }
    return (v >> bit) & 1;
}

__device__ __forceinline__ bool job_present(const Segment& g, const Work& w, int image, int job) {
    bool all = true;
    for (int q = 0; q < g.job_count[job]; ++q) all = all && w.has[image * g.planes + g.job_first[job] + q] != 0;
    return all;
}

// the group of job `job` rooted at pixel `root` survives the merge step (and, for a text job, the area filter)
__device__ __forceinline__ bool group_kept(const Segment& g, const Work& w, int image, int job, int root) {
    if (!job_present(g, w, image, job)) return false;
    const int64_t at = ((int64_t)image * g.jobs + job) * g.n + root;
    const bool fine = job == g.classes;
    if (g.job_count[job] > 1 && (fine || g.only_overlapping) && w.members[at] < 2) return false;
    return fine || w.area2[at] >= g.min_area2;
}

// ---- D of every plane, one lane per pixel ---------------------------------------------------------------------------------
__global__ __launch_bounds__(CTHREADS) void cluster_mask_kernel(Segment g, Work w) {
    const int plane = blockIdx.y, image = plane / g.planes, p = plane % g.planes;
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    bool on = false;
    if (i < g.n) {
        const int y = i / g.s, x = i % g.s, src = g.plane_sources[p], bit = g.plane_bit[p];
        on = mask_at(g, image, src, bit, y, x) || (y > 0 && mask_at(g, image, src, bit, y - 1, x)) ||
             (y < g.s - 1 && mask_at(g, image, src, bit, y + 1, x)) || (x > 0 && mask_at(g, image, src, bit, y, x - 1)) ||
             (x < g.s - 1 && mask_at(g, image, src, bit, y, x + 1));
        w.member[(int64_t)plane * g.n + i] = on;
    }
    if (__syncthreads_or(on) && threadIdx.x == 0) atomicOr(&w.has[plane], 1);
}

// region labels -> roots; the plane's pass-1 array becomes its part of the job's forest: entry (q, i) is its own root
__global__ __launch_bounds__(CTHREADS) void cluster_compress_kernel(Segment g, Work w) {
    const int plane = blockIdx.y, p = plane % g.planes;
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    if (i >= g.n) return;
    int job = 0;
    while (job + 1 < g.jobs && g.job_first[job + 1] <= p) ++job;
    int* lab = w.region + (int64_t)plane * g.n;
    int budget = g.n + 1;
    const int mine = lab[i];
    if (mine != 0) lab[i] = find_global<false>(lab, mine, budget);
    w.outside[(int64_t)plane * g.n + i] = (p - g.job_first[job]) * g.n + i + 1;
}

// regions of different planes that cover the same pixel belong to one group
__global__ __launch_bounds__(CTHREADS) void cluster_union_kernel(Segment g, Work w) {
    const int image = blockIdx.y / g.jobs, job = blockIdx.y % g.jobs;
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    if (i >= g.n || g.job_count[job] < 2) return;
    const int64_t base = ((int64_t)image * g.planes + g.job_first[job]) * g.n;
    const int budget = 4 * g.job_count[job] * g.n + 64;
    int first = 0;
    for (int q = 0; q < g.job_count[job]; ++q) {
        const int r = w.region[base + (int64_t)q * g.n + i];
        if (r == 0) continue;
        if (first == 0) first = q * g.n + r;
        else union_global(w.outside + base, first, q * g.n + r, budget);
    }
}

// gid, the union's membership byte and the member count of every group
__global__ __launch_bounds__(CTHREADS) void cluster_group_kernel(Segment g, Work w) {
    const int image = blockIdx.y / g.jobs, job = blockIdx.y % g.jobs;
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    if (i >= g.n) return;
    const int64_t base = ((int64_t)image * g.planes + g.job_first[job]) * g.n, at = (int64_t)blockIdx.y * g.n;
    int group = 0;
    for (int q = 0; q < g.job_count[job]; ++q) {
        const int r = w.region[base + (int64_t)q * g.n + i];
        if (r == 0) continue;
        if (group == 0 || r == i + 1) {
            int budget = g.job_count[job] * g.n + 1;
            const int root = find_global<false>(w.outside + base, q * g.n + r, budget);
            group = (root - 1) % g.n + 1;
            if (r == i + 1) atomicAdd(&w.members[at + group - 1], 1);   // pixel i is the root of a region of plane q
        }
    }
    w.gid[at + i] = group;
    w.covered[at + i] = group != 0;
}

// gap labels -> roots, and the largest / smallest group a gap borders
__global__ __launch_bounds__(CTHREADS) void cluster_gap_border_kernel(Segment g, Work w) {
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    if (i >= g.n) return;
    const int64_t at = (int64_t)blockIdx.y * g.n;
    if (w.covered[at + i]) return;
    int* lab = w.outside + at;
    int budget = g.n + 1;
    const int root = find_global<false>(lab, lab[i], budget);
    lab[i] = root;
    if (root == 0) return;
    const int y = i / g.s, x = i % g.s;
    const int* gid = w.gid + at;
    const int nb[4] = {y > 0 ? gid[i - g.s] : 0, y < g.s - 1 ? gid[i + g.s] : 0, x > 0 ? gid[i - 1] : 0,
                       x < g.s - 1 ? gid[i + 1] : 0};
#pragma unroll
    for (int d = 0; d < 4; ++d)
        if (nb[d] != 0) {
            atomicMax(&w.gap_hi[at + root - 1], nb[d]);
            atomicMax(&w.gap_lo[at + root - 1], g.n + 1 - nb[d]);
        }
}

__global__ __launch_bounds__(CTHREADS) void cluster_gap_fill_kernel(Segment g, Work w) {
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    if (i >= g.n) return;
    const int64_t at = (int64_t)blockIdx.y * g.n;
    if (w.covered[at + i]) return;
    const int root = w.outside[at + i];
    if (root == 0) return;
    const int hi = w.gap_hi[at + root - 1];
    if (hi != 0 && hi == g.n + 1 - w.gap_lo[at + root - 1]) w.gid[at + i] = hi;
}

// One lane per 2x2 block of the zero-padded image; at most one group has three or four of its pixels.
__global__ __launch_bounds__(CTHREADS) void cluster_area_kernel(Segment g, Work w) {
    const int id = blockIdx.x * CTHREADS + threadIdx.x, side = g.s + 1;
    const int64_t at = (int64_t)blockIdx.y * g.n;
    int add = 0, group = 0;
    if (id < side * side) {
        const int by = id / side, bx = id % side;   // pixels (by-1 .. by, bx-1 .. bx)
        int v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = by - 1 + (k >> 1), x = bx - 1 + (k & 1);
            v[k] = (y >= 0 && y < g.s && x >= 0 && x < g.s) ? w.gid[at + y * g.s + x] : 0;
        }
        const int c0 = (v[1] == v[0]) + (v[2] == v[0]) + (v[3] == v[0]) + 1;
        const int c1 = (v[0] == v[1]) + (v[2] == v[1]) + (v[3] == v[1]) + 1;
        if (c0 >= 3) { group = v[0]; add = c0 == 4 ? 2 : 1; }
        else if (c1 >= 3) { group = v[1]; add = 1; }
    }
    if (group == 0) add = 0;
    wave_add_by_key(w.area2 + at, group - 1, add);
}

// score[f][c] and the bounding boxes of the fine groups
__global__ __launch_bounds__(CTHREADS) void cluster_score_kernel(Segment g, Work w) {
    const int image = blockIdx.y;
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    const int64_t fine = ((int64_t)image * g.jobs + g.classes) * g.n;
    int f = i < g.n ? w.gid[fine + i] : 0;
    if (f != 0 && !group_kept(g, w, image, g.classes, f - 1)) f = 0;
    for (int c = 0; c < g.classes; ++c) {
        int add = 0;
        if (f != 0) {
            const int t = w.gid[((int64_t)image * g.jobs + c) * g.n + i];
            add = t != 0 && group_kept(g, w, image, c, t - 1);
        }
        wave_add_by_key(w.score + ((int64_t)image * g.classes + c) * g.n, f - 1, add);
    }
    if (f == 0) return;
    const int y = i / g.s, x = i % g.s;
    const int* gid = w.gid + fine;
    int* box = w.box + (int64_t)image * 4 * g.n + f - 1;
    if (y == 0 || gid[i - g.s] != f) atomicMax(box, g.s - 1 - y);
    if (y == g.s - 1 || gid[i + g.s] != f) atomicMax(box + g.n, y);
    if (x == 0 || gid[i - 1] != f) atomicMax(box + 2 * g.n, g.s - 1 - x);
    if (x == g.s - 1 || gid[i + 1] != f) atomicMax(box + 3 * g.n, x);
}

__global__ __launch_bounds__(CTHREADS) void cluster_classify_kernel(Segment g, Work w) {
    const int image = blockIdx.y;
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    if (i >= g.n) return;
    const int64_t fine = ((int64_t)image * g.jobs + g.classes) * g.n;
    if (w.gid[fine + i] != i + 1) return;   // not the root of a fine group
    int best = 0, which = 0;
    if (group_kept(g, w, image, g.classes, i))
        for (int c = 0; c < g.classes; ++c) {
            const int v = w.score[((int64_t)image * g.classes + c) * g.n + i];
            if (v > best) { best = v; which = c + 1; }
        }
    if (w.area2[fine + i] < g.min_area2) which = 0;
    w.assigned[(int64_t)image * g.n + i] = which;
    if (which == 0) return;
    const int* box = w.box + (int64_t)image * 4 * g.n + i;
    const int height = box[g.n] - (g.s - 1 - box[0]) + 1, width = box[3 * g.n] - (g.s - 1 - box[2 * g.n]) + 1;
    if (height > g.max_extent) atomicOr(&w.flags[image * 2], 1 << (which - 1));
    if (width > g.max_extent) atomicOr(&w.flags[image * 2 + 1], 1 << (which - 1));
}

__global__ __launch_bounds__(CTHREADS) void cluster_paint_kernel(uint8_t* __restrict__ class_map, uint8_t* __restrict__ colour,
                                                                 uint8_t* __restrict__ drop, Segment g, Work w) {
    const int image = blockIdx.y;
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    if (i >= g.n) return;
    if (i == 0) drop[image] = (w.flags[image * 2] & w.flags[image * 2 + 1]) != 0;
    const int f = w.gid[((int64_t)image * g.jobs + g.classes) * g.n + i];
    int which = f != 0 ? w.assigned[(int64_t)image * g.n + f - 1] : 0;
    if (which != 0 && !mask_at(g, image, g.paint_sources, g.paint_bit, i / g.s, i % g.s)) which = 0;
    const int64_t at = (int64_t)image * g.n + i;
    class_map[at] = g.class_id[which];
    colour[at * 3] = g.colour[which][0];
    colour[at * 3 + 1] = g.colour[which][1];
    colour[at * 3 + 2] = g.colour[which][2];
}

constexpr int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }

// offsets of the workspace's arrays; returns its size
int64_t carve(Work* w, char* base, int64_t batch, int64_t n, int64_t planes, int64_t jobs, int64_t classes, int64_t* zero_from) {
    int64_t at = 0;
    auto take = [&](int64_t bytes) { const int64_t here = at; at += align16(bytes); return base + here; };
    int* outside = (int*)take(batch * planes * n * 4);
    int* region = (int*)take(batch * planes * n * 4);
    uint8_t* member = (uint8_t*)take(batch * planes * n);
    int* gid = (int*)take(batch * jobs * n * 4);
    uint8_t* covered = (uint8_t*)take(batch * jobs * n);
    uint8_t* assigned = (uint8_t*)take(batch * n);
    *zero_from = at;
    int* members = (int*)take(batch * jobs * n * 4);
    int* area2 = (int*)take(batch * jobs * n * 4);
    int* gap_hi = (int*)take(batch * jobs * n * 4);
    int* gap_lo = (int*)take(batch * jobs * n * 4);
    int* score = (int*)take(batch * classes * n * 4);
    int* box = (int*)take(batch * 4 * n * 4);
    int* flags = (int*)take(batch * 2 * 4);
    int* has = (int*)take(batch * planes * 4);
    if (w) *w = Work{outside, region, member, gid, covered, members, area2, gap_hi, gap_lo, score, box, flags, has, assigned};
    return at;
}

}  // namespace

extern "C" int64_t sis_cluster_segment_workspace_bytes(int batch, int size, int num_determination, int num_fine, int classes) {
    if (batch <= 0 || size <= 0 || num_determination <= 0 || num_fine <= 0 || classes <= 0) return 0;
    int64_t zero_from;
    return carve(nullptr, nullptr, batch, (int64_t)size * size, (int64_t)classes * num_determination + num_fine, classes + 1,
                 classes, &zero_from);
}

extern "C" int sis_cluster_segment(uint8_t* class_map, uint8_t* colour, uint8_t* drop, const int64_t* const* cluster_maps,
                                   const int* resolutions, int num_keys, const uint8_t* lut, const uint8_t* determination_sources,
                                   int num_determination, const uint8_t* fine_sources, int num_fine, int classes, int fine_class,
                                   const uint8_t* class_ids, const uint8_t* colours, int batch, int size,
                                   int only_keep_overlapping, int min_class_contour_area, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    SIS_REQUIRE(class_map && colour && drop && cluster_maps && resolutions && lut && determination_sources && fine_sources &&
                    class_ids && colours && workspace,
                "sis_cluster_segment: null pointer");
    SIS_REQUIRE(batch > 0 && size > 0, "sis_cluster_segment: non-positive size");
    SIS_REQUIRE(size <= CMAXP, "sis_cluster_segment: image size %d above %d", size, CMAXP);
    SIS_REQUIRE(num_keys >= 1 && num_keys <= CS_MAX_KEYS, "sis_cluster_segment: %d cluster maps, 1 to %d are supported", num_keys,
                CS_MAX_KEYS);
    SIS_REQUIRE(num_determination >= 1 && num_determination <= CS_MAX_KEYS && num_fine >= 1 && num_fine <= CS_MAX_KEYS,
                "sis_cluster_segment: 1 to %d keys per step are supported", CS_MAX_KEYS);
    SIS_REQUIRE(classes >= 1 && classes <= CS_MAX_CLASSES, "sis_cluster_segment: %d non-background classes, 1 to %d are supported",
                classes, CS_MAX_CLASSES);
    SIS_REQUIRE(fine_class >= 0 && fine_class < classes, "sis_cluster_segment: fine-grained class out of range");
    SIS_REQUIRE(min_class_contour_area >= 0 && min_class_contour_area <= (1 << 29),
                "sis_cluster_segment: min_class_contour_area out of range");
    Segment g{};
    g.s = size;
    g.n = size * size;
    g.batch = batch;
    g.classes = classes;
    g.jobs = classes + 1;
    g.planes = classes * num_determination + num_fine;
    SIS_REQUIRE((int64_t)batch * g.planes <= 65535, "sis_cluster_segment: more than 65535 planes");
    const int all_keys = (1 << num_keys) - 1;
    for (int k = 0; k < num_keys; ++k) {
        SIS_REQUIRE(cluster_maps[k], "sis_cluster_segment: null cluster map");
        SIS_REQUIRE(resolutions[k] >= 1 && resolutions[k] <= size, "sis_cluster_segment: cluster map of edge %d for image size %d",
                    resolutions[k], size);
        g.maps[k] = cluster_maps[k];
        g.res[k] = resolutions[k];
    }
    for (int k = num_keys; k < CS_MAX_KEYS; ++k) g.res[k] = 1;
    for (int job = 0; job < g.jobs; ++job) {
        const bool fine = job == classes;
        g.job_first[job] = job * num_determination;
        g.job_count[job] = fine ? num_fine : num_determination;
        for (int q = 0; q < g.job_count[job]; ++q) {
            const int src = fine ? fine_sources[q] : determination_sources[q];
            SIS_REQUIRE(src != 0 && (src & ~all_keys) == 0, "sis_cluster_segment: key sources 0x%x outside the %d cluster maps", src,
                        num_keys);
            g.plane_sources[g.job_first[job] + q] = (uint8_t)src;
            g.plane_bit[g.job_first[job] + q] = (uint8_t)(fine ? fine_class : job);
        }
    }
    g.lut = lut;
    g.only_overlapping = only_keep_overlapping != 0;
    g.min_area2 = 2 * min_class_contour_area;
    g.max_extent = (int)(size * 0.95);
    g.paint_sources = fine_sources[num_fine - 1];
    g.paint_bit = fine_class;
    for (int c = 0; c <= classes; ++c) {
        g.class_id[c] = class_ids[c];
        for (int k = 0; k < 3; ++k) g.colour[c][k] = colours[c * 3 + k];
    }
    SIS_REQUIRE(((uintptr_t)workspace & 15) == 0, "sis_cluster_segment: workspace not 16-byte aligned");
    Work w;
    int64_t zero_from;
    const int64_t need = carve(&w, (char*)workspace, batch, g.n, g.planes, g.jobs, classes, &zero_from);
    SIS_REQUIRE(workspace_bytes >= need, "sis_cluster_segment: workspace too small");

    hipStream_t st = (hipStream_t)stream;
    const int all_planes = batch * g.planes, all_jobs = batch * g.jobs, lines = (size - 1) / CT;
    const dim3 threads(CTHREADS);
    const int blocks = sis_cdiv(g.n, CTHREADS);
    const dim3 plane_tiles(sis_cdiv(size, CT), sis_cdiv(size, CT), all_planes), job_tiles(plane_tiles.x, plane_tiles.y, all_jobs);
    const int border_blocks = sis_cdiv((int64_t)2 * lines * size, CTHREADS);
    const Plane all{size, size, g.n, 1, -1, 0u};   // no plane is skipped

    if (hipMemsetAsync((char*)workspace + zero_from, 0, need - zero_from, st) != hipSuccess)
        return sis_fail("sis_cluster_segment: clearing the accumulators failed");
    hipLaunchKernelGGL(cluster_mask_kernel, dim3(blocks, all_planes), threads, 0, st, g, w);
    SIS_CHECK_LAUNCH("cluster_mask_kernel");
    hipLaunchKernelGGL(contour_label_tile_kernel<false>, plane_tiles, threads, 0, st, w.outside, w.member, (const int*)nullptr, all);
    SIS_CHECK_LAUNCH("contour_label_tile_kernel<outside>");
    if (lines > 0) {
        hipLaunchKernelGGL(contour_merge_borders_kernel<false>, dim3(border_blocks, all_planes), threads, 0, st, w.outside,
                           w.member, all);
        SIS_CHECK_LAUNCH("contour_merge_borders_kernel<outside>");
    }
    hipLaunchKernelGGL(contour_label_tile_kernel<true>, plane_tiles, threads, 0, st, w.region, w.member, (const int*)w.outside, all);
    SIS_CHECK_LAUNCH("contour_label_tile_kernel<region>");
    if (lines > 0) {
        hipLaunchKernelGGL(contour_merge_borders_kernel<true>, dim3(border_blocks, all_planes), threads, 0, st, w.region, w.member,
                           all);
        SIS_CHECK_LAUNCH("contour_merge_borders_kernel<region>");
    }
    hipLaunchKernelGGL(cluster_compress_kernel, dim3(blocks, all_planes), threads, 0, st, g, w);
    SIS_CHECK_LAUNCH("cluster_compress_kernel");
    hipLaunchKernelGGL(cluster_union_kernel, dim3(blocks, all_jobs), threads, 0, st, g, w);
    SIS_CHECK_LAUNCH("cluster_union_kernel");
    hipLaunchKernelGGL(cluster_group_kernel, dim3(blocks, all_jobs), threads, 0, st, g, w);
    SIS_CHECK_LAUNCH("cluster_group_kernel");
    // gaps: the 4-connected background of the union, one plane per job, labelled into the array the forests lived in
    hipLaunchKernelGGL(contour_label_tile_kernel<false>, job_tiles, threads, 0, st, w.outside, w.covered, (const int*)nullptr, all);
    SIS_CHECK_LAUNCH("contour_label_tile_kernel<gaps>");
    if (lines > 0) {
        hipLaunchKernelGGL(contour_merge_borders_kernel<false>, dim3(border_blocks, all_jobs), threads, 0, st, w.outside, w.covered,
                           all);
        SIS_CHECK_LAUNCH("contour_merge_borders_kernel<gaps>");
    }
    hipLaunchKernelGGL(cluster_gap_border_kernel, dim3(blocks, all_jobs), threads, 0, st, g, w);
    SIS_CHECK_LAUNCH("cluster_gap_border_kernel");
    hipLaunchKernelGGL(cluster_gap_fill_kernel, dim3(blocks, all_jobs), threads, 0, st, g, w);
    SIS_CHECK_LAUNCH("cluster_gap_fill_kernel");
    hipLaunchKernelGGL(cluster_area_kernel, dim3(sis_cdiv((int64_t)(size + 1) * (size + 1), CTHREADS), all_jobs), threads, 0, st, g,
                       w);
    SIS_CHECK_LAUNCH("cluster_area_kernel");
    hipLaunchKernelGGL(cluster_score_kernel, dim3(blocks, batch), threads, 0, st, g, w);
    SIS_CHECK_LAUNCH("cluster_score_kernel");
    hipLaunchKernelGGL(cluster_classify_kernel, dim3(blocks, batch), threads, 0, st, g, w);
    SIS_CHECK_LAUNCH("cluster_classify_kernel");
    hipLaunchKernelGGL(cluster_paint_kernel, dim3(blocks, batch), threads, 0, st, class_map, colour, drop, g, w);
    SIS_CHECK_LAUNCH("cluster_paint_kernel");
    return 0;
}
