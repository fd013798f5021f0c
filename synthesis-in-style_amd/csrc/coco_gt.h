// Dataset ground truth on the device (reference segmentation/evaluation/coco_gt.py:38-92 and
// create_dataset_for_segmentation.py:151-206): per class plane of a label image, the outermost contours with their holes
// filled (contour_cc.h), one table row per region (root, tight box, area, where its run lengths
// lie) and COCO's uncompressed column-major run lengths of every region that is not a straight stroke.  DESIGN.md §16 states
// the contract.  Included at the end of contour_ops.hip, which has the labelling kernels in scope.
// Every value is an integer and every accumulation a min, a max or a sum of integers: the bytes do not depend on timing.
// The launch sequence is fixed (ten launches, nine without run lengths), nothing is read back.  Workgroups of one launch
// meet only through device-scope atomics on the table rows, which no kernel reads with a plain load before the launch ends.
#pragma once
#include <limits.h>

namespace {

constexpr int GT_MAX_CLASSES = 8;
constexpr int GT_SCAN_THREADS = 1024;
constexpr int GT_EMIT_BLOCKS = 16;   // per plane, four waves each: a wave takes the slots w, w + 64, ...
// workspace row of a region
enum { GT_ROOT, GT_MINX, GT_MAXX, GT_MINY, GT_MAXY, GT_MIND, GT_MAXD, GT_MINS, GT_MAXS, GT_AREA, GT_TRANS, GT_OFFSET, GT_ROW };

struct GtColours {
    uint8_t rgb[GT_MAX_CLASSES][3];
};

// An aligned 2x2 block holds pixels of one region at most (they are 8-neighbours of each other).
inline int gt_region_capacity(int p) { return ((p + 1) / 2) * ((p + 1) / 2); }

// M[b][k] = (label[b] == colours[k]) on all three bytes
__global__ __launch_bounds__(CTHREADS) void gt_mask_kernel(uint8_t* __restrict__ mask, const uint8_t* __restrict__ label, GtColours c,
                                                           int classes, int n) {
    const int b = blockIdx.y, i = blockIdx.x * CTHREADS + threadIdx.x;
    if (i >= n) return;
    const uint8_t* px = label + ((int64_t)b * n + i) * 3;
    const uint8_t r = px[0], g = px[1], bl = px[2];
    for (int k = 0; k < classes; ++k)
        mask[((int64_t)b * classes + k) * n + i] = r == c.rgb[k][0] && g == c.rgb[k][1] && bl == c.rgb[k][2];
}

// Exclusive scan of one value per thread over the block (a multiple of 64 threads, 1024 at most); `total` is the block's sum.
__device__ __forceinline__ int gt_block_scan(int v, int* wave_sums, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    __syncthreads();   // the previous round's sums have been read
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    int base = 0;
    total = 0;
    for (int w = 0; w < waves; ++w) {
        const int s = wave_sums[w];
        base += w < wave ? s : 0;
        total += s;
    }
    return base + incl - v;
}

// One workgroup per plane.  A root is the pixel whose label names itself; its slot is the number of roots before it in raster
// order.  slot_of (the pass-1 label array, dead by now) keeps the slot at the root's pixel; the root's lane clears the row.
__global__ __launch_bounds__(GT_SCAN_THREADS) void gt_rank_kernel(int* __restrict__ slot_of, int* __restrict__ table,
                                                                  int* __restrict__ region_count, const int* __restrict__ labels,
                                                                  Plane g, int cap) {
    const int plane = blockIdx.x;
    const int* lab = labels + (int64_t)plane * g.n;
    int* slots = slot_of + (int64_t)plane * g.n;
    int* rows = table + (int64_t)plane * cap * GT_ROW;
    __shared__ int sums[GT_SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = GT_SCAN_THREADS / 64;
    const int segment = ((g.n + waves - 1) / waves + 63) / 64 * 64;   // a wave walks one contiguous segment, 64 pixels a step
    const int seg0 = min(wave * segment, g.n), seg1 = min(seg0 + segment, g.n);
    int count = 0;
    for (int i0 = seg0; i0 < seg1; i0 += 64) {
        const int i = i0 + lane;
        count += __popcll(__ballot(i < seg1 && lab[i] == i + 1));
    }
    if (lane == 0) sums[wave] = count;
    __syncthreads();
    int running = 0, total = 0;
    for (int w = 0; w < waves; ++w) {
        running += w < wave ? sums[w] : 0;
        total += sums[w];
    }
    for (int i0 = seg0; i0 < seg1; i0 += 64) {
        const int i = i0 + lane;
        const bool root = i < seg1 && lab[i] == i + 1;
        const unsigned long long roots = __ballot(root);
        if (root) {
            const int s = running + __popcll(roots & ((1ull << lane) - 1ull));
            slots[i] = s;
            if (s < cap) {
                int* row = rows + (int64_t)s * GT_ROW;
                row[GT_ROOT] = i;
                row[GT_MINX] = INT_MAX, row[GT_MAXX] = INT_MIN, row[GT_MINY] = INT_MAX, row[GT_MAXY] = INT_MIN;
                row[GT_MIND] = INT_MAX, row[GT_MAXD] = INT_MIN, row[GT_MINS] = INT_MAX, row[GT_MAXS] = INT_MIN;
                row[GT_AREA] = 0, row[GT_TRANS] = 0, row[GT_OFFSET] = 0;
            }
        }
        running += __popcll(roots);
    }
    if (threadIdx.x == 0) region_count[plane] = total;
}

__device__ __forceinline__ int gt_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ int gt_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ int gt_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// An extent only ever moves one way, so a value read past the L1 (possibly already overtaken) that mine does not beat makes
// the atomic needless; what is stored never depends on that read.
__device__ __forceinline__ void gt_lower(int* at, int v) {
    if (v < __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(at, v);
}

__device__ __forceinline__ void gt_raise(int* at, int v) {
    if (v > __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(at, v);
}

// One lane per pixel.  Lanes of a wave in the same region combine their extents, area and transition count first (as
// wave_add_by_key does), then one lane applies them to the row.  A transition is a position of the column-major order whose
// indicator differs from its predecessor's; the predecessor of (x, 0) is (x - 1, p - 1), that of (0, 0) is "not in a region".
// Where the labels of a position and its predecessor differ, the position's region gains a transition and so does the
// predecessor's.
__global__ __launch_bounds__(CTHREADS) void gt_stats_kernel(int* __restrict__ table, const int* __restrict__ labels,
                                                            const int* __restrict__ slot_of, Plane g, int cap) {
    const int plane = blockIdx.y;
    const int* lab = labels + (int64_t)plane * g.n;
    const int* slots = slot_of + (int64_t)plane * g.n;
    int* rows = table + (int64_t)plane * cap * GT_ROW;
    const int i = blockIdx.x * CTHREADS + threadIdx.x, lane = threadIdx.x & 63;
    const bool valid = i < g.n;
    const int y = valid ? i / g.w : 0, x = valid ? i % g.w : 0;
    const int before = y > 0 ? i - g.w : (x > 0 ? (g.h - 1) * g.w + x - 1 : -1);
    const int mine = valid ? lab[i] : 0, pred = valid && before >= 0 ? lab[before] : 0;
    const int change = mine != pred;
    int slot = mine != 0 ? slots[mine - 1] : 0, pred_slot = pred != 0 ? slots[pred - 1] : 0;
    const bool own = mine != 0 && slot < cap;
    unsigned long long pending = __ballot(own);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int which = __shfl(mine, leader);
        const bool same = own && mine == which;
        const int min_x = gt_wave_min(same ? x : INT_MAX), max_x = gt_wave_max(same ? x : INT_MIN);
        const int min_y = gt_wave_min(same ? y : INT_MAX), max_y = gt_wave_max(same ? y : INT_MIN);
        const int min_d = gt_wave_min(same ? x - y : INT_MAX), max_d = gt_wave_max(same ? x - y : INT_MIN);
        const int min_s = gt_wave_min(same ? x + y : INT_MAX), max_s = gt_wave_max(same ? x + y : INT_MIN);
        const int area = gt_wave_sum(same ? 1 : 0), trans = gt_wave_sum(same ? change : 0);
        if (lane == leader) {
            int* row = rows + (int64_t)slot * GT_ROW;
            gt_lower(&row[GT_MINX], min_x), gt_raise(&row[GT_MAXX], max_x);
            gt_lower(&row[GT_MINY], min_y), gt_raise(&row[GT_MAXY], max_y);
            gt_lower(&row[GT_MIND], min_d), gt_raise(&row[GT_MAXD], max_d);
            gt_lower(&row[GT_MINS], min_s), gt_raise(&row[GT_MAXS], max_s);
            atomicAdd(&row[GT_AREA], area);
            if (trans) atomicAdd(&row[GT_TRANS], trans);
        }
        pending &= ~__ballot(same);
    }
    const bool left = pred != 0 && pred_slot < cap && change;
    wave_add_by_key(rows, left ? pred_slot * GT_ROW + GT_TRANS : 0, left ? 1 : 0);
}

// One workgroup per plane: degenerate regions (all pixels on one line of the eight-neighbour grid) get no runs, the others
// transitions + 1 counts; run_offset is the exclusive sum over the rows before.  Rows below max_regions go to the caller.
__global__ __launch_bounds__(CTHREADS) void gt_finish_kernel(uint8_t* __restrict__ has, int* __restrict__ run_total,
                                                             int* __restrict__ regions, int* __restrict__ table,
                                                             const int* __restrict__ region_count, int cap, int max_regions) {
    const int plane = blockIdx.x;
    int* rows = table + (int64_t)plane * cap * GT_ROW;
    __shared__ int sums[CTHREADS / 64];
    const int count = min(region_count[plane], cap);
    int running = 0, any = 0;
    for (int s0 = 0; s0 < count; s0 += CTHREADS) {
        const int s = s0 + threadIdx.x;
        int* row = rows + (int64_t)s * GT_ROW;
        int runs = 0;
        if (s < count) {
            const bool degenerate = row[GT_MINX] == row[GT_MAXX] || row[GT_MINY] == row[GT_MAXY] || row[GT_MIND] == row[GT_MAXD] ||
                                    row[GT_MINS] == row[GT_MAXS];
            runs = degenerate ? 0 : row[GT_TRANS] + 1;
        }
        int total;
        const int offset = running + gt_block_scan(runs, sums, total);
        if (s < count) {
            row[GT_TRANS] = runs;     // from here on the row holds run_count and run_offset
            row[GT_OFFSET] = offset;
            any |= runs > 0;
            if (regions != nullptr && s < max_regions) {
                int* out = regions + ((int64_t)plane * max_regions + s) * 8;
                out[0] = row[GT_ROOT], out[1] = row[GT_MINX], out[2] = row[GT_MINY];
                out[3] = row[GT_MAXX] - row[GT_MINX] + 1, out[4] = row[GT_MAXY] - row[GT_MINY] + 1;
                out[5] = row[GT_AREA], out[6] = offset, out[7] = runs;
            }
        }
        running += total;
    }
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) {
        has[plane] = any ? 1 : 0;
        run_total[plane] = running;
    }
}

// One wave per table slot, the region's box column by column, 64 rows at a time (one row below the box included, so that a
// run that ends inside a column closes there).  A ballot of label == root gives the transitions of a chunk, a prefix popcount
// their places; the previous transition's position and the state bit are carried across chunks and columns.  A count is the
// difference of two transition positions, the last count is p*p - the last position.
__global__ __launch_bounds__(CTHREADS) void gt_emit_kernel(int* __restrict__ runs, const int* __restrict__ table,
                                                           const int* __restrict__ region_count, const int* __restrict__ labels,
                                                           Plane g, int cap, int max_runs) {
    const int plane = blockIdx.y, lane = threadIdx.x & 63;
    const int* lab = labels + (int64_t)plane * g.n;
    const int* rows = table + (int64_t)plane * cap * GT_ROW;
    int* out = runs + (int64_t)plane * max_runs;
    const int count = min(region_count[plane], cap);
    const unsigned long long below_me = (1ull << lane) - 1ull;
    for (int s = blockIdx.x * (CTHREADS / 64) + (threadIdx.x >> 6); s < count; s += gridDim.x * (CTHREADS / 64)) {
        const int* row = rows + (int64_t)s * GT_ROW;
        const int offset = row[GT_OFFSET];
        if (row[GT_TRANS] == 0 || offset >= max_runs) continue;   // wave-uniform
        const int root = row[GT_ROOT] + 1, x0 = row[GT_MINX], x1 = row[GT_MAXX], y0 = row[GT_MINY], y1 = row[GT_MAXY];
        const int y_end = min(y1 + 1, g.h - 1);
        int k = 0, last = 0;
        unsigned long long state = 0;   // the indicator at the position before
        for (int x = x0; x <= x1; ++x) {
            for (int yc = y0; yc <= y_end; yc += 64) {
                const int y = yc + lane, rows_here = min(64, y_end - yc + 1);
                const unsigned long long in = __ballot(y <= y_end && lab[y * g.w + x] == root);
                const unsigned long long span = rows_here == 64 ? ~0ull : (1ull << rows_here) - 1ull;
                const unsigned long long turns = (in ^ ((in << 1) | state)) & span;
                if ((turns >> lane) & 1ull) {
                    const unsigned long long below = turns & below_me;
                    const int at = k + __popcll(below);
                    const int before = below ? x * g.h + yc + 63 - __clzll((long long)below) : last;
                    if (offset + at < max_runs) out[offset + at] = x * g.h + y - before;
                }
                if (turns) {
                    last = x * g.h + yc + 63 - __clzll((long long)turns);
                    k += __popcll(turns);
                }
                state = (in >> (rows_here - 1)) & 1ull;
            }
            // the column ended inside the region (its last row is the plane's): the next position is the top of column x + 1,
            // which is the region's only where the box starts at row 0 and has that column
            if (state && x + 1 < g.w && !(y0 == 0 && x < x1)) {
                if (lane == 0 && offset + k < max_runs) out[offset + k] = (x + 1) * g.h - last;
                last = (x + 1) * g.h;
                ++k;
                state = 0;
            }
        }
        if (lane == 0 && offset + k < max_runs) out[offset + k] = g.n - last;
    }
}

}  // namespace

extern "C" int64_t sis_label_regions_workspace_bytes(int batch, int classes, int p) {
    if (batch <= 0 || classes <= 0 || p <= 0 || p > CMAXP) return 0;
    const int64_t planes = (int64_t)batch * classes, n = (int64_t)p * p;
    return planes * (n * 9 + (int64_t)gt_region_capacity(p) * GT_ROW * 4);   // two label arrays, the table, the byte mask
}

extern "C" int sis_label_regions(uint8_t* has, int32_t* region_count, int32_t* regions, int32_t* run_total, int32_t* runs,
                                 const uint8_t* label, const uint8_t* colours, int classes, int batch, int p, int max_regions,
                                 int max_runs, void* workspace, int64_t workspace_bytes, void* stream) {
    SIS_REQUIRE(has && region_count && run_total && label && colours && workspace, "sis_label_regions: null pointer");
    SIS_REQUIRE(batch > 0 && p > 0, "sis_label_regions: non-positive size");
    SIS_REQUIRE(classes >= 1 && classes <= GT_MAX_CLASSES, "sis_label_regions: classes %d outside 1..%d", classes, GT_MAX_CLASSES);
    SIS_REQUIRE(p <= CMAXP, "sis_label_regions: plane edge %d above %d", p, CMAXP);
    SIS_REQUIRE((int64_t)batch * classes <= 65535, "sis_label_regions: more than 65535 planes");
    SIS_REQUIRE(regions == nullptr || max_regions >= 0, "sis_label_regions: negative max_regions");
    SIS_REQUIRE(runs == nullptr || max_runs >= 0, "sis_label_regions: negative max_runs");
    SIS_REQUIRE(workspace_bytes >= sis_label_regions_workspace_bytes(batch, classes, p), "sis_label_regions: workspace too small");
    SIS_REQUIRE(((uintptr_t)workspace & 3) == 0, "sis_label_regions: workspace not 4-byte aligned");
    const int planes = batch * classes, cap = gt_region_capacity(p);
    const Plane g{p, p, p * p, classes, -1, 0u};   // no plane is skipped
    const int64_t total = (int64_t)planes * g.n;
    int* outside = (int*)workspace;            // pass-1 labels, later the slot of every root
    int* region = outside + total;             // pass-2 labels
    int* table = region + total;
    uint8_t* mask = (uint8_t*)(table + (int64_t)planes * cap * GT_ROW);
    GtColours c;
    for (int k = 0; k < GT_MAX_CLASSES; ++k)
        for (int j = 0; j < 3; ++j) c.rgb[k][j] = k < classes ? colours[3 * k + j] : 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 tiles(sis_cdiv(p, CT), sis_cdiv(p, CT), planes), threads(CTHREADS);
    const dim3 pixels(sis_cdiv(g.n, CTHREADS), planes);
    const int lines = (p - 1) / CT;
    const dim3 borders(sis_cdiv((int64_t)2 * lines * p, CTHREADS), planes);

    hipLaunchKernelGGL(gt_mask_kernel, dim3(sis_cdiv(g.n, CTHREADS), batch), threads, 0, st, mask, label, c, classes, g.n);
    SIS_CHECK_LAUNCH("gt_mask_kernel");
    hipLaunchKernelGGL(contour_label_tile_kernel<false>, tiles, threads, 0, st, outside, mask, (const int*)nullptr, g);
    SIS_CHECK_LAUNCH("contour_label_tile_kernel<outside>");
    if (lines > 0) {
        hipLaunchKernelGGL(contour_merge_borders_kernel<false>, borders, threads, 0, st, outside, mask, g);
        SIS_CHECK_LAUNCH("contour_merge_borders_kernel<outside>");
    }
    hipLaunchKernelGGL(contour_label_tile_kernel<true>, tiles, threads, 0, st, region, mask, (const int*)outside, g);
    SIS_CHECK_LAUNCH("contour_label_tile_kernel<region>");
    if (lines > 0) {
        hipLaunchKernelGGL(contour_merge_borders_kernel<true>, borders, threads, 0, st, region, mask, g);
        SIS_CHECK_LAUNCH("contour_merge_borders_kernel<region>");
    }
    hipLaunchKernelGGL(contour_compress_kernel<false>, pixels, threads, 0, st, region, (int*)nullptr, g);
    SIS_CHECK_LAUNCH("contour_compress_kernel");
    hipLaunchKernelGGL(gt_rank_kernel, dim3(planes), dim3(GT_SCAN_THREADS), 0, st, outside, table, region_count, region, g, cap);
    SIS_CHECK_LAUNCH("gt_rank_kernel");
    hipLaunchKernelGGL(gt_stats_kernel, pixels, threads, 0, st, table, region, outside, g, cap);
    SIS_CHECK_LAUNCH("gt_stats_kernel");
    hipLaunchKernelGGL(gt_finish_kernel, dim3(planes), threads, 0, st, has, run_total, regions, table, region_count, cap, max_regions);
    SIS_CHECK_LAUNCH("gt_finish_kernel");
    if (runs != nullptr) {
        hipLaunchKernelGGL(gt_emit_kernel, dim3(GT_EMIT_BLOCKS, planes), threads, 0, st, runs, table, region_count, region, g, cap,
                           max_runs);
        SIS_CHECK_LAUNCH("gt_emit_kernel");
    }
    return 0;
}
