// Scanner-margin removal of the scan-patch tool (scripts/create_stylegan_train_dataset.py:49-111 of the reference,
// get_content_box with edge_detect=True: there OpenCV's blur, Canny, dilate, erode and findContours on one host thread).
// DESIGN.md §20 states the arithmetic, tests/scan_margin_restatement.py restates it; the statement follows OpenCV's DOCUMENTED
// behaviour and nothing here was compared with OpenCV.  Included at the end of contour_ops.hip, which has the labelling kernels
// (contour_cc.h) and the wave helpers of coco_gt.h in scope.
//
// The analysis image is uint8 [h][w][3] in device memory, 3 <= h, w <= 4096.  Every value is an integer (one double product
// in the decision, a single correctly rounded operation), every accumulation a min, a max, an OR or a sum of integers: the
// bytes do not depend on timing.  The launch sequence depends on (h, w) and on whether `contours` is asked for, nothing is
// read back, all launches go to the caller's stream:
//   margin_clear_kernel            the area bitmap and the counters
//   margin_front_kernel            blur, Sobel, channel choice, non-maximum suppression over an LDS tile with a 3-pixel apron:
//                                  a seed label per candidate and a byte per strong pixel
//   contour_label_tile_kernel<1>, contour_merge_borders_kernel<1>, contour_compress_kernel<1>
//                                  8-connected components of the candidates; the compression clears the flag array
//   margin_flag_kernel             flag[root] = 1 where the component holds a strong pixel
//   margin_close_kernel            edges = flagged candidates, then the cross dilation and erosion over an LDS tile: E
//   contour_label_tile_kernel<0>, contour_merge_borders_kernel<0>      the holes of E (background off the frame)
//   contour_label_tile_kernel<1>, contour_merge_borders_kernel<1>      the 8-connected components of E
//   margin_roots_kernel            both label arrays compressed; a root clears its box and is counted
//   margin_boxes_kernel            tight boxes by atomicMin / atomicMax per root, combined within a wave first
//   margin_areas_kernel            a bit per box area, the largest area
//   margin_decide_kernel           one workgroup: the decision and the threshold T from the largest gap of the bitmap
//   margin_keep_kernel             the union of the kept boxes
//   margin_finish_kernel           box and info
//   margin_table_kernel            (only with `contours`) one workgroup ranks the roots in raster order and writes the rows
#pragma once

namespace {

constexpr int MG_MIN_SIDE = 3;
constexpr int MG_MAX_SIDE = 4096;
constexpr int MG_MAX_AREA = MG_MAX_SIDE * MG_MAX_SIDE;          // of a box: 2^24
constexpr int MG_BITMAP_WORDS = MG_MAX_AREA / 32 + 64;          // bit a = "some box has area a", a <= 2^24
constexpr int MG_STATS_WORDS = 64;
constexpr int MG_RT = CT + 6, MG_BT = CT + 4, MG_MT = CT + 2;   // raw, blurred and magnitude tiles
constexpr int MG_DECIDE_THREADS = 1024;
// counters in the workspace
enum { MG_OUTERS, MG_HOLES, MG_LARGEST, MG_KEPT, MG_DECISION, MG_T, MG_EDGE_PIXELS, MG_FIRST_ROOT, MG_FIRST_ONLY, MG_X0, MG_Y0, MG_X1, MG_Y1 };

struct MarginWorkspace {
    int* stats;      // [MG_STATS_WORDS]
    unsigned* bitmap;   // [MG_BITMAP_WORDS]
    int* a;          // candidate seeds, then the strong flag per root, then the hole labels
    int* b;          // candidate labels, then the labels of E's components
    int* c;          // seeds of E, then box min x
    int* box_x1;
    int* box_y0;
    int* box_y1;
    uint8_t* strong;
    uint8_t* act;    // the membership byte that the labelling kernels write
    uint8_t* mask;   // E
};

inline int64_t margin_workspace_bytes(int h, int w) {
    const int64_t n = (int64_t)h * w;
    return (((int64_t)MG_STATS_WORDS + MG_BITMAP_WORDS + 6 * n) * 4 + 3 * n + 3) & ~(int64_t)3;
}

inline MarginWorkspace margin_carve(void* workspace, int h, int w) {
    const int64_t n = (int64_t)h * w;
    MarginWorkspace m;
    m.stats = (int*)workspace;
    m.bitmap = (unsigned*)(m.stats + MG_STATS_WORDS);
    m.a = (int*)(m.bitmap + MG_BITMAP_WORDS);
    m.b = m.a + n;
    m.c = m.b + n;
    m.box_x1 = m.c + n;
    m.box_y0 = m.box_x1 + n;
    m.box_y1 = m.box_y0 + n;
    m.strong = (uint8_t*)(m.box_y1 + n);
    m.act = m.strong + n;
    m.mask = m.act + n;
    return m;
}

__global__ __launch_bounds__(CTHREADS) void margin_clear_kernel(int* __restrict__ stats, unsigned* __restrict__ bitmap) {
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    if (i < MG_BITMAP_WORDS) bitmap[i] = 0u;
    if (i < MG_STATS_WORDS)
        stats[i] = (i == MG_FIRST_ROOT || i == MG_X0 || i == MG_Y0) ? INT_MAX : (i == MG_X1 || i == MG_Y1) ? INT_MIN : 0;
}

// cv2.blur's border: the mirror that does not repeat the edge pixel; clamped, so that no index leaves 0..n-1 for any v
__device__ __forceinline__ int margin_mirror(int v, int n) {
    const int r = v < 0 ? -v : (v >= n ? 2 * n - 2 - v : v);
    return min(max(r, 0), n - 1);
}

// Sobel of the blurred tile at (ly, lx) of the MG_BT grid: the channel with the largest |dx| + |dy|, the lowest on a tie
__device__ __forceinline__ void margin_gradient(const uint8_t (*bt)[MG_BT][3], int ly, int lx, int& dx, int& dy, int& m) {
    m = -1;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int a = bt[ly - 1][lx - 1][ch], b = bt[ly - 1][lx][ch], c = bt[ly - 1][lx + 1][ch];
        const int d = bt[ly][lx - 1][ch], f = bt[ly][lx + 1][ch];
        const int g = bt[ly + 1][lx - 1][ch], h = bt[ly + 1][lx][ch], i = bt[ly + 1][lx + 1][ch];
        const int gx = (c + 2 * f + i) - (a + 2 * d + g);
        const int gy = (g + 2 * h + i) - (a + 2 * b + c);
        const int mag = abs(gx) + abs(gy);
        if (mag > m) { m = mag; dx = gx; dy = gy; }
    }
}

// Steps 1 to 3 of §20 and the two thresholds.  seed[i] = i + 1 for a candidate and 0 elsewhere (what the labelling kernel
// reads as "root is not 0"), strong[i] = 1 for a candidate above `high`.
__global__ __launch_bounds__(CTHREADS) void margin_front_kernel(int* __restrict__ seed, uint8_t* __restrict__ strong,
                                                                 const uint8_t* __restrict__ page, int h, int w, int low, int high) {
    __shared__ uint8_t raw[MG_RT][MG_RT][3];    // raw[ly][lx] = page[mirror(y0 - 3 + ly)][mirror(x0 - 3 + lx)]
    __shared__ uint8_t bt[MG_BT][MG_BT][3];     // the blurred image at (y0 - 2 + ly, x0 - 2 + lx) CLAMPED into the image
    __shared__ int16_t mt[MG_MT][MG_MT];        // the magnitude at (y0 - 1 + ly, x0 - 1 + lx), 0 outside the image
    const int y0 = blockIdx.y * CT, x0 = blockIdx.x * CT;
    for (int k = threadIdx.x; k < MG_RT * MG_RT; k += CTHREADS) {
        const int ly = k / MG_RT, lx = k % MG_RT;
        const uint8_t* p = page + ((int64_t)margin_mirror(y0 - 3 + ly, h) * w + margin_mirror(x0 - 3 + lx, w)) * 3;
        raw[ly][lx][0] = p[0], raw[ly][lx][1] = p[1], raw[ly][lx][2] = p[2];
    }
    __syncthreads();
    for (int k = threadIdx.x; k < MG_BT * MG_BT; k += CTHREADS) {
        const int ly = k / MG_BT, lx = k % MG_BT;
        // the clamped pixel lies inside the tile's reach: its raw neighbourhood is rows ry - 1 .. ry + 1 of `raw`
        const int ry = min(max(y0 - 2 + ly, 0), h - 1) - (y0 - 3), rx = min(max(x0 - 2 + lx, 0), w - 1) - (x0 - 3);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            int s = 0;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) s += raw[ry + dy][rx + dx][ch];
            bt[ly][lx][ch] = (uint8_t)((s + 4) / 9);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < MG_MT * MG_MT; k += CTHREADS) {
        const int ly = k / MG_MT, lx = k % MG_MT;
        const int y = y0 - 1 + ly, x = x0 - 1 + lx;
        int dx = 0, dy = 0, m = 0;
        if (y >= 0 && y < h && x >= 0 && x < w) margin_gradient(bt, ly + 1, lx + 1, dx, dy, m);
        mt[ly][lx] = (int16_t)m;    // at most 2040
    }
    __syncthreads();
    for (int k = threadIdx.x; k < CT2; k += CTHREADS) {
        const int ly = k / CT, lx = k % CT;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= h || x >= w) continue;
        int dx = 0, dy = 0, m = 0;
        margin_gradient(bt, ly + 2, lx + 2, dx, dy, m);
        const int my = ly + 1, mx = lx + 1;
        const int ax = abs(dx), ay = abs(dy) << 15;          // <= 1020 and 1020 * 2^15: all of this fits 32 bits
        const int t22 = ax * 13573, t67 = t22 + (ax << 16);
        bool peak;
        if (ay < t22) {
            peak = m > mt[my][mx - 1] && m >= mt[my][mx + 1];
        } else if (ay > t67) {
            peak = m > mt[my - 1][mx] && m >= mt[my + 1][mx];
        } else {
            const int s = ((dx ^ dy) < 0) ? -1 : 1;
            peak = m > mt[my - 1][mx - s] && m > mt[my + 1][mx + s];
        }
        const bool candidate = peak && m > low;
        const int i = y * w + x;
        seed[i] = candidate ? i + 1 : 0;
        strong[i] = candidate && m > high;
    }
}

// labels hold roots (compressed); a plain store of the same 1 from every strong pixel of a component
__global__ __launch_bounds__(CTHREADS) void margin_flag_kernel(int* __restrict__ flag, const int* __restrict__ labels,
                                                                const uint8_t* __restrict__ strong, int n) {
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    if (i >= n) return;
    const int lab = labels[i];
    if (lab != 0 && strong[i]) flag[lab - 1] = 1;
}

// Steps 4 (the select) and 5: mask = E as 0 / 1, edges = E as 0 / 255 (or NULL), seed[i] = i + 1 on E and 0 elsewhere.
__global__ __launch_bounds__(CTHREADS) void margin_close_kernel(uint8_t* __restrict__ mask, uint8_t* __restrict__ edges,
                                                                 int* __restrict__ seed, int* __restrict__ stats,
                                                                 const int* __restrict__ labels, const int* __restrict__ flag, int h,
                                                                 int w) {
    __shared__ uint8_t edge[CT + 4][CT + 4];   // 0 outside the image
    __shared__ uint8_t dil[CT + 2][CT + 2];    // 1 outside the image: the erosion looks at neighbours inside it only
    const int y0 = blockIdx.y * CT, x0 = blockIdx.x * CT;
    for (int k = threadIdx.x; k < (CT + 4) * (CT + 4); k += CTHREADS) {
        const int ly = k / (CT + 4), lx = k % (CT + 4);
        const int y = y0 + ly - 2, x = x0 + lx - 2;
        uint8_t v = 0;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            const int lab = labels[y * w + x];
            v = lab != 0 && flag[lab - 1] != 0;
        }
        edge[ly][lx] = v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < (CT + 2) * (CT + 2); k += CTHREADS) {
        const int ly = k / (CT + 2), lx = k % (CT + 2);
        const int y = y0 + ly - 1, x = x0 + lx - 1;
        uint8_t v = 1;
        if (y >= 0 && y < h && x >= 0 && x < w)
            v = edge[ly + 1][lx + 1] | edge[ly][lx + 1] | edge[ly + 2][lx + 1] | edge[ly + 1][lx] | edge[ly + 1][lx + 2];
        dil[ly][lx] = v;
    }
    __syncthreads();
    int on_here = 0;
    for (int k = threadIdx.x; k < CT2; k += CTHREADS) {
        const int ly = k / CT, lx = k % CT;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= h || x >= w) continue;
        const uint8_t v = dil[ly + 1][lx + 1] & dil[ly][lx + 1] & dil[ly + 2][lx + 1] & dil[ly + 1][lx] & dil[ly + 1][lx + 2];
        const int i = y * w + x;
        mask[i] = v;
        if (edges != nullptr) edges[i] = v ? 255 : 0;
        seed[i] = v ? i + 1 : 0;
        on_here += v;
    }
    on_here = gt_wave_sum(on_here);
    if ((threadIdx.x & 63) == 0 && on_here > 0) atomicAdd(&stats[MG_EDGE_PIXELS], on_here);
}

// A hole pixel is a pixel off E whose background component does not hang on the outside (root 0); an outer pixel is on E.
__device__ __forceinline__ bool margin_is_root(const int* outer, const int* hole, const uint8_t* mask, int i, bool& is_hole) {
    is_hole = mask[i] == 0;
    return (is_hole ? hole[i] : outer[i]) == i + 1;
}

// Both label arrays compressed in place (a root names itself and is never rewritten, contour_compress_kernel's rule); a root
// clears its box and is counted.
__global__ __launch_bounds__(CTHREADS) void margin_roots_kernel(int* __restrict__ outer, int* __restrict__ hole,
                                                                 const uint8_t* __restrict__ mask, int* __restrict__ box_x0,
                                                                 int* __restrict__ box_x1, int* __restrict__ box_y0,
                                                                 int* __restrict__ box_y1, int* __restrict__ stats, int n) {
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    bool outer_root = false, hole_root = false;
    if (i < n) {
        int* lab = mask[i] ? outer : hole;
        const int mine = lab[i];
        int budget = n + 1;
        const int root = mine != 0 ? find_global<false>(lab, mine, budget) : 0;
        if (mine != 0) lab[i] = root;
        if (root == i + 1) {
            outer_root = mask[i] != 0;
            hole_root = !outer_root;
            box_x0[i] = INT_MAX, box_x1[i] = INT_MIN, box_y0[i] = INT_MAX, box_y1[i] = INT_MIN;
        }
    }
    const int lane = threadIdx.x & 63;
    const unsigned long long outers = __ballot(outer_root), holes = __ballot(hole_root);
    if (lane == 0) {
        if (outers) {
            atomicAdd(&stats[MG_OUTERS], __popcll(outers));
            atomicMin(&stats[MG_FIRST_ROOT], (int)(blockIdx.x * CTHREADS + (threadIdx.x & ~63)) + __ffsll((long long)outers) - 1);
        }
        if (holes) atomicAdd(&stats[MG_HOLES], __popcll(holes));
    }
}

// One lane per pixel; lanes of a wave in the same component combine their extents first (gt_stats_kernel's loop).
__global__ __launch_bounds__(CTHREADS) void margin_boxes_kernel(int* __restrict__ box_x0, int* __restrict__ box_x1,
                                                                 int* __restrict__ box_y0, int* __restrict__ box_y1,
                                                                 const int* __restrict__ outer, const int* __restrict__ hole,
                                                                 const uint8_t* __restrict__ mask, int w, int n) {
    const int i = blockIdx.x * CTHREADS + threadIdx.x, lane = threadIdx.x & 63;
    int key = 0;   // the root's 1-based index: roots of E and of the holes are different pixels, so one key space serves both
    if (i < n) key = mask[i] ? outer[i] : hole[i];
    const int y = i < n ? i / w : 0, x = i < n ? i % w : 0;
    unsigned long long pending = __ballot(key != 0);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int which = __shfl(key, leader);
        const bool same = key == which;
        const int min_x = gt_wave_min(same ? x : INT_MAX), max_x = gt_wave_max(same ? x : INT_MIN);
        const int min_y = gt_wave_min(same ? y : INT_MAX), max_y = gt_wave_max(same ? y : INT_MIN);
        if (lane == leader) {
            gt_lower(&box_x0[which - 1], min_x), gt_raise(&box_x1[which - 1], max_x);
            gt_lower(&box_y0[which - 1], min_y), gt_raise(&box_y1[which - 1], max_y);
        }
        pending &= ~__ballot(same);
    }
}

// x0, y0, width, height of a root's contour: an outer's tight box, a hole's tight box grown by one pixel on all sides (a
// hole touches no frame pixel, so the grown box stays inside the image)
__device__ __forceinline__ void margin_contour_box(const int* box_x0, const int* box_x1, const int* box_y0, const int* box_y1,
                                                   int i, bool is_hole, int& x0, int& y0, int& bw, int& bh) {
    const int grow = is_hole ? 1 : 0;
    x0 = box_x0[i] - grow, y0 = box_y0[i] - grow;
    bw = box_x1[i] - box_x0[i] + 1 + 2 * grow, bh = box_y1[i] - box_y0[i] + 1 + 2 * grow;
}

__global__ __launch_bounds__(CTHREADS) void margin_areas_kernel(unsigned* __restrict__ bitmap, int* __restrict__ stats,
                                                                 const int* __restrict__ box_x0, const int* __restrict__ box_x1,
                                                                 const int* __restrict__ box_y0, const int* __restrict__ box_y1,
                                                                 const int* __restrict__ outer, const int* __restrict__ hole,
                                                                 const uint8_t* __restrict__ mask, int n) {
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    int area = 0;
    bool is_hole;
    if (i < n && margin_is_root(outer, hole, mask, i, is_hole)) {
        int x0, y0, bw, bh;
        margin_contour_box(box_x0, box_x1, box_y0, box_y1, i, is_hole, x0, y0, bw, bh);
        area = min(max(bw * bh, 0), MG_MAX_AREA);   // 1 .. 2^24 by construction; the clamp keeps the bitmap index in range
        atomicOr(&bitmap[area >> 5], 1u << (area & 31));
    }
    const int largest = gt_wave_max(area);
    if ((threadIdx.x & 63) == 0 && largest > 0) gt_raise(&stats[MG_LARGEST], largest);
}

// Step 7 up to the threshold.  Thread t scans words [t * chunk, (t + 1) * chunk) of the bitmap up to the largest area, keeps
// its lowest and highest set bit and its widest gap; thread 0 joins the 1024 summaries in ascending order.  `>=` makes the
// gap at the highest areas win among equals.  All areas equal: T is that area and only the first contour is kept.
__global__ __launch_bounds__(MG_DECIDE_THREADS) void margin_decide_kernel(int* __restrict__ stats, const unsigned* __restrict__ bitmap,
                                                                           int h, int w) {
    __shared__ int s_lo[MG_DECIDE_THREADS], s_hi[MG_DECIDE_THREADS], s_gap[MG_DECIDE_THREADS], s_top[MG_DECIDE_THREADS];
    const int count = stats[MG_OUTERS] + stats[MG_HOLES];
    const int largest = min(max(stats[MG_LARGEST], 0), MG_MAX_AREA);
    int decision = 0;
    if (count <= 1) decision = 1;
    else if ((double)(h * w) * 0.6 > (double)largest) decision = 2;
    if (decision != 0) {   // uniform over the workgroup
        if (threadIdx.x == 0) stats[MG_DECISION] = decision, stats[MG_T] = 0;
        return;
    }
    const int words = largest / 32 + 1, chunk = (words + MG_DECIDE_THREADS - 1) / MG_DECIDE_THREADS;
    const int first = min((int)threadIdx.x * chunk, words), last = min(first + chunk, words);
    int lo = -1, hi = -1, gap = 0, top = 0;
    for (int k = first; k < last; ++k) {
        unsigned bits = bitmap[k];
        while (bits) {
            const int a = k * 32 + __ffs((int)bits) - 1;
            bits &= bits - 1u;
            if (lo < 0) lo = a;
            else if (a - hi >= gap) gap = a - hi, top = a;
            hi = a;
        }
    }
    s_lo[threadIdx.x] = lo, s_hi[threadIdx.x] = hi, s_gap[threadIdx.x] = gap, s_top[threadIdx.x] = top;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int before = -1, best = 0, best_top = 0;
    for (int t = 0; t < MG_DECIDE_THREADS; ++t) {
        if (s_lo[t] < 0) continue;
        if (before >= 0 && s_lo[t] - before >= best) best = s_lo[t] - before, best_top = s_lo[t];
        if (s_gap[t] > 0 && s_gap[t] >= best) best = s_gap[t], best_top = s_top[t];
        before = s_hi[t];
    }
    stats[MG_DECISION] = 0;
    stats[MG_T] = best > 0 ? best_top : largest;
    stats[MG_FIRST_ONLY] = best > 0 ? 0 : 1;   // "all areas equal": keep the first contour only
}

__global__ __launch_bounds__(CTHREADS) void margin_keep_kernel(int* __restrict__ stats, const int* __restrict__ box_x0,
                                                                const int* __restrict__ box_x1, const int* __restrict__ box_y0,
                                                                const int* __restrict__ box_y1, const int* __restrict__ outer,
                                                                const int* __restrict__ hole, const uint8_t* __restrict__ mask, int n) {
    const int i = blockIdx.x * CTHREADS + threadIdx.x;
    const bool decided = stats[MG_DECISION] == 0;
    const int threshold = stats[MG_T], first_only = stats[MG_FIRST_ONLY], first_root = stats[MG_FIRST_ROOT];
    bool keep = false, is_hole;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
    if (decided && i < n && margin_is_root(outer, hole, mask, i, is_hole)) {
        int bw, bh, bx, by;
        margin_contour_box(box_x0, box_x1, box_y0, box_y1, i, is_hole, bx, by, bw, bh);
        keep = first_only ? (!is_hole && i == first_root) : bw * bh >= threshold;
        if (keep) x0 = bx, y0 = by, x1 = bx + bw, y1 = by + bh;
    }
    const unsigned long long kept = __ballot(keep);
    if (!kept) return;   // wave-uniform
    x0 = gt_wave_min(x0), y0 = gt_wave_min(y0), x1 = gt_wave_max(x1), y1 = gt_wave_max(y1);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&stats[MG_KEPT], __popcll(kept));
        gt_lower(&stats[MG_X0], x0), gt_lower(&stats[MG_Y0], y0), gt_raise(&stats[MG_X1], x1), gt_raise(&stats[MG_Y1], y1);
    }
}

__global__ void margin_finish_kernel(int32_t* __restrict__ box, int32_t* __restrict__ info, const int* __restrict__ stats, int h, int w) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool whole = stats[MG_DECISION] != 0;
    box[0] = whole ? 0 : stats[MG_X0], box[1] = whole ? 0 : stats[MG_Y0];
    box[2] = whole ? w : stats[MG_X1], box[3] = whole ? h : stats[MG_Y1];
    info[0] = stats[MG_OUTERS] + stats[MG_HOLES], info[1] = stats[MG_OUTERS], info[2] = stats[MG_LARGEST];
    info[3] = whole ? 0 : stats[MG_KEPT], info[4] = stats[MG_DECISION], info[5] = whole ? 0 : stats[MG_T];
    info[6] = stats[MG_EDGE_PIXELS], info[7] = 0;
}

// One workgroup: the roots ranked in raster order (gt_rank_kernel's walk), outers first, then holes; a root below
// max_contours writes its row.
__global__ __launch_bounds__(GT_SCAN_THREADS) void margin_table_kernel(int32_t* __restrict__ contours, int max_contours,
                                                                        const int* __restrict__ box_x0, const int* __restrict__ box_x1,
                                                                        const int* __restrict__ box_y0, const int* __restrict__ box_y1,
                                                                        const int* __restrict__ outer, const int* __restrict__ hole,
                                                                        const uint8_t* __restrict__ mask, int n) {
    __shared__ int outer_sums[GT_SCAN_THREADS / 64], hole_sums[GT_SCAN_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = GT_SCAN_THREADS / 64;
    const int segment = ((n + waves - 1) / waves + 63) / 64 * 64;
    const int seg0 = min(wave * segment, n), seg1 = min(seg0 + segment, n);
    int outers = 0, holes = 0;
    for (int i0 = seg0; i0 < seg1; i0 += 64) {
        const int i = i0 + lane;
        bool is_hole = false;
        const bool root = i < seg1 && margin_is_root(outer, hole, mask, i, is_hole);
        outers += __popcll(__ballot(root && !is_hole));
        holes += __popcll(__ballot(root && is_hole));
    }
    if (lane == 0) outer_sums[wave] = outers, hole_sums[wave] = holes;
    __syncthreads();
    int outer_rank = 0, hole_rank = 0;   // holes follow ALL outers
    for (int v = 0; v < waves; ++v) {
        outer_rank += v < wave ? outer_sums[v] : 0;
        hole_rank += outer_sums[v] + (v < wave ? hole_sums[v] : 0);
    }
    const unsigned long long below_me = (1ull << lane) - 1ull;
    for (int i0 = seg0; i0 < seg1; i0 += 64) {
        const int i = i0 + lane;
        bool is_hole = false;
        const bool root = i < seg1 && margin_is_root(outer, hole, mask, i, is_hole);
        const unsigned long long outer_roots = __ballot(root && !is_hole), hole_roots = __ballot(root && is_hole);
        if (root) {
            const int slot = is_hole ? hole_rank + __popcll(hole_roots & below_me) : outer_rank + __popcll(outer_roots & below_me);
            if (slot < max_contours) {
                int x0, y0, bw, bh;
                margin_contour_box(box_x0, box_x1, box_y0, box_y1, i, is_hole, x0, y0, bw, bh);
                int32_t* row = contours + (int64_t)slot * 6;
                row[0] = is_hole ? 1 : 0, row[1] = i, row[2] = x0, row[3] = y0, row[4] = bw, row[5] = bh;
            }
        }
        outer_rank += __popcll(outer_roots);
        hole_rank += __popcll(hole_roots);
    }
}

inline bool margin_side_ok(int v) { return v >= MG_MIN_SIDE && v <= MG_MAX_SIDE; }

}  // namespace

extern "C" int64_t sis_scan_content_box_workspace_bytes(int height, int width) {
    if (!margin_side_ok(height) || !margin_side_ok(width)) return 0;
    return margin_workspace_bytes(height, width);
}

extern "C" int sis_scan_content_box(int32_t* box, int32_t* info, uint8_t* edges, int32_t* contours, int max_contours,
                                    const uint8_t* page, int height, int width, int low, int high, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
    SIS_REQUIRE(margin_side_ok(height) && margin_side_ok(width), "sis_scan_content_box: image %d x %d outside %d..%d a side", height,
                width, MG_MIN_SIDE, MG_MAX_SIDE);
    SIS_REQUIRE(low >= 0 && high >= low, "sis_scan_content_box: thresholds low %d, high %d: 0 <= low <= high is needed", low, high);
    SIS_REQUIRE(max_contours >= 0, "sis_scan_content_box: negative max_contours %d", max_contours);
    SIS_REQUIRE(box && info && page && workspace, "sis_scan_content_box: null pointer");
    SIS_REQUIRE((((uintptr_t)box | (uintptr_t)info | (uintptr_t)contours | (uintptr_t)workspace) & 3) == 0,
                "sis_scan_content_box: box, info, contours and workspace must be 4-byte aligned");
    SIS_REQUIRE(workspace_bytes >= margin_workspace_bytes(height, width), "sis_scan_content_box: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)margin_workspace_bytes(height, width));
    const int h = height, w = width, n = h * w;
    const MarginWorkspace m = margin_carve(workspace, h, w);
    const Plane g{w, h, n, 1, -1, 0u};   // one plane, never skipped
    hipStream_t st = (hipStream_t)stream;
    const dim3 tiles(sis_cdiv(w, CT), sis_cdiv(h, CT), 1), threads(CTHREADS);
    const dim3 pixels(sis_cdiv(n, CTHREADS), 1);
    const int64_t border_pixels = (int64_t)((w - 1) / CT) * h + (int64_t)((h - 1) / CT) * w;
    const dim3 borders(sis_cdiv(border_pixels, CTHREADS), 1);

    hipLaunchKernelGGL(margin_clear_kernel, dim3(sis_cdiv(MG_BITMAP_WORDS, CTHREADS)), threads, 0, st, m.stats, m.bitmap);
    SIS_CHECK_LAUNCH("margin_clear_kernel");
    hipLaunchKernelGGL(margin_front_kernel, tiles, threads, 0, st, m.a, m.strong, page, h, w, low, high);
    SIS_CHECK_LAUNCH("margin_front_kernel");
    // the candidates' 8-connected components: the labelling kernel takes "root of the seed is not 0" as membership
    hipLaunchKernelGGL(contour_label_tile_kernel<true>, tiles, threads, 0, st, m.b, m.act, (const int*)m.a, g);
    SIS_CHECK_LAUNCH("contour_label_tile_kernel<candidates>");
    if (border_pixels > 0) {
        hipLaunchKernelGGL(contour_merge_borders_kernel<true>, borders, threads, 0, st, m.b, (const uint8_t*)m.act, g);
        SIS_CHECK_LAUNCH("contour_merge_borders_kernel<candidates>");
    }
    hipLaunchKernelGGL(contour_compress_kernel<true>, pixels, threads, 0, st, m.b, m.a, g);   // and flag (= a) cleared
    SIS_CHECK_LAUNCH("contour_compress_kernel<candidates>");
    hipLaunchKernelGGL(margin_flag_kernel, pixels, threads, 0, st, m.a, (const int*)m.b, (const uint8_t*)m.strong, n);
    SIS_CHECK_LAUNCH("margin_flag_kernel");
    hipLaunchKernelGGL(margin_close_kernel, tiles, threads, 0, st, m.mask, edges, m.c, m.stats, (const int*)m.b, (const int*)m.a, h, w);
    SIS_CHECK_LAUNCH("margin_close_kernel");
    // holes: the 4-connected background of E that does not reach the frame (pass 1 of contour_cc.h)
    hipLaunchKernelGGL(contour_label_tile_kernel<false>, tiles, threads, 0, st, m.a, m.mask, (const int*)nullptr, g);
    SIS_CHECK_LAUNCH("contour_label_tile_kernel<holes>");
    if (border_pixels > 0) {
        hipLaunchKernelGGL(contour_merge_borders_kernel<false>, borders, threads, 0, st, m.a, (const uint8_t*)m.mask, g);
        SIS_CHECK_LAUNCH("contour_merge_borders_kernel<holes>");
    }
    // outers: the 8-connected components of E itself (holes stay open: an island in a hole is a contour of its own)
    hipLaunchKernelGGL(contour_label_tile_kernel<true>, tiles, threads, 0, st, m.b, m.act, (const int*)m.c, g);
    SIS_CHECK_LAUNCH("contour_label_tile_kernel<outers>");
    if (border_pixels > 0) {
        hipLaunchKernelGGL(contour_merge_borders_kernel<true>, borders, threads, 0, st, m.b, (const uint8_t*)m.act, g);
        SIS_CHECK_LAUNCH("contour_merge_borders_kernel<outers>");
    }
    int* box_x0 = m.c;   // the seeds of E are dead
    hipLaunchKernelGGL(margin_roots_kernel, pixels, threads, 0, st, m.b, m.a, (const uint8_t*)m.mask, box_x0, m.box_x1, m.box_y0,
                       m.box_y1, m.stats, n);
    SIS_CHECK_LAUNCH("margin_roots_kernel");
    hipLaunchKernelGGL(margin_boxes_kernel, pixels, threads, 0, st, box_x0, m.box_x1, m.box_y0, m.box_y1, (const int*)m.b,
                       (const int*)m.a, (const uint8_t*)m.mask, w, n);
    SIS_CHECK_LAUNCH("margin_boxes_kernel");
    hipLaunchKernelGGL(margin_areas_kernel, pixels, threads, 0, st, m.bitmap, m.stats, (const int*)box_x0, (const int*)m.box_x1,
                       (const int*)m.box_y0, (const int*)m.box_y1, (const int*)m.b, (const int*)m.a, (const uint8_t*)m.mask, n);
    SIS_CHECK_LAUNCH("margin_areas_kernel");
    hipLaunchKernelGGL(margin_decide_kernel, dim3(1), dim3(MG_DECIDE_THREADS), 0, st, m.stats, (const unsigned*)m.bitmap, h, w);
    SIS_CHECK_LAUNCH("margin_decide_kernel");
    hipLaunchKernelGGL(margin_keep_kernel, pixels, threads, 0, st, m.stats, (const int*)box_x0, (const int*)m.box_x1,
                       (const int*)m.box_y0, (const int*)m.box_y1, (const int*)m.b, (const int*)m.a, (const uint8_t*)m.mask, n);
    SIS_CHECK_LAUNCH("margin_keep_kernel");
    hipLaunchKernelGGL(margin_finish_kernel, dim3(1), dim3(64), 0, st, box, info, (const int*)m.stats, h, w);
    SIS_CHECK_LAUNCH("margin_finish_kernel");
    if (contours != nullptr && max_contours > 0) {
        hipLaunchKernelGGL(margin_table_kernel, dim3(1), dim3(GT_SCAN_THREADS), 0, st, contours, max_contours, (const int*)box_x0,
                           (const int*)m.box_x1, (const int*)m.box_y0, (const int*)m.box_y1, (const int*)m.b, (const int*)m.a,
                           (const uint8_t*)m.mask, n);
        SIS_CHECK_LAUNCH("margin_table_kernel");
    }
    return 0;
}
