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
#include "sis_common.h"

namespace {

constexpr int CT = 32;            // tile edge
constexpr int CT2 = CT * CT;
constexpr int CTHREADS = 256;
constexpr int CMAXP = 1024;

struct Plane {
    int p, n, classes, background;   // n = p*p
};

__device__ __forceinline__ bool skip_plane(const Plane& g, int plane) { return plane % g.classes == g.background; }

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
        if (y >= 0 && y < g.p && x >= 0 && x < g.p) v = (threshold(src[y * g.p + x], min_confidence) * 255.0f) >= 1.0f;
        m0[ly][lx] = v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < (CT + 4) * (CT + 4); k += CTHREADS) {
        const int ly = k / (CT + 4), lx = k % (CT + 4);
        const int y = y0 + ly - 2, x = x0 + lx - 2;
        uint8_t v = 1;
        if (y >= 0 && y < g.p && x >= 0 && x < g.p) {
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
        if (y >= g.p || x >= g.p) continue;
        uint8_t v = 1;
#pragma unroll
        for (int dy = 0; dy < 5; ++dy)
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) v &= dil[ly + dy][lx + dx];
        mask[(int64_t)plane * g.n + y * g.p + x] = v;
    }
}

// ---- union-find on 1-based labels; 0 is a root of its own --------------------------------------------------------------------
__device__ __forceinline__ int find_lds(const volatile int* s, int lab) {
    for (int steps = 0; steps <= CT2; ++steps) {
        const int parent = s[lab];
        if (parent == lab) break;
        lab = parent;
    }
    return lab;
}

__device__ __forceinline__ void union_lds(int* s, int a, int b) {
    for (int steps = 0; steps <= CT2; ++steps) {
        a = find_lds(s, a);
        b = find_lds(s, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&s[a], b);
        if (old == a) return;
        a = old;
    }
}

// labels[i] is the parent of label i + 1.  COHERENT: other workgroups of this launch lower parents with atomics, read past the
// caches that are not shared with them.
template <bool COHERENT>
__device__ __forceinline__ int find_global(const int* labels, int lab, int& budget) {
    while (lab != 0 && budget > 0) {
        const int parent = COHERENT ? __hip_atomic_load(const_cast<int*>(labels) + lab - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                    : labels[lab - 1];
        if (parent == lab) break;
        lab = parent;
        --budget;
    }
    return lab;
}

__device__ __forceinline__ void union_global(int* labels, int a, int b, int budget) {
    while (budget > 0) {
        a = find_global<true>(labels, a, budget);
        b = find_global<true>(labels, b, budget);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&labels[a - 1], b);   // a > b >= 0, so a >= 1
        if (old == a) return;
        a = old;
        --budget;
    }
}

// ---- pass 1 (REGION = false): 4-connected background of M, plane-edge background belongs to the outside (label 0); foreground
//      pixels keep their own label.  pass 2 (REGION = true): 8-connected pixels whose pass-1 root is not 0; the others get label
//      0 and `active` (which held M) becomes the membership byte of (not O). ------------------------------------------------------
template <bool REGION>
__global__ __launch_bounds__(CTHREADS) void contour_label_tile_kernel(int* __restrict__ labels, uint8_t* __restrict__ active,
                                                                      const int* __restrict__ outside_labels, Plane g) {
    const int plane = blockIdx.z;
    if (skip_plane(g, plane)) return;
    __shared__ int s[CT2 + 1];
    __shared__ uint8_t act[CT2];
    const int y0 = blockIdx.y * CT, x0 = blockIdx.x * CT;
    const int64_t base = (int64_t)plane * g.n;
    if (threadIdx.x == 0) s[0] = 0;
    // A wave holds two rows of the tile per round, so a ballot gives every pixel its row: all pixels of a horizontal run start
    // with the label of the run's first pixel and no horizontal union is needed.
    const int lane = threadIdx.x & 63;
    int run_label[CT2 / CTHREADS];
    bool seeded[CT2 / CTHREADS];
#pragma unroll
    for (int j = 0; j < CT2 / CTHREADS; ++j) {
        const int k = threadIdx.x + j * CTHREADS;
        const int lx = k % CT, y = y0 + k / CT, x = x0 + lx;
        bool on = false, edge = false;
        if (y < g.p && x < g.p) {
            const int i = y * g.p + x;
            if (REGION) {
                int budget = g.n + 1;
                on = find_global<false>(outside_labels + base, i + 1, budget) != 0;
            } else {
                on = active[base + i] == 0;
                edge = y == 0 || x == 0 || y == g.p - 1 || x == g.p - 1;
            }
        }
        const unsigned row = (unsigned)(__ballot(on) >> (lane & 32));
        const unsigned gaps = ~row & ((1u << lx) - 1u);          // pixels of the row left of this one that are off
        const int first = gaps ? 32 - __clz((int)gaps) : 0;      // where this pixel's run begins
        run_label[j] = k - lx + first + 1;
        seeded[j] = on && edge;
        act[k] = on;
        s[k + 1] = on ? run_label[j] : k + 1;
    }
    __syncthreads();
    if (!REGION) {   // a run with a pixel on the plane's edge hangs on the outside
#pragma unroll
        for (int j = 0; j < CT2 / CTHREADS; ++j)
            if (seeded[j]) s[run_label[j]] = 0;
        __syncthreads();
    }
    // Two runs in adjacent rows are joined once, at the first column they share; diagonal neighbours (pass 2) only where
    // neither of the two pixels between them makes the connection already.
    for (int k = threadIdx.x; k < CT2; k += CTHREADS) {
        if (!act[k]) continue;
        const int ly = k / CT, lx = k % CT;
        if (ly == 0) continue;
        const bool up = act[k - CT], left = lx > 0 && act[k - 1], right = lx < CT - 1 && act[k + 1];
        const bool up_left = lx > 0 && act[k - CT - 1], up_right = lx < CT - 1 && act[k - CT + 1];
        if (up && (lx == 0 || !left || !up_left)) union_lds(s, k + 1, k + 1 - CT);
        if (REGION && !up) {
            if (up_left && !left) union_lds(s, k + 1, k - CT);
            if (up_right && !right) union_lds(s, k + 1, k + 2 - CT);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < CT2; k += CTHREADS) {
        const int y = y0 + k / CT, x = x0 + k % CT;
        if (y >= g.p || x >= g.p) continue;
        const int i = y * g.p + x;
        int lab;
        if (act[k]) {
            const int root = find_lds(s, k + 1);
            lab = root == 0 ? 0 : (y0 + (root - 1) / CT) * g.p + x0 + (root - 1) % CT + 1;
        } else {
            lab = REGION ? 0 : i + 1;
        }
        labels[base + i] = lab;
        if (REGION) active[base + i] = act[k];
    }
}

// One lane per pixel of a tile's first column / first row: joins it to its neighbours across the tile border.
template <bool REGION>
__global__ __launch_bounds__(CTHREADS) void contour_merge_borders_kernel(int* __restrict__ labels,
                                                                         const uint8_t* __restrict__ active, Plane g) {
    const int plane = blockIdx.y;
    if (skip_plane(g, plane)) return;
    const int lines = (g.p - 1) / CT;   // interior tile borders per direction
    const int id = blockIdx.x * CTHREADS + threadIdx.x;
    if (id >= 2 * lines * g.p) return;
    const bool vertical = id < lines * g.p;
    const int r = vertical ? id : id - lines * g.p;
    const int line = (r / g.p + 1) * CT, along = r % g.p;
    const int y = vertical ? along : line, x = vertical ? line : along;
    int* lab = labels + (int64_t)plane * g.n;
    const uint8_t* act = active + (int64_t)plane * g.n;
    const uint8_t on = REGION ? 1 : 0;
    if (act[y * g.p + x] != on) return;
    const int me = y * g.p + x + 1, budget = 4 * g.n + 64;
    for (int d = -1; d <= 1; ++d) {
        if (!REGION && d != 0) continue;
        const int ny = vertical ? y + d : y - 1, nx = vertical ? x - 1 : x + d;
        if (ny < 0 || ny >= g.p || nx < 0 || nx >= g.p) continue;
        if (act[ny * g.p + nx] == on) union_global(lab, me, ny * g.p + nx + 1, budget);
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
    const int id = blockIdx.x * CTHREADS + threadIdx.x, side = g.p + 1;
    const int64_t base = (int64_t)plane * g.n;
    int add = 0, lab = 0;
    if (id < side * side) {
        const int by = id / side, bx = id % side;   // pixels (by-1 .. by, bx-1 .. bx)
        int count = 0;
        for (int dy = -1; dy <= 0; ++dy)
            for (int dx = -1; dx <= 0; ++dx) {
                const int y = by + dy, x = bx + dx;
                if (y >= 0 && y < g.p && x >= 0 && x < g.p && member[base + y * g.p + x]) {
                    ++count;
                    lab = labels[base + y * g.p + x];
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
    const Plane g{p, p * p, classes, background_class_id};
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
