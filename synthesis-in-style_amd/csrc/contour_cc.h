// Connected-component labelling shared by the contour filter (contour_ops.hip) and the cluster-based labeller
// (cluster_segment.hip): union-find on a 32x32 tile in LDS, tile borders merged with atomicMin on the global label array.
// Labels are 1-based pixel indices within the plane, a parent is never larger than its child, so the root of a set is its
// smallest member whatever the order the atomics land in.  Every find / union loop runs on a step budget; workgroups of one
// launch only meet through device-scope atomics: a stale plain read of a label yields an older parent of the same set, which
// costs a retry and never a wrong merge.  DESIGN.md §10.2.
#pragma once
#include "sis_common.h"

namespace {

constexpr int CT = 32;            // tile edge
constexpr int CT2 = CT * CT;
constexpr int CTHREADS = 256;
constexpr int CMAXP = 1024;

// A plane is w pixels wide and h high (the square callers pass p, p); pixel (y, x) has index y * w + x.  skip_classes: bit k set
// skips class k as the background class is skipped (the page entries' filter_classes; 0 elsewhere).
struct Plane {
    int w, h, n, classes, background;   // n = w*h
    unsigned skip_classes;
};

__device__ __forceinline__ bool skip_plane(const Plane& g, int plane) {
    const int k = plane % g.classes;
    return k == g.background || ((g.skip_classes >> (k & 31)) & 1u) != 0;
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
        if (y < g.h && x < g.w) {
            const int i = y * g.w + x;
            if (REGION) {
                int budget = g.n + 1;
                on = find_global<false>(outside_labels + base, i + 1, budget) != 0;
            } else {
                on = active[base + i] == 0;
                edge = y == 0 || x == 0 || y == g.h - 1 || x == g.w - 1;
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
        if (y >= g.h || x >= g.w) continue;
        const int i = y * g.w + x;
        int lab;
        if (act[k]) {
            const int root = find_lds(s, k + 1);
            lab = root == 0 ? 0 : (y0 + (root - 1) / CT) * g.w + x0 + (root - 1) % CT + 1;
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
    const int across = ((g.w - 1) / CT) * g.h;   // pixels on the first columns of the tiles right of an interior tile border
    const int below = ((g.h - 1) / CT) * g.w;    // pixels on the first rows of the tiles under one
    const int id = blockIdx.x * CTHREADS + threadIdx.x;
    if (id >= across + below) return;
    const bool vertical = id < across;
    const int r = vertical ? id : id - across, length = vertical ? g.h : g.w;
    const int line = (r / length + 1) * CT, along = r % length;
    const int y = vertical ? along : line, x = vertical ? line : along;
    int* lab = labels + (int64_t)plane * g.n;
    const uint8_t* act = active + (int64_t)plane * g.n;
    const uint8_t on = REGION ? 1 : 0;
    if (act[y * g.w + x] != on) return;
    const int me = y * g.w + x + 1, budget = 4 * g.n + 64;
    for (int d = -1; d <= 1; ++d) {
        if (!REGION && d != 0) continue;
        const int ny = vertical ? y + d : y - 1, nx = vertical ? x - 1 : x + d;
        if (ny < 0 || ny >= g.h || nx < 0 || nx >= g.w) continue;
        if (act[ny * g.w + nx] == on) union_global(lab, me, ny * g.w + nx + 1, budget);
    }
}

// Lanes of a wave that hold the same key add their values once: one atomicAdd per distinct key and wave.
__device__ __forceinline__ void wave_add_by_key(int* acc, int key, int add) {
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(add > 0);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int which = __shfl(key, leader);
        const bool same = add > 0 && key == which;
        int sum = same ? add : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == leader) atomicAdd(&acc[which], sum);
        pending &= ~__ballot(same);
    }
}

}  // namespace
