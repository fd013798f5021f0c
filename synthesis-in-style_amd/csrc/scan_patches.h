// GAN training patches cut from document scans (scripts/create_stylegan_train_dataset.py:18-46 of the reference: there Pillow's
// thumbnail and crop on one host thread).  Included by dataset_ops.hip.  DESIGN.md §18 states the arithmetic;
// tests/scan_patches_restatement.py restates it, and the bytes written here EQUAL Pillow's for 8-bit RGB.
//
// Pages are uint8 [H][W][3] in device memory, 1 <= H, W <= 16384.  Integer arithmetic only, no atomics, every sum in a fixed
// order: two calls give the same bytes.  All launches on the caller's stream, no host sync.
//   scan_reduce_kernel   Pillow's reduce((fx, fy)): one thread per output pixel, the fy x fx box (ragged at the last row and
//                        column) summed in row order, then ((sum + n / 2) * multiplier(n)) >> 24 in uint32
//   scan_hpass_kernel    horizontal pass of the antialiased resample: a workgroup takes 64 output columns and 16 rows; the tap
//                        table of its columns is staged in LDS once, the source segment of four rows at a time
//   scan_vpass_kernel    vertical pass: a thread takes four consecutive bytes of an output row (coalesced along x), the row's
//                        coefficients are wave-uniform
//   scan_patches_kernel  n windows of size x size gathered into one packed buffer, black outside the page
// The float helpers of sis_device.h (sis_load4 / sis_load8) convert to float and do not apply to bytes: four bytes travel as one
// aligned 32-bit word here wherever the address allows, as in png_load_bytes.

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_MAX_SIDE = 16384;
constexpr int SCAN_MAX_BOX = 65536;        // fx * fy of a reduce: 255 * n + n / 2 and 256 * n stay far inside uint32
constexpr int SCAN_MAX_TAPS = 67;          // ksize = 2 * ceil(2 * scale) + 1: an axis shrinks by at most 16 in one call
constexpr int SCAN_TX = 64;                // output columns of a horizontal tile
constexpr int SCAN_TY = 4;                 // rows of a horizontal tile in flight (64 threads each)
constexpr int SCAN_ROWS = 16;              // rows per workgroup: the tap table is staged once for all of them
constexpr int SCAN_PRECISION_BITS = 22;    // Pillow's 32 - 8 - 2
constexpr int SCAN_MAX_PATCH = 4096;       // what sis_png_encode_pairs takes

// Upper bound on the source pixels that the taps of SCAN_TX consecutive outputs span: ceil(support) = (ksize - 1) / 2 >=
// support >= 2 * scale, the centres of the tile lie (SCAN_TX - 1) * scale apart, and both ends round once.
__host__ __device__ inline int scan_seg_cap(int ksize) { return ((SCAN_TX - 1) * (ksize - 1) + 3) / 4 + ksize + 2; }
__host__ __device__ inline int scan_seg_bytes(int ksize) { return (3 * scan_seg_cap(ksize) + 3) & ~3; }
__host__ __device__ inline int64_t scan_pitch(int width) { return (3 * (int64_t)width + 3) & ~(int64_t)3; }

// Pillow's clip8: the table lookup of acc >> PRECISION_BITS (arithmetic), i.e. that value clamped to 0..255.  Written as a clamp
// of the ACCUMULATOR followed by a logical shift: the compiler turns clamp(acc >> 22, 0, 255) of two neighbouring bytes into
// v_ashr_pk_u8_i32 and ORs the other two bytes onto its result, but on the MI355X that instruction left bits 16..31 of its
// destination register as they were, so bytes 2 and 3 of a stored word came out ORed with stale bits.
__device__ __forceinline__ uint32_t scan_clip8(int acc) {
    constexpr int top = (255 << SCAN_PRECISION_BITS) | ((1 << SCAN_PRECISION_BITS) - 1);   // the largest accumulator of byte 255
    return (uint32_t)min(max(acc, 0), top) >> SCAN_PRECISION_BITS;
}

// `nbytes` bytes from global memory to LDS by `lanes` threads (this one is `lane`), 4-byte loads over the aligned middle
__device__ __forceinline__ void scan_load_bytes(uint8_t* dst, const uint8_t* __restrict__ src, int nbytes, int lane, int lanes) {
    const int head = min((int)((4 - ((uintptr_t)src & 3)) & 3), nbytes);
    const int words = (nbytes - head) >> 2;
    for (int i = lane; i < head; i += lanes) dst[i] = src[i];
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src + head);
    for (int k = lane; k < words; k += lanes) {
        const uint32_t v = s4[k];
        uint8_t* d = dst + head + 4 * k;
        d[0] = (uint8_t)v; d[1] = (uint8_t)(v >> 8); d[2] = (uint8_t)(v >> 16); d[3] = (uint8_t)(v >> 24);
    }
    for (int i = head + 4 * words + lane; i < nbytes; i += lanes) dst[i] = src[i];
}

// mult: Pillow's division_UINT32(n, 8) for n = fy * fx, fy * rx, ry * fx, ry * rx (rx, ry: the ragged last column / row)
__global__ __launch_bounds__(SCAN_THREADS) void scan_reduce_kernel(uint8_t* __restrict__ out, const uint8_t* __restrict__ page, int height,
                                                                   int width, int out_w, int fx, int fy, uint32_t m_full, uint32_t m_right,
                                                                   uint32_t m_bottom, uint32_t m_corner) {
    const int ox = blockIdx.x * SCAN_THREADS + threadIdx.x, oy = blockIdx.y;
    if (ox >= out_w) return;
    const int x0 = ox * fx, y0 = oy * fy;
    const int nx = min(fx, width - x0), ny = min(fy, height - y0);
    uint32_t s0 = 0, s1 = 0, s2 = 0;
    for (int y = 0; y < ny; ++y) {
        const uint8_t* p = page + ((int64_t)(y0 + y) * width + x0) * 3;
        for (int x = 0; x < nx; ++x) { s0 += p[3 * x]; s1 += p[3 * x + 1]; s2 += p[3 * x + 2]; }
    }
    const uint32_t amend = (uint32_t)(nx * ny) / 2;
    const uint32_t mult = nx == fx ? (ny == fy ? m_full : m_bottom) : (ny == fy ? m_right : m_corner);
    uint8_t* o = out + ((int64_t)oy * out_w + ox) * 3;
    o[0] = (uint8_t)(((s0 + amend) * mult) >> 24);
    o[1] = (uint8_t)(((s1 + amend) * mult) >> 24);
    o[2] = (uint8_t)(((s2 + amend) * mult) >> 24);
}

// out[y][x][c] = clip8((2^21 + sum_j src[y][first[x] + j][c] * coef[x][j]) >> 22), j < count[x], in tap order.
// A table entry that would leave the row or the staged segment is clamped, so no table can make a read leave the page.
__global__ __launch_bounds__(SCAN_THREADS) void scan_hpass_kernel(uint8_t* __restrict__ out, int64_t out_pitch, const uint8_t* __restrict__ src,
                                                                  int64_t src_pitch, int rows, int in_w, int out_w,
                                                                  const int32_t* __restrict__ coef, const int32_t* __restrict__ first,
                                                                  const int32_t* __restrict__ count, int ksize) {
    extern __shared__ __attribute__((aligned(16))) uint8_t scan_lds[];
    int32_t* s_coef = reinterpret_cast<int32_t*>(scan_lds);   // [SCAN_TX][ksize]: ksize is odd, so a wave's reads hit 64 banks
    int32_t* s_first = s_coef + SCAN_TX * ksize;              // [SCAN_TX], relative to the segment
    int32_t* s_count = s_first + SCAN_TX;                     // [SCAN_TX]
    uint8_t* s_seg = reinterpret_cast<uint8_t*>(s_count + SCAN_TX);   // [SCAN_TY][seg_bytes]
    const int seg_bytes = scan_seg_bytes(ksize);
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * SCAN_TX, nx = min(SCAN_TX, out_w - x0);
    for (int i = t; i < nx * ksize; i += SCAN_THREADS) s_coef[i] = coef[(int64_t)x0 * ksize + i];
    const int seg0 = min(max(first[x0], 0), in_w - 1);        // first[] does not decrease with x
    const int seg_len = min(scan_seg_cap(ksize), in_w - seg0);
    if (t < nx) {
        const int f = min(max(first[x0 + t] - seg0, 0), seg_len);
        s_first[t] = f;
        s_count[t] = max(min(min(count[x0 + t], ksize), seg_len - f), 0);
    }
    __syncthreads();
    const int r = t >> 6, px = t & 63;
    const int y_end = min(rows, (int)(blockIdx.y + 1) * SCAN_ROWS);
    for (int yb = blockIdx.y * SCAN_ROWS; yb < y_end; yb += SCAN_TY) {
        const int y = yb + r;
        uint8_t* seg = s_seg + r * seg_bytes;
        if (y < y_end) scan_load_bytes(seg, src + (int64_t)y * src_pitch + (int64_t)seg0 * 3, seg_len * 3, px, 64);
        __syncthreads();
        if (y < y_end && px < nx) {
            const uint8_t* p = seg + 3 * s_first[px];
            const int32_t* k = s_coef + px * ksize;
            const int c = s_count[px];
            int a0 = 1 << (SCAN_PRECISION_BITS - 1), a1 = a0, a2 = a0;
            for (int j = 0; j < c; ++j) {
                const int kj = k[j];
                a0 += (int)p[3 * j] * kj;
                a1 += (int)p[3 * j + 1] * kj;
                a2 += (int)p[3 * j + 2] * kj;
            }
            uint8_t* o = out + (int64_t)y * out_pitch + (int64_t)(x0 + px) * 3;
            o[0] = (uint8_t)scan_clip8(a0); o[1] = (uint8_t)scan_clip8(a1); o[2] = (uint8_t)scan_clip8(a2);
        }
        __syncthreads();
    }
}

// out[y][b] = clip8((2^21 + sum_j src[first[y] + j][b] * coef[y][j]) >> 22) over the row_bytes = 3 * width bytes of a row.
// WORDS: src and src_pitch are 4-byte aligned and every row may be read up to its pitch (the workspace's rows).
template <bool WORDS>
__global__ __launch_bounds__(SCAN_THREADS) void scan_vpass_kernel(uint8_t* __restrict__ out, int64_t out_pitch, const uint8_t* __restrict__ src,
                                                                  int64_t src_pitch, int in_h, int row_bytes,
                                                                  const int32_t* __restrict__ coef, const int32_t* __restrict__ first,
                                                                  const int32_t* __restrict__ count, int ksize) {
    const int b = (blockIdx.x * SCAN_THREADS + threadIdx.x) * 4, y = blockIdx.y;
    if (b >= row_bytes) return;
    const int f = min(max(first[y], 0), in_h - 1);
    const int c = max(min(min(count[y], ksize), in_h - f), 0);
    const int32_t* k = coef + (int64_t)y * ksize;
    int a[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = 1 << (SCAN_PRECISION_BITS - 1);
    const uint8_t* p = src + (int64_t)f * src_pitch + b;
    const int live = min(4, row_bytes - b);
    for (int j = 0; j < c; ++j, p += src_pitch) {
        const int kj = k[j];
        if (WORDS) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] += (int)((v >> (8 * e)) & 255u) * kj;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < live) a[e] += (int)p[e] * kj;
        }
    }
    uint8_t* o = out + (int64_t)y * out_pitch + b;
    if (live == 4 && (((uintptr_t)o) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(o) = scan_clip8(a[0]) | (scan_clip8(a[1]) << 8) | (scan_clip8(a[2]) << 16) | (scan_clip8(a[3]) << 24);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < live) o[e] = (uint8_t)scan_clip8(a[e]);
    }
}

// out [n][size][size][3] as one run of bytes; a thread takes four of them (the buffer starts 4-byte aligned)
__global__ __launch_bounds__(SCAN_THREADS) void scan_patches_kernel(uint8_t* __restrict__ out, int64_t out_bytes, const uint8_t* __restrict__ page,
                                                                    const int32_t* __restrict__ origins, int size, int height, int width) {
    const int64_t at = ((int64_t)blockIdx.x * SCAN_THREADS + threadIdx.x) * 4;
    if (at >= out_bytes) return;
    const int row_bytes = 3 * size;
    const int64_t patch_bytes = (int64_t)size * row_bytes;
    int n = (int)(at / patch_bytes);
    const int in_patch = (int)(at - n * patch_bytes);
    int y = in_patch / row_bytes, xb = in_patch - y * row_bytes;
    const int live = (int)min((int64_t)4, out_bytes - at);
    uint32_t word = 0;
    for (int e = 0; e < live; ++e) {
        const int x = xb / 3, ch = xb - 3 * x;
        const int64_t sx = (int64_t)origins[2 * n] + x, sy = (int64_t)origins[2 * n + 1] + y;
        const uint32_t v = (sx >= 0 && sx < width && sy >= 0 && sy < height) ? page[(sy * width + sx) * 3 + ch] : 0u;
        word |= v << (8 * e);
        if (++xb == row_bytes) {
            xb = 0;
            if (++y == size) { y = 0; ++n; }
        }
    }
    if (live == 4) *reinterpret_cast<uint32_t*>(out + at) = word;
    else
        for (int e = 0; e < live; ++e) out[at + e] = (uint8_t)(word >> (8 * e));
}

// Pillow's division_UINT32(divider, 8): 2^32 / (256 * divider) in FLOAT arithmetic, truncated
inline uint32_t scan_reduce_multiplier(int n) {
    const uint32_t max_dividend = (uint32_t)256 * (uint32_t)n;
    const float max_int = (float)(1 << 30) * 4.0f;
    return (uint32_t)(max_int / (float)max_dividend);
}

inline bool scan_side_ok(int v) { return v >= 1 && v <= SCAN_MAX_SIDE; }

}  // namespace

extern "C" int sis_scan_reduce(uint8_t* out, const uint8_t* page, int height, int width, int fx, int fy, void* stream) {
    SIS_REQUIRE(scan_side_ok(height) && scan_side_ok(width), "sis_scan_reduce: page %d x %d outside 1..%d", height, width, SCAN_MAX_SIDE);
    SIS_REQUIRE(fx >= 1 && fy >= 1 && (int64_t)fx * fy <= SCAN_MAX_BOX, "sis_scan_reduce: factors (%d, %d): both >= 1, product <= %d", fx, fy,
                SCAN_MAX_BOX);
    SIS_REQUIRE(out && page, "sis_scan_reduce: null pointer");
    const int out_w = sis_cdiv(width, fx), out_h = sis_cdiv(height, fy);
    const int rx = width - (out_w - 1) * fx, ry = height - (out_h - 1) * fy;   // 1..fx, 1..fy
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(sis_cdiv(out_w, SCAN_THREADS), out_h), dim3(SCAN_THREADS), 0, (hipStream_t)stream, out, page,
                       height, width, out_w, fx, fy, scan_reduce_multiplier(fx * fy), scan_reduce_multiplier(rx * fy),
                       scan_reduce_multiplier(fx * ry), scan_reduce_multiplier(rx * ry));
    SIS_CHECK_LAUNCH("scan_reduce_kernel");
    return 0;
}

extern "C" int64_t sis_scan_resample_workspace_bytes(int in_h, int in_w, int out_h, int out_w) {
    if (!scan_side_ok(in_h) || !scan_side_ok(in_w) || !scan_side_ok(out_h) || !scan_side_ok(out_w)) return 0;
    return (int64_t)in_h * scan_pitch(out_w);   // the horizontal pass's result: in_h rows of out_w pixels, rows padded to words
}

extern "C" int sis_scan_resample(uint8_t* out, const uint8_t* page, int in_h, int in_w, int out_h, int out_w, const int32_t* coef_x,
                                 const int32_t* first_x, const int32_t* count_x, int ksize_x, const int32_t* coef_y, const int32_t* first_y,
                                 const int32_t* count_y, int ksize_y, void* workspace, int64_t workspace_bytes, void* stream) {
    SIS_REQUIRE(scan_side_ok(in_h) && scan_side_ok(in_w) && scan_side_ok(out_h) && scan_side_ok(out_w),
                "sis_scan_resample: %d x %d -> %d x %d: every side must lie in 1..%d", in_h, in_w, out_h, out_w, SCAN_MAX_SIDE);
    SIS_REQUIRE(ksize_x >= 0 && ksize_x <= SCAN_MAX_TAPS && (ksize_x == 0 || (ksize_x & 1)),
                "sis_scan_resample: ksize_x %d: 0 (pass skipped) or odd and <= %d", ksize_x, SCAN_MAX_TAPS);
    SIS_REQUIRE(ksize_y >= 0 && ksize_y <= SCAN_MAX_TAPS && (ksize_y == 0 || (ksize_y & 1)),
                "sis_scan_resample: ksize_y %d: 0 (pass skipped) or odd and <= %d", ksize_y, SCAN_MAX_TAPS);
    SIS_REQUIRE(ksize_x > 0 || out_w == in_w, "sis_scan_resample: no horizontal pass, but width %d -> %d", in_w, out_w);
    SIS_REQUIRE(ksize_y > 0 || out_h == in_h, "sis_scan_resample: no vertical pass, but height %d -> %d", in_h, out_h);
    SIS_REQUIRE(out && page, "sis_scan_resample: null pointer");
    SIS_REQUIRE((ksize_x > 0) == (coef_x && first_x && count_x) && (ksize_x > 0 || !(coef_x || first_x || count_x)),
                "sis_scan_resample: the horizontal tables go with ksize_x > 0, all three or none");
    SIS_REQUIRE((ksize_y > 0) == (coef_y && first_y && count_y) && (ksize_y > 0 || !(coef_y || first_y || count_y)),
                "sis_scan_resample: the vertical tables go with ksize_y > 0, all three or none");
    const bool two = ksize_x > 0 && ksize_y > 0;
    if (two) {
        SIS_REQUIRE(workspace && (((uintptr_t)workspace) & 3) == 0, "sis_scan_resample: two passes need a 4-byte aligned workspace");
        SIS_REQUIRE(workspace_bytes >= sis_scan_resample_workspace_bytes(in_h, in_w, out_h, out_w),
                    "sis_scan_resample: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                    (long long)sis_scan_resample_workspace_bytes(in_h, in_w, out_h, out_w));
    }
    hipStream_t st = (hipStream_t)stream;
    if (ksize_x == 0 && ksize_y == 0) {   // Pillow returns a copy
        if (hipMemcpyAsync(out, page, (size_t)in_h * in_w * 3, hipMemcpyDeviceToDevice, st) != hipSuccess)
            return sis_fail("sis_scan_resample: cannot copy the page");
        return 0;
    }
    const uint8_t* mid = page;
    int64_t mid_pitch = 3 * (int64_t)in_w;
    if (ksize_x > 0) {
        uint8_t* h_out = two ? reinterpret_cast<uint8_t*>(workspace) : out;
        const int64_t h_pitch = two ? scan_pitch(out_w) : 3 * (int64_t)out_w;
        const size_t lds = (size_t)SCAN_TX * ksize_x * 4 + 2 * SCAN_TX * 4 + (size_t)SCAN_TY * scan_seg_bytes(ksize_x);
        hipLaunchKernelGGL(scan_hpass_kernel, dim3(sis_cdiv(out_w, SCAN_TX), sis_cdiv(in_h, SCAN_ROWS)), dim3(SCAN_THREADS), lds, st, h_out,
                           h_pitch, page, 3 * (int64_t)in_w, in_h, in_w, out_w, coef_x, first_x, count_x, ksize_x);
        SIS_CHECK_LAUNCH("scan_hpass_kernel");
        mid = h_out;
        mid_pitch = h_pitch;
    }
    if (ksize_y > 0) {
        const int row_bytes = 3 * out_w;
        const dim3 grid(sis_cdiv(sis_cdiv(row_bytes, 4), SCAN_THREADS), out_h);
        if (two)
            hipLaunchKernelGGL(scan_vpass_kernel<true>, grid, dim3(SCAN_THREADS), 0, st, out, (int64_t)row_bytes, mid, mid_pitch, in_h, row_bytes,
                               coef_y, first_y, count_y, ksize_y);
        else
            hipLaunchKernelGGL(scan_vpass_kernel<false>, grid, dim3(SCAN_THREADS), 0, st, out, (int64_t)row_bytes, mid, mid_pitch, in_h, row_bytes,
                               coef_y, first_y, count_y, ksize_y);
        SIS_CHECK_LAUNCH("scan_vpass_kernel");
    }
    return 0;
}

extern "C" int sis_scan_patches(uint8_t* out, const uint8_t* page, const int32_t* origins, int n, int size, int height, int width,
                                void* stream) {
    SIS_REQUIRE(scan_side_ok(height) && scan_side_ok(width), "sis_scan_patches: page %d x %d outside 1..%d", height, width, SCAN_MAX_SIDE);
    SIS_REQUIRE(n >= 1 && n <= 65535, "sis_scan_patches: %d windows outside 1..65535", n);
    SIS_REQUIRE(size >= 1 && size <= SCAN_MAX_PATCH, "sis_scan_patches: size %d outside 1..%d", size, SCAN_MAX_PATCH);
    SIS_REQUIRE(out && page && origins, "sis_scan_patches: null pointer");
    SIS_REQUIRE((((uintptr_t)out) & 3) == 0 && (((uintptr_t)origins) & 3) == 0, "sis_scan_patches: out and origins must be 4-byte aligned");
    const int64_t out_bytes = (int64_t)n * size * size * 3;
    const int64_t blocks = (out_bytes + 4 * SCAN_THREADS - 1) / (4 * SCAN_THREADS);
    SIS_REQUIRE(blocks < ((int64_t)1 << 31), "sis_scan_patches: %d windows of %d x %d in one call", n, size, size);
    hipLaunchKernelGGL(scan_patches_kernel, dim3((unsigned)blocks), dim3(SCAN_THREADS), 0, (hipStream_t)stream, out, out_bytes, page, origins,
                       size, height, width);
    SIS_CHECK_LAUNCH("scan_patches_kernel");
    return 0;
}
