// sis_seg_eval: one validation pass over a batch of segmentation logits and its labels.  Included by seg_ops.hip,
// after CeParams / interp_logits: the low-resolution route takes its logits from the function the training loss (ce_fwd_kernel)
// takes them from, with the same scales (the same source text: whether the compiler contracts its multiply-adds alike in the
// two kernels is not pinned by any test, so "the same bits" is not claimed).  The reference has no such pass: its evaluator hook
// is empty for the segmenters (training_builder/base_train_builder.py:64-65); tests/seg_eval_restatement.py restates the
// definitions in float64.
//
// Per output pixel: the C values v[c] (the stored element widened to float, or the align-corners bilinear value), the first
// maximal class, and with the label l
//   l in [0, C):  matrix[l][pred] += 1, counted += 1, ce += log(sum_c exp(v[c] - max)) + (max - v[l])   (two non-negative parts:
//                 nothing cancels where the softmax saturates)
//   otherwise:    ignored += 1
//   always:       I_c += p_c [l == c],  P_c += p_c^2;  T_c = number of pixels labelled c = row c of this workgroup's histogram.
//   seg_eval_kernel         a lane takes four consecutive pixels of one image at a time (16-byte loads where the plane size and
//                           the pointers allow, element loads otherwise) and adds its terms in double; the cells are counted in
//                           an LDS histogram by integer atomics and leave the workgroup as one 64-bit atomic per non-empty cell
//                           (integers: exact, any order); the floating sums leave it as one row of `partial`
//   seg_eval_finish_kernel  adds the rows in workgroup order onto `sums`: two calls give the same bits
// exp: expf of the float difference, corrected by the part of the difference the float subtraction rounded away, so its relative
// error does not grow with the distance from the maximum; everything after it (softmax sum, division, squares, sums) is double.
// Non-finite logits (a diverged network): unlike torch.argmax, which takes a NaN for the maximum, the comparison `v[c] > max` is
// false for a NaN, so the prediction is the first maximal class among the values before it / class 0; a NaN or an infinite
// maximum makes the pixel's terms NaN (inf - inf), so `sums` turns NaN while `counts` stays a well-formed matrix.

namespace {

constexpr int SE_MAXC = 16;
constexpr int SE_MAX_BLOCKS = 512;        // workgroups of a launch; more than 512 x 1024 pixels are walked with the grid's stride
constexpr int SE_FINISH_RANGES = 16;

template <typename T, int C, bool LOW>
__global__ __launch_bounds__(256) void seg_eval_kernel(unsigned long long* __restrict__ counts, double* __restrict__ partial,
                                                       const T* __restrict__ logits, const long* __restrict__ labels,
                                                       CeParams p, int vec) {
    constexpr int NV = 1 + 2 * C;   // per lane: ce, I_c, P_c
    __shared__ int hist[C * C + 1]; // the cells, then `ignored`
    __shared__ double red[4][NV];
    for (int i = threadIdx.x; i < C * C + 1; i += 256) hist[i] = 0;
    __syncthreads();
    p.C = C;                        // compile-time class count for interp_logits
    double acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.0;
    const int hw = p.H * p.W;
    const int quads_per_img = (hw + 3) >> 2;
    const long long quads = (long long)p.B * quads_per_img;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long long)gridDim.x * 256) {
        const int b = (int)(q / quads_per_img), pix = (int)(q - (long long)b * quads_per_img) * 4;
        const int n = min(4, hw - pix);
        long lab[4];
        float z[C][4];
        const long* lp = labels + (long long)b * hw + pix;
        if (vec) {
            const longlong2 l01 = *reinterpret_cast<const longlong2*>(lp), l23 = *reinterpret_cast<const longlong2*>(lp + 2);
            lab[0] = l01.x; lab[1] = l01.y; lab[2] = l23.x; lab[3] = l23.y;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) lab[e] = e < n ? lp[e] : -1;
        }
        if constexpr (LOW) {
            const float* xb = logits + (long long)b * C * p.h * p.w;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v[C];
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = 0.f;
                if (e < n) {
                    const int y = (pix + e) / p.W, xx = (pix + e) - y * p.W;
                    interp_logits(xb, p, sis_lerp_index(y, p.sy, p.h), sis_lerp_index(xx, p.sx, p.w), v);
                }
#pragma unroll
                for (int c = 0; c < C; ++c) z[c][e] = v[c];
            }
        } else {
            const T* zb = logits + (long long)b * C * hw + pix;
            if (vec) {
#pragma unroll
                for (int c = 0; c < C; ++c) sis_load4(zb + (long long)c * hw, z[c]);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int e = 0; e < 4; ++e) z[c][e] = e < n ? (float)sis_ld(zb + (long long)c * hw, e) : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= n) break;
            float m = z[0][e];
            int pred = 0;
#pragma unroll
            for (int c = 1; c < C; ++c)
                if (z[c][e] > m) { m = z[c][e]; pred = c; }   // the first maximal class
            double ex[C], r = 0.0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float d = z[c][e] - m;
                const float d_lo = (float)(((double)z[c][e] - (double)m) - (double)d);   // what the float subtraction lost
                const float x = expf(d);
                ex[c] = (double)fmaf(x, d_lo, x);
                r += c == pred ? 0.0 : ex[c];     // the maximum's own term is exactly 1: kept out, for log1p
            }
            const double inv = 1.0 / (1.0 + r);
            const long l = lab[e];
            float zl = m;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double pc = ex[c] * inv;
                const bool hit = l == c;
                if (hit) zl = z[c][e];
                acc[1 + c] += hit ? pc : 0.0;
                acc[1 + C + c] += pc * pc;
            }
            if (l >= 0 && l < C) {
                acc[0] += (double)log1pf((float)r) + (double)(m - zl);
                atomicAdd(&hist[(int)l * C + pred], 1);
            } else {
                atomicAdd(&hist[C * C], 1);
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double v = acc[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();   // the histogram and the four waves' sums are complete
    const int t = threadIdx.x;
    double* row = partial + (long long)blockIdx.x * (1 + 3 * C);
    if (t < NV) {      // ORDER: (r0 + r1) + (r2 + r3); row layout = the layout of `sums`
        const int dst = t == 0 ? 0 : (t <= C ? 1 + 3 * (t - 1) : 2 + 3 * (t - 1 - C));
        row[dst] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    }
    if (t >= 64 && t < 64 + C) {   // T_c: the pixels labelled c, an integer
        int n_c = 0;
        for (int k = 0; k < C; ++k) n_c += hist[(t - 64) * C + k];
        row[3 + 3 * (t - 64)] = (double)n_c;
    }
    if (t == 128) {
        int counted = 0;
        for (int k = 0; k < C * C; ++k) counted += hist[k];
        if (counted) atomicAdd(&counts[C * C], (unsigned long long)counted);
        if (hist[C * C]) atomicAdd(&counts[C * C + 1], (unsigned long long)hist[C * C]);
    }
    if (t < C * C && hist[t] != 0) atomicAdd(&counts[t], (unsigned long long)hist[t]);
}

// sums[v] += sum over the workgroups' rows of partial[k][v]: SE_FINISH_RANGES contiguous ranges of rows, each added in order by
// one lane, then the range sums in order -- a fixed association
__global__ __launch_bounds__(1024) void seg_eval_finish_kernel(double* __restrict__ sums, const double* __restrict__ partial,
                                                               int blocks, int nv) {
    __shared__ double part[SE_FINISH_RANGES][64];
    const int v = threadIdx.x & 63, r = threadIdx.x >> 6;
    const int per = (blocks + SE_FINISH_RANGES - 1) / SE_FINISH_RANGES, k0 = r * per, k1 = min(blocks, k0 + per);
    double s = 0.0;
    if (v < nv)
        for (int k = k0; k < k1; ++k) s += partial[(long long)k * nv + v];
    part[r][v] = s;
    __syncthreads();
    if ((int)threadIdx.x < nv) {
        double t = 0.0;
        for (int j = 0; j < SE_FINISH_RANGES; ++j) t += part[j][threadIdx.x];
        sums[threadIdx.x] += t;
    }
}

int seg_eval_blocks(int batch, int out_h, int out_w) {
    const long long quads = (long long)batch * (((long long)out_h * out_w + 3) / 4);
    return (int)(quads < (long long)SE_MAX_BLOCKS * 256 ? (quads + 255) / 256 : SE_MAX_BLOCKS);
}

bool seg_eval_sizes_ok(int batch, int classes, int out_h, int out_w) {
    return classes >= 2 && classes <= SE_MAXC && batch >= 1 && out_h >= 1 && out_w >= 1 &&
           (long long)out_h * out_w <= (1ll << 30) &&
           (long long)batch * out_h * out_w <= (1ll << 39);  // a workgroup's histogram counts in int: at most 2^39 / 512 = 2^30
                                                             // pixels per workgroup, were they all in one cell
}

}  // namespace

extern "C" int64_t sis_seg_eval_workspace_bytes(int batch, int classes, int out_h, int out_w) {
    if (!seg_eval_sizes_ok(batch, classes, out_h, out_w)) return 0;
    return (int64_t)seg_eval_blocks(batch, out_h, out_w) * (1 + 3 * classes) * (int64_t)sizeof(double);
}

#define SE_SWITCH_C(CV, CALL)                                                                                            \
    switch (CV) {                                                                                                        \
        case 2: { constexpr int C = 2; CALL; } break;                                                                    \
        case 3: { constexpr int C = 3; CALL; } break;                                                                    \
        case 4: { constexpr int C = 4; CALL; } break;                                                                    \
        case 5: { constexpr int C = 5; CALL; } break;                                                                    \
        case 6: { constexpr int C = 6; CALL; } break;                                                                    \
        case 7: { constexpr int C = 7; CALL; } break;                                                                    \
        case 8: { constexpr int C = 8; CALL; } break;                                                                    \
        case 9: { constexpr int C = 9; CALL; } break;                                                                    \
        case 10: { constexpr int C = 10; CALL; } break;                                                                  \
        case 11: { constexpr int C = 11; CALL; } break;                                                                  \
        case 12: { constexpr int C = 12; CALL; } break;                                                                  \
        case 13: { constexpr int C = 13; CALL; } break;                                                                  \
        case 14: { constexpr int C = 14; CALL; } break;                                                                  \
        case 15: { constexpr int C = 15; CALL; } break;                                                                  \
        case 16: { constexpr int C = 16; CALL; } break;                                                                  \
        default: return sis_fail("sis_seg_eval: %d classes outside 2..%d", (CV), SE_MAXC);                               \
    }

extern "C" int sis_seg_eval(int64_t* counts, double* sums, void* workspace, const void* logits, int dtype, const int64_t* labels,
                            int batch, int classes, int h, int w, int out_h, int out_w, void* stream) {
    SIS_REQUIRE(counts && sums && workspace && logits && labels, "sis_seg_eval: null pointer");
    SIS_REQUIRE(classes >= 2 && classes <= SE_MAXC, "sis_seg_eval: %d classes outside 2..%d", classes, SE_MAXC);
    SIS_REQUIRE(seg_eval_sizes_ok(batch, classes, out_h, out_w), "sis_seg_eval: batch %d, output %d x %d out of range", batch,
                out_h, out_w);
    SIS_REQUIRE(h >= 1 && w >= 1 && h <= out_h && w <= out_w, "sis_seg_eval: logits %d x %d do not fit the output %d x %d", h, w,
                out_h, out_w);
    const bool low = h != out_h || w != out_w;
    SIS_REQUIRE(dtype == SIS_F32 || (dtype == SIS_BF16 && !low),
                "sis_seg_eval: logits must be float32, or bfloat16 at the size of the labels (dtype code %d, %d x %d -> %d x %d)",
                dtype, h, w, out_h, out_w);
    SIS_REQUIRE((uintptr_t)workspace % 8 == 0 && (uintptr_t)sums % 8 == 0 && (uintptr_t)counts % 8 == 0 && (uintptr_t)labels % 8 == 0,
                "sis_seg_eval: counts, sums, workspace and labels must be 8-byte aligned");
    CeParams p;
    if (ce_setup(p, batch, classes, h, w, out_h, out_w, -1)) return 1;   // the scales sis_upsample_ce_fwd computes
    const int hw = out_h * out_w;
    const int elem = dtype == SIS_F32 ? 4 : 2;
    const int vec = hw % 4 == 0 && (uintptr_t)labels % 16 == 0 && (low || (uintptr_t)logits % (4 * elem) == 0);
    const int blocks = seg_eval_blocks(batch, out_h, out_w);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* cnt = (unsigned long long*)counts;
    double* partial = (double*)workspace;
    if (low) {
        SE_SWITCH_C(classes, hipLaunchKernelGGL((seg_eval_kernel<float, C, true>), dim3(blocks), dim3(256), 0, st, cnt, partial,
                                                (const float*)logits, (const long*)labels, p, vec))
    } else if (dtype == SIS_F32) {
        SE_SWITCH_C(classes, hipLaunchKernelGGL((seg_eval_kernel<float, C, false>), dim3(blocks), dim3(256), 0, st, cnt, partial,
                                                (const float*)logits, (const long*)labels, p, vec))
    } else {
        SE_SWITCH_C(classes, hipLaunchKernelGGL((seg_eval_kernel<__hip_bfloat16, C, false>), dim3(blocks), dim3(256), 0, st, cnt,
                                                partial, (const __hip_bfloat16*)logits, (const long*)labels, p, vec))
    }
    SIS_CHECK_LAUNCH("seg_eval_kernel");
    hipLaunchKernelGGL(seg_eval_finish_kernel, dim3(1), dim3(1024), 0, st, sums, (const double*)partial, blocks, 1 + 3 * classes);
    SIS_CHECK_LAUNCH("seg_eval_finish_kernel");
    return 0;
}
