// Fitting spherical k-means activation catalogs on the device: the arithmetic of the reference's
// MiniBatchSphericalKMeans.fit (segmentation/gan_local_edit/spherical_kmeans.py:161-312, the mini-batch step :36-156) on
// activations that stay in the generator's NCHW layout.
//  * skm_gather_kernel    index list -> contiguous unit rows (validation / init rows, a chunk of planned mini-batch rows)
//  * skm_loop_kernel      one workgroup per fit, up to T mini-batch iterations per launch, centres and counts in LDS
//  * skm_label_kernel     labels, inertia and per-centre pixel counts over all pixels in one read of the activation
//  * skm_label_finish_kernel   adds the per-workgroup partials in a fixed order
// Everything is deterministic: no floating-point atomics, partial sums are added in a fixed order that depends on the shape only.
#include "sis_device.h"

#include <type_traits>

#define SKM_KMAX 32
#define SKM_CMAX 512
#define SKM_BMAX 256
#define SKM_STATE 40   // doubles per fit
// state layout (doubles; the integers among them are small and exact)
enum { SKM_EWA = 0, SKM_EWA_MIN = 1, SKM_T = 2, SKM_NOIMP = 3, SKM_DONE = 4, SKM_INERTIA = 5, SKM_K = 6, SKM_HAS_EWA = 7, SKM_COUNTS = 8 };
#define SKM_CS 33      // LDS row stride of the [channel][centre] image: lanes along the centres AND lanes along the channels are conflict-free

// ------------------------------------------------------------------------------------------------------------- gather
// One wave per listed pixel: row n = (b HW + p) of partial_flat(x) -> out[row][0..C) = x[b, :, p] / |x[b, :, p]| (a zero row stays
// zero).  The squares are summed in double (lane partials in channel order, then a butterfly: the same value in every lane).
__global__ __launch_bounds__(256) void skm_gather_kernel(float* __restrict__ out, const float* __restrict__ x,
                                                         const int* __restrict__ idx, int64_t n_rows, int C, int HW, int64_t N) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    int64_t n = idx[row];
    n = n < 0 ? 0 : (n >= N ? N - 1 : n);   // (the host checks the plan; never read out of bounds)
    const int64_t b = n / HW, p = n - b * HW;
    const float* xp = x + b * C * HW + p;
    float v[SKM_CMAX / 64];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < SKM_CMAX / 64; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < C ? xp[(int64_t)c * HW] : 0.f;
        s += (double)v[i] * (double)v[i];
    }
    s = sis_wave_sum(s);
    const double inv = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
#pragma unroll
    for (int i = 0; i < SKM_CMAX / 64; ++i) {
        const int c = lane + 64 * i;
        if (c < C) out[row * C + c] = (float)((double)v[i] * inv);
    }
}

// ------------------------------------------------------------------------------------------------------ mini-batch loop
// Normalise the centres in LDS: thread (j = tid & 31, part = tid >> 5) owns the channels c = part (mod 8) of centre j.  Returns
// with the scaled centres and, in part2, the partial squared norms of the SCALED centres written but not yet published (the
// caller's barrier does that).
__device__ __forceinline__ void skm_normalise(float* cen, double* part, double* part2, int C) {
    const int j = threadIdx.x & 31, p = threadIdx.x >> 5;
    double s = 0.0;
    for (int c = p; c < C; c += 8) {
        const double v = cen[c * SKM_CS + j];
        s += v * v;
    }
    part[p * 32 + j] = s;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) tot += part[q * 32 + j];
    const double scale = tot > 0.0 ? 1.0 / sqrt(tot) : 1.0;
    double s2 = 0.0;
    for (int c = p; c < C; c += 8) {
        const float v = (float)((double)cen[c * SKM_CS + j] * scale);
        cen[c * SKM_CS + j] = v;
        s2 += (double)v * (double)v;
    }
    part2[p * 32 + j] = s2;
}

// One workgroup per fit.  rows: [T][batch][C] unit rows of the planned mini-batches of this chunk, picks: [T][32] distinct
// mini-batch positions per iteration (used by a reassignment only).  Every loop is bounded by T, batch or 32; there is no waiting
// on another workgroup.  Per iteration (the contract of DESIGN.md §9): normalise, nearest centre per row (matrix cores: the
// [32 centres] x [32 rows] tile of v_mfma_f32_32x32x2_f32, one wave per 32 rows), reassignment rule, per-centre update,
// normalise, convergence bookkeeping.  Counts, sums over members, norms and the stop rule are kept in double.
__global__ __launch_bounds__(256) void skm_loop_kernel(double* __restrict__ state, float* __restrict__ centres,
                                                       int* __restrict__ last_labels, const float* __restrict__ rows,
                                                       const int* __restrict__ picks, int C, int batch, int T, double alpha,
                                                       int max_no_imp, double ratio, int64_t max_iterations) {
    extern __shared__ __attribute__((aligned(16))) float skm_lds[];
    float* cen = skm_lds;                                                       // [C][33]
    double* part = reinterpret_cast<double*>(cen + ((C * SKM_CS + 3) & ~3));    // [8][32]
    double* part2 = part + 256;                                                 // [8][32]
    double* cnt = part2 + 256;                                                  // [32]
    double* red = cnt + 32;                                                     // [8]: [0] inertia of the mini-batch
    double* ccl = red + 8;                                                      // [32] squared norms of the centres
    double* dmin = ccl + 32;                                                    // [256]
    int* lab = reinterpret_cast<int*>(dmin + SKM_BMAX);                         // [256]
    int* order = lab + SKM_BMAX;                                                // [256] rows sorted by label (stable)
    int* slab = order + SKM_BMAX;                                               // [256] their labels
    int* wj = slab + SKM_BMAX;                                                  // [32] members per centre
    int* flag = wj + 32;                                                        // [32] centre is replaced in this iteration
    int* pickrow = flag + 32;                                                   // [32] by this row of the mini-batch
    int* ctl = pickrow + 32;                                                    // [0] stop after this iteration

    const int f = blockIdx.x, tid = threadIdx.x;
    double* st = state + (int64_t)f * SKM_STATE;
    if (st[SKM_DONE] != 0.0) return;   // (uniform: a finished fit is skipped)
    const int K = (int)st[SKM_K];
    if (K < 1 || K > SKM_KMAX) return;
    float* cg = centres + (int64_t)f * SKM_KMAX * C;
    for (int e = tid; e < SKM_KMAX * C; e += 256) {
        const int j = e / C, c = e - j * C;
        cen[c * SKM_CS + j] = j < K ? cg[e] : 0.f;
    }
    if (tid < 32) cnt[tid] = tid < K ? st[SKM_COUNTS + tid] : 0.0;
    if (tid == 0) ctl[0] = 0;
    const int64_t t0 = (int64_t)st[SKM_T];
    double ewa = st[SKM_EWA], ewa_min = st[SKM_EWA_MIN], noimp = st[SKM_NOIMP], last_inertia = st[SKM_INERTIA];   // (thread 0's are used)
    bool has_ewa = st[SKM_HAS_EWA] != 0.0;
    bool finished = false;
    int64_t t_next = t0;
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int ntiles = (batch + 31) >> 5;
    for (int s = 0; s < T; ++s) {
        const float* xb = rows + (int64_t)s * batch * C;
        const int64_t t = t0 + s;
        // ---- normalise; squared norms of the unit centres
        skm_normalise(cen, part, part2, C);
        __syncthreads();
        if (tid < 32) {
            double tot = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) tot += part2[q * 32 + tid];
            ccl[tid] = tot;
        }
        // ---- distances on the matrix cores: S[centre][row] = sum_c cen[c][centre] x[row][c]; a lane's 16-byte load of channels
        // c0 + 4 half .. + 3 of its row feeds four MFMAs (channel pair (c0 + e, c0 + 4 + e) in step e: A is read to match)
        sis_f32x16 acc[2];
        float xx[2] = {0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int tile = wave + 4 * u;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[u][i] = 0.f;
            if (tile < ntiles) {   // (wave-uniform)
                const int row = tile * 32 + l31;
                const float* xr = xb + (int64_t)(row < batch ? row : batch - 1) * C + 4 * half;
                const float* ar = cen + (4 * half) * SKM_CS + l31;
                sis_f32x4 ring[4];   // four loads in flight (the rows come from L2)
#pragma unroll
                for (int q = 0; q < 4; ++q) ring[q] = *reinterpret_cast<const sis_f32x4*>(xr + (8 * q < C ? 8 * q : C - 8));
                for (int c0 = 0; c0 < C; c0 += 32) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = c0 + 8 * q;
                        if (c < C) {   // (uniform)
                            const sis_f32x4 v = ring[q];
                            ring[q] = *reinterpret_cast<const sis_f32x4*>(xr + (c + 32 < C ? c + 32 : C - 8));
                            acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[(c + 0) * SKM_CS], v.x, acc[u], 0, 0, 0);
                            acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[(c + 1) * SKM_CS], v.y, acc[u], 0, 0, 0);
                            acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[(c + 2) * SKM_CS], v.z, acc[u], 0, 0, 0);
                            acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[(c + 3) * SKM_CS], v.w, acc[u], 0, 0, 0);
                            xx[u] = fmaf(v.x, v.x, xx[u]); xx[u] = fmaf(v.y, v.y, xx[u]); xx[u] = fmaf(v.z, v.z, xx[u]); xx[u] = fmaf(v.w, v.w, xx[u]);
                        }
                    }
                }
            }
        }
        __syncthreads();   // ccl
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int tile = wave + 4 * u;
            if (tile < ntiles) {
                const double xxr = (double)(xx[u] + __shfl_xor(xx[u], 32, 64));
                double d1 = __builtin_inf();
                int arg = 0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int k = (i & 3) + 8 * (i >> 2) + 4 * half;   // this register's centre (ascending in i)
                    if (k < K) {
                        const double d = fmax(xxr - 2.0 * (double)acc[u][i] + ccl[k], 0.0);
                        if (d < d1) { d1 = d; arg = k; }
                    }
                }
                const double p1 = __shfl_xor(d1, 32, 64);
                const int pa = __shfl_xor(arg, 32, 64);
                if (p1 < d1 || (p1 == d1 && pa < arg)) { d1 = p1; arg = pa; }   // ties: lowest index
                const int row = tile * 32 + l31;
                if (half == 0 && row < batch) { lab[row] = arg; dmin[row] = d1; }
            }
        }
        __syncthreads();
        // ---- members per centre, rank of every row among the rows of its label, inertia of the mini-batch
        int rank = 0, w = 0;
        {
            const int mine = tid < batch ? lab[tid] : -1;
            for (int i = 0; i < batch; ++i) {
                const int l = lab[i];
                rank += (l == mine) & (i < tid);
                w += (l == tid);
            }
            if (tid < 32) wj[tid] = w;
            if (wave == 1) {   // rows lane, lane + 64, ... in order, then a butterfly
                double e = 0.0;
                for (int i = lane; i < batch; i += 64) e += dmin[i];
                e = sis_wave_sum(e);
                if (lane == 0) red[0] = e;
            }
        }
        __syncthreads();
        if (tid < batch) {
            const int mine = lab[tid];
            int start = 0;
            for (int j = 0; j < mine; ++j) start += wj[j];
            order[start + rank] = tid;
            slab[start + rank] = mine;
            last_labels[(int64_t)f * SKM_BMAX + tid] = mine;
        }
        if (tid == 255) {   // the reassignment rule (spherical_kmeans.py:66-93), counts in double
            double cmin = cnt[0], cmax = cnt[0];
            for (int j = 1; j < K; ++j) { cmin = fmin(cmin, cnt[j]); cmax = fmax(cmax, cnt[j]); }
            const bool reassign = ratio > 0.0 && ((t + 1) % (10 + (int64_t)cmin) == 0);
            unsigned mask = 0;
            if (reassign) {
                const int cap = batch / 2;   // int(.5 * batch)
                int n_to = 0, nr = 0;
                for (int j = 0; j < K; ++j)
                    if (cnt[j] < ratio * cmax) { mask |= 1u << j; ++n_to; }
                if (n_to > cap) {   // keep the `cap` lowest counts (ordered by count, then index)
                    for (int j = 0; j < K; ++j) {
                        int r = 0;
                        for (int i = 0; i < K; ++i) r += (cnt[i] < cnt[j]) || (cnt[i] == cnt[j] && i < j);
                        if (r >= cap) mask &= ~(1u << j);
                    }
                }
                double others = __builtin_inf();
                for (int j = 0; j < K; ++j)
                    if (!((mask >> j) & 1)) others = fmin(others, cnt[j]);
                for (int j = 0; j < K; ++j)
                    if ((mask >> j) & 1) {
                        const int pr = picks[(int64_t)s * 32 + nr];
                        pickrow[j] = pr < 0 ? 0 : (pr >= batch ? batch - 1 : pr);
                        cnt[j] = others;
                        ++nr;
                    }
            }
            for (int j = 0; j < 32; ++j) flag[j] = (mask >> j) & 1;
        }
        __syncthreads();
        // ---- replacement, then the per-centre update with the labels computed BEFORE the replacement; thread per channel
        for (int c = tid; c < C; c += 256) {
            for (int j = 0; j < K; ++j)
                if (flag[j]) cen[c * SKM_CS + j] = xb[(int64_t)pickrow[j] * C + c];
            double S = 0.0;
            int cur = -1;
            for (int p0 = 0; p0 < batch; p0 += 16) {
                float v[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int p = p0 + q < batch ? p0 + q : batch - 1;
                    v[q] = xb[(int64_t)order[p] * C + c];
                }
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    if (p0 + q < batch) {
                        const int j = slab[p0 + q];
                        if (j != cur) {
                            if (cur >= 0)
                                cen[c * SKM_CS + cur] = (float)(((double)cen[c * SKM_CS + cur] * cnt[cur] + S) / (cnt[cur] + (double)wj[cur]));
                            cur = j;
                            S = 0.0;
                        }
                        S += (double)v[q];
                    }
                }
            }
            if (cur >= 0) cen[c * SKM_CS + cur] = (float)(((double)cen[c * SKM_CS + cur] * cnt[cur] + S) / (cnt[cur] + (double)wj[cur]));
        }
        __syncthreads();
        if (tid < 32) cnt[tid] += (double)wj[tid];
        // ---- normalise, stop rule (the reference's _mini_batch_convergence with tol = 0)
        skm_normalise(cen, part, part2, C);
        if (tid == 0) {
            const double e = red[0] / (double)batch;
            ewa = has_ewa ? ewa * (1.0 - alpha) + e * alpha : e;
            if (!has_ewa || ewa < ewa_min) { ewa_min = ewa; noimp = 0.0; }
            else noimp += 1.0;
            has_ewa = true;
            last_inertia = red[0];
            t_next = t + 1;
            if (noimp >= (double)max_no_imp || t + 1 >= max_iterations) { finished = true; ctl[0] = 1; }
        }
        __syncthreads();
        if (ctl[0]) break;   // (uniform)
    }
    for (int e = tid; e < K * C; e += 256) {
        const int j = e / C, c = e - j * C;
        cg[e] = cen[c * SKM_CS + j];
    }
    if (tid < 32) st[SKM_COUNTS + tid] = cnt[tid];
    if (tid == 0) {
        st[SKM_EWA] = ewa; st[SKM_EWA_MIN] = ewa_min; st[SKM_NOIMP] = noimp; st[SKM_INERTIA] = last_inertia;
        st[SKM_HAS_EWA] = has_ewa ? 1.0 : 0.0; st[SKM_T] = (double)t_next; st[SKM_DONE] = finished ? 1.0 : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------------ full label pass
// Pixels x centres x channels on v_mfma_f32_32x32x2_f32 with the centres staged [C][32] (zero beyond K) as kmeans_mfma_kernel of
// dataset_ops.hip stages them; a wave tile is 128 consecutive rows of partial_flat(x).  VEC = 4: a lane loads four consecutive
// pixels of one channel (HW % 4 == 0), VEC = 1: four pixels 32 apart (any HW).  Epilogue per pixel: score_k = x.c_k / |x| - |c_k|^2 / 2,
// label = argmax (lowest index on ties), inertia term |xhat|^2 - 2 x.c / |x| + |c|^2 (clipped at 0), one count for the label.
template <int VEC, int U>
__global__ __launch_bounds__(256) void skm_label_kernel(int64_t* __restrict__ labels, double* __restrict__ ws,
                                                        const float* __restrict__ x, const float* __restrict__ centres, int C,
                                                        int HW, int K, int64_t N, int64_t tiles) {
    extern __shared__ __attribute__((aligned(16))) float skm_cen[];   // [C][32]; doubles: [8][32] partial, [32] squared norms, [4]; [32] counts
    double* ccp = reinterpret_cast<double*>(skm_cen + C * 32);
    double* ccl = ccp + 8 * 32;
    double* lred = ccl + 32;
    int* lcount = reinterpret_cast<int*>(lred + 4);
    for (int e = threadIdx.x; e < C * 32; e += 256) {
        const int c = e >> 5, k = e & 31;
        skm_cen[e] = k < K ? centres[(int64_t)k * C + c] : 0.f;
    }
    if (threadIdx.x < 32) lcount[threadIdx.x] = 0;
    __syncthreads();
    {
        const int k = threadIdx.x & 31, part = threadIdx.x >> 5;
        double s = 0.0;
        for (int c = part; c < C; c += 8) s += (double)skm_cen[c * 32 + k] * (double)skm_cen[c * 32 + k];
        ccp[part * 32 + k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        double s = 0.0;
        for (int p = 0; p < 8; ++p) s += ccp[p * 32 + threadIdx.x];
        ccl[threadIdx.x] = s;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, half = lane >> 5;
    const float* ab = skm_cen + half * 32 + l31;
    double inertia = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < tiles; t += (int64_t)gridDim.x * 4) {
        // this lane's four pixels and where their channel `half` lies
        int64_t n[4];
        const float* xp[4];
        bool valid[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            n[j] = t * 128 + (VEC == 4 ? 4 * l31 + j : 32 * j + l31);
            valid[j] = n[j] < N;
            const int64_t nn = valid[j] ? n[j] : 0;
            const int64_t b = nn / HW, p = nn - b * HW;
            xp[j] = x + (b * C + half) * HW + p;
        }
        sis_f32x16 acc[4];
        float xx[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
        sis_f32x4 xs[2][U];
        auto request = [&](auto setc, int c0) {
            constexpr int S = decltype(setc)::value;
#pragma unroll
            for (int s = 0; s < U; ++s) {
                const int64_t off = (int64_t)(c0 + 2 * s) * HW;
                if (VEC == 4) xs[S][s] = *reinterpret_cast<const sis_f32x4*>(xp[0] + off);
                else xs[S][s] = sis_f32x4{xp[0][off], xp[1][off], xp[2][off], xp[3][off]};
            }
        };
        auto block = [&](auto setc, int c0) {
            constexpr int S = decltype(setc)::value;
            request(std::integral_constant<int, S ^ 1>(), c0 + 2 * U < C ? c0 + 2 * U : c0);   // (past the end: this block again, unused)
#pragma unroll
            for (int s = 0; s < U; ++s) {
                const float a = ab[(c0 + 2 * s) * 32];
                const sis_f32x4 v = xs[S][s];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v.y, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v.z, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v.w, acc[3], 0, 0, 0);
                xx[0] = fmaf(v.x, v.x, xx[0]); xx[1] = fmaf(v.y, v.y, xx[1]); xx[2] = fmaf(v.z, v.z, xx[2]); xx[3] = fmaf(v.w, v.w, xx[3]);
            }
        };
        request(std::integral_constant<int, 0>(), 0);
        for (int c0 = 0; c0 < C; c0 += 4 * U) {   // C % (2 U) == 0 (host-checked); an odd number of blocks ends after the first
            block(std::integral_constant<int, 0>(), c0);
            if (c0 + 2 * U < C) block(std::integral_constant<int, 1>(), c0 + 2 * U);
        }
        int64_t lab[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xxj = xx[j] + __shfl_xor(xx[j], 32, 64);
            const double inv = xxj > 0.f ? 1.0 / sqrt((double)xxj) : 0.0;
            double best = -__builtin_inf(), bdot = 0.0;
            int arg = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int k = (i & 3) + 8 * (i >> 2) + 4 * half;   // this register's centre (ascending in i)
                if (k < K) {
                    const double dot = (double)acc[j][i] * inv;
                    const double sc = dot - 0.5 * ccl[k];
                    if (sc > best) { best = sc; arg = k; bdot = dot; }
                }
            }
            const double pb = __shfl_xor(best, 32, 64), pd = __shfl_xor(bdot, 32, 64);
            const int pa = __shfl_xor(arg, 32, 64);
            if (pb > best || (pb == best && pa < arg)) { best = pb; arg = pa; bdot = pd; }
            lab[j] = arg;
            if (half == 0 && valid[j]) {
                inertia += fmax((xxj > 0.f ? 1.0 : 0.0) - 2.0 * bdot + ccl[arg], 0.0);
                atomicAdd(&lcount[arg], 1);   // (integer: the order does not matter)
            }
        }
        if (half == 0) {
            if (VEC == 4) {
                if (valid[0]) {   // N % 4 == 0: the four are valid together
                    *reinterpret_cast<sis_i64x2*>(labels + n[0]) = sis_i64x2{lab[0], lab[1]};
                    *reinterpret_cast<sis_i64x2*>(labels + n[0] + 2) = sis_i64x2{lab[2], lab[3]};
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (valid[j]) labels[n[j]] = lab[j];
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) inertia += __shfl_xor(inertia, off, 64);   // written out: a call of sis_wave_sum here changes the generated code
    if (lane == 0) lred[wave] = inertia;
    __syncthreads();
    double* out = ws + (int64_t)blockIdx.x * 33;
    if (threadIdx.x == 0) out[0] = ((lred[0] + lred[1]) + lred[2]) + lred[3];
    if (threadIdx.x < 32) out[1 + threadIdx.x] = (double)lcount[threadIdx.x];
}

// result[0] = inertia, result[1 + k] = pixels of centre k.  One wave per result: lane l adds the partials of the workgroups
// l, l + 64, ... in that order, then a butterfly over the lanes -- a fixed order for a given number of workgroups.
__global__ __launch_bounds__(64) void skm_label_finish_kernel(double* __restrict__ result, const double* __restrict__ ws, int blocks) {
    const int i = blockIdx.x, lane = threadIdx.x;
    double s = 0.0;
    for (int b = lane; b < blocks; b += 64) s += ws[(int64_t)b * 33 + i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);   // written out: a call of sis_wave_sum here changes the generated code
    if (lane == 0) result[i] = s;
}

static int skm_label_blocks(int64_t n_pixels) {
    const int64_t tiles = (n_pixels + 127) / 128;
    const int64_t want = (tiles + 3) / 4;
    return (int)(want < 1 ? 1 : (want > 1024 ? 1024 : want));
}

static int skm_check_shape(const char* who, int64_t n_pixels, int C, int K) {
    SIS_REQUIRE(K >= 1 && K <= SKM_KMAX, "%s: %d centres (1 .. %d are supported)", who, K, SKM_KMAX);
    SIS_REQUIRE(C >= 8 && C <= SKM_CMAX && C % 8 == 0, "%s: %d channels (a multiple of 8 up to %d is supported)", who, C, SKM_CMAX);
    SIS_REQUIRE(n_pixels >= 1 && n_pixels < ((int64_t)1 << 31), "%s: %lld pixels (1 .. 2^31 - 1 are supported)", who, (long long)n_pixels);
    return 0;
}

template <int VEC, int U>
static int skm_launch_label(int64_t* labels, double* ws, const float* x, const float* centres, int C, int HW, int K, int64_t N,
                            hipStream_t st) {
    const size_t lds = (size_t)(C * 32 + 32) * 4 + (8 * 32 + 32 + 4) * 8;
    static bool raised = false;
    if (lds > 48 * 1024 && !raised) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&skm_label_kernel<VEC, U>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        if (e != hipSuccess) return sis_fail("sis_skm_label: cannot raise the LDS limit: %s", hipGetErrorString(e));
        raised = true;
    }
    const int64_t tiles = (N + 127) / 128;
    const int blocks = skm_label_blocks(N);
    SIS_OCC_REPORT((skm_label_kernel<VEC, U>), 256, lds);
    hipLaunchKernelGGL((skm_label_kernel<VEC, U>), dim3(blocks), dim3(256), lds, st, labels, ws, x, centres, C, HW, K, N, tiles);
    SIS_CHECK_LAUNCH("skm_label_kernel");
    return 0;
}

extern "C" {

int sis_skm_state_doubles(void) { return SKM_STATE; }

int sis_skm_gather(float* out, const float* x, const int* idx, int64_t n_rows, int batch, int channels, int hw, void* stream) {
    SIS_REQUIRE(batch >= 1 && hw >= 1, "sis_skm_gather: empty activation");
    const int64_t N = (int64_t)batch * hw;
    if (skm_check_shape("sis_skm_gather", N, channels, 1)) return 1;
    SIS_REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 31) / 4, "sis_skm_gather: %lld rows", (long long)n_rows);
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(skm_gather_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, out, x, idx, n_rows,
                       channels, hw, N);
    SIS_CHECK_LAUNCH("skm_gather_kernel");
    return 0;
}

int sis_skm_loop(double* state, float* centres, int* last_labels, const float* rows, const int* picks, int n_fits, int channels,
                 int batch_size, int iters, double alpha, int max_no_improvement, double reassignment_ratio, int64_t max_iterations,
                 void* stream) {
    if (skm_check_shape("sis_skm_loop", 1, channels, 1)) return 1;
    SIS_REQUIRE(batch_size >= 1 && batch_size <= SKM_BMAX, "sis_skm_loop: batch_size %d (1 .. %d are supported)", batch_size, SKM_BMAX);
    SIS_REQUIRE(n_fits >= 1 && n_fits <= 65535, "sis_skm_loop: %d fits", n_fits);
    SIS_REQUIRE(iters >= 1 && iters <= 4096, "sis_skm_loop: %d iterations per launch (1 .. 4096)", iters);
    SIS_REQUIRE(max_no_improvement >= 1 && max_iterations >= 1, "sis_skm_loop: max_no_improvement and max_iterations must be positive");
    const size_t lds = (size_t)((channels * SKM_CS + 3) & ~3) * 4 + (256 + 256 + 32 + 8 + 32 + SKM_BMAX) * 8 +
                       (3 * SKM_BMAX + 32 * 3 + 4) * 4;
    static bool raised = false;
    if (!raised) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&skm_loop_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           96 * 1024);
        if (e != hipSuccess) return sis_fail("sis_skm_loop: cannot raise the LDS limit: %s", hipGetErrorString(e));
        raised = true;
    }
    hipLaunchKernelGGL(skm_loop_kernel, dim3(n_fits), dim3(256), lds, (hipStream_t)stream, state, centres, last_labels, rows, picks,
                       channels, batch_size, iters, alpha, max_no_improvement, reassignment_ratio, max_iterations);
    SIS_CHECK_LAUNCH("skm_loop_kernel");
    return 0;
}

int64_t sis_skm_label_workspace_doubles(int64_t n_pixels) { return (int64_t)skm_label_blocks(n_pixels) * 33; }

int sis_skm_label(int64_t* labels, double* result, double* workspace, const float* x, const float* centres, int batch, int channels,
                  int hw, int n_centres, void* stream) {
    SIS_REQUIRE(batch >= 1 && hw >= 1, "sis_skm_label: empty activation");
    const int64_t N = (int64_t)batch * hw;
    if (skm_check_shape("sis_skm_label", N, channels, n_centres)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = hw % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)labels & 15) == 0;
    int rc;
    if (vec) rc = channels % 16 == 0 ? skm_launch_label<4, 8>(labels, workspace, x, centres, channels, hw, n_centres, N, st)
                                     : skm_launch_label<4, 4>(labels, workspace, x, centres, channels, hw, n_centres, N, st);
    else rc = channels % 16 == 0 ? skm_launch_label<1, 8>(labels, workspace, x, centres, channels, hw, n_centres, N, st)
                                 : skm_launch_label<1, 4>(labels, workspace, x, centres, channels, hw, n_centres, N, st);
    if (rc) return rc;
    hipLaunchKernelGGL(skm_label_finish_kernel, dim3(33), dim3(64), 0, st, result, workspace, skm_label_blocks(N));
    SIS_CHECK_LAUNCH("skm_label_finish_kernel");
    return 0;
}

}  // extern "C"
