// DatasetGAN training: one optimisation step of every member of a PixelEnsembleClassifier (reference
// networks/pixel_classifier/model.py:124-171, updater/dataset_gan_updater.py) on P pixels drawn from resident generator
// activations.  Included by pixel_ensemble.hip (inside its anonymous namespace, after pe_bilinear_src and PE_KC).
//
// Narrow members only: Linear(F, 128) ReLU BatchNorm1d Linear(128, 32) ReLU BatchNorm1d Linear(32, C), C < 32.  The members
// are batched along the column axis: M = N * 128 first-layer outputs, N * 32 second-layer outputs.  No launch count depends on N.
//
//   pe_gather_kernel      X [P][F]: the features of P pixels (image, y, x), bilinear (align_corners=False) per layer
//   pe_l1_fwd_kernel      a1 [P][M] = relu(X W1^T + b1)                      fp32 MFMA, 128 x 128 tiles, K = F
//   pe_colsum_kernel      per 128-row tile: column sums (and sums of squares) in double
//   pe_bn_finish_kernel   mean, 1 / sqrt(var + eps), running statistics, num_batches_tracked
//   pe_l2_fwd_kernel      a2 [P][N*32] = relu(bn1(a1) W2^T + b2) and its per-tile column sums
//   pe_l3_ce_kernel       logits, cross-entropy, d logits, dy2 = d logits . W3; per-tile sums for dW3, db3, dg2, dbe2, loss
//   pe_finish3_kernel     those sums over the tiles, in tile order, in double
//   pe_l2_bwd_kernel      dz2 (BatchNorm 2 and ReLU backward), dy1 = dz2 . W2; per-tile sums for dW2, db2, dg1, dbe1
//   pe_finish2_kernel     those sums over the tiles
//   pe_dz1_kernel         dz1 (BatchNorm 1 and ReLU backward), in place on dy1
//   pe_l1_wgrad_kernel    dW1 [M][F] = dz1^T X                               fp32 MFMA, 128 x 128 tiles, K = P in slabs
//   pe_slab_sum_kernel    the slabs added in slab order, in double
//
// Determinism: every sum has a fixed order -- a thread's loop over the rows of its tile, then the tiles (or slabs) in index
// order in double; no atomics.  A member's numbers do not depend on how many members are trained beside it: tiles never span
// two members, and the slab count depends on P only.

constexpr int PT_H1 = 128, PT_H2 = 32, PT_CP = 32;
constexpr int PT_MAX_LAYERS = 64;
constexpr int PT_ROWS = 128;                     // rows per tile of the column sums, the layer-1 GEMM and the layer-3 pass
constexpr int PT_L2_ROWS = 64;                   // rows per workgroup of the layer-2 forward
constexpr int PT_BW_SUB = 64, PT_BW_ROWS = 256;  // layer-2 backward: sub-tile in LDS, rows per workgroup
constexpr int PT_R3 = 1152;                      // doubles per (tile, member) of pe_l3_ce_kernel: dW3 [32][32], db3 [32], sum dy2 [32],
constexpr int PT_R3_DB = 1024, PT_R3_SDY = 1056, PT_R3_SDYX = 1088, PT_R3_LOSS = 1120;   //   sum dy2 * xhat2 [32], loss
constexpr int PT_R2 = 4384;                      // pe_l2_bwd_kernel: dW2 [32][128], db2 [32], sum dy1 [128], sum dy1 * xhat1 [128]
constexpr int PT_R2_DB = 4096, PT_R2_SDY = 4128, PT_R2_SDYX = 4256;
constexpr int PT_SLAB_MIN = 2048, PT_MAX_SLABS = 8;
constexpr double PT_EPS = 1e-5, PT_MOMENTUM = 0.1;

// ------------------------------------------------------------------------------------------------ gather
// table: DEVICE int64 [layers][4] = {activations [images][c][res][res], c, res, first column}
__global__ __launch_bounds__(256) void pe_gather_kernel(const int64_t* __restrict__ table, const int* __restrict__ pix,
                                                       float* __restrict__ X, int F, int S, int images) {
    const int p = blockIdx.x, l = blockIdx.y;
    const float* a = reinterpret_cast<const float*>(table[4 * l]);
    const int C = (int)table[4 * l + 1], res = (int)table[4 * l + 2], col0 = (int)table[4 * l + 3];
    const int img = min(max(pix[3 * p], 0), images - 1);   // indices are data: an index outside the set is clamped, not followed
    const int y = min(max(pix[3 * p + 1], 0), S - 1), x = min(max(pix[3 * p + 2], 0), S - 1);
    const int64_t hw = (int64_t)res * res;
    const float* base = a + (int64_t)img * C * hw;
    float* out = X + (int64_t)p * F + col0;
    if (res == S) {
        const int o = y * res + x;
        for (int c = threadIdx.x; c < C; c += 256) out[c] = base[c * hw + o];
        return;
    }
    const float scale = (float)res / (float)S;
    int y0, y1, x0, x1;
    float ly1, lx1;
    pe_bilinear_src(y, scale, res, y0, y1, ly1);
    pe_bilinear_src(x, scale, res, x0, x1, lx1);
    const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const int o00 = y0 * res + x0, o01 = y0 * res + x1, o10 = y1 * res + x0, o11 = y1 * res + x1;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float* q = base + c * hw;
        out[c] = ly0 * (lx0 * q[o00] + lx1 * q[o01]) + ly1 * (lx0 * q[o10] + lx1 * q[o11]);
    }
}

// ------------------------------------------------------------------------------------------------ layer 1 forward
constexpr int PT_LD = PE_KC + 4;   // LDS row of a [row][k] tile: 16-byte aligned rows, operand reads two-way at worst

__global__ __launch_bounds__(256, 2) void pe_l1_fwd_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                          const float* __restrict__ bias, float* __restrict__ A, int P, int F, int M) {
    __shared__ __attribute__((aligned(16))) float sx[PT_ROWS][PT_LD];   // X [row][k]
    __shared__ __attribute__((aligned(16))) float sw[PT_ROWS][PT_LD];   // W1 [m][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int p0 = blockIdx.x * PT_ROWS, m0 = blockIdx.y * PT_ROWS, nch = F / PE_KC;

    sis_f32x4 rx[4], rw[4];
    auto load = [&](int c) {
        const int k0 = c * PE_KC;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, row = e >> 3, v = e & 7;
            rx[i] = p0 + row < P ? *reinterpret_cast<const sis_f32x4*>(X + (int64_t)(p0 + row) * F + k0 + 4 * v)
                                 : sis_f32x4{0.f, 0.f, 0.f, 0.f};
            rw[i] = *reinterpret_cast<const sis_f32x4*>(W + (int64_t)(m0 + row) * F + k0 + 4 * v);
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, row = e >> 3, v = e & 7;
            *reinterpret_cast<sis_f32x4*>(&sx[row][4 * v]) = rx[i];
            *reinterpret_cast<sis_f32x4*>(&sw[row][4 * v]) = rw[i];
        }
    };

    // wave tile: 64 pixels x 64 outputs; the result's column (the lane) runs along m: a row store is 128 contiguous bytes
    const int wp = wave & 1, wm = wave >> 1;
    sis_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

    load(0);
    store();
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        if (c + 1 < nch) load(c + 1);
#pragma unroll
        for (int kk = 0; kk < PE_KC / 2; ++kk) {
            const int k = 2 * kk + h;
            float av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) av[a] = sx[wp * 64 + a * 32 + r][k];
#pragma unroll
            for (int b = 0; b < 2; ++b) bv[b] = sw[wm * 64 + b * 32 + r][k];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
        if (c + 1 < nch) {
            store();
            __syncthreads();
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = p0 + wp * 64 + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (p >= P) continue;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int m = m0 + wm * 64 + b * 32 + r;
                A[(int64_t)p * M + m] = fmaxf(acc[a][b][i] + bias[m], 0.f);
            }
        }
}

// ------------------------------------------------------------------------------------------------ column sums, BatchNorm statistics
// partial [tile][W] (SQ: [tile][W][2] = sum, sum of squares): a thread adds the rows of its tile in row order
template <bool SQ>
__global__ __launch_bounds__(128) void pe_colsum_kernel(const float* __restrict__ src, double* __restrict__ partial, int P, int W) {
    const int col = blockIdx.x * 128 + threadIdx.x, t = blockIdx.y;
    const int r0 = t * PT_ROWS, r1 = min(P, r0 + PT_ROWS);
    double s = 0.0, q = 0.0;
    for (int row = r0; row < r1; ++row) {
        const float v = src[(int64_t)row * W + col];
        s += (double)v;
        if (SQ) q += (double)v * (double)v;
    }
    if (SQ) {
        partial[((int64_t)t * W + col) * 2] = s;
        partial[((int64_t)t * W + col) * 2 + 1] = q;
    } else {
        partial[(int64_t)t * W + col] = s;
    }
}

// out [W] = the tiles' sums in tile order
__global__ __launch_bounds__(128) void pe_colsum_finish_kernel(const double* __restrict__ partial, float* __restrict__ out, int T, int W) {
    const int col = blockIdx.x * 128 + threadIdx.x;
    if (col >= W) return;
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += partial[(int64_t)t * W + col];
    out[col] = (float)s;
}

// mean and 1 / sqrt(biased variance + eps) of W columns from [T][W][2] partials; running statistics (momentum 0.1, unbiased
// variance) and num_batches_tracked where given
__global__ __launch_bounds__(128) void pe_bn_finish_kernel(const double* __restrict__ partial, int T, int W, int P, float* __restrict__ mean,
                                                          float* __restrict__ rstd, float* __restrict__ run_mean,
                                                          float* __restrict__ run_var, int64_t* __restrict__ tracked, int members) {
    const int col = blockIdx.x * 128 + threadIdx.x;
    if (blockIdx.x == 0 && tracked && (int)threadIdx.x < members) tracked[threadIdx.x] += 1;
    if (col >= W) return;
    double s = 0.0, q = 0.0;
    for (int t = 0; t < T; ++t) {
        s += partial[((int64_t)t * W + col) * 2];
        q += partial[((int64_t)t * W + col) * 2 + 1];
    }
    const double m = s / P, var = fmax(q / P - m * m, 0.0);
    mean[col] = (float)m;
    rstd[col] = (float)(1.0 / sqrt(var + PT_EPS));
    if (run_mean) run_mean[col] = (float)((1.0 - PT_MOMENTUM) * (double)run_mean[col] + PT_MOMENTUM * m);
    if (run_var) run_var[col] = (float)((1.0 - PT_MOMENTUM) * (double)run_var[col] + PT_MOMENTUM * var * ((double)P / (double)(P - 1)));
}

// ------------------------------------------------------------------------------------------------ layer 2 forward
__global__ __launch_bounds__(256) void pe_l2_fwd_kernel(const float* __restrict__ a1, const float* __restrict__ mean1,
                                                       const float* __restrict__ rstd1, const float* __restrict__ g1,
                                                       const float* __restrict__ be1, const float* __restrict__ W2,
                                                       const float* __restrict__ b2, float* __restrict__ a2, double* __restrict__ partial,
                                                       int P, int N) {
    __shared__ float w2s[PT_H1][PT_H2 + 1];     // [k][j]
    __shared__ float ys[PT_L2_ROWS][PT_H1];     // y1 = BatchNorm 1 of a1
    __shared__ double red[8][PT_H2][2];
    const int tid = threadIdx.x, n = blockIdx.y, r0 = blockIdx.x * PT_L2_ROWS, M = N * PT_H1, M2 = N * PT_H2;
    for (int e = tid; e < PT_H2 * PT_H1; e += 256) w2s[e & 127][e >> 7] = W2[(int64_t)n * PT_H2 * PT_H1 + e];
    for (int e = tid; e < PT_L2_ROWS * PT_H1; e += 256) {
        const int rr = e >> 7, col = n * PT_H1 + (e & 127), p = r0 + rr;
        ys[rr][e & 127] = p < P ? g1[col] * ((a1[(int64_t)p * M + col] - mean1[col]) * rstd1[col]) + be1[col] : 0.f;
    }
    __syncthreads();
    const int j = tid & 31, g = tid >> 5;
    const float bias = b2[n * PT_H2 + j];
    double s = 0.0, q = 0.0;
#pragma unroll 1
    for (int i = 0; i < PT_L2_ROWS / 8; ++i) {
        const int rr = g + 8 * i, p = r0 + rr;
        float acc = 0.f;
#pragma unroll 16
        for (int k = 0; k < PT_H1; ++k) acc = fmaf(ys[rr][k], w2s[k][j], acc);
        const float v = fmaxf(acc + bias, 0.f);
        if (p < P) {
            a2[(int64_t)p * M2 + n * PT_H2 + j] = v;
            s += (double)v;
            q += (double)v * (double)v;
        }
    }
    red[g][j][0] = s;
    red[g][j][1] = q;
    __syncthreads();
    if (tid < PT_H2) {
        double ts = 0.0, tq = 0.0;
#pragma unroll
        for (int gg = 0; gg < 8; ++gg) {
            ts += red[gg][tid][0];
            tq += red[gg][tid][1];
        }
        const int64_t o = ((int64_t)blockIdx.x * M2 + n * PT_H2 + tid) * 2;
        partial[o] = ts;
        partial[o + 1] = tq;
    }
}

// ------------------------------------------------------------------------------------------------ layer 3, cross-entropy, dy2
struct PtL3Params {
    const float *a2, *mean2, *rstd2, *g2, *be2, *W3, *b3;   // W3 [N][C][32], b3 [N][C]
    const int64_t* labels;                                  // [P]
    float* dy2;                                             // [P][N * 32]
    float* logits;                                          // [N][P][C] or null
    double* rec;                                            // [tiles][N][PT_R3]
    int P, N, C;
};

__global__ __launch_bounds__(128) void pe_l3_ce_kernel(PtL3Params q) {
    __shared__ float w3s[PT_CP][PT_H2 + 1];      // [c][j]; rows >= C are zero
    __shared__ float dls[PT_ROWS][PT_CP + 1];    // d loss / d logits
    __shared__ float xhs[PT_ROWS][PT_H2 + 1];    // xhat2
    __shared__ float dys[PT_ROWS][PT_H2 + 1];    // dy2
    __shared__ float lss[PT_ROWS];
    const int tid = threadIdx.x, n = blockIdx.y, p = blockIdx.x * PT_ROWS + tid, M2 = q.N * PT_H2, C = q.C;
    const bool valid = p < q.P;
    for (int e = tid; e < PT_CP * PT_H2; e += 128) {
        const int c = e >> 5, j = e & 31;
        w3s[c][j] = c < C ? q.W3[((int64_t)n * C + c) * PT_H2 + j] : 0.f;
    }
    __syncthreads();
    float xh[PT_H2], y[PT_H2], lg[PT_CP];
#pragma unroll
    for (int j = 0; j < PT_H2; ++j) {
        const int col = n * PT_H2 + j;
        xh[j] = valid ? (q.a2[(int64_t)p * M2 + col] - q.mean2[col]) * q.rstd2[col] : 0.f;
        y[j] = q.g2[col] * xh[j] + q.be2[col];
    }
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < PT_CP; ++c) {
        lg[c] = 0.f;
        if (c < C) {
            float acc = q.b3[n * C + c];
#pragma unroll
            for (int j = 0; j < PT_H2; ++j) acc = fmaf(y[j], w3s[c][j], acc);
            lg[c] = acc;
            mx = fmaxf(mx, acc);
        }
    }
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < PT_CP; ++c)
        if (c < C) se += expf(lg[c] - mx);
    const float lse = mx + logf(se);
    const int t = valid ? (int)min(max(q.labels[p], (int64_t)0), (int64_t)(C - 1)) : 0;
    const float invP = 1.f / (float)q.P;
    float picked = 0.f;
#pragma unroll
    for (int c = 0; c < PT_CP; ++c) {
        float d = 0.f;
        if (c < C && valid) {
            if (q.logits) q.logits[((int64_t)n * q.P + p) * C + c] = lg[c];
            if (c == t) picked = lg[c];
            d = (expf(lg[c] - lse) - (c == t ? 1.f : 0.f)) * invP;
        }
        lg[c] = d;
        dls[tid][c] = d;
    }
    lss[tid] = valid ? lse - picked : 0.f;
#pragma unroll
    for (int j = 0; j < PT_H2; ++j) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < PT_CP; ++c) acc = fmaf(lg[c], w3s[c][j], acc);
        xhs[tid][j] = xh[j];
        dys[tid][j] = acc;
        if (valid) q.dy2[(int64_t)p * M2 + n * PT_H2 + j] = acc;
    }
    __syncthreads();
    // ---- the tile's sums: every thread walks the 128 rows in row order
    double* rec = q.rec + ((int64_t)blockIdx.x * q.N + n) * PT_R3;
    const int j = tid & 31, cg = tid >> 5;
    const float gj = q.g2[n * PT_H2 + j], bj = q.be2[n * PT_H2 + j];
#pragma unroll 1
    for (int i = 0; i < PT_CP / 4; ++i) {
        const int c = cg + 4 * i;
        double acc = 0.0;
        for (int rr = 0; rr < PT_ROWS; ++rr) acc += (double)(dls[rr][c] * (gj * xhs[rr][j] + bj));
        rec[c * PT_H2 + j] = acc;
    }
    if (cg == 0) {
        double acc = 0.0;
        for (int rr = 0; rr < PT_ROWS; ++rr) acc += (double)dls[rr][j];
        rec[PT_R3_DB + j] = acc;
    } else if (cg == 1) {
        double s = 0.0, sx = 0.0;
        for (int rr = 0; rr < PT_ROWS; ++rr) {
            s += (double)dys[rr][j];
            sx += (double)(dys[rr][j] * xhs[rr][j]);
        }
        rec[PT_R3_SDY + j] = s;
        rec[PT_R3_SDYX + j] = sx;
    } else if (tid == 64) {
        double acc = 0.0;
        for (int rr = 0; rr < PT_ROWS; ++rr) acc += (double)lss[rr];
        rec[PT_R3_LOSS] = acc;
    }
}

__global__ __launch_bounds__(256) void pe_finish3_kernel(const double* __restrict__ rec, int T, int N, int C, int P, float* __restrict__ dW3,
                                                        float* __restrict__ db3, float* __restrict__ dg2, float* __restrict__ dbe2,
                                                        float* __restrict__ loss) {
    const int n = blockIdx.x, idx = blockIdx.y * 256 + threadIdx.x;
    if (idx > PT_R3_LOSS) return;
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += rec[((int64_t)t * N + n) * PT_R3 + idx];
    if (idx < PT_R3_DB) {
        const int c = idx >> 5, j = idx & 31;
        if (c < C) dW3[((int64_t)n * C + c) * PT_H2 + j] = (float)s;
    } else if (idx < PT_R3_SDY) {
        if (idx - PT_R3_DB < C) db3[n * C + idx - PT_R3_DB] = (float)s;
    } else if (idx < PT_R3_SDYX) {
        dbe2[n * PT_H2 + idx - PT_R3_SDY] = (float)s;
    } else if (idx < PT_R3_LOSS) {
        dg2[n * PT_H2 + idx - PT_R3_SDYX] = (float)s;
    } else {
        loss[n] = (float)(s / P);
    }
}

// ------------------------------------------------------------------------------------------------ layer 2 backward
struct PtL2BwdParams {
    const float *a1, *mean1, *rstd1, *g1, *be1;
    const float *a2, *mean2, *rstd2, *g2, *dy2, *dg2, *dbe2;
    const float* W2;    // [N][32][128]
    float* dy1;         // [P][N * 128]
    double* rec;        // [workgroups][N][PT_R2]
    int P, N;
};

__global__ __launch_bounds__(256) void pe_l2_bwd_kernel(PtL2BwdParams q) {
    __shared__ float w2s[PT_H2][PT_H1];            // [j][k]
    __shared__ float dzs[PT_BW_SUB][PT_H2 + 1];    // dz2
    __shared__ float xhs[PT_BW_SUB][PT_H1];        // xhat1
    __shared__ float dys[PT_BW_SUB][PT_H1];        // dy1
    const int tid = threadIdx.x, n = blockIdx.y, R0 = blockIdx.x * PT_BW_ROWS, M = q.N * PT_H1, M2 = q.N * PT_H2;
    const int k = tid & 127, hf = tid >> 7;
    const float invP = 1.f / (float)q.P;
    for (int e = tid; e < PT_H2 * PT_H1; e += 256) w2s[e >> 7][e & 127] = q.W2[(int64_t)n * PT_H2 * PT_H1 + e];
    const float g1k = q.g1[n * PT_H1 + k], be1k = q.be1[n * PT_H1 + k];
    double accW[PT_H2 / 2];
#pragma unroll
    for (int i = 0; i < PT_H2 / 2; ++i) accW[i] = 0.0;
    double s1 = 0.0, s2 = 0.0, sb = 0.0;
#pragma unroll 1
    for (int sub = 0; sub < PT_BW_ROWS / PT_BW_SUB; ++sub) {
        const int r0 = R0 + sub * PT_BW_SUB;
        if (r0 >= q.P) break;
        __syncthreads();   // the previous sub-tile's readers are done (and w2s is complete)
        for (int e = tid; e < PT_BW_SUB * PT_H2; e += 256) {
            const int rr = e >> 5, col = n * PT_H2 + (e & 31), p = r0 + rr;
            float v = 0.f;
            if (p < q.P) {
                const float a = q.a2[(int64_t)p * M2 + col], xh = (a - q.mean2[col]) * q.rstd2[col];
                const float d = q.dy2[(int64_t)p * M2 + col];
                v = a > 0.f ? q.g2[col] * q.rstd2[col] * (d - q.dbe2[col] * invP - xh * (q.dg2[col] * invP)) : 0.f;
            }
            dzs[rr][e & 31] = v;
        }
        for (int e = tid; e < PT_BW_SUB * PT_H1; e += 256) {
            const int rr = e >> 7, col = n * PT_H1 + (e & 127), p = r0 + rr;
            xhs[rr][e & 127] = p < q.P ? (q.a1[(int64_t)p * M + col] - q.mean1[col]) * q.rstd1[col] : 0.f;
        }
        __syncthreads();
#pragma unroll 1
        for (int i = 0; i < PT_BW_SUB / 2; ++i) {
            const int rr = hf + 2 * i, p = r0 + rr;
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < PT_H2; ++j) acc = fmaf(dzs[rr][j], w2s[j][k], acc);
            dys[rr][k] = acc;
            if (p < q.P) q.dy1[(int64_t)p * M + n * PT_H1 + k] = acc;
        }
        __syncthreads();
#pragma unroll 1
        for (int rr = 0; rr < PT_BW_SUB; ++rr) {
            const float xh = xhs[rr][k], y = g1k * xh + be1k;
#pragma unroll
            for (int i = 0; i < PT_H2 / 2; ++i) accW[i] += (double)(dzs[rr][hf + 2 * i] * y);
            if (hf == 0) {
                const float d = dys[rr][k];
                s1 += (double)d;
                s2 += (double)(d * xh);
            } else if (k < PT_H2) {
                sb += (double)dzs[rr][k];
            }
        }
    }
    double* rec = q.rec + ((int64_t)blockIdx.x * q.N + n) * PT_R2;
#pragma unroll
    for (int i = 0; i < PT_H2 / 2; ++i) rec[(hf + 2 * i) * PT_H1 + k] = accW[i];
    if (hf == 0) {
        rec[PT_R2_SDY + k] = s1;
        rec[PT_R2_SDYX + k] = s2;
    } else if (k < PT_H2) {
        rec[PT_R2_DB + k] = sb;
    }
}

__global__ __launch_bounds__(256) void pe_finish2_kernel(const double* __restrict__ rec, int T, int N, float* __restrict__ dW2,
                                                        float* __restrict__ db2, float* __restrict__ dg1, float* __restrict__ dbe1) {
    const int n = blockIdx.x, idx = blockIdx.y * 256 + threadIdx.x;
    if (idx >= PT_R2) return;
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += rec[((int64_t)t * N + n) * PT_R2 + idx];
    if (idx < PT_R2_DB) dW2[(int64_t)n * PT_H2 * PT_H1 + idx] = (float)s;
    else if (idx < PT_R2_SDY) db2[n * PT_H2 + idx - PT_R2_DB] = (float)s;
    else if (idx < PT_R2_SDYX) dbe1[n * PT_H1 + idx - PT_R2_SDY] = (float)s;
    else dg1[n * PT_H1 + idx - PT_R2_SDYX] = (float)s;
}

// dz1 = BatchNorm 1 and ReLU backward of dy1, in place
__global__ __launch_bounds__(256) void pe_dz1_kernel(float* __restrict__ dz, const float* __restrict__ a1, const float* __restrict__ mean1,
                                                    const float* __restrict__ rstd1, const float* __restrict__ g1,
                                                    const float* __restrict__ dg1, const float* __restrict__ dbe1, int P, int M) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)P * M) return;
    const int col = (int)(idx % M);
    const float invP = 1.f / (float)P, a = a1[idx], xh = (a - mean1[col]) * rstd1[col];
    dz[idx] = a > 0.f ? g1[col] * rstd1[col] * (dz[idx] - dbe1[col] * invP - xh * (dg1[col] * invP)) : 0.f;
}

// ------------------------------------------------------------------------------------------------ layer 1 weight gradient
// out [slab][M][F] = dz [rows of the slab][M]^T . X [rows of the slab][F]
__global__ __launch_bounds__(256, 2) void pe_l1_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ X, float* __restrict__ out,
                                                            int P, int F, int M, int slab_rows) {
    __shared__ __attribute__((aligned(16))) float sa[PE_KC][PT_ROWS + PE_PAD];   // dz [k][m]
    __shared__ __attribute__((aligned(16))) float sb[PE_KC][PT_ROWS + PE_PAD];   // X [k][f]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int f0 = blockIdx.x * PT_ROWS, m0 = blockIdx.y * PT_ROWS;
    const int kb = blockIdx.z * slab_rows, ke = min(P, kb + slab_rows), nch = ke > kb ? (ke - kb + PE_KC - 1) / PE_KC : 0;
    out += (int64_t)blockIdx.z * M * F;

    sis_f32x4 ra[4], rb[4];
    auto load = [&](int c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, row = kb + c * PE_KC + (e >> 5), v = e & 31;
            const bool in = row < ke;
            ra[i] = in ? *reinterpret_cast<const sis_f32x4*>(dz + (int64_t)row * M + m0 + 4 * v) : sis_f32x4{0.f, 0.f, 0.f, 0.f};
            rb[i] = in && f0 + 4 * v < F ? *reinterpret_cast<const sis_f32x4*>(X + (int64_t)row * F + f0 + 4 * v)
                                         : sis_f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, kk = e >> 5, v = e & 31;
            *reinterpret_cast<sis_f32x4*>(&sa[kk][4 * v]) = ra[i];
            *reinterpret_cast<sis_f32x4*>(&sb[kk][4 * v]) = rb[i];
        }
    };

    const int wq = wave & 1, wf = wave >> 1;   // wave tile: 64 outputs m x 64 features f; the lane runs along f
    sis_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

    if (nch > 0) {
        load(0);
        store();
    }
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        if (c + 1 < nch) load(c + 1);
#pragma unroll
        for (int kk = 0; kk < PE_KC / 2; ++kk) {
            const int k = 2 * kk + h;
            float av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) av[a] = sa[k][wq * 64 + a * 32 + r];
#pragma unroll
            for (int b = 0; b < 2; ++b) bv[b] = sb[k][wf * 64 + b * 32 + r];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
        if (c + 1 < nch) {
            store();
            __syncthreads();
        }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = m0 + wq * 64 + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int f = f0 + wf * 64 + b * 32 + r;
                if (f < F) out[(int64_t)m * F + f] = acc[a][b][i];
            }
        }
}

__global__ __launch_bounds__(256) void pe_slab_sum_kernel(const float* __restrict__ slabs, float* __restrict__ out, int64_t count, int nslab) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    double s = 0.0;
    for (int i = 0; i < nslab; ++i) s += (double)slabs[(int64_t)i * count + idx];
    out[idx] = (float)s;
}

// ------------------------------------------------------------------------------------------------ host side
inline int pt_slabs(int P) { return (int)std::min<int64_t>(PT_MAX_SLABS, sis_cdiv(P, PT_SLAB_MIN)); }
inline int pt_slab_rows(int P) { return (sis_cdiv(P, pt_slabs(P)) + PE_KC - 1) / PE_KC * PE_KC; }
inline int64_t pt_align(int64_t bytes) { return (bytes + 255) / 256 * 256; }

struct PtTailWs {   // byte offsets into the tail's workspace
    int64_t stat1, stat2, rec3, rec2, mean1, rstd1, mean2, rstd2, a2, dy2, total;
    int t1, t2, t3, tb;
};

inline PtTailWs pt_tail_ws(int P, int N) {
    PtTailWs w;
    w.t1 = sis_cdiv(P, PT_ROWS); w.t2 = sis_cdiv(P, PT_L2_ROWS); w.t3 = sis_cdiv(P, PT_ROWS); w.tb = sis_cdiv(P, PT_BW_ROWS);
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t at = o; o += pt_align(bytes); return at; };
    w.stat1 = take((int64_t)w.t1 * N * PT_H1 * 2 * 8);
    w.stat2 = take((int64_t)w.t2 * N * PT_H2 * 2 * 8);
    w.rec3 = take((int64_t)w.t3 * N * PT_R3 * 8);
    w.rec2 = take((int64_t)w.tb * N * PT_R2 * 8);
    w.mean1 = take((int64_t)N * PT_H1 * 4); w.rstd1 = take((int64_t)N * PT_H1 * 4);
    w.mean2 = take((int64_t)N * PT_H2 * 4); w.rstd2 = take((int64_t)N * PT_H2 * 4);
    w.a2 = take((int64_t)P * N * PT_H2 * 4); w.dy2 = take((int64_t)P * N * PT_H2 * 4);
    w.total = o;
    return w;
}

inline int64_t pt_wgrad_ws(int P, int F, int N) {
    const int64_t colsum = pt_align((int64_t)sis_cdiv(P, PT_ROWS) * N * PT_H1 * 8);
    return colsum + (pt_slabs(P) > 1 ? pt_align((int64_t)pt_slabs(P) * N * PT_H1 * F * 4) : 0);
}

inline bool pt_shape_ok(int P, int N) { return P >= 2 && P <= (1 << 21) && N >= 1 && N <= 10; }
