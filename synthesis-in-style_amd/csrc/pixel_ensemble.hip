// DatasetGAN labelling: the PixelEnsembleClassifier (reference networks/pixel_classifier/model.py:13-121) applied to a
// generator's bilinearly upsampled activations (data/dataset_gan_dataset.py:12-34, segmentation/dataset_gan_segmenter.py),
// without ever forming the [B, S, S, F] feature tensor.
//
// Bilinear upsampling is linear and per channel, so it commutes with the first Linear of every member:
//
//     W1 . up(a_r) = up(W1[:, cols_r] . a_r)
//
// pe_project_kernel: for every activation resolution r below the output size S, P_r = W1[:, cols_r] . concat(layers at r)
//   for all N members stacked (M = N * H1 outputs), written pixel-major [B][r * r][M].  One launch covers every group
//   (pointer table); the layers of a group are one K range read through their own base pointers.
// pe_head_kernel: a workgroup owns 128 output pixels of one image and loops over the members.  Per member: the fp32 MFMA GEMM
//   of the full-resolution layers (K = their channels), plus the bilinear interpolation of every P_r
//   (align_corners=False: src = (dst + 0.5) * r / S - 0.5, clamped at 0, upper neighbour clamped at r - 1), + b1, ReLU,
//   then H1 -> H2 and H2 -> C on the matrix cores with the preceding BatchNorm folded into their weights on the host, + ReLU
//   between them; argmax (first maximum on ties), vote.  After the last member: the voted label (int64) and, optionally,
//   the class colour (uint8 RGB from a lookup table).
//
// v_mfma_f32_32x32x2_f32 throughout (exact fp32 products, k-ordered fp32 accumulation).  A layer's result tile X [rows h]
// [cols pixel] has its column on the lane and rows (i & 3) + 8 (i >> 2) + 4 (lane >> 5) in register i, so the next layer's
// product W . X takes register i of every lane as its B operand for k = {row_i, row_i + 4} -- no LDS round trip.
// Every output element is computed by the same instruction sequence whatever the batch size or tile position: the labels of
// an image do not depend on the batch it is labelled in.
#include "sis_device.h"
#include <algorithm>

namespace {

constexpr int PE_MAX_GROUPS = 8;   // resolutions below the output size (a 2^8 : 1 range)
constexpr int PE_KC = 32;          // K chunk: one chunk never straddles two layers (channel counts % 32 == 0)
constexpr int PE_PAD = 32;         // LDS row padding: the two lane halves of an operand read hit disjoint banks

struct PeLayers {   // one K range over at most two activation layers [B][c][res * res] (c1 = 0: one layer)
    const float* a0;
    const float* a1;
    int c0, c1;
};

struct PeGroup {
    PeLayers L;
    const float* wt;   // [K][M] k-major
    float* out;        // [B][res * res][M]
    int res, tile0;
};

struct PeProjParams {
    PeGroup g[PE_MAX_GROUPS];
    int ngroups, B, M;
};

// Base pointer of the 32 channels [k0, k0 + 32) of sample b (a chunk lies inside one layer).
__device__ __forceinline__ const float* chunk_base(const PeLayers& L, int k0, int b, int hw) {
    return k0 < L.c0 ? L.a0 + ((int64_t)b * L.c0 + k0) * hw : L.a1 + ((int64_t)b * L.c1 + (k0 - L.c0)) * hw;
}

// Bilinear source of destination index d (align_corners=False): src = (d + 0.5) * scale - 0.5 clamped at 0, scale = res / S;
// lower neighbour i0, upper neighbour i1 clamped at res - 1, weight l1 of the upper one.  The label pass and the training
// gather (pixel_ensemble_train.h) both take their taps from here: they see the same features.
__device__ __forceinline__ void pe_bilinear_src(int d, float scale, int res, int& i0, int& i1, float& l1) {
    const float s = fmaxf(((float)d + 0.5f) * scale - 0.5f, 0.f);
    i0 = (int)s;
    i1 = i0 + (i0 < res - 1 ? 1 : 0);
    l1 = s - (float)i0;
}

// ------------------------------------------------------------------------------------------------ projection
constexpr int PJ_TQ = 128, PJ_TM = 128;

__global__ __launch_bounds__(256, 2) void pe_project_kernel(PeProjParams p) {
    __shared__ __attribute__((aligned(16))) float sa[PE_KC][PJ_TQ + PE_PAD];   // activations [k][pixel]
    __shared__ __attribute__((aligned(16))) float sw[PE_KC][PJ_TM + PE_PAD];   // weights [k][m]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int gi = 0;
#pragma unroll
    for (int i = 1; i < PE_MAX_GROUPS; ++i)
        if (i < p.ngroups && (int)blockIdx.x >= p.g[i].tile0) gi = i;
    // field by field, constant indices only: a run-time index into the argument array, or a conditional copy of the whole
    // struct, puts a copy of it in scratch
    PeGroup G;
    G.L.a0 = p.g[0].L.a0; G.L.a1 = p.g[0].L.a1; G.L.c0 = p.g[0].L.c0; G.L.c1 = p.g[0].L.c1;
    G.wt = p.g[0].wt; G.out = p.g[0].out; G.res = p.g[0].res; G.tile0 = p.g[0].tile0;
#pragma unroll
    for (int i = 1; i < PE_MAX_GROUPS; ++i) {
        const bool s = i == gi;
        G.L.a0 = s ? p.g[i].L.a0 : G.L.a0; G.L.a1 = s ? p.g[i].L.a1 : G.L.a1;
        G.L.c0 = s ? p.g[i].L.c0 : G.L.c0; G.L.c1 = s ? p.g[i].L.c1 : G.L.c1;
        G.wt = s ? p.g[i].wt : G.wt; G.out = s ? p.g[i].out : G.out;
        G.res = s ? p.g[i].res : G.res; G.tile0 = s ? p.g[i].tile0 : G.tile0;
    }
    const int hw = G.res * G.res, Q = p.B * hw, M = p.M;
    const int mtiles = M / PJ_TM, local = blockIdx.x - G.tile0;
    const int q0 = (local / mtiles) * PJ_TQ, m0 = (local % mtiles) * PJ_TM;
    const int nch = (G.L.c0 + G.L.c1) / PE_KC;

    sis_f32x4 ra[4], rw[4];
    auto load = [&](int c) {
        const int k0 = c * PE_KC;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, k = e >> 5, v = e & 31;
            const int q = q0 + 4 * v;
            if (q < Q) {   // hw % 4 == 0: the four pixels belong to one sample
                const int b = q / hw, px = q - b * hw;
                ra[i] = *reinterpret_cast<const sis_f32x4*>(chunk_base(G.L, k0, b, hw) + (int64_t)k * hw + px);
            } else {
                ra[i] = sis_f32x4{0.f, 0.f, 0.f, 0.f};
            }
            rw[i] = *reinterpret_cast<const sis_f32x4*>(G.wt + (int64_t)(k0 + k) * M + m0 + 4 * v);
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, k = e >> 5, v = e & 31;
            *reinterpret_cast<sis_f32x4*>(&sa[k][4 * v]) = ra[i];
            *reinterpret_cast<sis_f32x4*>(&sw[k][4 * v]) = rw[i];
        }
    };

    // wave tile: 64 pixels x 64 outputs; A = activations (rows = pixels), B = weights (columns = outputs), so the result's
    // column (the lane) runs along m and a row store is 128 contiguous bytes of the pixel-major output
    const int wq = wave & 1, wm = wave >> 1, r = lane & 31, h = lane >> 5;
    sis_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][bb][i] = 0.f;

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
            for (int qb = 0; qb < 2; ++qb) av[qb] = sa[k][wq * 64 + qb * 32 + r];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) bv[mb] = sw[k][wm * 64 + mb * 32 + r];
#pragma unroll
            for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
                    acc[qb][mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[qb], bv[mb], acc[qb][mb], 0, 0, 0);
        }
        __syncthreads();
        if (c + 1 < nch) {
            store();
            __syncthreads();
        }
    }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int q = q0 + wq * 64 + qb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (q >= Q) continue;
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) G.out[(int64_t)q * M + m0 + wm * 64 + mb * 32 + r] = acc[qb][mb][i];
        }
}

// ------------------------------------------------------------------------------------------------ fused head
constexpr int HD_TP = 128;   // output pixels per workgroup (4 waves x 32)

struct PeHeadParams {
    PeLayers full;                        // full-resolution layers (c0 = 0: none)
    const float* proj[PE_MAX_GROUPS];     // P_r [B][r * r][M]
    int pres[PE_MAX_GROUPS];
    int nproj, Kf;
    const float* w1f;   // [Kf][M] k-major
    const float* b1;    // [M]
    const float* w2t;   // [N][H1][H2], BatchNorm 1 folded in
    const float* b2;    // [N][H2]
    const float* w3t;   // [N][H2][CP], BatchNorm 2 folded in, columns >= C zero
    const float* b3;    // [N][CP]
    const uint8_t* lut; // [C][3] or null
    int64_t* labels;    // [B][S * S]
    uint8_t* rgb;       // [B][S * S][3] or null
    float* logits;      // [N][B][S * S][C] or null (test entry point)
    int B, S, N, C, M;
};

template <int H1, int H2, int CP>
__global__ __launch_bounds__(256) void pe_head_kernel(PeHeadParams p) {
    __shared__ __attribute__((aligned(16))) float sa[PE_KC][HD_TP + PE_PAD];   // activations [k][pixel]
    __shared__ __attribute__((aligned(16))) float sw[PE_KC][H1 + PE_PAD];      // first-layer weights [k][h]
    __shared__ unsigned char votes[10][HD_TP];
    constexpr int HB = H1 / 32, OB = H2 / 32, CB = CP / 32;
    constexpr int WV = PE_KC * H1 / 4 / 256;   // sis_f32x4 weight loads per thread per chunk
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int SS = p.S * p.S, tiles = SS / HD_TP;
    const int b = blockIdx.x / tiles, p0 = (blockIdx.x - b * tiles) * HD_TP;
    const int pix = p0 + wave * 32 + r, y = pix / p.S, x = pix - y * p.S;
    const int nch = p.Kf / PE_KC;

    for (int n = 0; n < p.N; ++n) {
        sis_f32x16 acc[HB];
#pragma unroll
        for (int hb = 0; hb < HB; ++hb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[hb][i] = 0.f;

        // ---- full-resolution layers: acc[h][pixel] = W1[n][h][k] . act[k][pixel]
        if (nch > 0) {
            sis_f32x4 ra[4], rw[WV];
            auto load = [&](int c) {
                const int k0 = c * PE_KC;
                const float* base = chunk_base(p.full, k0, b, SS) + p0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int e = tid + 256 * i, k = e >> 5, v = e & 31;
                    ra[i] = *reinterpret_cast<const sis_f32x4*>(base + (int64_t)k * SS + 4 * v);
                }
#pragma unroll
                for (int i = 0; i < WV; ++i) {
                    const int e = tid + 256 * i, k = e / (H1 / 4), v = e % (H1 / 4);
                    rw[i] = *reinterpret_cast<const sis_f32x4*>(p.w1f + (int64_t)(k0 + k) * p.M + n * H1 + 4 * v);
                }
            };
            auto store = [&]() {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int e = tid + 256 * i, k = e >> 5, v = e & 31;
                    *reinterpret_cast<sis_f32x4*>(&sa[k][4 * v]) = ra[i];
                }
#pragma unroll
                for (int i = 0; i < WV; ++i) {
                    const int e = tid + 256 * i, k = e / (H1 / 4), v = e % (H1 / 4);
                    *reinterpret_cast<sis_f32x4*>(&sw[k][4 * v]) = rw[i];
                }
            };
            load(0);
            __syncthreads();   // the previous member's readers of sa / sw are done
            store();
            __syncthreads();
            for (int c = 0; c < nch; ++c) {
                if (c + 1 < nch) load(c + 1);
#pragma unroll
                for (int kk = 0; kk < PE_KC / 2; ++kk) {
                    const int k = 2 * kk + h;
                    const float bv = sa[k][wave * 32 + r];
#pragma unroll
                    for (int hb = 0; hb < HB; ++hb)
                        acc[hb] = __builtin_amdgcn_mfma_f32_32x32x2f32(sw[k][hb * 32 + r], bv, acc[hb], 0, 0, 0);
                }
                __syncthreads();
                if (c + 1 < nch) {
                    store();
                    __syncthreads();
                }
            }
        }

        // ---- lower resolutions: + bilinear interpolation of P_r (rows h = hb*32 + 8g + 4h + j are 4 consecutive floats)
#pragma unroll
        for (int g = 0; g < PE_MAX_GROUPS; ++g) {
            if (g >= p.nproj) break;
            const int res = p.pres[g];
            const float scale = (float)res / (float)p.S;
            int y0, y1, x0, x1;
            float ly1, lx1;
            pe_bilinear_src(y, scale, res, y0, y1, ly1);
            pe_bilinear_src(x, scale, res, x0, x1, lx1);
            const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
            const float* base = p.proj[g] + (int64_t)b * res * res * p.M + n * H1 + 4 * h;
            const float* r00 = base + (int64_t)(y0 * res + x0) * p.M;
            const float* r01 = base + (int64_t)(y0 * res + x1) * p.M;
            const float* r10 = base + (int64_t)(y1 * res + x0) * p.M;
            const float* r11 = base + (int64_t)(y1 * res + x1) * p.M;
#pragma unroll
            for (int hb = 0; hb < HB; ++hb)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const int o = hb * 32 + 8 * gq;
                    const sis_f32x4 a00 = *reinterpret_cast<const sis_f32x4*>(r00 + o), a01 = *reinterpret_cast<const sis_f32x4*>(r01 + o);
                    const sis_f32x4 a10 = *reinterpret_cast<const sis_f32x4*>(r10 + o), a11 = *reinterpret_cast<const sis_f32x4*>(r11 + o);
                    acc[hb][4 * gq + 0] += ly0 * (lx0 * a00.x + lx1 * a01.x) + ly1 * (lx0 * a10.x + lx1 * a11.x);
                    acc[hb][4 * gq + 1] += ly0 * (lx0 * a00.y + lx1 * a01.y) + ly1 * (lx0 * a10.y + lx1 * a11.y);
                    acc[hb][4 * gq + 2] += ly0 * (lx0 * a00.z + lx1 * a01.z) + ly1 * (lx0 * a10.z + lx1 * a11.z);
                    acc[hb][4 * gq + 3] += ly0 * (lx0 * a00.w + lx1 * a01.w) + ly1 * (lx0 * a10.w + lx1 * a11.w);
                    if (gq == 3) __builtin_amdgcn_sched_barrier(0);   // bound the loads in flight (registers)
                }
        }

        // ---- + b1, ReLU
#pragma unroll
        for (int hb = 0; hb < HB; ++hb)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const sis_f32x4 bb = *reinterpret_cast<const sis_f32x4*>(p.b1 + n * H1 + hb * 32 + 8 * gq + 4 * h);
                acc[hb][4 * gq + 0] = fmaxf(acc[hb][4 * gq + 0] + bb.x, 0.f);
                acc[hb][4 * gq + 1] = fmaxf(acc[hb][4 * gq + 1] + bb.y, 0.f);
                acc[hb][4 * gq + 2] = fmaxf(acc[hb][4 * gq + 2] + bb.z, 0.f);
                acc[hb][4 * gq + 3] = fmaxf(acc[hb][4 * gq + 3] + bb.w, 0.f);
            }

        // ---- H1 -> H2 (BatchNorm 1 folded), + b2, ReLU
        const float* w2 = p.w2t + (int64_t)n * H1 * H2;
        sis_f32x16 acc2[OB];
#pragma unroll
        for (int ob = 0; ob < OB; ++ob) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc2[ob][i] = 0.f;
#pragma unroll
            for (int hb = 0; hb < HB; ++hb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = hb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    acc2[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[row * H2 + ob * 32 + r], acc[hb][i], acc2[ob], 0, 0, 0);
                    if (i == 15) __builtin_amdgcn_sched_barrier(0);
                }
        }
#pragma unroll
        for (int ob = 0; ob < OB; ++ob)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const sis_f32x4 bb = *reinterpret_cast<const sis_f32x4*>(p.b2 + n * H2 + ob * 32 + 8 * gq + 4 * h);
                acc2[ob][4 * gq + 0] = fmaxf(acc2[ob][4 * gq + 0] + bb.x, 0.f);
                acc2[ob][4 * gq + 1] = fmaxf(acc2[ob][4 * gq + 1] + bb.y, 0.f);
                acc2[ob][4 * gq + 2] = fmaxf(acc2[ob][4 * gq + 2] + bb.z, 0.f);
                acc2[ob][4 * gq + 3] = fmaxf(acc2[ob][4 * gq + 3] + bb.w, 0.f);
            }

        // ---- H2 -> C (BatchNorm 2 folded), + b3
        const float* w3 = p.w3t + (int64_t)n * H2 * CP;
        sis_f32x16 acc3[CB];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc3[cb][i] = 0.f;
#pragma unroll
            for (int ob = 0; ob < OB; ++ob)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = ob * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    acc3[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w3[row * CP + cb * 32 + r], acc2[ob][i], acc3[cb], 0, 0, 0);
                }
        }

        // ---- argmax over c < C, first maximum on ties (a lane's classes ascend with (cb, i); the two halves interleave)
        float best = -INFINITY;
        int bc = 0x7fffffff;
        float* lg = p.logits ? p.logits + (((int64_t)n * p.B + b) * SS + pix) * p.C : nullptr;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int c = cb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (c >= p.C) continue;
                const float v = acc3[cb][i] + p.b3[n * CP + c];
                if (lg) lg[c] = v;
                if (v > best || bc == 0x7fffffff) { best = v; bc = c; }
            }
        const float ob_ = __shfl_xor(best, 32);
        const int oc = __shfl_xor(bc, 32);
        if (ob_ > best || (ob_ == best && oc < bc)) bc = oc;
        if (h == 0) votes[n][wave * 32 + r] = (unsigned char)bc;   // read back by the same lane: no barrier
    }

    // ---- vote: the label torch.mode returns on the device for the members' labels as a float row (the reference ran there,
    // model.py:40-49).  Its kernel (ATen hip/TensorModeKernel.cuh, compute_mode) sorts the row, gives sorted position i the
    // pair (i, c_i) with c_i = i - (start of i's run), lets thread t combine positions 2t and 2t + 1, then reduces the threads'
    // pairs with shuffles down by 4, 2, 1 (the positions of a row of <= 10 lie in threads 0..4), where combine(a, b) keeps a
    // unless b's count is larger; the mode is the sorted value at the surviving position.  So among equally frequent labels
    // the winner follows that tree, neither the smallest nor the largest.  Positions past the row are (0, 0).
    if (h == 0) {
        const int slot = wave * 32 + r;
        for (int i = 1; i < p.N; ++i) {   // insertion sort of this pixel's column (same lane: no barrier)
            const unsigned char v = votes[i][slot];
            int j = i - 1;
            for (; j >= 0 && votes[j][slot] > v; --j) votes[j + 1][slot] = votes[j][slot];
            votes[j + 1][slot] = v;
        }
        auto pos = [&](int i) {   // (position, run count) packed as count * 16 + position
            if (i >= p.N) return 0;
            int c = 0;
            for (int k = i - 1; k >= 0 && votes[k][slot] == votes[i][slot]; --k) ++c;
            return c * 16 + i;
        };
        auto comb = [](int a, int b) { return (b >> 4) > (a >> 4) ? b : a; };
        int t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = comb(pos(2 * k), pos(2 * k + 1));
        const int win = comb(comb(comb(t[0], t[4]), comb(t[2], t[6])), comb(comb(t[1], t[5]), comb(t[3], t[7])));
        const int mode = votes[win & 15][slot];
        const int64_t o = (int64_t)b * SS + pix;
        p.labels[o] = mode;
        if (p.rgb) {
            p.rgb[3 * o + 0] = p.lut[3 * mode + 0];
            p.rgb[3 * o + 1] = p.lut[3 * mode + 1];
            p.rgb[3 * o + 2] = p.lut[3 * mode + 2];
        }
    }
}

bool unpack_layers(PeLayers& L, const int64_t* d) {   // {act0, act1, ch0, ch1}; ch1 = 0: one layer
    L.a0 = reinterpret_cast<const float*>(d[0]);
    L.a1 = reinterpret_cast<const float*>(d[1]);
    L.c0 = (int)d[2];
    L.c1 = (int)d[3];
    if (L.c0 < 0 || L.c1 < 0 || L.c0 % PE_KC || L.c1 % PE_KC || (L.c0 == 0 && L.c1 > 0)) return false;
    return (L.c0 == 0 || (L.a0 && !(d[0] & 15))) && (L.c1 == 0 || (L.a1 && !(d[1] & 15)));
}

#include "pixel_ensemble_train.h"

}  // namespace

extern "C" int sis_pixel_ensemble_project(const int64_t* groups, int ngroups, int batch, int m, void* stream) {
    if (batch <= 0 || ngroups == 0) return 0;
    SIS_REQUIRE(groups && ngroups > 0 && ngroups <= PE_MAX_GROUPS, "sis_pixel_ensemble_project: 1..%d groups", PE_MAX_GROUPS);
    SIS_REQUIRE(m > 0 && m % PJ_TM == 0, "sis_pixel_ensemble_project: %d outputs (a multiple of %d)", m, PJ_TM);
    PeProjParams p;
    p.ngroups = ngroups; p.B = batch; p.M = m;
    int tiles = 0;
    for (int i = 0; i < ngroups; ++i) {
        const int64_t* d = groups + i * 7;   // {res, wt, out, act0, act1, ch0, ch1}
        PeGroup& G = p.g[i];
        SIS_REQUIRE(unpack_layers(G.L, d + 3) && G.L.c0 > 0, "sis_pixel_ensemble_project: group %d: one or two layers whose "
                    "channel counts are multiples of %d, pointers 16-byte aligned", i, PE_KC);
        G.res = (int)d[0];
        G.wt = reinterpret_cast<const float*>(d[1]);
        G.out = reinterpret_cast<float*>(d[2]);
        SIS_REQUIRE(G.res >= 2 && G.wt && G.out && !((d[1] | d[2]) & 15),
                    "sis_pixel_ensemble_project: group %d: bad layout (res %d)", i, G.res);
        SIS_REQUIRE((int64_t)batch * G.res * G.res * m < (1LL << 31) * 4LL, "sis_pixel_ensemble_project: output too large");
        G.tile0 = tiles;
        tiles += sis_cdiv((int64_t)batch * G.res * G.res, PJ_TQ) * (m / PJ_TM);
    }
    hipLaunchKernelGGL(pe_project_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, p);
    SIS_CHECK_LAUNCH("pe_project_kernel");
    return 0;
}

extern "C" int sis_pixel_ensemble_head(const int64_t* full, const int64_t* proj, int nproj, const float* w1f, const float* b1,
                                       const float* w2t, const float* b2, const float* w3t, const float* b3, const uint8_t* lut,
                                       int64_t* labels, uint8_t* rgb, float* logits, int batch, int size, int members,
                                       int classes, int hidden1, void* stream) {
    if (batch <= 0) return 0;
    SIS_REQUIRE(full && labels && b1 && w2t && b2 && w3t && b3, "sis_pixel_ensemble_head: null pointer");
    SIS_REQUIRE(members >= 1 && members <= 10, "sis_pixel_ensemble_head: %d members (1..10)", members);
    SIS_REQUIRE((hidden1 == 128 && classes >= 2 && classes < 32) || (hidden1 == 256 && classes >= 32 && classes <= 64),
                "sis_pixel_ensemble_head: %d classes with hidden width %d (2..31 -> 128, 32..64 -> 256)", classes, hidden1);
    SIS_REQUIRE(size >= 16 && (size & (size - 1)) == 0, "sis_pixel_ensemble_head: output size %d (a power of two >= 16)", size);
    SIS_REQUIRE(nproj >= 0 && nproj <= PE_MAX_GROUPS && (nproj == 0 || proj), "sis_pixel_ensemble_head: 0..%d projections",
                PE_MAX_GROUPS);
    SIS_REQUIRE(!rgb || lut, "sis_pixel_ensemble_head: a colour image needs the lookup table");
    SIS_REQUIRE((int64_t)batch * size * size < (1LL << 31), "sis_pixel_ensemble_head: too many pixels");
    PeHeadParams p;
    SIS_REQUIRE(unpack_layers(p.full, full), "sis_pixel_ensemble_head: at most two full-resolution layers whose channel counts "
                "are multiples of %d, pointers 16-byte aligned", PE_KC);
    p.Kf = p.full.c0 + p.full.c1;
    SIS_REQUIRE(p.Kf == 0 || w1f, "sis_pixel_ensemble_head: full-resolution weights missing");
    SIS_REQUIRE(p.Kf > 0 || nproj > 0, "sis_pixel_ensemble_head: no activations");
    p.nproj = nproj;
    for (int g = 0; g < nproj; ++g) {
        p.proj[g] = reinterpret_cast<const float*>(proj[2 * g]);
        p.pres[g] = (int)proj[2 * g + 1];
        SIS_REQUIRE(p.proj[g] && !(proj[2 * g] & 15) && p.pres[g] >= 1 && p.pres[g] < size && size % p.pres[g] == 0,
                    "sis_pixel_ensemble_head: projection %d: resolution %d for output %d", g, p.pres[g], size);
    }
    p.w1f = w1f; p.b1 = b1; p.w2t = w2t; p.b2 = b2; p.w3t = w3t; p.b3 = b3; p.lut = lut;
    p.labels = labels; p.rgb = rgb; p.logits = logits;
    p.B = batch; p.S = size; p.N = members; p.C = classes; p.M = members * hidden1;
    const dim3 grid((unsigned)((int64_t)batch * size * size / HD_TP));
    hipStream_t st = (hipStream_t)stream;
    if (hidden1 == 128) {
        hipLaunchKernelGGL((pe_head_kernel<128, 32, 32>), grid, dim3(256), 0, st, p);
        SIS_CHECK_LAUNCH("pe_head_kernel<128,32,32>");
    } else {
        hipLaunchKernelGGL((pe_head_kernel<256, 128, 64>), grid, dim3(256), 0, st, p);
        SIS_CHECK_LAUNCH("pe_head_kernel<256,128,64>");
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ training (pixel_ensemble_train.h)
extern "C" int64_t sis_pe_train_workspace_bytes(int piece, int pixels, int features, int members) {
    if (!pt_shape_ok(pixels, members) || features <= 0 || features % PE_KC) return -1;
    if (piece == 0) return pt_tail_ws(pixels, members).total;
    if (piece == 1) return pt_wgrad_ws(pixels, features, members);
    return -1;
}

extern "C" int sis_pe_train_gather(const int64_t* table_host, const int64_t* table_dev, int layers, const int32_t* pixels, float* x,
                                   int npix, int features, int size, int images, void* stream) {
    if (npix <= 0) return 0;
    SIS_REQUIRE(table_host && table_dev && pixels && x, "sis_pe_train_gather: null pointer");
    SIS_REQUIRE(layers >= 1 && layers <= PT_MAX_LAYERS, "sis_pe_train_gather: %d layers (1..%d)", layers, PT_MAX_LAYERS);
    SIS_REQUIRE(size >= 1 && (size & (size - 1)) == 0 && images >= 1, "sis_pe_train_gather: output size %d (a power of two), %d images",
                size, images);
    SIS_REQUIRE(features > 0 && features % PE_KC == 0, "sis_pe_train_gather: %d features (a multiple of %d)", features, PE_KC);
    int64_t cols = 0;
    for (int l = 0; l < layers; ++l) {   // {activations, channels, resolution, first column}: the columns tile [0, features)
        const int64_t* d = table_host + 4 * l;
        SIS_REQUIRE(d[0] && !(d[0] & 3) && d[1] >= 1 && d[3] == cols, "sis_pe_train_gather: layer %d: bad pointer, channel count or column", l);
        SIS_REQUIRE(d[2] >= 1 && d[2] <= size && size % d[2] == 0, "sis_pe_train_gather: layer %d: resolution %d is no power-of-two "
                    "fraction of %d", l, (int)d[2], size);
        SIS_REQUIRE((int64_t)images * d[1] * d[2] * d[2] < (1LL << 40), "sis_pe_train_gather: layer %d too large", l);
        cols += d[1];
    }
    SIS_REQUIRE(cols == features, "sis_pe_train_gather: the layers have %lld channels, the features %d", (long long)cols, features);
    hipLaunchKernelGGL(pe_gather_kernel, dim3(npix, layers), dim3(256), 0, (hipStream_t)stream, table_dev, pixels, x, features, size, images);
    SIS_CHECK_LAUNCH("pe_gather_kernel");
    return 0;
}

extern "C" int sis_pe_train_l1_forward(const float* x, const float* w1, const float* b1, float* a1, int npix, int features, int members,
                                       void* stream) {
    SIS_REQUIRE(x && w1 && b1 && a1, "sis_pe_train_l1_forward: null pointer");
    SIS_REQUIRE(npix >= 1 && npix <= (1 << 21), "sis_pe_train_l1_forward: %d pixels", npix);
    SIS_REQUIRE(members >= 1 && members <= 10, "sis_pe_train_l1_forward: %d members (1..10)", members);
    SIS_REQUIRE(features > 0 && features % PE_KC == 0, "sis_pe_train_l1_forward: %d features (a multiple of %d)", features, PE_KC);
    SIS_REQUIRE(!(((intptr_t)x | (intptr_t)w1) & 15), "sis_pe_train_l1_forward: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(pe_l1_fwd_kernel, dim3(sis_cdiv(npix, PT_ROWS), members), dim3(256), 0, (hipStream_t)stream, x, w1, b1, a1, npix,
                       features, members * PT_H1);
    SIS_CHECK_LAUNCH("pe_l1_fwd_kernel");
    return 0;
}

// params: {g1, be1, w2, b2, g2, be2, w3, b3}; running: {mean1, var1, mean2, var2, tracked1, tracked2} (each may be null);
// grads: the gradients of params, in the same order
extern "C" int sis_pe_train_tail(const float* a1, const int64_t* labels, const void* const* params, void* const* running,
                                 void* const* grads, float* dz1, float* loss, float* logits, void* workspace, int npix, int members,
                                 int classes, void* stream) {
    SIS_REQUIRE(a1 && labels && params && running && grads && dz1 && loss && workspace, "sis_pe_train_tail: null pointer");
    SIS_REQUIRE(npix >= 2, "sis_pe_train_tail: %d pixels: BatchNorm in training mode needs more than one row", npix);
    SIS_REQUIRE(pt_shape_ok(npix, members), "sis_pe_train_tail: %d pixels, %d members (1..10)", npix, members);
    SIS_REQUIRE(classes >= 2 && classes < PT_CP, "sis_pe_train_tail: %d classes (2..31)", classes);
    for (int i = 0; i < 8; ++i) SIS_REQUIRE(params[i] && grads[i], "sis_pe_train_tail: null parameter or gradient %d", i);
    SIS_REQUIRE(!((intptr_t)workspace & 255), "sis_pe_train_tail: the workspace must be 256-byte aligned");
    const float *g1 = (const float*)params[0], *be1 = (const float*)params[1], *w2 = (const float*)params[2], *b2 = (const float*)params[3];
    const float *g2 = (const float*)params[4], *be2 = (const float*)params[5], *w3 = (const float*)params[6], *b3 = (const float*)params[7];
    float *dg1 = (float*)grads[0], *dbe1 = (float*)grads[1], *dw2 = (float*)grads[2], *db2 = (float*)grads[3];
    float *dg2 = (float*)grads[4], *dbe2 = (float*)grads[5], *dw3 = (float*)grads[6], *db3 = (float*)grads[7];
    const PtTailWs w = pt_tail_ws(npix, members);
    char* ws = (char*)workspace;
    double *stat1 = (double*)(ws + w.stat1), *stat2 = (double*)(ws + w.stat2), *rec3 = (double*)(ws + w.rec3), *rec2 = (double*)(ws + w.rec2);
    float *mean1 = (float*)(ws + w.mean1), *rstd1 = (float*)(ws + w.rstd1), *mean2 = (float*)(ws + w.mean2), *rstd2 = (float*)(ws + w.rstd2);
    float *a2 = (float*)(ws + w.a2), *dy2 = (float*)(ws + w.dy2);
    const int N = members, M = N * PT_H1, M2 = N * PT_H2;
    hipStream_t st = (hipStream_t)stream;

    hipLaunchKernelGGL(pe_colsum_kernel<true>, dim3(M / 128, w.t1), dim3(128), 0, st, a1, stat1, npix, M);
    SIS_CHECK_LAUNCH("pe_colsum_kernel");
    hipLaunchKernelGGL(pe_bn_finish_kernel, dim3(sis_cdiv(M, 128)), dim3(128), 0, st, (const double*)stat1, w.t1, M, npix, mean1, rstd1,
                       (float*)running[0], (float*)running[1], (int64_t*)running[4], N);
    SIS_CHECK_LAUNCH("pe_bn_finish_kernel");
    hipLaunchKernelGGL(pe_l2_fwd_kernel, dim3(w.t2, N), dim3(256), 0, st, a1, (const float*)mean1, (const float*)rstd1, g1, be1, w2, b2, a2,
                       stat2, npix, N);
    SIS_CHECK_LAUNCH("pe_l2_fwd_kernel");
    hipLaunchKernelGGL(pe_bn_finish_kernel, dim3(sis_cdiv(M2, 128)), dim3(128), 0, st, (const double*)stat2, w.t2, M2, npix, mean2, rstd2,
                       (float*)running[2], (float*)running[3], (int64_t*)running[5], N);
    SIS_CHECK_LAUNCH("pe_bn_finish_kernel");
    PtL3Params p3;
    p3.a2 = a2; p3.mean2 = mean2; p3.rstd2 = rstd2; p3.g2 = g2; p3.be2 = be2; p3.W3 = w3; p3.b3 = b3; p3.labels = labels;
    p3.dy2 = dy2; p3.logits = logits; p3.rec = rec3; p3.P = npix; p3.N = N; p3.C = classes;
    hipLaunchKernelGGL(pe_l3_ce_kernel, dim3(w.t3, N), dim3(128), 0, st, p3);
    SIS_CHECK_LAUNCH("pe_l3_ce_kernel");
    hipLaunchKernelGGL(pe_finish3_kernel, dim3(N, sis_cdiv(PT_R3_LOSS + 1, 256)), dim3(256), 0, st, (const double*)rec3, w.t3, N, classes, npix,
                       dw3, db3, dg2, dbe2, loss);
    SIS_CHECK_LAUNCH("pe_finish3_kernel");
    PtL2BwdParams p2;
    p2.a1 = a1; p2.mean1 = mean1; p2.rstd1 = rstd1; p2.g1 = g1; p2.be1 = be1; p2.a2 = a2; p2.mean2 = mean2; p2.rstd2 = rstd2; p2.g2 = g2;
    p2.dy2 = dy2; p2.dg2 = dg2; p2.dbe2 = dbe2; p2.W2 = w2; p2.dy1 = dz1; p2.rec = rec2; p2.P = npix; p2.N = N;
    hipLaunchKernelGGL(pe_l2_bwd_kernel, dim3(w.tb, N), dim3(256), 0, st, p2);
    SIS_CHECK_LAUNCH("pe_l2_bwd_kernel");
    hipLaunchKernelGGL(pe_finish2_kernel, dim3(N, sis_cdiv(PT_R2, 256)), dim3(256), 0, st, (const double*)rec2, w.tb, N, dw2, db2, dg1, dbe1);
    SIS_CHECK_LAUNCH("pe_finish2_kernel");
    hipLaunchKernelGGL(pe_dz1_kernel, dim3(sis_cdiv((int64_t)npix * M, 256)), dim3(256), 0, st, dz1, a1, (const float*)mean1,
                       (const float*)rstd1, g1, (const float*)dg1, (const float*)dbe1, npix, M);
    SIS_CHECK_LAUNCH("pe_dz1_kernel");
    return 0;
}

extern "C" int sis_pe_train_l1_wgrad(const float* dz1, const float* x, float* dw1, float* db1, void* workspace, int npix, int features,
                                     int members, void* stream) {
    SIS_REQUIRE(dz1 && x && dw1 && db1 && workspace, "sis_pe_train_l1_wgrad: null pointer");
    SIS_REQUIRE(npix >= 1 && npix <= (1 << 21), "sis_pe_train_l1_wgrad: %d pixels", npix);
    SIS_REQUIRE(members >= 1 && members <= 10, "sis_pe_train_l1_wgrad: %d members (1..10)", members);
    SIS_REQUIRE(features > 0 && features % PE_KC == 0, "sis_pe_train_l1_wgrad: %d features (a multiple of %d)", features, PE_KC);
    SIS_REQUIRE(!(((intptr_t)x | (intptr_t)dz1 | (intptr_t)dw1) & 15) && !((intptr_t)workspace & 255),
                "sis_pe_train_l1_wgrad: operands must be 16-byte aligned, the workspace 256-byte aligned");
    const int M = members * PT_H1, T = sis_cdiv(npix, PT_ROWS), nslab = pt_slabs(npix);
    hipStream_t st = (hipStream_t)stream;
    double* colsum = (double*)workspace;
    float* slabs = (float*)((char*)workspace + pt_align((int64_t)T * M * 8));
    hipLaunchKernelGGL(pe_colsum_kernel<false>, dim3(M / 128, T), dim3(128), 0, st, dz1, colsum, npix, M);
    SIS_CHECK_LAUNCH("pe_colsum_kernel");
    hipLaunchKernelGGL(pe_colsum_finish_kernel, dim3(sis_cdiv(M, 128)), dim3(128), 0, st, (const double*)colsum, db1, T, M);
    SIS_CHECK_LAUNCH("pe_colsum_finish_kernel");
    hipLaunchKernelGGL(pe_l1_wgrad_kernel, dim3(sis_cdiv(features, PT_ROWS), members, nslab), dim3(256), 0, st, dz1, x,
                       nslab > 1 ? slabs : dw1, npix, features, M, pt_slab_rows(npix));
    SIS_CHECK_LAUNCH("pe_l1_wgrad_kernel");
    if (nslab > 1) {
        const int64_t count = (int64_t)M * features;
        hipLaunchKernelGGL(pe_slab_sum_kernel, dim3(sis_cdiv(count, 256)), dim3(256), 0, st, (const float*)slabs, dw1, count, nslab);
        SIS_CHECK_LAUNCH("pe_slab_sum_kernel");
    }
    return 0;
}
