// Transposed stride-2 3x3 modulated convolution (StyleGAN2's up-convolutions, reference networks/stylegan2/model.py:251-262:
// conv_transpose2d(stride 2) on per-sample weights) with 25 instead of 36 multiplies per 2 x 2 input positions: the fast-FIR
// form of the four output phases.
//
// Per axis, position h contributes out[2h] = g0 x[h] + g2 x[h-1] (a 2-tap FIR over the positions) and out[2h+1] = g1 x[h]
// (csrc/modconv_mfma2.hip computes exactly these, 3 multiplies per position and axis, 9 per position in 2-D).  For a PAIR of
// positions 2b, 2b+1 with d0 = x[2b-1], d1 = x[2b], d2 = x[2b+1] the two even outputs are F(2,2) of a 2-tap filter:
//     m0 = (d0 - d1) g2     m1 = d1 (g0 + g2)     m2 = (d2 - d1) g0        out[4b] = m0 + m1,  out[4b+2] = m1 + m2
//     m3 = d1 g1            m4 = d2 g1                                     out[4b+1] = m3,     out[4b+3] = m4
// 5 products instead of 6; in two dimensions 25 instead of 36 per 2 x 2 block of positions (-30.6 % matrix work), with
// 4 x 4 = 16 distinct transformed weight planes U[u][v] = sum_{ky in K(u), kx in K(v)} W[ky][kx], K = ({2}, {0, 2}, {0}, {1}),
// prepacked once per checkpoint, and a 4 x 4 data transform T = (row transform) (column transform) of the block's 3 x 3
// input patch, transform t = (d0 - d1, d1, d2 - d1, d2): 14 subtractions, done per lane in registers on the way from the
// LDS to the MFMA (no transformed image).  Product (p, q), p, q = 0..4, multiplies plane (pu[p], pu[q]) with
// T[dp[p]][dp[q]], pu = (0, 1, 2, 3, 3), dp = (0, 1, 2, 1, 3); the 4 x 4 outputs of a block are
// out[r][s] = sum_{p in R(r), q in R(s)} acc[p][q], R = ({0, 1}, {3}, {1, 2}, {4}).
//
// GEMM view: M = output channels, N = 2 x 2 position BLOCKS, K = input channels, 25 accumulator planes.  25 planes of a
// 32 x 32 tile (400 registers) leave one wave per SIMD; on v_mfma_f32_16x16x4_f32 (same rate: 64 FLOP/clk/SIMD, exact fp32) a
// wave holds 32 channels x 16 blocks x 25 planes in 200 registers and two waves share a SIMD.  Workgroup = 4 waves =
// 64 channels x 32 blocks (128 positions), 4 input channels per chunk, 46 080 B of LDS (52 224 B for 128 x 128 maps): TWO workgroups per CU, one wave of each
// on every SIMD, so that one's barrier, patch transform, fragment reads, prologue and epilogue fall under the other's MFMAs
// (an earlier 8-wave / 64-block / 8-channel tile had both waves of a SIMD behind the same barrier and was 5 % slower on the three
// large layers).  Lane l of a wave: block l & 15, input channel (l >> 4) of the 4-deep MFMA step.
//
// The transposed convolution has H + 1 position rows and W + 1 position columns.  Two passes, one C call:
//   interior: the (H/2) x (W/2) blocks of positions (0 .. H-1) x (0 .. W-1) per sample, all 25 products (this kernel): T rows
//             0 .. 2H - 1, columns 0 .. 2W - 1;
//   edge:     position row H and position column W (modconv_upfir_edge_kernel below): T row 2H, T column 2W, the pad columns.
// A block of the edge has zero padding for two of its three patch rows (columns), so 20 of its 25 products (24 in the corner)
// would multiply zeros; numbering (H/2 + 1) x (W/2 + 1) blocks through this kernel, as it once did, also left every layer of
// Generator(256) half a round of workgroups past a whole number of rounds ("Up-convolution").
// Interior blocks are numbered row-major over (sample, block row, block column) and a workgroup takes 32 CONSECUTIVE blocks
// (no tile classes; H W / 4 per sample: a multiple of 32 for every layer of the generator, no padding blocks).  Its input tile
// is the run of image rows those blocks touch -- a 32-block tile of a 64 x 64 map is one block row, 3 image rows -- each staged
// whole as [4 zeros | W pixels | 4 zeros] by LDS-DMA through a buffer descriptor whose out-of-range lanes write the zeros
// (row -1 and the pad columns alike); "virtual" row v of sample b, v = h + 1 in [0, H + 1), has index b (H + 1) + v, so a run
// that crosses from one sample into the next is still one range.
// Staging: one input channel per wave and chunk, wave w moves channel w (4 pieces of weights: 16 planes x 64 channels, and
// <= 4 pieces of input rows), double-buffered, one barrier per chunk (as modconv_mfma2.hip).  The style factor s[b, ci] multiplies the
// raw patch values after their LDS read; demodulation in the epilogue; noise / bias / activation belong to the blur kernel
// that reads this kernel's (2H+1) x (2W+4)-strided result.
#include <type_traits>
#include "modconv_common.h"

namespace {

constexpr int UF_MBLK = 64;                           // output channels per workgroup
constexpr int UF_CC = 4;                              // input channels per chunk: one channel's DMA per wave
constexpr int UF_NBLK = 32;                           // position blocks per workgroup
constexpr int UF_THREADS = 256;
constexpr int UF_PLANES = 16;
constexpr int UF_WROW = UF_PLANES * UF_MBLK + 32;     // floats per channel row of the weight stage [8 plane pairs][64 co][2]:
                                                      // +32 puts the two channels a 32-lane group of a ds_read_b64 touches 32
                                                      // banks (of 64) apart: conflict-free
constexpr int UF_XP_MAX = 4;                          // 1 KiB pieces per channel of the input tile (xs <= 1024 floats)
constexpr unsigned UF_OOB = 0x80000000u;

struct UpFirParams {
    const float* x; const float* u; const float* s; const float* dscale; float* out;
    int B, Cin, Cout, H, W, OH, ORS;
    int nbw, bps, total_blocks;    // block columns per row, blocks per sample, blocks in the batch
    int vr;                        // virtual rows per sample = H + 1
    int rw4;                       // float4 per staged row = W / 4 + 2
    int xs;                        // floats per channel of the staged tile (multiple of 256)
};

__global__ __launch_bounds__(UF_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void modconv_upfir_kernel(const UpFirParams p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Wl = lds;                              // [2][CC][WROW]
    float* Xl = Wl + 2 * UF_CC * UF_WROW;         // [2][CC][xs]
    float* Sl = Xl + 2 * UF_CC * p.xs;            // [2 samples][Cin]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kq = lane >> 4;
    const int wm = wave & 1, wn = wave >> 1;

    // output-channel block fastest: the n_co workgroups that share an input tile run at the same time on different XCDs
    const int n_co = p.Cout / UF_MBLK;
    const int tile = blockIdx.x / n_co, o0 = (blockIdx.x % n_co) * UF_MBLK;
    const int g0 = tile * UF_NBLK;
    const int b_first = g0 / p.bps, bh_first = (g0 % p.bps) / p.nbw;
    const int R0 = b_first * p.vr + 2 * bh_first;     // first virtual row of the tile (position row 2 bh - 1)
    const int RW = 4 * p.rw4;
    const int HW = p.H * p.W;

    // ---- this lane's block
    const int g = g0 + wn * 16 + l15;
    const bool live = g < p.total_blocks;
    const int gc = live ? g : p.total_blocks - 1;
    const int b = gc / p.bps, rem = gc % p.bps, bh = rem / p.nbw, bw = rem % p.nbw;
    const int xoff = (b * p.vr + 2 * bh - R0) * RW + 3 + 2 * bw;    // patch element (0, 0): row 2 bh - 1, column 2 bw - 1 (+ 4 pad)
    const int soff = (b - b_first) * p.Cin;

    // ---- style rows of the (at most two) samples of this tile
    for (int e = tid; e < 2 * p.Cin; e += UF_THREADS) {
        const int n = e / p.Cin, ci = e - n * p.Cin;
        Sl[e] = p.s[(int64_t)min(b_first + n, p.B - 1) * p.Cin + ci];
    }

    // ---- DMA plan.  Weights: wave w moves channel ci0 + w, piece q = planes 4 q .. 4 q + 3 (lane >> 4) x 64 channels.
    // Input: wave w moves channel ci0 + w, piece q = float4 q * 64 + lane of the [rows][rw4] tile.
    const __amdgpu_buffer_rsrc_t w_rsrc = sis_buffer_rsrc(p.u + 2 * o0);
    const __amdgpu_buffer_rsrc_t x_rsrc = sis_buffer_rsrc(p.x);
    // weight image of a channel: [plane pair 0..7][co][2 planes]; a 1 KiB piece = two pairs x 64 channels x 2
    const unsigned w_voff = (unsigned)(((lane >> 5) * p.Cout * 2 + (lane & 31) * 4) * 4);
    const int xpieces = p.xs >> 8;
    unsigned x_voff[UF_XP_MAX];
#pragma unroll
    for (int q = 0; q < UF_XP_MAX; ++q) {
        const int i = q * 64 + lane;
        const int row = i / p.rw4, c4 = i - row * p.rw4;
        const int v = R0 + row;
        const int bb = v / p.vr, h = v - bb * p.vr - 1, col = 4 * (c4 - 1);
        const bool ok = q < xpieces && bb < p.B && h >= 0 && h < p.H && col >= 0 && col < p.W;
        x_voff[q] = ok ? (unsigned)((bb * p.Cin * HW + h * p.W + col) * 4) : UF_OOB;
    }
    auto stage = [&](int ci0, int buf) {
        float* wdst = Wl + (buf * UF_CC + wave) * UF_WROW;
        const unsigned wbase = (unsigned)((ci0 + wave) * UF_PLANES * p.Cout * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) sis_buffer_load_lds16(w_rsrc, wdst + q * 256, w_voff, wbase + (unsigned)(q * 2 * p.Cout * 2 * 4));
        float* xdst = Xl + (buf * UF_CC + wave) * p.xs;
        const unsigned xbase = (unsigned)((ci0 + wave) * HW * 4);
#pragma unroll
        for (int q = 0; q < UF_XP_MAX; ++q)
            if (q < xpieces) sis_buffer_load_lds16(x_rsrc, xdst + q * 256, x_voff[q], xbase);   // (wave-uniform)
    };

    sis_f32x4 acc[5][5][2];
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int c = 0; c < 5; ++c)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[a][c][t] = sis_f32x4{0.f, 0.f, 0.f, 0.f};

    __syncthreads();   // style rows
    stage(0, 0);
    __syncthreads();   // vmcnt(0) + barrier: chunk 0 landed

    // Chunks software-pipelined across the barrier (one MFMA step per chunk).  A plain loop starts every chunk behind
    // its barrier with 10 LDS reads and ~25 VALU of transform before its first MFMA.  Here the barrier of chunk c sits behind the
    // request for its last fragment pair (pair 7, asked for in iteration 5): from there on nobody reads buffer c & 1 any more, chunk
    // c + 1 has landed (its DMA was issued a whole chunk earlier) -- so the DMA of chunk c + 2 goes into the freed buffer and the
    // transform of chunk c + 1 runs in slices between the 20 MFMAs of plane row 3, and the next chunk starts with MFMAs.
    const int n_chunks = p.Cin / UF_CC;
    if (n_chunks > 1) stage(UF_CC, 1);
    __syncthreads();   // (chunk 1 landed as well: once per workgroup)
    float tA[4][4], tB[4][4], cm0[4], raw[3][3], svn;
    auto tr_read = [&](int c, int bufc) {   // patch and style of chunk c (clamped past the end: values unused)
        const int cl = min(c, n_chunks - 1) * UF_CC + kq;
        svn = Sl[soff + cl];
        const float* xb = Xl + (bufc * UF_CC + kq) * p.xs + xoff;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int j = 0; j < 3; ++j) raw[r][j] = xb[r * RW + j];
    };
    // column transform of patch row r: rows 1 and 2 ARE rows 1 and 3 of t, row 0 waits in cm0 for the row transform
    auto tr_col = [&](int r, float (&t)[4][4]) {
        const float d0 = raw[r][0] * svn, d1 = raw[r][1] * svn, d2 = raw[r][2] * svn;
        float* o = r == 0 ? cm0 : (r == 1 ? t[1] : t[3]);
        o[0] = d0 - d1; o[1] = d1; o[2] = d2 - d1; o[3] = d2;
        // (pinned where it stands: the results are used in the NEXT chunk only, and the compiler otherwise sinks the arithmetic
        // into that chunk's block, in front of its first MFMA)
        asm volatile("" : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]));
    };
    auto tr_row = [&](float (&t)[4][4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            t[0][j] = cm0[j] - t[1][j]; t[2][j] = t[3][j] - t[1][j];
            asm volatile("" : "+v"(t[0][j]), "+v"(t[2][j]));
        }
    };
    tr_read(0, 0);
#pragma unroll
    for (int r = 0; r < 3; ++r) tr_col(r, tA);
    tr_row(tA);
    const int woff = kq * UF_WROW + (wm * 32 + l15) * 2;
    // ring of three fragment pairs, carried from chunk to chunk: pair 0 of chunk c + 1 takes pair 6's slot once that is used up
    sis_f32x2 ra[3][2];
    ra[0][0] = *reinterpret_cast<const sis_f32x2*>(Wl + woff); ra[0][1] = *reinterpret_cast<const sis_f32x2*>(Wl + woff + 32);
    auto chunk = [&](auto parity, int c, const float (&t)[4][4], float (&tn)[4][4]) {
        constexpr int B = decltype(parity)::value;
        const float* wb = Wl + B * UF_CC * UF_WROW + woff;
        auto fetch = [&](int k) {
            ra[k % 3][0] = *reinterpret_cast<const sis_f32x2*>(wb + k * 2 * UF_MBLK);
            ra[k % 3][1] = *reinterpret_cast<const sis_f32x2*>(wb + k * 2 * UF_MBLK + 32);
        };
        fetch(1);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k + 2 < 8) fetch(k + 2);
            if (k == 7) {   // (behind the barrier: chunk c + 1 has landed)
                ra[0][0] = *reinterpret_cast<const sis_f32x2*>(Wl + (B ^ 1) * UF_CC * UF_WROW + woff);
                ra[0][1] = *reinterpret_cast<const sis_f32x2*>(Wl + (B ^ 1) * UF_CC * UF_WROW + woff + 32);
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int i = 2 * k + e, u = i >> 2, v = i & 3;
                const float a0 = ra[k % 3][0][e], a1 = ra[k % 3][1][e];
#pragma unroll
                for (int pp = 0; pp < 2; ++pp)
#pragma unroll
                    for (int qq = 0; qq < 2; ++qq) {
                        if ((pp && u != 3) || (qq && v != 3)) continue;
                        const int pi = u + pp, qi = v + qq;
                        const int di = pi == 3 ? 1 : (pi == 4 ? 3 : pi), dj = qi == 3 ? 1 : (qi == 4 ? 3 : qi);
                        acc[pi][qi][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, t[di][dj], acc[pi][qi][0], 0, 0, 0);
                        acc[pi][qi][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, t[di][dj], acc[pi][qi][1], 0, 0, 0);
                    }
                if (k >= 5) {   // side work of the chunk's tail, one piece behind each MFMA group
                    if (k == 5 && e == 1) {
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of chunk c + 1 (the compiler does not see them across the back edge)
                        __syncthreads();
                        if (c + 2 < n_chunks) stage((c + 2) * UF_CC, B);
                        tr_read(c + 1, B ^ 1);
                    }
                    if (k == 6 && e == 0) { tr_col(0, tn); tr_col(1, tn); }
                    if (k == 6 && e == 1) tr_col(2, tn);
                    if (k == 7 && e == 0) tr_row(tn);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (k < 5) {
                if (k + 2 < 8) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                const int u = (2 * k) >> 2, vhi = ((2 * k) & 3) + 1;
                if (u == 3 && vhi == 3) __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
                else if (u == 3) __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
                else if (vhi == 3) __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
                else __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            }
        }
    };
    for (int c = 0; c < n_chunks; c += 2) {
        chunk(std::integral_constant<int, 0>(), c, tA, tB);
        if (c + 1 < n_chunks) chunk(std::integral_constant<int, 1>(), c + 1, tB, tA);
    }

    // ---- epilogue: output transform, demodulation, 16-byte stores of the block's 4 x 4 outputs per channel
    // (the block's coordinates are worked out again from the lane number -- the loop has no register to carry them)
    int eg = g0 + wn * 16 + (int)(threadIdx.x & 15);
    asm volatile("" : "+v"(eg));
    if (eg >= p.total_blocks) return;
    const int eb = eg / p.bps, erem = eg % p.bps, ebh = erem / p.nbw, ebw = erem % p.nbw;
    const int OHW = p.OH * p.ORS;
    const float* db = p.dscale + (int64_t)eb * p.Cout;
    float* ob = p.out + (int64_t)eb * p.Cout * OHW + (int64_t)(4 * ebh) * p.ORS + 4 * ebw;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = o0 + wm * 32 + tt * 16 + 4 * kq + r;
            const float d = db[co];
            float cs[5][4];                                   // column sums per product row p
#pragma unroll
            for (int pi = 0; pi < 5; ++pi) {
                cs[pi][0] = acc[pi][0][tt][r] + acc[pi][1][tt][r];
                cs[pi][1] = acc[pi][3][tt][r];
                cs[pi][2] = acc[pi][1][tt][r] + acc[pi][2][tt][r];
                cs[pi][3] = acc[pi][4][tt][r];
            }
            float* oc = ob + (int64_t)co * OHW;
#pragma unroll
            for (int ro = 0; ro < 4; ++ro) {   // (interior blocks: rows 4 bh .. 4 bh + 3 <= 2H - 1 all exist)
                float4 v;
                if (ro == 0) v = make_float4(cs[0][0] + cs[1][0], cs[0][1] + cs[1][1], cs[0][2] + cs[1][2], cs[0][3] + cs[1][3]);
                else if (ro == 1) v = make_float4(cs[3][0], cs[3][1], cs[3][2], cs[3][3]);
                else if (ro == 2) v = make_float4(cs[1][0] + cs[2][0], cs[1][1] + cs[2][1], cs[1][2] + cs[2][2], cs[1][3] + cs[2][3]);
                else v = make_float4(cs[4][0], cs[4][1], cs[4][2], cs[4][3]);
                *reinterpret_cast<float4*>(oc + ro * p.ORS) = make_float4(v.x * d, v.y * d, v.z * d, v.w * d);
            }
        }
}

// ---- Edge pass: position row H (T row 2H, corner included) and position column W (T column 2W, rows 0 .. 2H - 1).
// In the block numbering over (H/2 + 1) x (W/2 + 1) these are the last block row and column, where patch rows (columns) 1 and 2
// are zero padding: of the 25 products only p = 0 (bottom row: t[0][j] = cm0[j] - 0, planes (0, v)) or q = 0 (right column:
// column transform d0 - 0, planes (u, 0)) multiply anything but zeros.  A wave takes 16 edge blocks of one kind x 16 output
// channels, 5 accumulators, the same MFMA, the same channel order (ascending, lane group kq = channel ci0 + kq of the step) and the
// same output sums as the 25-product kernel, whose operations on these blocks it repeats one for one (the "+ 0.f" stand for its
// sums with the all-zero products: they turn a -0 into +0 as there).  The NWV waves of a workgroup share the 16 blocks: the
// column pass reads ONE float per image row (a cache line each), so the patch values and the style factor
// (x0, x1, x2, s) of a 64-channel chunk are gathered once per workgroup into the LDS, one chunk ahead through registers, and every wave
// reads its MFMA operand from there; weights by plain loads, a chunk ahead as well.  One barrier per chunk.  The 16-byte store at
// column 2W also writes the pad columns 2W+1 .. 2W+3.
constexpr int UE_KC = 64;                             // channels per chunk of the edge pass: 16 MFMA steps

template <bool ROWK, int NWV>
__device__ __forceinline__ void upfir_edge_tile(const UpFirParams& p, int tile, int cgb, float4* Dl) {
    constexpr int CSTEP = 4 * NWV, NR = UE_KC / CSTEP;  // staging: thread = (block tid & 15, channel (tid >> 4) + k CSTEP), k < NR
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kq = lane >> 4, sc = tid >> 4;
    const int co0 = (cgb * NWV + wave) * 16;
    const int per = ROWK ? p.W / 2 + 1 : p.H / 2;         // edge blocks of this kind per sample
    const int n_items = p.B * per;
    const int it = tile * 16 + l15;                       // (the same block in the staging and in the MFMA role: tid & 15 == lane & 15)
    const int itc = it < n_items ? it : n_items - 1;
    const int b = itc / per, j = itc - b * per;           // block column (ROWK) or block row
    const int HW = p.H * p.W;
    // the three patch values that are not padding: row H - 1, columns 2 j - 1 .. 2 j + 1 (ROWK); column W - 1, rows 2 j - 1 .. 2 j + 1
    // (32-bit element offsets: the plan keeps x and u below 2 GiB; padding: address clamped, value dropped after the load)
    unsigned xo[3];
    bool ok[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int pos = 2 * j - 1 + r;
        ok[r] = pos >= 0 && pos < (ROWK ? p.W : p.H);
        xo[r] = (unsigned)(b * p.Cin * HW + (!ok[r] ? 0 : (ROWK ? (p.H - 1) * p.W + pos : pos * p.W + p.W - 1)));
    }
    const unsigned uo = (unsigned)(kq * UF_PLANES * p.Cout + (co0 + l15) * 2);   // u[ci][plane pair][co][2]

    float raw[NR][3], sv[NR];
    auto load_patch = [&](int c0) {      // (channels past Cin: clamped, their steps are not computed)
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const int ci = min(c0 + sc + k * CSTEP, p.Cin - 1);
            sv[k] = p.s[b * p.Cin + ci];
#pragma unroll
            for (int r = 0; r < 3; ++r) raw[k][r] = p.x[xo[r] + (unsigned)(ci * HW)];
        }
    };
    auto store_patch = [&](int buf) {
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            Dl[(buf * UE_KC + sc + k * CSTEP) * 16 + l15] =
                make_float4(ok[0] ? raw[k][0] : 0.f, ok[1] ? raw[k][1] : 0.f, ok[2] ? raw[k][2] : 0.f, sv[k]);
        }
    };
    auto load_w = [&](int c0, float (&w)[16][4]) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float* uc = p.u + (int64_t)min(c0 + 4 * k, p.Cin - 4) * UF_PLANES * p.Cout;   // (wave-uniform)
            if constexpr (ROWK) {     // planes (0, 0 .. 3): pairs 0 and 1
                const sis_f32x2 w0 = *reinterpret_cast<const sis_f32x2*>(uc + uo), w1 = *reinterpret_cast<const sis_f32x2*>(uc + 2 * p.Cout + uo);
                w[k][0] = w0[0]; w[k][1] = w0[1]; w[k][2] = w1[0]; w[k][3] = w1[1];
            } else {                  // planes (0 .. 3, 0): first plane of pairs 0, 2, 4, 6
#pragma unroll
                for (int u = 0; u < 4; ++u) w[k][u] = (uc + u * 4 * p.Cout)[uo];
            }
        }
    };

    sis_f32x4 acc[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) acc[a] = sis_f32x4{0.f, 0.f, 0.f, 0.f};
    float wc[16][4], wn[16][4];
    load_patch(0);
    load_w(0, wc);
    store_patch(0);
    __syncthreads();
    for (int c0 = 0, buf = 0; c0 < p.Cin; c0 += UE_KC, buf ^= 1) {
        const bool more = c0 + UE_KC < p.Cin;
        if (more) { load_patch(c0 + UE_KC); load_w(c0 + UE_KC, wn); }
        const int ns = min(16, (p.Cin - c0) >> 2);
        auto step = [&](int k) {
            {
#pragma clang fp contract(off)
                const float4 dv = Dl[(buf * UE_KC + 4 * k + kq) * 16 + l15];
                // The data transform, operation for operation as the compiler emits it for the 25-product kernel (its source says
                // d = raw * s; o0 = d0 - d1; o2 = d2 - d1 and is contracted to d1 = s x1, o0 = fma(s, x0, -d1), o2 = fma(s, x2, -d1)),
                // with the padding's zeros put in: explicit fma, contraction off, so that this kernel cannot be contracted
                // another way.  z = s * 0 is a padding value after the style factor (a signed zero).
                const float sf = dv.w, z = sf * 0.f;
                float t[4];
                if constexpr (ROWK) {     // patch row 0 = (x0, x1, x2), rows 1 and 2 padding: t[0][j] = cm0[j] - t[1][j], t[1] = (+0, z, +0, z)
                    const float d1 = sf * dv.y, d2 = sf * dv.z;
                    t[0] = __builtin_fmaf(sf, dv.x, -d1); t[1] = d1 - z; t[2] = __builtin_fmaf(sf, dv.z, -d1); t[3] = d2 - z;
                } else {                  // patch column 0 = three rows' x, columns 1 and 2 padding: c_r = fma(s, x_r, -z), then the row transform
                    const float e0 = __builtin_fmaf(sf, dv.x, -z), e1 = __builtin_fmaf(sf, dv.y, -z), e2 = __builtin_fmaf(sf, dv.z, -z);
                    t[0] = e0 - e1; t[1] = e1; t[2] = e2 - e1; t[3] = e2;
                }
                // products 0 .. 4: plane pu = (0, 1, 2, 3, 3) x data dp = (0, 1, 2, 1, 3)
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[k][0], t[0], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[k][1], t[1], acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[k][2], t[2], acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[k][3], t[1], acc[3], 0, 0, 0);
                acc[4] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[k][3], t[3], acc[4], 0, 0, 0);
            }
        };
        if (ns == 16) {               // a whole chunk: one block of code, the LDS reads ahead of the MFMAs
#pragma unroll
            for (int k = 0; k < 16; ++k) step(k);
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < ns) step(k);
        }
        if (more) {
            store_patch(buf ^ 1);     // (last read in the chunk before this one: behind that chunk's barrier)
#pragma unroll
            for (int k = 0; k < 16; ++k)
#pragma unroll
                for (int u = 0; u < 4; ++u) wc[k][u] = wn[k][u];
        }
        __syncthreads();
    }
    if (it >= n_items) return;
    const int OHW = p.OH * p.ORS;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int co = co0 + 4 * kq + r;
        const float dm = p.dscale[(int64_t)b * p.Cout + co];
        float* oc = p.out + ((int64_t)b * p.Cout + co) * OHW;
        if constexpr (ROWK) {     // T row 2H, columns 4 j .. 4 j + 3 (j = W/2: column 2W and the three pad columns, zeros)
            const float v0 = (acc[0][r] + acc[1][r]) + 0.f, v1 = acc[3][r] + 0.f, v2 = (acc[1][r] + acc[2][r]) + 0.f, v3 = acc[4][r] + 0.f;
            *reinterpret_cast<float4*>(oc + (int64_t)(2 * p.H) * p.ORS + 4 * j) = make_float4(v0 * dm, v1 * dm, v2 * dm, v3 * dm);
        } else {                  // T column 2W, rows 4 j .. 4 j + 3
            const float c0 = acc[0][r] + 0.f, c1 = acc[1][r] + 0.f, c2 = acc[2][r] + 0.f, c3 = acc[3][r] + 0.f, c4 = acc[4][r] + 0.f;
            const float v[4] = {c0 + c1, c3, c1 + c2, c4};
            const float z = 0.f * dm;
#pragma unroll
            for (int ro = 0; ro < 4; ++ro)
                *reinterpret_cast<float4*>(oc + (int64_t)(4 * j + ro) * p.ORS + 2 * p.W) = make_float4(v[ro] * dm, z, z, z);
        }
    }
}

// workgroup = NWV waves = one tile of 16 edge blocks x 16 NWV output channels: channel block fastest, bottom-row tiles first
template <int NWV>
__global__ __launch_bounds__(64 * NWV) void modconv_upfir_edge_kernel(const UpFirParams p, int n_row_tiles) {
    __shared__ float4 Dl[2 * UE_KC * 16];
    const int n_cgb = p.Cout / (16 * NWV);
    const int tile = blockIdx.x / n_cgb, cgb = blockIdx.x - tile * n_cgb;
    if (tile < n_row_tiles) upfir_edge_tile<true, NWV>(p, tile, cgb, Dl);
    else upfir_edge_tile<false, NWV>(p, tile - n_row_tiles, cgb, Dl);
}

// u[ci][plane pair 2 pu + pv / 2][co][pv % 2] = sum_{ky in K(pu), kx in K(pv)} w[co][ci][ky][kx]
__global__ __launch_bounds__(256) void upfir_prepack_kernel(float* __restrict__ u, const float* __restrict__ w, int cout, int cin) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // i = ci * cout + co (co fastest: coalesced writes)
    if (i >= (int64_t)cout * cin) return;
    const int co = (int)(i % cout), ci = (int)(i / cout);
    const float* src = w + ((int64_t)co * cin + ci) * 9;
    float g[3][3];
#pragma unroll
    for (int t = 0; t < 9; ++t) g[t / 3][t % 3] = src[t];
    // rows: K(0) = {2}, K(1) = {0, 2}, K(2) = {0}, K(3) = {1}
    float rows[4][3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
        rows[0][kx] = g[2][kx]; rows[1][kx] = g[0][kx] + g[2][kx]; rows[2][kx] = g[0][kx]; rows[3][kx] = g[1][kx];
    }
#pragma unroll
    for (int pu = 0; pu < 4; ++pu) {
        const float v4[4] = {rows[pu][2], rows[pu][0] + rows[pu][2], rows[pu][0], rows[pu][1]};
#pragma unroll
        for (int h = 0; h < 2; ++h)   // plane pair (pu, 2 h), (pu, 2 h + 1): the two planes of a channel side by side
            *reinterpret_cast<float2*>(u + (((int64_t)ci * 8 + pu * 2 + h) * cout + co) * 2) = make_float2(v4[2 * h], v4[2 * h + 1]);
    }
}

bool upfir_plan(UpFirParams& p, int batch, int cin, int cout, int h, int w, int row_stride, size_t* lds_bytes) {
    constexpr int min_side = 16;   // (smaller maps: the 4-phase kernel)
    if (batch <= 0 || h < min_side || w < min_side || (h & 1) || (w & 3) || cin % UF_CC || cout % UF_MBLK) return false;
    if ((row_stride & 3) || row_stride < 2 * w + 4) return false;
    if ((int64_t)batch * cin * h * w * 4 >= (1LL << 31) || (int64_t)cin * UF_PLANES * cout * 4 >= (1LL << 31)) return false;
    p.B = batch; p.Cin = cin; p.Cout = cout; p.H = h; p.W = w; p.OH = 2 * h + 1; p.ORS = row_stride;
    // interior blocks only: position row H and position column W belong to the edge pass
    p.nbw = w / 2;
    const int nbh = h / 2;
    p.bps = nbh * p.nbw;
    if (p.bps < UF_NBLK) return false;      // a tile spans at most two samples
    p.total_blocks = batch * p.bps;
    p.vr = h + 1;
    p.rw4 = w / 4 + 2;
    const int n_tiles = sis_cdiv(p.total_blocks, UF_NBLK);
    int rows_max = 0;
    for (int t = 0; t < n_tiles; ++t) {
        const int g0 = t * UF_NBLK, g1 = (g0 + UF_NBLK - 1 < p.total_blocks ? g0 + UF_NBLK - 1 : p.total_blocks - 1);
        const int r0 = (g0 / p.bps) * p.vr + 2 * ((g0 % p.bps) / p.nbw);
        const int r1 = (g1 / p.bps) * p.vr + 2 * ((g1 % p.bps) / p.nbw) + 2;
        rows_max = r1 - r0 + 1 > rows_max ? r1 - r0 + 1 : rows_max;
    }
    p.xs = sis_cdiv(rows_max * 4 * p.rw4, 256) * 256;
    if (p.xs > 256 * UF_XP_MAX) return false;
    *lds_bytes = (size_t)(2 * UF_CC * UF_WROW + 2 * UF_CC * p.xs + 2 * cin) * sizeof(float);
    return *lds_bytes <= 160 * 1024;
}

}  // namespace

extern "C" int sis_modconv_up_fir_supported(int batch, int cin, int cout, int h, int w, int t_row_stride) {
    UpFirParams p;
    size_t lds;
    return upfir_plan(p, batch, cin, cout, h, w, t_row_stride, &lds) ? 1 : 0;
}

extern "C" int sis_modconv_up_fir_prepack(float* u, const float* w, int cout, int cin, void* stream) {
    SIS_REQUIRE(u && w, "sis_modconv_up_fir_prepack: null pointer");
    SIS_REQUIRE(cout > 0 && cin > 0, "sis_modconv_up_fir_prepack: bad sizes");
    const int64_t n = (int64_t)cout * cin;
    hipLaunchKernelGGL(upfir_prepack_kernel, dim3(sis_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, u, w, cout, cin);
    SIS_CHECK_LAUNCH("upfir_prepack_kernel");
    return 0;
}

extern "C" int sis_modconv2d_up_fir(float* t, const float* x, const float* u, const float* s, const float* dscale, int batch,
                                    int cin, int cout, int h, int w, int t_row_stride, void* stream) {
    if (batch == 0) return 0;
    SIS_REQUIRE(t && x && u && s && dscale, "sis_modconv2d_up_fir: null pointer");
    SIS_REQUIRE((((uintptr_t)t | (uintptr_t)x | (uintptr_t)u) & 15) == 0, "sis_modconv2d_up_fir: pointers must be 16-byte aligned");
    UpFirParams p;
    size_t lds;
    SIS_REQUIRE(upfir_plan(p, batch, cin, cout, h, w, t_row_stride, &lds),
                "sis_modconv2d_up_fir: %d x (%d -> %d) on %d x %d with row stride %d is not supported (sis_modconv_up_fir_supported)", batch,
                cin, cout, h, w, t_row_stride);
    p.x = x; p.u = u; p.s = s; p.dscale = dscale; p.out = t;
    static bool attr_set = false;
    if (!attr_set) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&modconv_upfir_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        if (e != hipSuccess) return sis_fail("sis_modconv2d_up_fir: cannot raise the dynamic LDS limit: %s", hipGetErrorString(e));
        attr_set = true;
    }
    const int64_t grid = (int64_t)sis_cdiv(p.total_blocks, UF_NBLK) * (cout / UF_MBLK);
    SIS_REQUIRE(grid > 0 && grid < ((int64_t)1 << 31), "sis_modconv2d_up_fir: bad grid");
    hipLaunchKernelGGL(modconv_upfir_kernel, dim3((unsigned)grid), dim3(UF_THREADS), lds, (hipStream_t)stream, p);
    SIS_CHECK_LAUNCH("modconv_upfir_kernel");
    // edge pass: T row 2H and T column 2W (and the pad columns), disjoint from the interior's outputs
    const int n_row_tiles = sis_cdiv(batch * (w / 2 + 1), 16), n_tiles = n_row_tiles + sis_cdiv(batch * (h / 2), 16);
    if (cout % 128 == 0) hipLaunchKernelGGL(modconv_upfir_edge_kernel<8>, dim3((unsigned)(n_tiles * (cout / 128))), dim3(512), 0, (hipStream_t)stream, p, n_row_tiles);
    else hipLaunchKernelGGL(modconv_upfir_edge_kernel<4>, dim3((unsigned)(n_tiles * (cout / 64))), dim3(256), 0, (hipStream_t)stream, p, n_row_tiles);
    SIS_CHECK_LAUNCH("modconv_upfir_edge_kernel");
    sis_kernel_name = "modconv_upfir_kernel";
    return 0;
}
