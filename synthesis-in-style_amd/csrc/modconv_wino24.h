// Stride-1 3x3 modulated convolution in Winograd F(2x4, 3x3) form: 2 output rows x 4 output columns per tile from a
// 4 x 6 input patch, 24 multiplies per 8 outputs (24/72 of the direct form; F(2x2,3x3) in modconv_wino.hip: 16/36).
// Included at the end of modconv_wino.hip behind modconv_wino_tile512.h, which holds what this form shares with F(4x4,3x3).
//
//   U[ci][xi][co] = (G2 g G4^T)[xi]     xi = 6 i + j, i = 0..3 (F(2,3) on the row axis), j = 0..5 (F(4,3), points
//                                        0, +-1, +-2, inf, on the column axis); prepacked once per checkpoint
//                                        (sis_modconv_prepack_wino24) as [ci][q][g][co][4]: wave q owns the columns
//                                        j = 3 q + jj, jj = 0..2, and its 12 planes e = 3 i + jj = 4 g + k sit in
//                                        three 16-byte LDS reads
//   V[xi]         = (B2^T d B4)[xi]      once per workgroup and chunk into a second LDS image of the same order,
//                                        one chunk ahead of the MFMAs: lane = tile, wave = (channel of the chunk, q),
//                                        i.e. half a patch per lane (5 of the 6 patch columns: one aligned 16-byte
//                                        read and one 4-byte read per row, the address of the latter selected by q)
//   M[xi]        += U[xi] (co x ci) * V[xi] (ci x tile)      12 MFMA chains per wave (v_mfma_f32_32x32x2_f32)
//   Y             = A2^T M A4            A2^T M is lane-local; the column sum mixes the two q waves of a (co, tile):
//                                        each sends the 2 x 3 row sums of 8 accumulator rows to its partner through
//                                        the idle U / V buffers and finalises the other 8 (layer tail, 16-byte stores)
//
// Workgroup = 8 waves = (co half) x (tile half) x q = 64 co x 64 tiles (512 pixels: 8 x 64 or 16 x 32), 4-channel
// chunks: U and V 24 KB each per buffer, double-buffered, plus the raw input tile 2 x 11.25 KB: 121 KB of LDS.
//
// modconv_wino24_kernel<true> also forms the channel sum of the ToRGB layer that follows, per 64-channel block, from the values
// it stores (3 FMAs per finished value; the eight lanes that hold a pixel's 64 channels meet through the exchange area in one
// fixed order): that layer then reads 3 x Cout / 64 planes (rgb_finish_kernel, gen_small_ops.hip) instead of the activation.

namespace {

constexpr int W24_UF = W512_CC * 24 * WMBLK;    // floats of a weight chunk  [ch][q][g][co][4]
constexpr int W24_VF = W512_CC * 24 * WTILES;   // floats of a V chunk       [ch][q][g][tile][4]
constexpr int W24_BAR = 19;                     // MFMA slot of a chunk behind which its barrier sits
// MFMA slots of a chunk's five DMA instructions, all in front of the barrier: the two input pieces first (they come from HBM or
// from the L2 of another XCD, and the barrier's vmcnt(0) waits for them), the three weight rows (L2-resident) behind them.  With
// the input pieces at slots 13 and 15 -- four to six MFMAs in front of the wait -- every chunk stood at its barrier for the rest
// of their latency: 1.77 / 1.93 / 2.02 ms per launch at 64^2 / 128^2 / 256^2 against 1.65 / 1.74 / 1.82 ms
// (profiles/wino24_tile_pipeline.txt).  The piece goes to Xl[cur], whose last readers were the transforms of the previous chunk,
// in front of that chunk's barrier.
constexpr int W24_SX[2] = {2, 4};
constexpr int W24_SU[3] = {6, 8, 10};

// u[ci][q][g][co][k]: plane e = 3 i + jj = 4 g + k of column half q (j = 3 q + jj), from w[co][ci][3][3]
__global__ __launch_bounds__(256) void wino24_prepack_kernel(float* __restrict__ u, const float* __restrict__ w, int cout, int cin) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;  // idx = ci * cout + co
    if (idx >= (int64_t)cout * cin) return;
    const int co = (int)(idx % cout), ci = (int)(idx / cout);
    const float* g = w + ((int64_t)co * cin + ci) * 9;
    float t[4][3];  // G2 g
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float g0 = g[c], g1 = g[3 + c], g2 = g[6 + c];
        t[0][c] = g0;
        t[1][c] = 0.5f * (g0 + g1 + g2);
        t[2][c] = 0.5f * (g0 - g1 + g2);
        t[3][c] = g2;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float o[6];
        wino_g6<1, 1>(t[i], o);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int q = j / 3, e = 3 * i + j % 3;
            u[((((int64_t)ci * 2 + q) * 3 + (e >> 2)) * cout + co) * 4 + (e & 3)] = o[j];
        }
    }
}

#ifdef SIS_WINO_TRACE
// Development build only (tools/wino_trace.sh, tools/wino24_trace.py): per-wave cycle stamps around the tile boundary, 4 workgroups.
// Slots of tile k: 0 chunk loop entered, 1 chunk loop left, 2 exchange written and its barrier passed, 3 stores issued,
// 4 first DMA and operand loads of the tile issued, 5 vmcnt(0) and barrier passed.
__device__ unsigned int sis_wino24_trace_tile[TR_NWG][8][16][8];
#define W24_TRACE(slot)                                                                                           \
    do {                                                                                                          \
        if (blockIdx.x >= TR_WG0 && blockIdx.x < TR_WG0 + TR_NWG && k < 16) {                                     \
            const unsigned int now_ = (unsigned int)__builtin_readcyclecounter();                                 \
            if ((threadIdx.x & 63) == 0) sis_wino24_trace_tile[blockIdx.x - TR_WG0][wave][k][slot] = now_;        \
        }                                                                                                         \
    } while (0)
#else
#define W24_TRACE(slot) do {} while (0)
#endif

// RGB: a workgroup additionally writes part[o0 / 64][b][c][y][x] = sum over its 64 channels of wr[b][c][co] * out[b][co][y][x],
// wr = scale * w[c][co] * s[b][co] (ToRGB's modulated weight, no demodulation), from the values it stores to out.
template <bool RGB>
__global__ __launch_bounds__(WNTHR, 2) void modconv_wino24_kernel(const ConvParams p, const int tiles_per_wg, const int xcd_group,
                                                                  const std::conditional_t<RGB, WinoRgb, WinoNoRgb> rgb) {
    constexpr int CC = W512_CC, UF = W24_UF, VF = W24_VF, XT = W512_XT;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Ul = lds;                  // [2][UF]
    float* Vl = Ul + 2 * UF;          // [2][VF]   (Ul and Vl together: the column exchange of the epilogue, 96 KB)
    float* Xl = Vl + 2 * VF;          // [2][CC * XT]
    float* Sl = Xl + 2 * CC * XT;     // [Cin]     style row of the tile's sample
    float* Dl = Sl + p.Cin;           // [WMBLK]   scale * demodulation
    float* Bl = Dl + WMBLK;           // [WMBLK]   bias
    float* Nl = Bl + WMBLK;           // [WTILES][2][4] noise_weight * noise of the tile's pixels
    [[maybe_unused]] float* Wl = Nl + WTILES * 8;  // [3][WMBLK] RGB: ToRGB weight of the tile's sample and channel block

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int q = wave & 1, wn = (wave >> 1) & 1, wm = wave >> 2;

    // workgroup order: as modconv_wino2_kernel (output-channel block fastest; xcd_group: the blocks of a pixel tile on one XCD)
    // (twin: modconv_wino44_kernel, down to txs, without the weight rows)
    const int n_co = p.Cout / WMBLK;
    const int wg = xcd_group ? (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    const int o0 = (wg % n_co) * WMBLK;
    const TileClass tc = p.cls[0];
    const int thl = tc.th_log2, twl = tc.tw_log2;
    const int tw = 1 << twl;
    // staged input tile: rows h0-1 .. h0+th, columns w0-4 .. w0+tw+3 (16-byte aligned superset of the 1-pixel halo)
    const int ew = tw + 8, ew4 = ew >> 2;
    const int HW = p.H * p.W;
    const int k_hi = p.Cin, k_last = k_hi - CC;

    // weights: a chunk is 24 rows (ch, q, g) of 64 co x 4 floats = one 1 KB DMA instruction per row, rows wave + 8 it
    const __amdgpu_buffer_rsrc_t u_rsrc = sis_buffer_rsrc(p.wpk + (int64_t)o0 * 4);
    const unsigned u_voff = (unsigned)lane * 16u;
    const unsigned u_row_bytes = (unsigned)p.Cout * 16u;
    auto stage_u_piece = [&](int ci0, int buf, int it) {
        sis_buffer_load_lds16(u_rsrc, Ul + buf * UF + (wave + it * 8) * 256, u_voff, (unsigned)(ci0 * 6 + wave + it * 8) * u_row_bytes);
    };
    // input tile: 4 channels x 3 pieces of 64 float4 = 12 DMA instructions per chunk; wave w moves pieces w and (w + 8) % 12
    // (waves 4..7 repeat pieces 0..3: the same values to the same place, so that every wave runs the same instructions)
    int xp_ch[2], xp_base[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int piece = k == 0 ? wave : (wave + 8) % (CC * W512_XP);
        xp_ch[k] = piece / W512_XP;
        xp_base[k] = min((piece % W512_XP) * 256, XT - 256);
    }
    struct TileState {
        int b, h0, w0;
        unsigned xv[2];                 // byte offset of this lane's float4 of each piece inside the channel plane
        __amdgpu_buffer_rsrc_t x_rsrc;  // descriptor based at the tile's sample
    } T;
    auto tile_setup = [&](int pt, TileState& S, int lane) {
        const int twi = pt % tc.ntw; pt /= tc.ntw;
        const int thi = pt % tc.nth;
        S.b = pt / tc.nth; S.h0 = thi << thl; S.w0 = twi << twl;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int f4 = (xp_base[k] >> 2) + lane;
            const int r = f4 / ew4, c4 = f4 - r * ew4;
            const int h = S.h0 - 1 + r, w = S.w0 - 4 + 4 * c4;
            S.xv[k] = (h >= 0 && h < p.H && w >= 0 && w < p.W) ? (unsigned)(h * p.W + w) * 4u : BUF_OOB;
        }
        S.x_rsrc = sis_buffer_rsrc(p.x + (int64_t)S.b * p.Cin * HW);
    };
    auto stage_x_piece = [&](int ci0, int buf, int k) {
        sis_buffer_load_lds16(T.x_rsrc, Xl + buf * CC * XT + xp_ch[k] * XT + xp_base[k], T.xv[k], (unsigned)((ci0 + xp_ch[k]) * HW) * 4u);
    };
    const int pt_first = wg / n_co, pt_step = gridDim.x / n_co;
    const int txs = twl - 2;  // log2(tiles per tile row)
    const float noise_w0 = (p.fuse && p.noise) ? p.noise_w[0] : 0.f;

    // Everything below is compiled once per column half Q (wave-uniform): the two halves differ in the patch columns they read
    // and in the transform's coefficients, and a branch inside the chunk would sit between its loads.
    auto run = [&](auto qc) {
        constexpr int Q = decltype(qc)::value;
        // input transform: lane = tile, wave = (channel tch of the chunk, column half Q)
        const int tch = wave >> 1;
        const int txo = tch * XT + 2 * (lane >> txs) * ew + 4 * (lane & ((1 << txs) - 1));  // patch columns d0..d5 at + 3 .. + 8
        constexpr int teo = Q == 0 ? 3 : 8;  // Q = 0 needs d0..d4, Q = 1 needs d1..d5: d1..d4 is the aligned float4 at + 4
        const int tvo = (tch * 2 + Q) * 3 * (WTILES * 4) + lane * 4;
        float sv = 1.f, de[4], ee[4][3], oo[4][3];
        sis_f32x4 dm[4];
        auto t_read = [&](const float* xb, int r) {
            dm[r] = lds_ld4(xb + r * ew + 4);
            de[r] = xb[r * ew + teo];
        };
        auto t_col = [&](int r) {  // (d B4)[r][3 Q + jj]
            const float a = dm[r].x, b = dm[r].y, c = dm[r].z, d = dm[r].w, e = de[r];
            const float lo[5] = {e, a, b, c, d}, hi[5] = {a, b, c, d, e};  // d0..d4, d1..d5
            wino_b6_half<Q>(Q == 0 ? lo : hi, 1.f, ee[r]);
        };
        auto t_row = [&](int jj) {  // B2^T (d B4), scaled by the style
            oo[0][jj] = (ee[0][jj] - ee[2][jj]) * sv;
            oo[1][jj] = (ee[1][jj] + ee[2][jj]) * sv;
            oo[2][jj] = (ee[2][jj] - ee[1][jj]) * sv;
            oo[3][jj] = (ee[1][jj] - ee[3][jj]) * sv;
        };
        auto t_write = [&](float* vw) {
            *reinterpret_cast<sis_f32x4*>(vw) = sis_f32x4{oo[0][0], oo[0][1], oo[0][2], oo[1][0]};
            *reinterpret_cast<sis_f32x4*>(vw + WTILES * 4) = sis_f32x4{oo[1][1], oo[1][2], oo[2][0], oo[2][1]};
            *reinterpret_cast<sis_f32x4*>(vw + 2 * WTILES * 4) = sis_f32x4{oo[2][2], oo[3][0], oo[3][1], oo[3][2]};
        };
        // A / B operands of this lane: float4 k of row (channel 2 cp + half, Q, g) at column co / tile
        const int aoff = (half * 2 + Q) * 3 * (WMBLK * 4) + (wm * 32 + l31) * 4;    // + (12 cp + g) * WMBLK * 4
        const int voff = (half * 2 + Q) * 3 * (WTILES * 4) + (wn * 32 + l31) * 4;   // + (12 cp + g) * WTILES * 4

        sis_f32x16 acc[12];  // plane e = 3 i + jj of this wave's column half
        sis_f32x4 ou[2], ov[2];

        for (int k = 0; k < tiles_per_wg; ++k) {
#pragma unroll
            for (int e = 0; e < 12; ++e)
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[e][j] = 0.f;
            const int tp = wino_opaque_tid();
            tile_setup(pt_first + k * pt_step, T, tp & 63);
            if (k > 0) __syncthreads();  // everyone is done with the previous tile's exchange area and tail operands
            // first DMA of the tile: weights chunk 0, input chunks 0 and 1
#pragma unroll
            for (int it = 0; it < 3; ++it) stage_u_piece(0, 0, it);
#pragma unroll
            for (int kx = 0; kx < 2; ++kx) stage_x_piece(0, 0, kx);
#pragma unroll
            for (int kx = 0; kx < 2; ++kx) stage_x_piece(min(CC, k_last), 1, kx);
            // style row (twin: modconv_wino44_kernel) and layer-tail operands of the tile
            for (int e = tp; e < p.Cin; e += WNTHR) Sl[e] = p.s[(int64_t)T.b * p.Cin + e];
            wino512_stage_tail_operands<RGB>(p, rgb, T.b, o0, tp, Dl, Bl, Wl);
            {
                const int tt_ = tp >> 3, e = tp & 7;
                const int yy = T.h0 + 2 * (tt_ >> txs) + (e >> 2), xx = T.w0 + 4 * (tt_ & ((1 << txs) - 1)) + (e & 3);
                float nv = 0.f;
                if (p.fuse && p.noise && yy < p.H && xx < p.W) nv = noise_w0 * p.noise[(int64_t)T.b * p.noise_bstride + yy * p.W + xx];
                Nl[tp] = nv;
            }
            W24_TRACE(4);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // chunk 0 (and input chunk 1) landed, styles visible
            W24_TRACE(5);
            sv = Sl[tch];
#pragma unroll
            for (int r = 0; r < 4; ++r) t_read(Xl + txo, r);
#pragma unroll
            for (int r = 0; r < 4; ++r) t_col(r);
#pragma unroll
            for (int jj = 0; jj < 3; ++jj) t_row(jj);
            t_write(Vl + tvo);
            __syncthreads();  // V(0) visible
            ou[0] = lds_ld4(Ul + aoff);
            ov[0] = lds_ld4(Vl + voff);
            W24_TRACE(0);

            // One straight-line block per chunk c (see modconv_wino2_kernel): DMA weights(c+1) and input(c+2), transform(c+1) -> V,
            // 24 MFMAs on U(c) / V(c), one side item per MFMA slot, the barrier at slot W24_BAR with the first operands of c+1
            // behind it.  Operand group g = 3 cp + (float4 of the 12 planes) is requested at the first MFMA of group g - 1.
            auto chunk = [&](auto parity, const int ci0) {
                constexpr int cur = decltype(parity)::value, nxt = cur ^ 1;
                const int uci = ci0 + CC >= k_hi ? 0 : ci0 + CC;   // (the last chunk's prefetches are not used: any valid chunk)
                const int xci = min(ci0 + 2 * CC, k_last);
                const int tci = min(ci0 + CC, k_last);
                const float* Ub = Ul + cur * UF + aoff;
                const float* Vb = Vl + cur * VF + voff;
                const float* xb = Xl + nxt * CC * XT + txo;
                float* vw = Vl + nxt * VF + tvo;
#pragma unroll
                for (int sl = 0; sl < 24; ++sl) {
                    const int g = sl >> 2, part = sl & 3, slot = g & 1;
                    const int e = (g % 3) * 4 + part;
                    const float ua = part == 0 ? ou[slot].x : part == 1 ? ou[slot].y : part == 2 ? ou[slot].z : ou[slot].w;
                    const float va = part == 0 ? ov[slot].x : part == 1 ? ov[slot].y : part == 2 ? ov[slot].z : ov[slot].w;
                    acc[e] = __builtin_amdgcn_mfma_f32_32x32x2f32(ua, va, acc[e], 0, 0, 0);
                    if (part == 0 && g < 5) {
                        ou[slot ^ 1] = lds_ld4(Ub + (12 * ((g + 1) / 3) + (g + 1) % 3) * WMBLK * 4);
                        ov[slot ^ 1] = lds_ld4(Vb + (12 * ((g + 1) / 3) + (g + 1) % 3) * WTILES * 4);
                    }
#pragma unroll
                    for (int kx = 0; kx < 2; ++kx)
                        if (sl == W24_SX[kx]) stage_x_piece(xci, cur, kx);
#pragma unroll
                    for (int it = 0; it < 3; ++it)
                        if (sl == W24_SU[it]) stage_u_piece(uci, nxt, it);
                    if (sl == 1) { sv = Sl[tci + tch]; t_read(xb, 0); t_read(xb, 1); }
                    if (sl == 3) t_read(xb, 2);
                    if (sl == 5) { t_read(xb, 3); t_col(0); }
                    if (sl == 7) t_col(1);
                    if (sl == 9) t_col(2);
                    if (sl == 11) t_col(3);
                    if (sl == 12) t_row(0);
                    if (sl == 14) t_row(1);
                    if (sl == 16) t_row(2);
                    if (sl == 17) t_write(vw);
                    if (sl == W24_BAR) {
                        // by this slot the wave has issued its DMA pieces, written its V(c+1) and read its last operands of U(c) / V(c)
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        __syncthreads();
                    }
                    if (sl == 23) {  // group 0 of the next chunk (slot 0: group 4 is done)
                        ou[0] = lds_ld4(Ul + nxt * UF + aoff);
                        ov[0] = lds_ld4(Vl + nxt * VF + voff);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            for (int ci0 = 0; ci0 < k_hi; ci0 += 2 * CC) {  // Cin % 8 == 0 (host-checked): buffer parity is a compile-time constant
                chunk(std::integral_constant<int, 0>(), ci0);
                chunk(std::integral_constant<int, 1>(), ci0 + CC);
            }
            W24_TRACE(1);

            // ---- epilogue.  m[r][jj] = (A2^T M)[r][column 3 Q + jj], r = 0, 1.  Wave Q finalises the accumulator rows j in
            // [8 Q, 8 Q + 8) and hands its m of the other 8 rows to its partner: [pair][sender Q][8 rows][6][64 lanes] over Ul / Vl.
            float mine[8][2][3];
            const int te = wino_opaque_tid();
            const int lane = te & 63, l31 = te & 31, half = (te >> 5) & 1;
            float* xch = lds + (wave >> 1) * (2 * 48 * 64);
#pragma unroll
            for (int jo = 0; jo < 16; ++jo) {  // the rows that leave first: they free their registers
                const int j = (jo + 8 * (1 - Q)) & 15;
#pragma unroll
                for (int jj = 0; jj < 3; ++jj) {
                    const float a0 = acc[jj][j], a1 = acc[3 + jj][j], a2 = acc[6 + jj][j], a3 = acc[9 + jj][j];
                    const float m0 = a0 + a1 + a2, m1 = a1 - a2 - a3;
                    if ((j >> 3) == Q) {
                        mine[j & 7][0][jj] = m0;
                        mine[j & 7][1][jj] = m1;
                    } else {
                        xch[(Q * 48 + (j & 7) * 6 + jj) * 64 + lane] = m0;
                        xch[(Q * 48 + (j & 7) * 6 + 3 + jj) * 64 + lane] = m1;
                    }
                }
            }
            __syncthreads();
            W24_TRACE(2);

            const int t = wn * 32 + l31;
            const int oh = T.h0 + 2 * (t >> txs), ow = T.w0 + 4 * (t & ((1 << txs) - 1));
            if (oh < p.H && ow < p.W) {
                const float slope = p.fuse ? 0.2f : 1.f, gain = p.fuse ? 1.4142135623730951f : 1.f;
                const int cl0 = wm * 32 + 16 * Q + 4 * half;  // row j = 8 Q + jr sits at channel cl0 + (jr & 3) + 8 * (jr >> 2)
                float* obase = p.out + ((int64_t)T.b * p.Cout + o0 + cl0) * HW + oh * p.W + ow;
                const float* xin = xch + (1 - Q) * 48 * 64 + lane;
                const sis_f32x4 nz0 = lds_ld4(Nl + t * 8), nz1 = lds_ld4(Nl + t * 8 + 4);
                [[maybe_unused]] float pr[3][2][4];  // RGB: this lane's 8 channels (ascending) of its 2 x 4 pixels
                if constexpr (RGB) {
#pragma unroll
                    for (int e = 0; e < 24; ++e) pr[e >> 3][(e >> 2) & 1][e & 3] = 0.f;
                }
#pragma unroll
                for (int jr = 0; jr < 8; ++jr) {
                    const int ro = (jr & 3) + 8 * (jr >> 2);
                    const float dd = Dl[cl0 + ro], bb = Bl[cl0 + ro];
                    [[maybe_unused]] float wc[3];
                    if constexpr (RGB) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) wc[c] = Wl[c * WMBLK + cl0 + ro];
                    }
                    float theirs[2][3];
#pragma unroll
                    for (int e = 0; e < 6; ++e) theirs[e / 3][e % 3] = xin[(jr * 6 + e) * 64];
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        const float* ma = Q == 0 ? mine[jr][r] : theirs[r];  // columns j = 0..2
                        const float* mb = Q == 0 ? theirs[r] : mine[jr][r];  // columns j = 3..5
                        float y[4];
                        wino_a4(ma, mb, y);
                        const sis_f32x4 nz = r == 0 ? nz0 : nz1;
                        const float nzv[4] = {nz.x, nz.y, nz.z, nz.w};
                        float o[4];
#pragma unroll
                        for (int x = 0; x < 4; ++x) o[x] = wino_layer_tail(y[x], dd, nzv[x], bb, slope, gain);
                        *reinterpret_cast<sis_f32x4*>(obase + (int64_t)ro * HW + r * p.W) = sis_f32x4{o[0], o[1], o[2], o[3]};
                        if constexpr (RGB) {
#pragma unroll
                            for (int c = 0; c < 3; ++c)
#pragma unroll
                                for (int x = 0; x < 4; ++x) pr[c][r][x] = fmaf(wc[c], o[x], pr[c][r][x]);
                        }
                    }
                }
                if constexpr (RGB) {
                    // The partner's half of the exchange area was read by this wave alone and is behind its last read (a wave's
                    // LDS accesses keep their order): the lane's 24 sums go there as [colour][row][lane][4 pixels].
                    float* pw = xch + (1 - Q) * 48 * 64 + lane * 4;
#pragma unroll
                    for (int e = 0; e < 6; ++e)
                        *reinterpret_cast<sis_f32x4*>(pw + e * 256) = sis_f32x4{pr[e >> 1][e & 1][0], pr[e >> 1][e & 1][1], pr[e >> 1][e & 1][2], pr[e >> 1][e & 1][3]};
                }
            }
            if constexpr (RGB) {
                // A pixel's 64 channels sit in eight lanes: (co half wm) x (column half Q) x (lane half), 8 channels each.  Wave
                // 2 c + r adds them for colour c and pixel row r of the 64 tiles, in the fixed order wm, Q, lane half (each
                // ascending), and stores one float4 per tile.  The next tile's first barrier stands between these reads and the
                // DMA that reuses the area.
                __syncthreads();
                if (wave < 6) {
                    const int oh2 = T.h0 + 2 * (lane >> txs), ow2 = T.w0 + 4 * (lane & ((1 << txs) - 1));
                    if (oh2 < p.H && ow2 < p.W) {
                        const float* ps = lds + (lane >> 5) * (2 * 48 * 64) + (wave * 64 + (lane & 31)) * 4;
                        sis_f32x4 a = lds_ld4(ps + 48 * 64);  // wm = 0, Q = 0 (in its partner's half), lanes 0..31
#pragma unroll
                        for (int src = 1; src < 8; ++src)
                            a += lds_ld4(ps + (src >> 2) * (4 * 48 * 64) + (1 - ((src >> 1) & 1)) * (48 * 64) + (src & 1) * 128);
                        float* pd = rgb.part + ((((int64_t)(o0 / WMBLK) * p.B + T.b) * 3 + (wave >> 1)) * p.H + oh2 + (wave & 1)) * p.W + ow2;
                        *reinterpret_cast<sis_f32x4*>(pd) = a;
                    }
                }
            }
            W24_TRACE(3);
        }
    };
    if (q == 0) run(std::integral_constant<int, 0>());
    else run(std::integral_constant<int, 1>());
}

}  // namespace

#ifdef SIS_WINO_TRACE
extern "C" int sis_wino24_trace_tile_read(unsigned int* host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(sis_wino24_trace_tile), sizeof(unsigned int) * TR_NWG * 8 * 16 * 8);
}
#endif

extern "C" int sis_modconv_prepack_wino24(float* u, const float* w, int cout, int cin, void* stream) {
    SIS_REQUIRE(u && w, "sis_modconv_prepack_wino24: null pointer");
    SIS_REQUIRE(cout > 0 && cin > 0, "sis_modconv_prepack_wino24: bad sizes");
    hipLaunchKernelGGL(wino24_prepack_kernel, dim3(sis_cdiv((int64_t)cout * cin, 256)), dim3(256), 0, (hipStream_t)stream, u, w, cout, cin);
    SIS_CHECK_LAUNCH("sis_modconv_prepack_wino24");
    return 0;
}

namespace {
constexpr Wino512Form WINO24_FORM = {2, 24, W24_UF, W24_VF, WTILES * 8, "modconv_wino24_kernel", "sis_modconv_wino24_eligible",
                                     modconv_wino24_kernel<true>, modconv_wino24_kernel<false>};
}

// wino512_plan's rule (2 x 4 outputs per tile: H % 2, W % 4)
extern "C" int sis_modconv_wino24_eligible(int cin, int cout, int h, int w) {
    ConvParams p;
    return wino512_plan(WINO24_FORM, p, cin, cout, h, w) > 0 ? 1 : 0;
}

extern "C" int sis_modconv2d_wino24(float* out, const float* x, const float* u24, const float* s, const float* dscale,
                                    const float* noise, int64_t noise_batch_stride, const float* noise_weight, const float* bias,
                                    int batch, int cin, int cout, int h, int w, int fuse_act, int tiles_per_wg, void* stream) {
    if (batch == 0) return 0;
    return wino512_launch<WINO24_FORM>("sis_modconv2d_wino24", out, x, u24, s, dscale, noise, noise_batch_stride, noise_weight, bias,
                                       batch, cin, cout, h, w, fuse_act, tiles_per_wg, nullptr, stream);
}

extern "C" int sis_modconv2d_wino24_rgb(float* out, float* rgb_part, const float* x, const float* u24, const float* s, const float* dscale,
                                        const float* noise, int64_t noise_batch_stride, const float* noise_weight, const float* bias,
                                        const float* rgb_w, const float* rgb_s, float rgb_scale, int batch, int cin, int cout, int h,
                                        int w, int fuse_act, int tiles_per_wg, void* stream) {
    if (batch == 0) return 0;
    SIS_REQUIRE(rgb_part && rgb_w && rgb_s, "sis_modconv2d_wino24_rgb: null pointer");
    SIS_REQUIRE(((uintptr_t)rgb_part & 15) == 0, "sis_modconv2d_wino24_rgb: rgb_part must be 16-byte aligned");
    const WinoRgb rgb = {rgb_w, rgb_s, rgb_part, rgb_scale};
    return wino512_launch<WINO24_FORM>("sis_modconv2d_wino24_rgb", out, x, u24, s, dscale, noise, noise_batch_stride, noise_weight,
                                       bias, batch, cin, cout, h, w, fuse_act, tiles_per_wg, &rgb, stream);
}
