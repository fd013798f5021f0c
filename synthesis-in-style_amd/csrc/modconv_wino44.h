// Stride-1 3x3 modulated convolution in Winograd F(4x4, 3x3) form: 4 x 4 outputs per tile from a 6 x 6 input patch, 36 multiplies
// per 16 outputs (36/144 of the direct form; F(2x4,3x3): 24/72).  Included at the end of modconv_wino.hip
// behind modconv_wino_tile512.h, which holds what this form shares with F(2x4,3x3).
//
//   U[ci][i][j][co] = (G4 g G4^T)[i][j]  i, j = 0..5: the 6-point transform (points 0, +-1, +-2, inf) on both axes; prepacked once
//                                        per checkpoint (sis_modconv_prepack_wino44) as [ci][row][co][4], 9 rows per channel.
//                                        Wave q owns the columns j = 3 q + jj, jj = 0..2, i.e. 18 planes a = 0..17:
//                                        a < 16: i = 3 (a >> 3) + (a & 7) / 3, jj = (a & 7) % 3, in row 4 q + (a >> 2) at k = a & 3;
//                                        a = 16, 17: (i, jj) = (2, 2), (5, 2), in row 8 at k = 2 q + a - 16
//                                        (so that a thread of the input transform, which forms three rows i of one column half,
//                                        writes two float4 and one float)
//   V[i][j]          = (B6^T d B6)[i][j]  once per workgroup and chunk into a second LDS image of the same order, one chunk ahead of
//                                        the MFMAs: wave = (column half Q, row half S, channel pair), lane = (channel, tile); rows
//                                        i = 3 S .. 3 S + 2 need the patch rows S .. S + 4, columns j = 3 Q .. 3 Q + 2 the patch
//                                        columns Q .. Q + 4 (one aligned 16-byte read and one 4-byte read per row)
//   M[i][j]         += U[i][j] (co x ci) * V[i][j] (ci x tile)   36 MFMAs per wave and chunk (v_mfma_f32_16x16x4_f32: a wave holds
//                                        32 co x 16 tiles x 18 planes in 144 accumulator registers)
//   Y                = A4^T M A4         A4^T M is lane-local; the column sum mixes the two q waves of a (co, tile): each sends the
//                                        4 x 3 row sums of one 16-channel fragment to its partner through the idle U / V buffers
//                                        and finalises the other (layer tail, 16-byte stores)
//
// Workgroup = 8 waves = (co half wm) x (tile half wn) x q = 64 co x 32 tiles (512 pixels: 8 x 64 or 16 x 32, the pixel block and
// the staged input of the F(2x4) kernel), 4-channel chunks: U 36 KB and V 18 KB per buffer, double-buffered, plus the raw input
// tile 2 x 11.25 KB: 139 KB of LDS.
//
// modconv_wino44_kernel<true> also forms the channel sum of the ToRGB layer that follows, per 64-channel block, in the layout of
// the F(2x4) kernel.  Sum order within a block: a lane adds its 4 channels in ascending order (FMA chain from 0), the 16
// lanes that hold a pixel's 64 channels are then added in the order wm, q, lane group (each ascending), i.e. by ascending channel.

namespace {

constexpr int W44_T = 32;                        // 4 x 4 tiles per workgroup
constexpr int W44_UC = 9 * WMBLK * 4;            // floats of a channel's weight rows  [row][co][4]
constexpr int W44_VC = 9 * W44_T * 4;            // floats of a channel's V rows       [row][tile][4]
constexpr int W44_UF = W512_CC * W44_UC;         // floats of a weight chunk
constexpr int W44_VF = W512_CC * W44_VC;         // floats of a V chunk
constexpr int W44_XCH = 48 * 64;                 // floats one wave sends to its partner in the epilogue
constexpr int W44_BAR = 30;                      // MFMA slot of a chunk behind which its barrier sits
// MFMA slots of a chunk's DMA instructions: the two input pieces first (they come from HBM or from the L2 of another XCD, and the
// barrier's vmcnt(0) waits for them; see the F(2x4) form), the weight rows behind them.  A third input buffer with the input two
// chunks ahead and the barrier at vmcnt(2) measured no faster (profiles/wino44_layers.txt).
constexpr int W44_SX[2] = {2, 4};
constexpr int W44_SU[5] = {6, 10, 12, 14, 18};

constexpr int w44_plane(int i, int jj) {  // plane a of (row i, column 3 q + jj)
    const int n = 3 * (i % 3) + jj;
    return n < 8 ? 8 * (i / 3) + n : 16 + i / 3;
}

// u[ci][row][co][k] from w[co][ci][3][3] (plane order: head of this file)
__global__ __launch_bounds__(256) void wino44_prepack_kernel(float* __restrict__ u, const float* __restrict__ w, int cout, int cin) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;  // idx = ci * cout + co
    if (idx >= (int64_t)cout * cin) return;
    const int co = (int)(idx % cout), ci = (int)(idx / cout);
    const float* g = w + ((int64_t)co * cin + ci) * 9;
    float t[6][3];  // G4 g
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        wino_g6<3, 3>(g + c, &t[0][c]);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        float o[6];
        wino_g6<1, 1>(t[i], o);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int q = j / 3, pl = w44_plane(i, j % 3);
            const int row = pl < 16 ? 4 * q + (pl >> 2) : 8, k = pl < 16 ? (pl & 3) : 2 * q + pl - 16;
            u[(((int64_t)ci * 9 + row) * cout + co) * 4 + k] = o[j];
        }
    }
}

template <bool RGB>
__global__ __launch_bounds__(WNTHR, 2) void modconv_wino44_kernel(const ConvParams p, const int tiles_per_wg, const int xcd_group,
                                                                  const std::conditional_t<RGB, WinoRgb, WinoNoRgb> rgb) {
    constexpr int CC = W512_CC, UF = W44_UF, VF = W44_VF, XT = W512_XT, UC = W44_UC, VC = W44_VC;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Ul = lds;                  // [2][UF]
    float* Vl = Ul + 2 * UF;          // [2][VF]   (Ul and Vl together, 108 KB: the first 96 KB are the column exchange of the epilogue)
    float* Xl = Vl + 2 * VF;          // [2][CC * XT]
    float* Sl = Xl + 2 * CC * XT;     // [Cin]     style row of the tile's sample
    float* Dl = Sl + p.Cin;           // [WMBLK]   scale * demodulation
    float* Bl = Dl + WMBLK;           // [WMBLK]   bias
    float* Nl = Bl + WMBLK;           // [W44_T][4][4] noise_weight * noise of the tile's pixels
    [[maybe_unused]] float* Wl = Nl + W44_T * 16;  // [3][WMBLK] RGB: ToRGB weight of the tile's sample and channel block

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const int q = wave & 1, wn = (wave >> 1) & 1, wm = wave >> 2;

    // workgroup order (twin: modconv_wino24_kernel, down to txs, without the weight rows)
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

    // weights: a chunk is 36 rows (ch, row) of 64 co x 4 floats = one 1 KB DMA instruction per row, rows wave + 8 it: five for
    // the waves 0..3, four for the others (a wave-uniform branch around the fifth)
    const __amdgpu_buffer_rsrc_t u_rsrc = sis_buffer_rsrc(p.wpk + (int64_t)o0 * 4);
    const unsigned u_voff = (unsigned)lane * 16u;
    const unsigned u_row_bytes = (unsigned)p.Cout * 16u;
    auto stage_u_piece = [&](int ci0, int buf, int it) {
        const int row = wave + it * 8;
        if (it < 4 || wave < 4) sis_buffer_load_lds16(u_rsrc, Ul + buf * UF + row * 256, u_voff, (unsigned)(ci0 * 9 + row) * u_row_bytes);
    };
    // input tile: the pieces of the F(2x4) kernel (4 channels x 3 pieces of 64 float4); wave w moves piece w, and the waves
    // 0..3 piece w + 8 (a wave-uniform branch around the second)
    int xp_ch[2], xp_base[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int piece = k == 0 ? wave : (wave + 8) % (CC * W512_XP);   // (k = 1 is used by the waves 0..3 only)
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
        if (k == 0 || wave < 4) sis_buffer_load_lds16(T.x_rsrc, Xl + buf * CC * XT + xp_ch[k] * XT + xp_base[k], T.xv[k], (unsigned)((ci0 + xp_ch[k]) * HW) * 4u);
    };
    const int pt_first = wg / n_co, pt_step = gridDim.x / n_co;
    const int txs = twl - 2;  // log2(tiles per tile row)
    const float noise_w0 = (p.fuse && p.noise) ? p.noise_w[0] : 0.f;

    // Everything below is compiled once per (column half Q, row half S), both wave-uniform: the variants differ in the patch rows
    // and columns they read and in the transform's coefficients, and a branch inside the chunk would sit between its loads.
    auto run = [&](auto qc, auto sc) {
        constexpr int Q = decltype(qc)::value, S = decltype(sc)::value;
        // input transform: wave = (Q, S, channel pair wm), lane = (channel of the pair, tile)
        // With 16 tiles in a tile row (8 x 64) the lanes of the second row take their tiles rotated by 8: the row is 1152 bytes
        // further on, half an LDS line, and the fixed lane groups of a 16-byte read (0-3, 12-15, 20-27 / 4-11, 16-19, 28-31) would
        // otherwise meet on the same banks two-way.  (8 tiles in a row, 16 x 32: rows 640 bytes apart, conflict-free as it is.)
        const int tl = lane & 31;
        const int tch = 2 * wm + (lane >> 5), tt = txs == 4 ? (tl & 16) | ((tl + ((tl >> 4) << 3)) & 15) : tl;
        const int txo = tch * XT + (4 * (tt >> txs) + S) * ew + 4 * (tt & ((1 << txs) - 1)) + 4;  // patch columns d0..d5 at - 1 .. + 4
        // Q = 0 needs d0..d4, Q = 1 needs d1..d5: d1..d4 is the aligned float4 at + 0, the fifth value comes with an aligned 8-byte
        // read (a 4-byte read at this 16-byte lane stride is a four-way bank conflict, the 8-byte one two-way)
        constexpr int teo = Q == 0 ? -2 : 4;
        const int tvo = tch * VC + (4 * Q + 2 * S) * (W44_T * 4) + tt * 4;
        const int tvt = tch * VC + 8 * (W44_T * 4) + tt * 4 + 2 * Q + S;
        float sv = 1.f, de[5], ee[5][3], oo[3][3];
        sis_f32x4 dm[5];
        auto t_read = [&](const float* xb, int r) {
            dm[r] = lds_ld4(xb + r * ew);
            const float2 d2 = lds_ld2(xb + r * ew + teo);
            de[r] = Q == 0 ? d2.y : d2.x;
        };
        auto t_col = [&](int r) {  // (d B6)[S + r][3 Q + jj]
            const float a = dm[r].x, b = dm[r].y, c = dm[r].z, d = dm[r].w, e = de[r];
            const float lo[5] = {e, a, b, c, d}, hi[5] = {a, b, c, d, e};  // d0..d4, d1..d5
            wino_b6_half<Q>(Q == 0 ? lo : hi, 1.f, ee[r]);
        };
        auto t_row = [&](int jj) {  // rows 3 S .. 3 S + 2 of B6^T (d B6), scaled by the style
            const float e[5] = {ee[0][jj], ee[1][jj], ee[2][jj], ee[3][jj], ee[4][jj]};
            float o[3];
            wino_b6_half<S>(e, sv, o);
#pragma unroll
            for (int i = 0; i < 3; ++i) oo[i][jj] = o[i];
        };
        auto t_write = [&](float* vc) {
            *reinterpret_cast<sis_f32x4*>(vc + tvo) = sis_f32x4{oo[0][0], oo[0][1], oo[0][2], oo[1][0]};
            *reinterpret_cast<sis_f32x4*>(vc + tvo + W44_T * 4) = sis_f32x4{oo[1][1], oo[1][2], oo[2][0], oo[2][1]};
            vc[tvt] = oo[2][2];
        };
        // A / B operands of this lane: channel lg of the chunk, float4 of row 4 Q + g at column co (fragment h: + 16) / tile
        const int aoff = lg * UC + 4 * Q * (WMBLK * 4) + (wm * 32 + l15) * 4;     // + g * WMBLK * 4 + h * 64
        const int voff = lg * VC + 4 * Q * (W44_T * 4) + (wn * 16 + l15) * 4;     // + g * W44_T * 4
        const int atail = lg * UC + 8 * (WMBLK * 4) + (wm * 32 + l15) * 4 + 2 * Q;  // + h * 64
        const int vtail = lg * VC + 8 * (W44_T * 4) + (wn * 16 + l15) * 4 + 2 * Q;

        sis_f32x4 acc[18][2];  // [plane][16-channel fragment]
        sis_f32x4 oa[2][2], ob[2];
        sis_f32x2 ta[2], tb;
        auto ld_group = [&](const float* Ub, const float* Vb, int g) {
            oa[g & 1][0] = lds_ld4(Ub + aoff + g * (WMBLK * 4));
            oa[g & 1][1] = lds_ld4(Ub + aoff + g * (WMBLK * 4) + 64);
            ob[g & 1] = lds_ld4(Vb + voff + g * (W44_T * 4));
        };

        for (int k = 0; k < tiles_per_wg; ++k) {
#pragma unroll
            for (int e = 0; e < 18; ++e)
#pragma unroll
                for (int h = 0; h < 2; ++h) acc[e][h] = sis_f32x4{0.f, 0.f, 0.f, 0.f};
            const int tp = wino_opaque_tid();
            tile_setup(pt_first + k * pt_step, T, tp & 63);
            if (k > 0) __syncthreads();  // everyone is done with the previous tile's exchange area and tail operands
            // first DMA of the tile: weights chunk 0, input chunks 0 and 1
#pragma unroll
            for (int it = 0; it < 5; ++it) stage_u_piece(0, 0, it);
#pragma unroll
            for (int kx = 0; kx < 2; ++kx) stage_x_piece(0, 0, kx);
#pragma unroll
            for (int kx = 0; kx < 2; ++kx) stage_x_piece(min(CC, k_last), 1, kx);
            // style row (twin: modconv_wino24_kernel) and layer-tail operands of the tile
            for (int e = tp; e < p.Cin; e += WNTHR) Sl[e] = p.s[(int64_t)T.b * p.Cin + e];
            wino512_stage_tail_operands<RGB>(p, rgb, T.b, o0, tp, Dl, Bl, Wl);
            {
                const int tt_ = tp >> 4, e = tp & 15;
                const int yy = T.h0 + 4 * (tt_ >> txs) + (e >> 2), xx = T.w0 + 4 * (tt_ & ((1 << txs) - 1)) + (e & 3);
                float nv = 0.f;
                if (p.fuse && p.noise && yy < p.H && xx < p.W) nv = noise_w0 * p.noise[(int64_t)T.b * p.noise_bstride + yy * p.W + xx];
                Nl[tp] = nv;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();  // chunk 0 (and input chunk 1) landed, styles visible
            sv = Sl[tch];
#pragma unroll
            for (int r = 0; r < 5; ++r) t_read(Xl + txo, r);
#pragma unroll
            for (int r = 0; r < 5; ++r) t_col(r);
#pragma unroll
            for (int jj = 0; jj < 3; ++jj) t_row(jj);
            t_write(Vl);
            __syncthreads();  // V(0) visible
            ld_group(Ul, Vl, 0);

            // One straight-line block per chunk c: DMA weights(c+1) and input(c+2), transform(c+1) -> V, 36 MFMAs on U(c) / V(c), one
            // side item per MFMA slot, the barrier at slot W44_BAR with the first operands of c+1 behind it.  Operand group g (the
            // float4 of planes 4 g .. 4 g + 3, both fragments) is requested at the first MFMA of group g - 1, the 8-byte tail
            // (planes 16, 17) with group 3.  The input piece goes to Xl[cur], whose last readers were the transforms of the previous
            // chunk, in front of that chunk's barrier.
            auto chunk = [&](auto parity, const int ci0) {
                constexpr int cur = decltype(parity)::value, nxt = cur ^ 1;
                const int uci = ci0 + CC >= k_hi ? 0 : ci0 + CC;   // (the last chunks' prefetches are not used: any valid chunk)
                const int xci = min(ci0 + 2 * CC, k_last);
                const int tci = min(ci0 + CC, k_last);
                const float* Ub = Ul + cur * UF;
                const float* Vb = Vl + cur * VF;
                const float* xb = Xl + nxt * CC * XT + txo;
                float* vw = Vl + nxt * VF;
#pragma unroll
                for (int sl = 0; sl < 36; ++sl) {
                    if (sl < 32) {
                        const int g = sl >> 3, part = (sl >> 1) & 3, h = sl & 1, slot = g & 1;
                        const sis_f32x4 ua4 = oa[slot][h], va4 = ob[slot];
                        const float ua = part == 0 ? ua4.x : part == 1 ? ua4.y : part == 2 ? ua4.z : ua4.w;
                        const float va = part == 0 ? va4.x : part == 1 ? va4.y : part == 2 ? va4.z : va4.w;
                        acc[4 * g + part][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(ua, va, acc[4 * g + part][h], 0, 0, 0);
                        if ((sl & 7) == 0 && g < 3) ld_group(Ub, Vb, g + 1);
                        if (sl == 16) {
                            ta[0] = *reinterpret_cast<const sis_f32x2*>(Ub + atail);
                            ta[1] = *reinterpret_cast<const sis_f32x2*>(Ub + atail + 64);
                            tb = *reinterpret_cast<const sis_f32x2*>(Vb + vtail);
                        }
                    } else {
                        const int part = (sl - 32) >> 1, h = sl & 1;
                        const float ua = part == 0 ? ta[h].x : ta[h].y, va = part == 0 ? tb.x : tb.y;
                        acc[16 + part][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(ua, va, acc[16 + part][h], 0, 0, 0);
                    }
                    if (sl == W44_BAR + 1) ld_group(Ul + nxt * UF, Vl + nxt * VF, 0);  // group 0 of the next chunk (slot 0 is free behind group 2)
#pragma unroll
                    for (int kx = 0; kx < 2; ++kx)
                        if (sl == W44_SX[kx]) stage_x_piece(xci, cur, kx);
#pragma unroll
                    for (int it = 0; it < 5; ++it)
                        if (sl == W44_SU[it]) stage_u_piece(uci, nxt, it);
                    if (sl == 1) { sv = Sl[tci + tch]; t_read(xb, 0); t_read(xb, 1); }
                    if (sl == 3) t_read(xb, 2);
                    if (sl == 5) t_read(xb, 3);
                    if (sl == 7) { t_read(xb, 4); t_col(0); }
                    if (sl == 9) t_col(1);
                    if (sl == 11) t_col(2);
                    if (sl == 13) t_col(3);
                    if (sl == 15) t_col(4);
                    if (sl == 17) t_row(0);
                    if (sl == 19) t_row(1);
                    if (sl == 21) t_row(2);
                    if (sl == 23) t_write(vw);
                    if (sl == W44_BAR) {
                        // by this slot the wave has issued its DMA pieces, written its V(c+1) and read its last operands of U(c) / V(c)
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        __syncthreads();
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            for (int ci0 = 0; ci0 < k_hi; ci0 += 2 * CC) {  // Cin % 8 == 0 (host-checked): buffer parity is a compile-time constant
                chunk(std::integral_constant<int, 0>(), ci0);
                chunk(std::integral_constant<int, 1>(), ci0 + CC);
            }

            // ---- epilogue.  m[r][jj] = (A4^T M)[r][column 3 Q + jj], r = 0..3.  Wave Q finalises fragment h = Q (channels
            // wm * 32 + 16 Q + 4 lg + reg) and hands its m of the other fragment to its partner:
            // [pair][sender Q][reg][r][jj][64 lanes] over Ul / Vl.
            float mine[4][4][3];
            const int te = wino_opaque_tid();
            const int lane = te & 63, l15 = te & 15, lg = (te >> 4) & 3;
            float* xch = lds + (wave >> 1) * (2 * W44_XCH);
#pragma unroll
            for (int ho = 0; ho < 2; ++ho) {  // the fragment that leaves first: it frees its registers
                const int h = ho == 0 ? 1 - Q : Q;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
#pragma unroll
                    for (int jj = 0; jj < 3; ++jj) {
                        const float a0 = acc[w44_plane(0, jj)][h][reg], a1 = acc[w44_plane(1, jj)][h][reg], a2 = acc[w44_plane(2, jj)][h][reg];
                        const float a3 = acc[w44_plane(3, jj)][h][reg], a4 = acc[w44_plane(4, jj)][h][reg], a5 = acc[w44_plane(5, jj)][h][reg];
                        const float a6[6] = {a0, a1, a2, a3, a4, a5};
                        float m[4];
                        wino_a4(a6, a6 + 3, m);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if (h == Q) mine[reg][r][jj] = m[r];
                            else xch[(Q * 48 + reg * 12 + r * 3 + jj) * 64 + lane] = m[r];
                        }
                    }
            }
            __syncthreads();

            const int t = wn * 16 + l15;
            const int oh = T.h0 + 4 * (t >> txs), ow = T.w0 + 4 * (t & ((1 << txs) - 1));
            if (oh < p.H && ow < p.W) {
                const float slope = p.fuse ? 0.2f : 1.f, gain = p.fuse ? 1.4142135623730951f : 1.f;
                const int cl0 = wm * 32 + 16 * Q + 4 * lg;
                float* obase = p.out + ((int64_t)T.b * p.Cout + o0 + cl0) * HW + oh * p.W + ow;
                const float* xin = xch + (1 - Q) * W44_XCH + lane;
                sis_f32x4 nz[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) nz[r] = lds_ld4(Nl + t * 16 + r * 4);
                [[maybe_unused]] float pr[3][4][4];  // RGB: this lane's 4 channels (ascending) of its 4 x 4 pixels
                if constexpr (RGB) {
#pragma unroll
                    for (int e = 0; e < 48; ++e) pr[e >> 4][(e >> 2) & 3][e & 3] = 0.f;
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const float dd = Dl[cl0 + reg], bb = Bl[cl0 + reg];
                    [[maybe_unused]] float wc[3];
                    if constexpr (RGB) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) wc[c] = Wl[c * WMBLK + cl0 + reg];
                    }
                    float theirs[4][3];
#pragma unroll
                    for (int e = 0; e < 12; ++e) theirs[e / 3][e % 3] = xin[(reg * 12 + e) * 64];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float* ma = Q == 0 ? mine[reg][r] : theirs[r];  // columns j = 0..2
                        const float* mb = Q == 0 ? theirs[r] : mine[reg][r];  // columns j = 3..5
                        float y[4];
                        wino_a4(ma, mb, y);
                        const float nzv[4] = {nz[r].x, nz[r].y, nz[r].z, nz[r].w};
                        float o[4];
#pragma unroll
                        for (int x = 0; x < 4; ++x) o[x] = wino_layer_tail(y[x], dd, nzv[x], bb, slope, gain);
                        *reinterpret_cast<sis_f32x4*>(obase + (int64_t)reg * HW + r * p.W) = sis_f32x4{o[0], o[1], o[2], o[3]};
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
                    // LDS accesses keep their order): the lane's 48 sums go there as [colour][row][lane][4 pixels].
                    float* pw = xch + (1 - Q) * W44_XCH + lane * 4;
#pragma unroll
                    for (int e = 0; e < 12; ++e)
                        *reinterpret_cast<sis_f32x4*>(pw + e * 256) = sis_f32x4{pr[e >> 2][e & 3][0], pr[e >> 2][e & 3][1], pr[e >> 2][e & 3][2], pr[e >> 2][e & 3][3]};
                }
            }
            if constexpr (RGB) {
                // A pixel's 64 channels sit in sixteen lanes: (co half wm) x (column half Q) x (lane group lg), 4 channels each.
                // Wave 2 c + rh adds them for colour c and pixel rows 2 rh, 2 rh + 1 of the 32 tiles, in the fixed order wm, Q, lg
                // (each ascending), and stores one float4 per tile and row.  The next tile's first barrier stands between these
                // reads and the DMA that reuses the area.
                __syncthreads();
                if (wave < 6) {
                    const int t2 = lane & 31, r2 = 2 * (wave & 1) + (lane >> 5), c2 = wave >> 1;
                    const int oh2 = T.h0 + 4 * (t2 >> txs), ow2 = T.w0 + 4 * (t2 & ((1 << txs) - 1));
                    if (oh2 < p.H && ow2 < p.W) {
                        const float* ps = lds + (t2 >> 4) * (2 * W44_XCH) + (c2 * 4 + r2) * 256 + (t2 & 15) * 4;
                        sis_f32x4 a = lds_ld4(ps + W44_XCH);  // wm = 0, Q = 0 (in its partner's half), lane group 0
#pragma unroll
                        for (int src = 1; src < 16; ++src)
                            a += lds_ld4(ps + (src >> 3) * (4 * W44_XCH) + (1 - ((src >> 2) & 1)) * W44_XCH + (src & 3) * 64);
                        float* pd = rgb.part + ((((int64_t)(o0 / WMBLK) * p.B + T.b) * 3 + c2) * p.H + oh2 + r2) * p.W + ow2;
                        *reinterpret_cast<sis_f32x4*>(pd) = a;
                    }
                }
            }
        }
    };
    if (q == 0) {
        if (wn == 0) run(std::integral_constant<int, 0>(), std::integral_constant<int, 0>());
        else run(std::integral_constant<int, 0>(), std::integral_constant<int, 1>());
    } else {
        if (wn == 0) run(std::integral_constant<int, 1>(), std::integral_constant<int, 0>());
        else run(std::integral_constant<int, 1>(), std::integral_constant<int, 1>());
    }
}

}  // namespace

extern "C" int sis_modconv_prepack_wino44(float* u, const float* w, int cout, int cin, void* stream) {
    SIS_REQUIRE(u && w, "sis_modconv_prepack_wino44: null pointer");
    SIS_REQUIRE(cout > 0 && cin > 0, "sis_modconv_prepack_wino44: bad sizes");
    hipLaunchKernelGGL(wino44_prepack_kernel, dim3(sis_cdiv((int64_t)cout * cin, 256)), dim3(256), 0, (hipStream_t)stream, u, w, cout, cin);
    SIS_CHECK_LAUNCH("sis_modconv_prepack_wino44");
    return 0;
}

namespace {
constexpr Wino512Form WINO44_FORM = {4, 36, W44_UF, W44_VF, W44_T * 16, "modconv_wino44_kernel", "sis_modconv_wino44_eligible",
                                     modconv_wino44_kernel<true>, modconv_wino44_kernel<false>};
}

// wino512_plan's rule (4 x 4 outputs per tile: H % 4, W % 4)
extern "C" int sis_modconv_wino44_eligible(int cin, int cout, int h, int w) {
    ConvParams p;
    return wino512_plan(WINO44_FORM, p, cin, cout, h, w) > 0 ? 1 : 0;
}

extern "C" int sis_modconv2d_wino44(float* out, const float* x, const float* u44, const float* s, const float* dscale,
                                    const float* noise, int64_t noise_batch_stride, const float* noise_weight, const float* bias,
                                    int batch, int cin, int cout, int h, int w, int fuse_act, int tiles_per_wg, void* stream) {
    if (batch == 0) return 0;
    return wino512_launch<WINO44_FORM>("sis_modconv2d_wino44", out, x, u44, s, dscale, noise, noise_batch_stride, noise_weight, bias,
                                       batch, cin, cout, h, w, fuse_act, tiles_per_wg, nullptr, stream);
}

extern "C" int sis_modconv2d_wino44_rgb(float* out, float* rgb_part, const float* x, const float* u44, const float* s, const float* dscale,
                                        const float* noise, int64_t noise_batch_stride, const float* noise_weight, const float* bias,
                                        const float* rgb_w, const float* rgb_s, float rgb_scale, int batch, int cin, int cout, int h,
                                        int w, int fuse_act, int tiles_per_wg, void* stream) {
    if (batch == 0) return 0;
    SIS_REQUIRE(rgb_part && rgb_w && rgb_s, "sis_modconv2d_wino44_rgb: null pointer");
    SIS_REQUIRE(((uintptr_t)rgb_part & 15) == 0, "sis_modconv2d_wino44_rgb: rgb_part must be 16-byte aligned");
    const WinoRgb rgb = {rgb_w, rgb_s, rgb_part, rgb_scale};
    return wino512_launch<WINO44_FORM>("sis_modconv2d_wino44_rgb", out, x, u44, s, dscale, noise, noise_batch_stride, noise_weight,
                                       bias, batch, cin, cout, h, w, fuse_act, tiles_per_wg, &rgb, stream);
}
