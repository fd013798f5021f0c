// Modulated stride-1 3x3 "same" convolution of the generator with bf16 operands on v_mfma_f32_32x32x16_bf16 (opt-in:
// SIS_GEN_PRECISION=bf16 / Generator.set_matrix_precision; reference call sites networks/stylegan2/model.py:272-276, :287-292).
// Included at the end of conv_bf16.hip: the tile configuration (ConvCfg), the X-tile interleave, the swizzled LDS-DMA weight
// image and the issue-early / write-late staging are that file's; what differs is stated here.
//
//   y[b,co,h,w] = dscale[b,co] * sum_{ci,kh,kw} bf16(W[co,ci,kh,kw]) * bf16(fl32(s[b,ci] * x[b,ci,h+kh-1,w+kw-1]))
//   fuse:  y = lrelu_0.2(y + noise_weight * noise + bias) * sqrt(2)          (the tail of sis_modconv2d, in fp32)
//
// * Activations are fp32 in HBM on both sides.  A staging task loads 4 pixels of 8 channel rows as 8 x 16 bytes (issued before the
//   MFMAs of the running chunk); after them it multiplies each row by its style factor in fp32 ("modulate on load"), rounds the
//   products to bf16 with v_cvt_pk_bf16_f32 (round to nearest even, once) and interleaves them into 4 units of 8 channels.
//   The sample's style vector sits in LDS behind the two stages.
// * Weights: the raw parameter rounded once (RNE) by modconv_bf16_pack_kernel into the LDS image
//   [co tile][chunk of 16 channels][tap][row][unit ^ swizzle(row)][8 channels]; the conv scale stays inside dscale.  Rows beyond
//   Cout and channels beyond Cin (Cin % 16 == 8: the last chunk is half empty) are zeros, and the staging writes zeros for those
//   channels without loading anything.
// * One workgroup = one sample's MT output channels x 256 pixels (4 x 64, or 8 x 32 on maps up to 32 wide), the whole
//   contraction, chunks ascending: no split-K, no atomics, and the plan depends on (Cin, Cout, H, W) only.  The sums of an
//   output element are formed in the same order whatever the batch.
#pragma once

namespace {

struct ModBf16Params {
    const float* x;         // [N, Cin, H, W]
    const sis_u16* wp;      // packed bf16 weights
    const float* s;         // [N, Cin]
    const float* dscale;    // [N, Cout]
    const float* noise;     // [1 or N, 1, H, W] or null
    int64_t noise_stride;   // 0 or H * W
    const float* noise_weight;
    const float* bias;      // [Cout] or null
    float* out;             // [N, Cout, H, W]
    int N, Cin, Cout, H, W;
    int tiles_x, tiles_y, co_tiles, nchunks;
    int fuse;
};

constexpr int MODBF16_KC = 16;
constexpr int MODBF16_MIN_PIXELS = 256;   // one whole 256-pixel tile (see sis_modconv_bf16_eligible)
constexpr int MODBF16_MIN_WIDTH = 32;     // one whole tile row

__host__ __device__ constexpr int modbf16_mt(int cout) { return cout >= 128 ? 128 : 64; }

__device__ __forceinline__ unsigned modbf16_cvt_pk(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}

// One thread per packed element (see the header): w [Cout][Cin][3][3] fp32 -> bf16, RNE.
__global__ __launch_bounds__(256) void modconv_bf16_pack_kernel(sis_u16* __restrict__ out, const float* __restrict__ w, int Cout, int Cin,
                                                                int MT, int nchunks, int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    constexpr int units = MODBF16_KC / 8;
    int64_t r = e;
    const int j = r % 8; r /= 8;
    const int upos = r % units; r /= units;
    const int row = r % MT; r /= MT;
    const int tap = r % 9; r /= 9;
    const int chunk = r % nchunks; r /= nchunks;
    const int co = (int)r * MT + row, ci = chunk * MODBF16_KC + swz(upos, row, units) * 8 + j;
    float v = 0.f;
    if (co < Cout && ci < Cin) v = w[((int64_t)co * Cin + ci) * 9 + tap];
    const __hip_bfloat16 b = __float2bfloat16(v);
    out[e] = *reinterpret_cast<const sis_u16*>(&b);
}

template <typename C>
__global__ __launch_bounds__(512) void modconv_bf16_kernel(ModBf16Params p) {
    static_assert(C::KC == MODBF16_KC && C::KH == 3 && C::S == 1 && C::NT == 1 && C::NPIX == 256, "the modulated form is built for these");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm = wave % C::WM, wn = wave / C::WM;

    // XCD-aware tile order, as conv_bf16_kernel: the channel tiles that share an input tile take consecutive slots of one XCD
    const int slot = blockIdx.x >> 3;
    int t = (slot / p.co_tiles) * 8 + (blockIdx.x & 7);
    if (t >= p.N * p.tiles_y * p.tiles_x) return;
    const int co_t = slot % p.co_tiles;
    const int tx_i = t % p.tiles_x; t /= p.tiles_x;
    const int ty_i = t % p.tiles_y; t /= p.tiles_y;
    const int n = t;
    const int ox0 = tx_i * C::TW, oy0 = ty_i * C::TR;
    const int ix0 = ox0 - C::HALO, iy0 = oy0 - C::PAD;
    const int nchunks = p.nchunks;
    const int plane = p.H * p.W;

    const float* xin = p.x + (int64_t)n * p.Cin * plane;
    const sis_u16* wsrc = p.wp + (int64_t)co_t * nchunks * (C::WBYTES / 2);
    float* sl = reinterpret_cast<float*>(lds + 2 * C::STAGE);   // the sample's style vector, zeros from Cin to nchunks * 16

    // ---- this thread's staging task (fixed over the chunk loop): 8 channels x 4 pixels.  W % 4 == 0 and ix % 4 == 0: the four
    // pixels are inside the row together or outside it together.
    int task_goff = -1;   // element offset of (channel 0 of the plane, row, first pixel) inside a chunk; -2: zeros; -1: no task
    int task_lds = 0;     // byte offset of the first unit inside a stage's X region
    int task_ch = 0;      // first channel of the plane inside the chunk (0 or 8)
    if (tid < C::TASKS) {
        const int q = tid % (C::LW / 4);
        const int ry = (tid / (C::LW / 4)) % C::RI;
        const int pl = tid / ((C::LW / 4) * C::RI);
        const int iy = iy0 + ry, ix = ix0 + 4 * q;
        task_lds = ((pl * C::RI + ry) * C::LW + 4 * q) * 16;
        task_ch = pl * 8;
        const bool inside = iy >= 0 && iy < p.H && ix >= 0 && ix + 3 < p.W;
        task_goff = inside ? ((pl * 8) * p.H + iy) * p.W + ix : -2;   // fits 31 bits: one image's planes of a chunk
    }

    sis_f32x4 xr[8];  // staged pixels, still fp32 and unmodulated: [channel] = 4 pixels

    auto load_x = [&](int chunk) {
        const float* base = xin + (int64_t)chunk * C::KC * plane;
        if (task_goff >= 0 && chunk * C::KC + task_ch < p.Cin) {
            const float* g = base + task_goff;
#pragma unroll
            for (int c = 0; c < 8; ++c) xr[c] = *reinterpret_cast<const sis_f32x4*>(g + (int64_t)c * plane);
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) xr[c] = sis_f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };

    // modulate (fp32 product), round once to bf16, interleave 8 channels per pixel, write 4 units
    auto store_x = [&](int chunk, int stage) {
        if (task_goff == -1) return;
        unsigned char* xs = lds + stage * C::STAGE + C::WBYTES;
        const sis_f32x4 s0 = *reinterpret_cast<const sis_f32x4*>(sl + chunk * C::KC + task_ch);
        const sis_f32x4 s1 = *reinterpret_cast<const sis_f32x4*>(sl + chunk * C::KC + task_ch + 4);
        const float sv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        unsigned lo[8], hi[8];   // [channel]: pixels 0, 1 and pixels 2, 3 as bf16 pairs
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const sis_f32x4 m = xr[c] * sv[c];
            lo[c] = modbf16_cvt_pk(m.x, m.y);
            hi[c] = modbf16_cvt_pk(m.z, m.w);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned sel = (e & 1) ? 0x07060302u : 0x05040100u;
            const unsigned* v = e < 2 ? lo : hi;
            sis_u32x4 u;
            u.x = __builtin_amdgcn_perm(v[1], v[0], sel);
            u.y = __builtin_amdgcn_perm(v[3], v[2], sel);
            u.z = __builtin_amdgcn_perm(v[5], v[4], sel);
            u.w = __builtin_amdgcn_perm(v[7], v[6], sel);
            *reinterpret_cast<sis_u32x4*>(xs + task_lds + e * 16) = u;
        }
    };

    auto dma_w = [&](int chunk, int stage) {
        const unsigned char* src = reinterpret_cast<const unsigned char*>(wsrc) + (int64_t)chunk * C::WBYTES;
        unsigned char* dst = lds + stage * C::STAGE;
        for (int piece = wave; piece < C::WDMA; piece += 8)
            sis_global_load_lds16(src + piece * 1024 + lane * 16, dst + piece * 1024);
    };

    // ---- fragment addresses (as conv_bf16_kernel, one k-step per chunk)
    int a_off[C::MB];
#pragma unroll
    for (int mb = 0; mb < C::MB; ++mb) {
        const int row = (wm * C::MB + mb) * 32 + r;
        a_off[mb] = row * (C::KC * 2) + swz(h, row, C::P) * 16;
    }
    int b_off[C::NB];
#pragma unroll
    for (int nb = 0; nb < C::NB; ++nb) {
        const int blk = wn * C::NB + nb;
        const int ty = blk / (C::TW / 32), tx = (blk % (C::TW / 32)) * 32;
        b_off[nb] = C::WBYTES + ((h * C::RI + ty) * C::LW + tx + r + C::HALO - C::PAD) * 16;
    }

    sis_f32x16 acc[C::MB][C::NB];
#pragma unroll
    for (int mb = 0; mb < C::MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < C::NB; ++nb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mb][nb][i] = 0.f;

    // ---- prologue: chunk 0 into stage 0, the style vector behind the stages
    dma_w(0, 0);
    load_x(0);
    for (int c = tid; c < nchunks * C::KC; c += 512) sl[c] = c < p.Cin ? p.s[(int64_t)n * p.Cin + c] : 0.f;
    __syncthreads();
    store_x(0, 0);
    // Every wave waits for its own LDS-DMA pieces before the barrier: the other waves read them.  A wave without a staging task
    // has no load behind the DMA whose use would wait for it, and the barrier's fence alone compiles to lgkmcnt(0) here.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const int cur = chunk & 1;
        const bool more = chunk + 1 < nchunks;
        if (more) {
            dma_w(chunk + 1, cur ^ 1);
            load_x(chunk + 1);
        }
        const unsigned char* st = lds + cur * C::STAGE;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap % 3;
            sis_bf16x8 a[C::MB], b[C::NB];
#pragma unroll
            for (int mb = 0; mb < C::MB; ++mb)
                a[mb] = *reinterpret_cast<const sis_bf16x8*>(st + tap * (C::MT * C::KC * 2) + a_off[mb]);
#pragma unroll
            for (int nb = 0; nb < C::NB; ++nb)
                b[nb] = *reinterpret_cast<const sis_bf16x8*>(st + b_off[nb] + (ky * C::LW + kx) * 16);
#pragma unroll
            for (int mb = 0; mb < C::MB; ++mb)
#pragma unroll
                for (int nb = 0; nb < C::NB; ++nb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mb], b[nb], acc[mb][nb], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the write-late half of the staging behind the MFMAs
        if (more) store_x(chunk + 1, cur ^ 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the next chunk's weight pieces of this wave (see the prologue)
        __syncthreads();
    }

    // ---- epilogue in fp32: dscale, then the layer tail; lanes 0-31 of a register write 32 consecutive pixels of one channel row
    const float nwv = (p.fuse && p.noise) ? p.noise_weight[0] : 0.f;
    const float* nz = p.noise ? p.noise + (int64_t)n * p.noise_stride : nullptr;
    auto store_tile = [&](auto checked) {
#pragma unroll
        for (int mb = 0; mb < C::MB; ++mb) {
            const int co0 = co_t * C::MT + (wm * C::MB + mb) * 32 + 4 * h;  // row i = co0 + (i & 3) + 8 * (i >> 2)
            float dd[16], bb[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int co = min(co0 + (i & 3) + 8 * (i >> 2), p.Cout - 1);   // (rows >= Cout are not stored)
                dd[i] = p.dscale[(int64_t)n * p.Cout + co];
                bb[i] = (p.fuse && p.bias) ? p.bias[co] : 0.f;
            }
#pragma unroll
            for (int nb = 0; nb < C::NB; ++nb) {
                const int blk = wn * C::NB + nb;
                const int oy = oy0 + blk / (C::TW / 32), ox = ox0 + (blk % (C::TW / 32)) * 32 + r;
                if (oy >= p.H || ox >= p.W) continue;
                const float nzv = (p.fuse && nz) ? nwv * nz[oy * p.W + ox] : 0.f;
                float* yb = p.out + ((int64_t)n * p.Cout + co0) * plane + oy * p.W + ox;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int ro = (i & 3) + 8 * (i >> 2);
                    if (!decltype(checked)::value || co0 + ro < p.Cout) {
                        float val = acc[mb][nb][i] * dd[i];
                        if (p.fuse) {
                            val += nzv;
                            val += bb[i];
                            val = fmaxf(val, val * 0.2f) * 1.4142135623730951f;  // = (val > 0 ? val : 0.2 val) * sqrt(2)
                        }
                        yb[(int64_t)ro * plane] = val;
                    }
                }
            }
        }
    };
    if ((co_t + 1) * C::MT <= p.Cout) store_tile(std::false_type());
    else store_tile(std::true_type());
}

template <typename C>
int launch_modconv_bf16(const ModBf16Params& p, hipStream_t st) {
    const int lds_bytes = 2 * C::STAGE + p.nchunks * C::KC * (int)sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&modconv_bf16_kernel<C>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return sis_fail("sis_modconv2d_bf16: cannot raise the LDS limit: %s", hipGetErrorString(e));
        attr_set = true;
    }
    dim3 grid(8 * p.co_tiles * sis_cdiv((int64_t)p.N * p.tiles_y * p.tiles_x, 8));
    SIS_OCC_REPORT((modconv_bf16_kernel<C>), 512, lds_bytes);
    hipLaunchKernelGGL((modconv_bf16_kernel<C>), grid, dim3(512), lds_bytes, st, p);
    SIS_CHECK_LAUNCH("sis_modconv2d_bf16");
    sis_kernel_name = "modconv_bf16_kernel";
    return 0;
}

// The layer shapes the kernel takes, by (Cin, Cout, H, W) alone (see sis_hip.h).
bool modconv_bf16_takes(int cin, int cout, int h, int w) {
    if (cin <= 0 || cout <= 0 || h <= 0 || w <= 0) return false;
    if (cin % 8 || cin > 1024 || cout % 64 || w % 4 || w < MODBF16_MIN_WIDTH) return false;
    if ((int64_t)h * w < MODBF16_MIN_PIXELS) return false;
    if ((int64_t)cin * h * w >= ((int64_t)1 << 31) || (int64_t)cout * h * w >= ((int64_t)1 << 31)) return false;  // 31-bit offsets per sample
    return true;
}

}  // namespace

extern "C" int sis_modconv_bf16_eligible(int cin, int cout, int h, int w) { return modconv_bf16_takes(cin, cout, h, w) ? 1 : 0; }

extern "C" int64_t sis_modconv_bf16_packed_elems(int cin, int cout) {
    if (cin <= 0 || cout <= 0 || cin % 8 || cout % 64) return -1;
    const int mt = modbf16_mt(cout);
    return (int64_t)sis_cdiv(cout, mt) * mt * sis_cdiv(cin, MODBF16_KC) * MODBF16_KC * 9;
}

extern "C" int sis_modconv_prepack_bf16(void* packed, const float* w, int cout, int cin, void* stream) {
    SIS_REQUIRE(packed && w, "sis_modconv_prepack_bf16: null pointer");
    const int64_t total = sis_modconv_bf16_packed_elems(cin, cout);
    SIS_REQUIRE(total > 0, "sis_modconv_prepack_bf16: %d -> %d channels: Cin %% 8 == 0 and Cout %% 64 == 0 are required", cin, cout);
    hipLaunchKernelGGL(modconv_bf16_pack_kernel, dim3(sis_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (sis_u16*)packed, w, cout, cin,
                       modbf16_mt(cout), sis_cdiv(cin, MODBF16_KC), total);
    SIS_CHECK_LAUNCH("sis_modconv_prepack_bf16");
    return 0;
}

extern "C" int sis_modconv2d_bf16(float* out, const float* x, const void* packed, const float* s, const float* dscale,
                                  const float* noise, int64_t noise_batch_stride, const float* noise_weight, const float* bias,
                                  int batch, int cin, int cout, int h, int w, int fuse_act, void* stream) {
    if (batch == 0) return 0;
    SIS_REQUIRE(out && x && packed && s && dscale, "sis_modconv2d_bf16: null pointer");
    SIS_REQUIRE(batch > 0, "sis_modconv2d_bf16: non-positive size");
    if (noise) SIS_REQUIRE(noise_weight, "sis_modconv2d_bf16: noise given without noise_weight");
    SIS_REQUIRE(modconv_bf16_takes(cin, cout, h, w), "sis_modconv2d_bf16: shape %dx%d, %d -> %d not eligible (sis_modconv_bf16_eligible)", h, w,
                cin, cout);
    SIS_REQUIRE(((((uintptr_t)x | (uintptr_t)packed) & 15) == 0) && (((uintptr_t)out | (uintptr_t)s | (uintptr_t)dscale) & 3) == 0,
                "sis_modconv2d_bf16: x and the packed weights must be 16-byte aligned");
    ModBf16Params p;
    p.x = x; p.wp = (const sis_u16*)packed; p.s = s; p.dscale = dscale; p.noise = noise; p.noise_stride = noise_batch_stride;
    p.noise_weight = noise_weight; p.bias = bias; p.out = out;
    p.N = batch; p.Cin = cin; p.Cout = cout; p.H = h; p.W = w; p.fuse = fuse_act != 0;
    const int mt = modbf16_mt(cout), tw = w <= 32 ? 32 : 64;
    p.tiles_x = sis_cdiv(w, tw); p.tiles_y = sis_cdiv(h, 256 / tw);
    p.co_tiles = sis_cdiv(cout, mt); p.nchunks = sis_cdiv(cin, MODBF16_KC);
    SIS_REQUIRE((int64_t)8 * p.co_tiles * sis_cdiv((int64_t)batch * p.tiles_y * p.tiles_x, 8) < ((int64_t)1 << 31), "sis_modconv2d_bf16: bad grid");
    hipStream_t st = (hipStream_t)stream;
    if (mt == 128 && tw == 64) return launch_modconv_bf16<ConvCfg<128, 256, 16, 3, 1, 64>>(p, st);
    if (mt == 128 && tw == 32) return launch_modconv_bf16<ConvCfg<128, 256, 16, 3, 1, 32>>(p, st);
    if (mt == 64 && tw == 64) return launch_modconv_bf16<ConvCfg<64, 256, 16, 3, 1, 64>>(p, st);
    return launch_modconv_bf16<ConvCfg<64, 256, 16, 3, 1, 32>>(p, st);
}
