// PNG files of the dataset's [image | label] pairs, encoded on the device (create_dataset_for_segmentation.py:84-90 of the
// reference, save_image: there PIL on the host, one file at a time).  Included by dataset_ops.hip.  DESIGN.md §"PNG pairs
// encoded on the device" states the byte format; tests/png_restatement.py restates it, and the bytes written here EQUAL its bytes.
//
// One file per image: signature, IHDR, ONE IDAT, IEND.  Scanline r = image row r followed by label row r (the pair is never
// put together in memory), filter type 1 (Sub, bpp 3) on every row.  The IDAT payload is 78 01, one deflate block with the
// fixed Huffman codes, the end-of-block code (seven zero bits), zero bits to the byte boundary, Adler-32 of the filtered bytes.
// Tokens are per filtered row: a maximal run of R equal bytes is one literal, (R - 1) / 258 matches of length 258 at distance 1
// and the remainder r = (R - 1) % 258 as one match (r >= 3) or r literals -- which is what a greedy left-to-right scan with
// matches capped at 258 emits, and needs nothing but each byte's offset in its run.
//
// Launches (all on the caller's stream, integer arithmetic only, no host sync):
//   memset              the whole output buffer: every later store into it is an OR (or covers a whole dword)
//   png_count_kernel    grid (image, row): filter the row into LDS, tokens, the row's bit count and Adler partial sums
//   png_offsets_kernel  one workgroup per image: exclusive scan of the row bit counts (from bit 43 * 8 + 3 of the FILE, so that
//                       stores stay dword-aligned), Adler-32 in row order, file size, and every byte outside the deflate block
//                       except the IDAT CRC
//   png_emit_kernel     grid (image, row): tokens again, their bits assembled in LDS, whole dwords stored; a row's first and
//                       last dword are shared with its neighbours and go out as integer atomicOr (order-independent)
//   png_crc_kernel      raw CRC-32 of 512-byte pieces of "IDAT" + stream, each multiplied by x^(8 * bytes behind it) mod P
//                       and XORed into one word per image (XOR: order-independent as well)
//   png_finish_kernel   the init / final-XOR terms of CRC-32 (as zlib's crc32_combine treats them), the CRC's four bytes
// The token pass (png_tokenize_chunk) and the code table (png_fixed_code) are separate functions: dynamic Huffman codes would
// replace the second and add a histogram between the two.

namespace {

constexpr int PNG_THREADS = 256;
constexpr int PNG_MAX_WIDTH = 4096;            // image + label width: 51 KiB of LDS per row
constexpr uint32_t PNG_FIRST_BIT = 43 * 8 + 3;  // signature 8, IHDR 25, IDAT length + type 8, zlib header 2; BFINAL + BTYPE
constexpr uint32_t PNG_IDAT_TYPE_AT = 37;       // the IDAT CRC covers the file from here to the end of the Adler-32
constexpr uint32_t PNG_ADLER_MOD = 65521;
constexpr uint32_t PNG_CRC_POLY = 0xEDB88320u;
constexpr int PNG_CRC_PIECE = 512;
constexpr uint32_t PNG_TOK_NONE = 0xFFFFu, PNG_TOK_MATCH = 0x8000u;   // token: literal value | MATCH + length | NONE (inside a match)
constexpr int PNG_MAX_MATCH = 258;

// per-image workspace words: [0, H) row bit counts, then row start bits; [H, 2H) / [2H, 3H) the rows' Adler sums;
// [3H] byte offset of the Adler-32 in the file; [3H + 1] CRC accumulator; two spare
__host__ __device__ inline int64_t png_ws_words(int height) { return 3 * (int64_t)height + 4; }

struct PngBits {
    uint32_t value;   // as it enters the stream, least significant bit first
    int count;
};

__device__ __forceinline__ uint32_t png_msb_first(uint32_t code, int bits) { return __brev(code) >> (32 - bits); }

// Fixed Huffman codes (RFC 1951 §3.2.6) of a token; a match is the length code with the largest base <= length, its extra
// bits, and distance code 0 (five zero bits).
__device__ __forceinline__ PngBits png_fixed_code(uint32_t tok) {
    if (tok == PNG_TOK_NONE) return {0u, 0};
    if (!(tok & PNG_TOK_MATCH)) return tok < 144 ? PngBits{png_msb_first(0x30 + tok, 8), 8} : PngBits{png_msb_first(0x190 + tok - 144, 9), 9};
    const uint32_t len = tok & 0x7FFFu;
    uint32_t sym, extra_value = 0;
    int extra = 0;
    if (len == PNG_MAX_MATCH) sym = 285;
    else if (len < 11) sym = 254 + len;
    else {
        const uint32_t l3 = len - 3;   // 8 .. 254
        extra = 29 - __clz(l3);        // floor(log2) - 2
        sym = 257 + 4 * extra + (l3 >> extra);
        extra_value = l3 & ((1u << extra) - 1);
    }
    const int code_bits = sym < 280 ? 7 : 8;
    const uint32_t code = sym < 280 ? png_msb_first(sym - 256, 7) : png_msb_first(0xC0 + sym - 280, 8);
    return {code | (extra_value << code_bits), code_bits + extra + 5};
}

// Inclusive scan of one int per thread, in the order of `pos` (a permutation of 0 .. 255).  buf: 2 * PNG_THREADS ints.
template <class Op>
__device__ __forceinline__ void png_block_scan(int v, int pos, int identity, int* buf, Op op, int& incl, int& excl, int& total) {
    int* a = buf;
    int* b = buf + PNG_THREADS;
    a[pos] = v;
    __syncthreads();
    for (int d = 1; d < PNG_THREADS; d <<= 1) {
        int x = a[pos];
        if (pos >= d) x = op(a[pos - d], x);
        b[pos] = x;
        __syncthreads();
        int* t = a; a = b; b = t;
    }
    incl = a[pos];
    excl = pos > 0 ? a[pos - 1] : identity;
    total = a[PNG_THREADS - 1];
    __syncthreads();
}

// `nbytes` bytes from global memory to LDS, 4-byte loads over the aligned middle
__device__ __forceinline__ void png_load_bytes(uint8_t* dst, const uint8_t* __restrict__ src, int nbytes) {
    const int head = min((int)((4 - ((uintptr_t)src & 3)) & 3), nbytes);
    const int words = (nbytes - head) >> 2;
    for (int i = threadIdx.x; i < head; i += PNG_THREADS) dst[i] = src[i];
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src + head);
    for (int k = threadIdx.x; k < words; k += PNG_THREADS) {
        const uint32_t v = s4[k];
        uint8_t* d = dst + head + 4 * k;
        d[0] = (uint8_t)v; d[1] = (uint8_t)(v >> 8); d[2] = (uint8_t)(v >> 16); d[3] = (uint8_t)(v >> 24);
    }
    for (int i = head + 4 * words + threadIdx.x; i < nbytes; i += PNG_THREADS) dst[i] = src[i];
}

// Token of every byte of this thread's chunk [c0, c1) of the filtered row f[0, wb): run_start is the start of the run that
// reaches into the chunk, next_start the first run start behind the chunk (wb: none).  Returns the chunk's bit count under `code`.
template <class Code>
__device__ __forceinline__ int png_tokenize_chunk(uint16_t* tok, const uint8_t* f, int c0, int c1, int run_start, int next_start, Code code,
                                                  uint32_t& adler_a, uint32_t& adler_b, int wb) {
    int bits = 0, start = run_start, end = -1;
    for (int i = c0; i < c1; ++i) {
        const uint32_t v = f[i];
        if (i == 0 || v != f[i - 1]) start = i;
        if (end <= i) {   // the run's end: the next run start behind i
            int j = i + 1;
            while (j < c1 && f[j] == f[j - 1]) ++j;
            end = j < c1 ? j : next_start;
        }
        uint32_t t = v;   // the run's first byte, and a remainder of one or two bytes: literals
        if (i > start) {
            const int q = i - start - 1, followers = end - start - 1;
            const int k = q / PNG_MAX_MATCH, o = q - k * PNG_MAX_MATCH;
            const int piece = min(PNG_MAX_MATCH, followers - k * PNG_MAX_MATCH);
            if (piece >= 3) t = o == 0 ? (PNG_TOK_MATCH | (uint32_t)piece) : PNG_TOK_NONE;
        }
        tok[i] = (uint16_t)t;
        bits += code(t).count;
        adler_a += v;
        adler_b += (uint32_t)(wb - i) * v;   // < 256 * wb per byte, a chunk has at most 49 bytes
    }
    return bits;
}

template <bool EMIT>
__device__ __forceinline__ void png_row(uint32_t* __restrict__ out, const uint8_t* __restrict__ image, const uint8_t* __restrict__ label,
                                        uint32_t* __restrict__ ws, int height, int image_width, int label_width, int64_t stride_words) {
    extern __shared__ __attribute__((aligned(16))) uint8_t png_lds[];
    __shared__ int scan[2 * PNG_THREADS];
    __shared__ uint32_t sum_a, sum_b;
    const int t = threadIdx.x;
    const int n = blockIdx.x / height, r = blockIdx.x - n * height;
    const int ib = 3 * image_width, lb = 3 * label_width, wb = 1 + ib + lb;
    uint8_t* f = png_lds;                                                       // [wb] filtered row
    uint16_t* tok = reinterpret_cast<uint16_t*>(png_lds + ((wb + 3) & ~3));     // [wb]
    uint32_t* bitbuf = reinterpret_cast<uint32_t*>(png_lds + ((wb + 3) & ~3) + ((2 * wb + 3) & ~3));   // [(9 wb + 62) / 32 + 1]
    uint8_t* raw = reinterpret_cast<uint8_t*>(bitbuf);                          // [wb - 1], dead before bitbuf is cleared
    const int bit_words = (9 * wb + 62) / 32 + 1;
    if (t == 0) { sum_a = 0; sum_b = 0; }
    png_load_bytes(raw, image + ((int64_t)n * height + r) * ib, ib);
    if (lb) png_load_bytes(raw + ib, label + ((int64_t)n * height + r) * lb, lb);
    __syncthreads();
    for (int i = t; i < wb; i += PNG_THREADS) f[i] = i == 0 ? 1 : (uint8_t)(raw[i - 1] - (i >= 4 ? raw[i - 4] : 0));
    __syncthreads();
    if (EMIT)
        for (int i = t; i < bit_words; i += PNG_THREADS) bitbuf[i] = 0;   // (the scans below synchronise before the first OR)

    const int chunk = (wb + PNG_THREADS - 1) / PNG_THREADS;
    const int c0 = min(t * chunk, wb), c1 = min(c0 + chunk, wb);
    int last_start = -1, first_start = wb;
    for (int i = c0; i < c1; ++i)
        if (i == 0 || f[i] != f[i - 1]) { if (first_start == wb) first_start = i; last_start = i; }
    int incl, run_start, next_start, total;
    png_block_scan(last_start, t, -1, scan, [](int a, int b) { return max(a, b); }, incl, run_start, total);
    png_block_scan(first_start, PNG_THREADS - 1 - t, wb, scan, [](int a, int b) { return min(a, b); }, incl, next_start, total);

    uint32_t adler_a = 0, adler_b = 0;
    const int my_bits = png_tokenize_chunk(tok, f, c0, c1, run_start, next_start, [](uint32_t tk) { return png_fixed_code(tk); }, adler_a,
                                           adler_b, wb);
    int bit_excl, row_bits;
    png_block_scan(my_bits, t, 0, scan, [](int a, int b) { return a + b; }, incl, bit_excl, row_bits);

    uint32_t* w = ws + n * png_ws_words(height);
    if (!EMIT) {
        atomicAdd(&sum_a, adler_a);                    // <= 255 * wb in all
        atomicAdd(&sum_b, adler_b % PNG_ADLER_MOD);    // 256 terms below 2^16
        __syncthreads();
        if (t == 0) {
            w[r] = (uint32_t)row_bits;
            w[height + r] = sum_a % PNG_ADLER_MOD;
            w[2 * height + r] = sum_b % PNG_ADLER_MOD;
        }
        return;
    }
    const uint32_t first_bit = w[r];   // of the file
    const int phase = first_bit & 31;
    int pos = phase + bit_excl;
    for (int i = c0; i < c1; ++i) {
        const PngBits b = png_fixed_code(tok[i]);
        if (b.count) {
            const uint64_t v = (uint64_t)b.value << (pos & 31);
            atomicOr(&bitbuf[pos >> 5], (uint32_t)v);
            if (v >> 32) atomicOr(&bitbuf[(pos >> 5) + 1], (uint32_t)(v >> 32));
            pos += b.count;
        }
    }
    __syncthreads();
    const int n_words = (phase + row_bits + 31) >> 5;
    uint32_t* dst = out + n * stride_words + (first_bit >> 5);
    for (int d = t; d < n_words; d += PNG_THREADS) {
        const uint32_t v = bitbuf[d];
        if (d == 0 || d == n_words - 1) { if (v) atomicOr(dst + d, v); }   // shared with the neighbouring rows (or the header / trailer)
        else dst[d] = v;
    }
}

__global__ __launch_bounds__(PNG_THREADS) void png_count_kernel(const uint8_t* __restrict__ image, const uint8_t* __restrict__ label,
                                                                uint32_t* __restrict__ ws, int height, int image_width, int label_width) {
    png_row<false>(nullptr, image, label, ws, height, image_width, label_width, 0);
}

__global__ __launch_bounds__(PNG_THREADS) void png_emit_kernel(uint32_t* __restrict__ out, const uint8_t* __restrict__ image,
                                                               const uint8_t* __restrict__ label, uint32_t* __restrict__ ws, int height,
                                                               int image_width, int label_width, int64_t stride_words) {
    png_row<true>(out, image, label, ws, height, image_width, label_width, stride_words);
}

// one byte of a file whose buffer starts zeroed and is shared with the rows' ORs
__device__ __forceinline__ void png_or_byte(uint32_t* file, uint32_t offset, uint32_t value) {
    if (value) atomicOr(file + (offset >> 2), value << (8 * (offset & 3)));
}
__device__ __forceinline__ void png_or_be32(uint32_t* file, uint32_t offset, uint32_t value) {
    for (int k = 0; k < 4; ++k) png_or_byte(file, offset + k, (value >> (24 - 8 * k)) & 255u);
}

__global__ __launch_bounds__(PNG_THREADS) void png_offsets_kernel(uint32_t* __restrict__ out, int* __restrict__ sizes, uint32_t* __restrict__ ws,
                                                                  int height, int width_total, int64_t stride_words, uint32_t ihdr_crc) {
    __shared__ uint32_t s_bits[PNG_THREADS], s_a[PNG_THREADS], s_b[PNG_THREADS];
    const int t = threadIdx.x, n = blockIdx.x;
    uint32_t* w = ws + n * png_ws_words(height);
    const uint32_t wb = 1 + 3 * (uint32_t)width_total;
    uint32_t bit = PNG_FIRST_BIT, a = 1, b = 0;   // thread 0's
    for (int base = 0; base < height; base += PNG_THREADS) {
        const int r = base + t;
        if (r < height) { s_bits[t] = w[r]; s_a[t] = w[height + r]; s_b[t] = w[2 * height + r]; }
        __syncthreads();
        if (t == 0) {
            const int rows = min(PNG_THREADS, height - base);
            for (int k = 0; k < rows; ++k) {
                const uint32_t bits = s_bits[k];
                s_bits[k] = bit;
                bit += bits;
                b = (uint32_t)((b + (uint64_t)wb * a + s_b[k]) % PNG_ADLER_MOD);   // a row of wb bytes behind (a, b)
                a = (a + s_a[k]) % PNG_ADLER_MOD;
            }
        }
        __syncthreads();
        if (r < height) w[r] = s_bits[t];
        __syncthreads();
    }
    if (t != 0) return;
    const uint32_t adler_at = (bit + 7 + 7) >> 3;   // end-of-block code: seven zero bits, then zero bits to the byte boundary
    w[3 * height] = adler_at;
    w[3 * height + 1] = 0;
    sizes[n] = (int)(adler_at + 4 + 4 + 12);
    uint32_t* file = out + n * stride_words;
    const uint8_t head[16] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
    for (int k = 0; k < 16; ++k) png_or_byte(file, k, head[k]);
    png_or_be32(file, 16, (uint32_t)width_total);
    png_or_be32(file, 20, (uint32_t)height);
    png_or_byte(file, 24, 8);    // bit depth
    png_or_byte(file, 25, 2);    // colour type: RGB (compression, filter method, interlace: 0)
    png_or_be32(file, 29, ihdr_crc);
    png_or_be32(file, 33, adler_at + 4 - 41);   // IDAT length: the zlib stream
    png_or_byte(file, 37, 'I'); png_or_byte(file, 38, 'D'); png_or_byte(file, 39, 'A'); png_or_byte(file, 40, 'T');
    png_or_byte(file, 41, 0x78); png_or_byte(file, 42, 0x01);
    png_or_byte(file, 43, 3);    // BFINAL = 1, BTYPE = 01
    png_or_be32(file, adler_at, (b << 16) | a);
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int k = 0; k < 12; ++k) png_or_byte(file, adler_at + 8 + k, iend[k]);
}

// a * b mod P over GF(2), reflected representation (bit 31 = x^0), 32 shift-and-add steps
__device__ __forceinline__ uint32_t png_gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b >> 1) ^ ((b & 1) ? PNG_CRC_POLY : 0u);
    }
    return p;
}
__device__ __forceinline__ uint32_t png_gf_xpow8(uint32_t nbytes) {   // x^(8 nbytes) mod P, square and multiply
    uint32_t r = 0x80000000u, base = 0x00800000u;
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1) r = png_gf_mul(r, base);
        base = png_gf_mul(base, base);
    }
    return r;
}

__global__ __launch_bounds__(PNG_THREADS) void png_crc_kernel(const uint32_t* __restrict__ out, uint32_t* __restrict__ ws, int height,
                                                              int64_t stride_words) {
    __shared__ uint32_t table[256];
    __shared__ uint32_t block_acc;
    const int t = threadIdx.x, n = blockIdx.y;
    {
        uint32_t c = t;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1) ? PNG_CRC_POLY : 0u);
        table[t] = c;
    }
    if (t == 0) block_acc = 0;
    __syncthreads();
    uint32_t* w = ws + n * png_ws_words(height);
    const uint32_t end = w[3 * height] + 4;   // behind the Adler-32
    const uint32_t* file = out + n * stride_words;
    const uint32_t piece = blockIdx.x * PNG_THREADS + t;
    const uint32_t lo = max(piece * PNG_CRC_PIECE, PNG_IDAT_TYPE_AT), hi = min((piece + 1) * PNG_CRC_PIECE, end);
    uint32_t term = 0;
    if (lo < hi) {
        uint32_t crc = 0;   // raw: no init, no final XOR -- linear, so pieces combine by multiplication
        for (uint32_t word = lo >> 2; 4 * word < hi; ++word) {
            const uint32_t v = file[word];
            for (int k = 0; k < 4; ++k) {
                const uint32_t at = 4 * word + k;
                if (at >= lo && at < hi) crc = table[(crc ^ (v >> (8 * k))) & 255u] ^ (crc >> 8);
            }
        }
        term = png_gf_mul(crc, png_gf_xpow8(end - hi));
    }
    for (int d = 32; d; d >>= 1) term ^= __shfl_xor(term, d, 64);
    if ((t & 63) == 0 && term) atomicXor(&block_acc, term);
    __syncthreads();
    if (t == 0 && block_acc) atomicXor(&w[3 * height + 1], block_acc);
}

__global__ __launch_bounds__(64) void png_finish_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ ws, int n_images, int height,
                                                        int64_t stride_words) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= n_images) return;
    const uint32_t* w = ws + n * png_ws_words(height);
    const uint32_t adler_at = w[3 * height];
    // crc32(M) = raw(M) ^ raw of the 0xFFFFFFFF init carried through |M| bytes ^ the final XOR
    const uint32_t crc = w[3 * height + 1] ^ png_gf_mul(0xFFFFFFFFu, png_gf_xpow8(adler_at + 4 - PNG_IDAT_TYPE_AT)) ^ 0xFFFFFFFFu;
    png_or_be32(out + n * stride_words, adler_at + 4, crc);
}

}  // namespace

extern "C" int64_t sis_png_capacity(int height, int width_total) {
    if (height < 1 || width_total < 1) return 0;
    const int64_t f = (int64_t)height * (1 + 3 * (int64_t)width_total);
    const int64_t z = 2 + (10 + 9 * f + 7) / 8 + 4;
    return (57 + z + 15) / 16 * 16;
}

extern "C" int64_t sis_png_encode_pairs_workspace_bytes(int n, int height) {
    return n < 1 || height < 1 ? 0 : (int64_t)n * png_ws_words(height) * 4;
}

extern "C" int sis_png_encode_pairs(uint8_t* out, int* sizes, const uint8_t* image, const uint8_t* label, int n, int height, int image_width,
                                    int label_width, int64_t out_stride, uint32_t ihdr_crc, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
    SIS_REQUIRE(n >= 1 && height >= 1 && image_width >= 1 && label_width >= 0, "sis_png_encode_pairs: n %d, height %d, widths %d + %d: all must be >= 1",
                n, height, image_width, label_width);
    SIS_REQUIRE((label != nullptr) == (label_width > 0), "sis_png_encode_pairs: a label needs a width >= 1, and no label width 0");
    SIS_REQUIRE((int64_t)image_width + label_width <= PNG_MAX_WIDTH, "sis_png_encode_pairs: total width %lld above %d",
                (long long)image_width + label_width, PNG_MAX_WIDTH);
    const int width_total = image_width + label_width;
    const int64_t capacity = sis_png_capacity(height, width_total);
    SIS_REQUIRE(capacity <= ((int64_t)1 << 28), "sis_png_encode_pairs: a file of up to %lld bytes (bit offsets are 32-bit)", (long long)capacity);
    SIS_REQUIRE(out_stride >= capacity, "sis_png_encode_pairs: out_stride %lld below sis_png_capacity = %lld", (long long)out_stride,
                (long long)capacity);
    SIS_REQUIRE(out_stride % 16 == 0, "sis_png_encode_pairs: out_stride %lld is no multiple of 16", (long long)out_stride);
    SIS_REQUIRE(n <= 65535 && (int64_t)n * height < ((int64_t)1 << 31), "sis_png_encode_pairs: %d images x %d rows in one call", n, height);
    SIS_REQUIRE(out && sizes && image && workspace, "sis_png_encode_pairs: null pointer");
    SIS_REQUIRE((((uintptr_t)out) & 15) == 0 && (((uintptr_t)workspace) & 3) == 0 && (((uintptr_t)sizes) & 3) == 0,
                "sis_png_encode_pairs: out must be 16-byte, sizes and workspace 4-byte aligned");
    SIS_REQUIRE(workspace_bytes >= sis_png_encode_pairs_workspace_bytes(n, height), "sis_png_encode_pairs: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)sis_png_encode_pairs_workspace_bytes(n, height));
    hipStream_t st = (hipStream_t)stream;
    uint32_t* out32 = reinterpret_cast<uint32_t*>(out);
    uint32_t* ws = reinterpret_cast<uint32_t*>(workspace);
    const int64_t stride_words = out_stride / 4;
    const int wb = 1 + 3 * width_total;
    const size_t lds = (size_t)((wb + 3) & ~3) + (size_t)((2 * wb + 3) & ~3) + 4 * (size_t)((9 * wb + 62) / 32 + 1);
    if (hipMemsetAsync(out, 0, (size_t)n * out_stride, st) != hipSuccess) return sis_fail("sis_png_encode_pairs: cannot clear the output");
    hipLaunchKernelGGL(png_count_kernel, dim3(n * height), dim3(PNG_THREADS), lds, st, image, label, ws, height, image_width, label_width);
    SIS_CHECK_LAUNCH("png_count_kernel");
    hipLaunchKernelGGL(png_offsets_kernel, dim3(n), dim3(PNG_THREADS), 0, st, out32, sizes, ws, height, width_total, stride_words, ihdr_crc);
    SIS_CHECK_LAUNCH("png_offsets_kernel");
    hipLaunchKernelGGL(png_emit_kernel, dim3(n * height), dim3(PNG_THREADS), lds, st, out32, image, label, ws, height, image_width, label_width,
                       stride_words);
    SIS_CHECK_LAUNCH("png_emit_kernel");
    const int pieces = sis_cdiv(capacity, PNG_CRC_PIECE);
    hipLaunchKernelGGL(png_crc_kernel, dim3(sis_cdiv(pieces, PNG_THREADS), n), dim3(PNG_THREADS), 0, st, (const uint32_t*)out32, ws, height,
                       stride_words);
    SIS_CHECK_LAUNCH("png_crc_kernel");
    hipLaunchKernelGGL(png_finish_kernel, dim3(sis_cdiv(n, 64)), dim3(64), 0, st, out32, (const uint32_t*)ws, n, height, stride_words);
    SIS_CHECK_LAUNCH("png_finish_kernel");
    return 0;
}
