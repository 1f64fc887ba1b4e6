// FLAC encoder kernels (flac_kernels.h).  The specification is the host writer, auralis_amd/api/flac.py:70-178: every choice below
// (predictor order, partition order, Rice parameters, VERBATIM fallback, STREAMINFO fields) is that file's, in integer arithmetic.
#include "flac_kernels.h"

namespace aur {

// _to_int(x, 2) of auralis_amd/api/codecs.py: clamp to [-1, 1], * 32767.0f in fp32, convert toward zero (inputs are finite)
__device__ __forceinline__ int flac_quantise(float v) { return (int)(fminf(fmaxf(v, -1.0f), 1.0f) * 32767.0f); }

// ------------------------------------------------------------------------------------------------ MD5 (RFC 1321)
// One wave per row.  The padded message is taken 128 samples (64 words, four 64-byte blocks) at a time: lane l loads and quantises
// the two samples of word l, the words go through LDS and every lane runs the same four compressions (the loads of the next chunk are
// issued before them).  Lane 0 stores the digest.
__device__ __forceinline__ uint32_t md5_word(const float* __restrict__ x, long w, long n, long words) {
    // word w of the padded little-endian int16 message of n samples: 0x80 behind the last byte, zeros, the bit count in the last two words
    if (w >= words) return 0u;
    if (w == words - 2) return (uint32_t)((unsigned long long)n * 16ull);
    if (w == words - 1) return (uint32_t)(((unsigned long long)n * 16ull) >> 32);
    const long i0 = 2 * w, i1 = 2 * w + 1;
    const uint32_t lo = i0 < n ? (uint32_t)(flac_quantise(x[i0]) & 0xFFFF) : (i0 == n ? 0x80u : 0u);
    const uint32_t hi = i1 < n ? (uint32_t)(flac_quantise(x[i1]) & 0xFFFF) : (i1 == n ? 0x80u : 0u);
    return lo | (hi << 16);
}

__device__ __forceinline__ void md5_block(uint32_t& a0, uint32_t& b0, uint32_t& c0, uint32_t& d0, const uint32_t* __restrict__ m) {
    constexpr uint32_t K[64] = {
        0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501, 0x698098d8, 0x8b44f7af, 0xffff5bb1,
        0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821, 0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453,
        0xd8a1e681, 0xe7d3fbc8, 0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a, 0xfffa3942,
        0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70, 0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05,
        0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665, 0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d,
        0x85845dd1, 0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391};
    constexpr int S[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};
    uint32_t M[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) M[i] = m[i];
    uint32_t A = a0, B = b0, C = c0, D = d0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        uint32_t F;
        int g;
        if (i < 16) F = (B & C) | (~B & D), g = i;
        else if (i < 32) F = (D & B) | (~D & C), g = (5 * i + 1) & 15;
        else if (i < 48) F = B ^ C ^ D, g = (3 * i + 5) & 15;
        else F = C ^ (B | ~D), g = (7 * i) & 15;
        F = F + A + K[i] + M[g];
        A = D, D = C, C = B;
        const int s = S[(i >> 4) * 4 + (i & 3)];
        B = B + ((F << s) | (F >> (32 - s)));
    }
    a0 += A, b0 += B, c0 += C, d0 += D;
}

__global__ __launch_bounds__(64) void flac_md5_kernel(const float* __restrict__ x, long x_bstride, const int* __restrict__ rows,
                                                      const int* __restrict__ len, uint8_t* __restrict__ md5) {
    __shared__ uint32_t s_m[64];
    const int b = blockIdx.x, lane = threadIdx.x;
    const long n = len[b];
    const float* row = x + (long)(rows ? rows[b] : b) * x_bstride;
    const long words = ((2 * n + 8) / 64 + 1) * 16;   // message + 0x80 + zeros + 8 length bytes, in whole 64-byte blocks
    uint32_t A = 0x67452301u, B = 0xefcdab89u, C = 0x98badcfeu, D = 0x10325476u;
    uint32_t next = md5_word(row, lane, n, words);
    for (long w0 = 0; w0 < words; w0 += 64) {
        __syncthreads();   // the previous chunk's reads are done
        s_m[lane] = next;
        __syncthreads();
        next = md5_word(row, w0 + 64 + lane, n, words);
        const int blocks = (int)((words - w0 < 64 ? words - w0 : 64) / 16);
        for (int k = 0; k < blocks; ++k) md5_block(A, B, C, D, s_m + 16 * k);
    }
    if (lane == 0) {
        uint32_t* o = reinterpret_cast<uint32_t*>(md5 + (long)b * 16);   // little-endian words: the digest's byte order
        o[0] = A, o[1] = B, o[2] = C, o[3] = D;
    }
}

// ------------------------------------------------------------------------------------------------ frames
constexpr int kBitWords = kFlacSlot / 4;              // the frame's bit buffer in LDS, 32-bit words holding big-endian bit order
constexpr int kCrcWords = (kBitWords + 255) / 256;    // words per thread of the CRC-16 pass
__device__ __forceinline__ int pad16(int i) { return i + (i >> 4); }   // thread t's 16 consecutive words: bank-conflict free

// `nbits` (1..16) bits of v at bit position pos of the frame (bit 0 = the MSB of byte 0).  Neighbouring codes share words: LDS atomic OR.
// A position outside the buffer is not written and raises *bad: the frame is then reported with length -1 and its stream with length 0,
// which every caller refuses (a frame is bounded by kFlacFrameMax, so this is a wrong offset, never a long frame).
__device__ __forceinline__ void put_bits(uint32_t* bits, int* bad, int pos, uint32_t v, int nbits) {
    const int w = pos >> 5, sh = 32 - (pos & 31) - nbits;
    if (sh >= 0) {
        if (w < 0 || w >= kBitWords) { *bad = 1; return; }
        atomicOr(bits + w, v << sh);
    } else {
        if (w < 0 || w + 1 >= kBitWords) { *bad = 1; return; }
        atomicOr(bits + w, v >> -sh);
        atomicOr(bits + w + 1, v << (32 + sh));
    }
}

__device__ __forceinline__ uint32_t crc8_step(uint32_t c, uint32_t byte) {   // poly 0x07, MSB first
    c ^= byte;
#pragma unroll
    for (int i = 0; i < 8; ++i) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xFFu : (c << 1) & 0xFFu;
    return c;
}
__device__ __forceinline__ uint32_t crc16_step(uint32_t c, uint32_t byte) {   // poly 0x8005, initial value 0, MSB first
    c ^= byte << 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xFFFFu : (c << 1) & 0xFFFFu;
    return c;
}
// a * b in GF(2)[x] / (x^16 + x^15 + x^2 + 1)
__device__ __forceinline__ uint32_t gf16_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 15; i >= 0; --i) {
        r = (r & 0x8000u) ? ((r << 1) ^ 0x8005u) & 0xFFFFu : (r << 1) & 0xFFFFu;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
// x^(8 m) in that field: what m zero bytes behind a message do to its CRC (initial value 0, no final XOR: the CRC is linear,
// crc(A || B) = crc(A) * x^(8 |B|) + crc(B))
__device__ __forceinline__ uint32_t gf16_xpow8(uint32_t m) {
    uint32_t r = 1u, sq = 0x0100u;   // x^8
    for (; m; m >>= 1) {
        if (m & 1u) r = gf16_mul(r, sq);
        sq = gf16_mul(sq, sq);
    }
    return r;
}

template <class T>
__device__ __forceinline__ T wave_add(T v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One workgroup per (block, row): 256 threads x 16 consecutive samples.
__global__ __launch_bounds__(256) void flac_frame_kernel(const float* __restrict__ x, long x_bstride, const int* __restrict__ rows,
                                                         const int* __restrict__ len, int max_frames, uint8_t* __restrict__ slots, int* __restrict__ flen) {
    __shared__ int s_v[kFlacBlock + kFlacBlock / 16];              // the samples, then the zigzagged residual (pad16 layout)
    __shared__ uint32_t s_bits[kBitWords];
    __shared__ unsigned long long s_fine[16][15];                  // sum of u >> k over each of the finest partitions, k = 0..14
    __shared__ unsigned s_cost[4][5];                              // per wave: sum |r| of the five orders
    __shared__ int s_neq[4];
    __shared__ unsigned long long s_pcost[31];                     // partition p of order po at (1 << po) - 1 + p: its Rice bits
    __shared__ int s_pk[31];                                       // ... and parameter
    __shared__ int s_k[16];                                        // the chosen partitioning's parameters
    __shared__ int s_choice[4];                                    // kind (0 CONSTANT, 1 VERBATIM, 2 FIXED), order, partition order, body bits
    __shared__ int s_wsum[4];
    __shared__ uint32_t s_crc[4];
    __shared__ int s_bad;                                          // put_bits refused a position

    const int b = blockIdx.y, blk = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const long total = len[b];
    if ((long)blk * kFlacBlock >= total) return;   // (uniform per workgroup)
    const int n = (int)(total - (long)blk * kFlacBlock < kFlacBlock ? total - (long)blk * kFlacBlock : kFlacBlock);
    const float* row = x + (long)(rows ? rows[b] : b) * x_bstride + (long)blk * kFlacBlock;

    for (int i = t; i < kFlacBlock; i += 256) s_v[pad16(i)] = i < n ? flac_quantise(row[i]) : 0;
    for (int i = t; i < kBitWords; i += 256) s_bits[i] = 0u;
    if (t < 16 * 15) s_fine[t / 15][t % 15] = 0ull;
    if (t == 0) s_bad = 0;
    __syncthreads();

    // ---- the five residuals of this thread's samples: s[4 + m] = x[16 t + m], s[0..3] the four samples in front
    const int j0 = t * 16;
    int s[20];
#pragma unroll
    for (int m = 0; m < 20; ++m) {
        const int i = j0 - 4 + m;
        s[m] = i >= 0 ? s_v[pad16(i)] : 0;
    }
    const int first = s_v[0];
    __syncthreads();   // s_v is rewritten below
    unsigned cost[5] = {0u, 0u, 0u, 0u, 0u};
    int neq = 0;
    int d[4][20];   // d[o - 1][m]: o-th difference at sample j0 - 4 + m (valid from m >= o on)
#pragma unroll
    for (int m = 1; m < 20; ++m) d[0][m] = s[m] - s[m - 1];
#pragma unroll
    for (int o = 1; o < 4; ++o)
#pragma unroll
        for (int m = o + 1; m < 20; ++m) d[o][m] = d[o - 1][m] - d[o - 1][m - 1];
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        const int i = j0 + m;
        if (i < n) neq |= s[4 + m] != first;
        if (i >= 4 && i < n) {   // every order over the same samples; |4th difference| <= 2^19 and 4092 of them stay below 2^31
            cost[0] += (unsigned)abs(s[4 + m]);
#pragma unroll
            for (int o = 0; o < 4; ++o) cost[o + 1] += (unsigned)abs(d[o][4 + m]);
        }
    }
#pragma unroll
    for (int o = 0; o < 5; ++o) {
        const unsigned c = wave_add(cost[o]);
        if (lane == 0) s_cost[wave][o] = c;
    }
    neq = wave_add(neq);
    if (lane == 0) s_neq[wave] = neq;
    __syncthreads();
    const bool constant = (s_neq[0] | s_neq[1] | s_neq[2] | s_neq[3]) == 0;
    int order = 0;
    if (n > 4) {
        unsigned best = 0xFFFFFFFFu;
#pragma unroll
        for (int o = 0; o < 5; ++o) {
            const unsigned c = s_cost[0][o] + s_cost[1][o] + s_cost[2][o] + s_cost[3][o];
            if (c < best) best = c, order = o;   // the first minimum
        }
    }
    // partition orders 0 .. po_max are valid: the first po with n % 2^po != 0 or (n >> po) <= order ends the list
    int po_max = 0;
    while (po_max < 4 && n % (2 << po_max) == 0 && (n >> (po_max + 1)) > order) ++po_max;
    const int fine = n >> po_max;   // samples per finest partition

    // ---- zigzag the chosen residual; sums of u >> k per finest partition
    if (!constant) {
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int e = order == 0 ? s[4 + m] : order == 1 ? d[0][4 + m] : order == 2 ? d[1][4 + m] : order == 3 ? d[2][4 + m] : d[3][4 + m];
            s_v[pad16(j0 + m)] = e >= 0 ? 2 * e : -2 * e - 1;
        }
        // (each thread reads back its own words only: no barrier)
        unsigned acc[15];
#pragma unroll
        for (int k = 0; k < 15; ++k) acc[k] = 0u;
        int cur = -1;
#pragma unroll 1
        for (int m = 0; m < 16; ++m) {
            const int i = j0 + m;
            if (i < order || i >= n) continue;
            const int p = i / fine;
            if (p != cur) {
                if (cur >= 0) {
#pragma unroll
                    for (int k = 0; k < 15; ++k) atomicAdd(&s_fine[cur][k], (unsigned long long)acc[k]), acc[k] = 0u;
                }
                cur = p;
            }
            const unsigned u = (unsigned)s_v[pad16(i)];
#pragma unroll
            for (int k = 0; k < 15; ++k) acc[k] += u >> k;
        }
        if (cur >= 0) {
#pragma unroll
            for (int k = 0; k < 15; ++k) atomicAdd(&s_fine[cur][k], (unsigned long long)acc[k]);
        }
    }
    __syncthreads();

    // ---- Rice parameter and bits of every partition of every valid order (31 at most), one thread each
    if (!constant && t < 31) {
        int po = 0;
        while ((2 << po) - 1 <= t) ++po;
        const int p = t - ((1 << po) - 1);
        if (po <= po_max) {
            const int c0 = p << (po_max - po), c1 = (p + 1) << (po_max - po);
            const unsigned long long cnt = (unsigned long long)((n >> po) - (p == 0 ? order : 0));
            unsigned long long su = 0ull;
            for (int c = c0; c < c1; ++c) su += s_fine[c][0];
            // k0 = min(14, floor(log2(mean + 1))): the largest k <= 14 with cnt * 2^k <= sum + cnt
            int k0 = 0;
            while (k0 < 14 && (cnt << (k0 + 1)) <= su + cnt) ++k0;
            unsigned long long best = ~0ull;
            int kb = 0;
            for (int k = (k0 > 0 ? k0 - 1 : 0); k <= (k0 < 14 ? k0 + 1 : 14); ++k) {
                unsigned long long sk = 0ull;
                for (int c = c0; c < c1; ++c) sk += s_fine[c][k];
                const unsigned long long bits = cnt * (unsigned long long)(k + 1) + sk;
                if (bits < best) best = bits, kb = k;   // the lower k wins ties
            }
            s_pcost[t] = best;
            s_pk[t] = kb;
        }
    }
    __syncthreads();
    if (t == 0) {
        int kind = 0, po_best = 0, body = 8 + 16;
        if (!constant) {
            unsigned long long best = ~0ull;
            for (int po = 0; po <= po_max; ++po) {
                unsigned long long bits = 6ull;
                for (int p = 0; p < (1 << po); ++p) bits += 4ull + s_pcost[(1 << po) - 1 + p];
                if (bits < best) best = bits, po_best = po;   // the lowest partition order wins ties
            }
            if (best >= (unsigned long long)(n - order) * 16ull) kind = 1, body = 8 + n * 16;
            else kind = 2, body = 8 + order * 16 + (int)best;
        }
        s_choice[0] = kind, s_choice[1] = order, s_choice[2] = po_best, s_choice[3] = body;
    }
    __syncthreads();
    const int kind = s_choice[0], po = s_choice[2], body_bits = s_choice[3];
    if (t < (1 << po)) s_k[t] = s_pk[(1 << po) - 1 + t];

    // ---- header (thread 0): sync, block size, sample size, frame number, CRC-8; the subframe's fixed fields
    const int n_utf = blk < 0x80 ? 1 : blk < 0x800 ? 2 : 3;
    const int head_bytes = 4 + n_utf + (n == kFlacBlock ? 0 : 2) + 1;
    const int body0 = head_bytes * 8;
    if (t == 0) {
        uint32_t crc = 0u;
        int pos = 0;
        auto emit = [&](uint32_t byte) {
            put_bits(s_bits, &s_bad, pos, byte, 8);
            crc = crc8_step(crc, byte);
            pos += 8;
        };
        emit(0xFFu), emit(0xF8u), emit(n == kFlacBlock ? 0xC0u : 0x70u), emit(0x08u);
        if (n_utf == 1) {
            emit((uint32_t)blk);
        } else if (n_utf == 2) {
            emit(0xC0u | (uint32_t)(blk >> 6)), emit(0x80u | (uint32_t)(blk & 0x3F));
        } else {
            emit(0xE0u | (uint32_t)(blk >> 12)), emit(0x80u | (uint32_t)((blk >> 6) & 0x3F)), emit(0x80u | (uint32_t)(blk & 0x3F));
        }
        if (n != kFlacBlock) emit((uint32_t)((n - 1) >> 8)), emit((uint32_t)((n - 1) & 0xFF));
        put_bits(s_bits, &s_bad, pos, crc, 8);
        if (kind == 0) {
            put_bits(s_bits, &s_bad, body0 + 8, (uint32_t)first & 0xFFFFu, 16);   // subframe header 0x00, the value
        } else if (kind == 1) {
            put_bits(s_bits, &s_bad, body0, 0x02u, 8);
        } else {
            put_bits(s_bits, &s_bad, body0, (uint32_t)((8 | order) << 1), 8);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < order) put_bits(s_bits, &s_bad, body0 + 8 + 16 * i, (uint32_t)s[4 + i] & 0xFFFFu, 16);   // warm-up samples (thread 0 holds them)
            put_bits(s_bits, &s_bad, body0 + 8 + 16 * order, (uint32_t)po, 6);   // method 00, partition order
        }
    }
    __syncthreads();   // s_k

    if (kind == 1) {
#pragma unroll
        for (int m = 0; m < 16; ++m)
            if (j0 + m < n) put_bits(s_bits, &s_bad, body0 + 8 + 16 * (j0 + m), (uint32_t)s[4 + m] & 0xFFFFu, 16);
    } else if (kind == 2) {
        // code lengths -> bit offsets: this thread's total, an exclusive scan over the workgroup
        const int psize = n >> po;
        int mine = 0;
#pragma unroll 1
        for (int m = 0; m < 16; ++m) {
            const int i = j0 + m;
            if (i < order || i >= n) continue;
            const int k = s_k[i / psize];
            mine += (int)((unsigned)s_v[pad16(i)] >> k) + 1 + k;
        }
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        int run = incl - mine;
        for (int w = 0; w < wave; ++w) run += s_wsum[w];
        const int res0 = body0 + 8 + 16 * order + 6;   // the first partition's parameter
#pragma unroll 1
        for (int m = 0; m < 16; ++m) {
            const int i = j0 + m;
            if (i < order || i >= n) continue;
            const int p = i / psize, k = s_k[p];
            const unsigned u = (unsigned)s_v[pad16(i)];
            const int q = (int)(u >> k);
            const int pos = res0 + 4 * (p + 1) + run;
            if (i == (p == 0 ? order : p * psize)) put_bits(s_bits, &s_bad, pos - 4, (uint32_t)k, 4);
            put_bits(s_bits, &s_bad, pos + q, (1u << k) | (u & ((1u << k) - 1u)), k + 1);   // q zeros, a one, k remainder bits
            run += q + 1 + k;
        }
    }
    __syncthreads();

    // ---- CRC-16 of the frame: every thread takes kCrcWords words, the pieces are combined by the CRC's linearity
    const int L = (body0 + body_bits + 7) >> 3;   // bytes in front of the CRC-16, zero padding to the byte included
    uint32_t crc = 0u;
    {
        const int byte0 = t * kCrcWords * 4;
        int nb = L - byte0;
        nb = nb < 0 ? 0 : nb > kCrcWords * 4 ? kCrcWords * 4 : nb;
        for (int i = 0; i < nb; ++i) {
            const uint32_t w = s_bits[(byte0 + i) >> 2];
            crc = crc16_step(crc, (w >> (24 - 8 * (i & 3))) & 0xFFu);
        }
        if (nb > 0) crc = gf16_mul(crc, gf16_xpow8((uint32_t)(L - byte0 - nb)));
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) crc ^= __shfl_xor(crc, o, 64);
    if (lane == 0) s_crc[wave] = crc;
    __syncthreads();
    if (t == 0) put_bits(s_bits, &s_bad, L * 8, s_crc[0] ^ s_crc[1] ^ s_crc[2] ^ s_crc[3], 16);
    __syncthreads();

    // ---- the frame into its slot (whole words; the slot's tail past the frame is scratch)
    const int bytes = L + 2 <= kFlacFrameMax ? L + 2 : kFlacFrameMax;
    uint32_t* slot = reinterpret_cast<uint32_t*>(slots + ((long)b * max_frames + blk) * kFlacSlot);
    for (int w = t; w < (bytes + 3) >> 2; w += 256) slot[w] = __builtin_bswap32(s_bits[w]);
    if (t == 0) flen[(long)b * max_frames + blk] = s_bad ? -1 : bytes;
}

// ------------------------------------------------------------------------------------------------ assembly
// One workgroup per (frame, row): sums the lengths of the frames in front of its own and copies its frame behind them (frames are
// byte-aligned: a byte copy).  The workgroup of frame 0 also writes the 42 header bytes and the stream's length.
__global__ __launch_bounds__(256) void flac_assemble_kernel(const int* __restrict__ len, const int* __restrict__ rate, int max_frames,
                                                            const uint8_t* __restrict__ slots, const int* __restrict__ flen,
                                                            const uint8_t* __restrict__ md5, uint8_t* __restrict__ out, long out_bstride,
                                                            int* __restrict__ out_len) {
    __shared__ long s_sum[4];
    __shared__ int s_min[4], s_max[4];
    const int b = blockIdx.y, blk = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const long total = len[b];
    const int frames = (int)((total + kFlacBlock - 1) / kFlacBlock);
    if (blk >= frames) return;
    const int* fl = flen + (long)b * max_frames;
    // frame 0's workgroup looks at every frame (sizes for STREAMINFO, the stream's length), the others at those in front of them
    const int upto = blk == 0 ? frames : blk;
    long sum = 0;
    int mn = 0x7FFFFFFF, mx = 0;
    for (int f = t; f < upto; f += 256) {
        const int v = fl[f];
        sum += v, mn = v < mn ? v : mn, mx = v > mx ? v : mx;
    }
    sum = wave_add(sum);
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const int a = __shfl_xor(mn, o, 64), c = __shfl_xor(mx, o, 64);
        mn = a < mn ? a : mn, mx = c > mx ? c : mx;
    }
    if (lane == 0) s_sum[wave] = sum, s_min[wave] = mn, s_max[wave] = mx;
    __syncthreads();
    sum = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    uint8_t* dst = out + (long)b * out_bstride;
    if (blk == 0 && t == 0) {
        mn = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
        mx = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        // min / max block size by the writer's rule: max(16, .), the minimum over all blocks but the last
        const int bs = frames >= 2 ? kFlacBlock : (int)(total > 16 ? total : 16);
        const unsigned long long v = ((unsigned long long)rate[b] << 44) | (15ull << 36) | (unsigned long long)total;
        const uint8_t head[26] = {'f', 'L', 'a', 'C', 0x80, 0, 0, 34, (uint8_t)(bs >> 8), (uint8_t)bs, (uint8_t)(bs >> 8), (uint8_t)bs,
                                  (uint8_t)(mn >> 16), (uint8_t)(mn >> 8), (uint8_t)mn, (uint8_t)(mx >> 16), (uint8_t)(mx >> 8), (uint8_t)mx,
                                  (uint8_t)(v >> 56), (uint8_t)(v >> 48), (uint8_t)(v >> 40), (uint8_t)(v >> 32), (uint8_t)(v >> 24),
                                  (uint8_t)(v >> 16), (uint8_t)(v >> 8), (uint8_t)v};
#pragma unroll
        for (int i = 0; i < 26; ++i) dst[i] = head[i];
#pragma unroll
        for (int i = 0; i < 16; ++i) dst[26 + i] = md5[(long)b * 16 + i];
        out_len[b] = mn < 0 ? 0 : kFlacHeader + (int)sum;   // (a frame that flac_frame_kernel refused: no stream)
    }
    const long off = kFlacHeader + (blk == 0 ? 0 : sum);
    const int mine = fl[blk];
    const uint8_t* src = slots + ((long)b * max_frames + blk) * kFlacSlot;
    for (int i = t; i < mine; i += 256) dst[off + i] = src[i];
}

void launch_flac_encode(const float* x, long x_bstride, const int* rows, const int* len, const int* rate, int B, int max_len, uint8_t* slots, int* flen,
                        uint8_t* md5, uint8_t* out, long out_bstride, int* out_len, hipStream_t st) {
    AUR_REQUIRE(B >= 1 && B <= 65535 && max_len >= 1 && max_len <= kFlacMaxSamples, "flac_encode: 1 <= B <= 65535, 1 <= samples <= 2^24");
    const int frames = (int)flac_frames(max_len);
    trace_launch("flac_md5_kernel");
    hipLaunchKernelGGL(flac_md5_kernel, dim3(B), dim3(64), 0, st, x, x_bstride, rows, len, md5);
    post_launch("flac_md5_kernel", st);
    trace_launch("flac_frame_kernel");
    hipLaunchKernelGGL(flac_frame_kernel, dim3(frames, B), dim3(256), 0, st, x, x_bstride, rows, len, frames, slots, flen);
    post_launch("flac_frame_kernel", st);
    trace_launch("flac_assemble_kernel");
    hipLaunchKernelGGL(flac_assemble_kernel, dim3(frames, B), dim3(256), 0, st, len, rate, frames, slots, flen, md5, out, out_bstride, out_len);
    post_launch("flac_assemble_kernel", st);
}

}  // namespace aur
