// FLAC encoder on the GPU (kernels: flac_kernels.hip): the bitstream of auralis_amd/api/flac.py's writer, byte for byte -- mono, 16 bit,
// 4096-sample blocks, CONSTANT / VERBATIM / FIXED order 0..4 subframes, partitioned Rice codes (method 0, partition order 0..4),
// CRC-8 / CRC-16, MD5 of the PCM in STREAMINFO.  An integer algorithm: there is no tolerance, the host writer is the specification.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "dev_buf.h"

namespace aur {

constexpr int kFlacBlock = 4096;                          // samples per frame (the last one of a stream is shorter)
constexpr int kFlacFrameMax = 9 + 1 + 1 + 8192 + 2;       // header (<= 9) + CRC-8, subframe header, 4096 verbatim samples, CRC-16
constexpr int kFlacSlot = 8208;                           // a frame's slot in device memory: kFlacFrameMax in whole 16-byte words
constexpr int kFlacHeader = 42;                           // "fLaC" + metadata block header + STREAMINFO
constexpr int kFlacMaxSamples = 1 << 24, kFlacMaxRate = 1 << 20;   // per stream: <= 4096 frames (3-byte frame numbers), a 20-bit rate

inline long flac_frames(long n) { return (n + kFlacBlock - 1) / kFlacBlock; }
// what a stream of n samples can take at most: the stride of a row that receives one
inline long flac_stream_bound(long n) { return kFlacHeader + flac_frames(n) * kFlacFrameMax; }

// x: B float rows (row b at x + (rows ? rows[b] : b) * x_bstride, len[b] >= 1 samples, rate[b] Hz; what a row holds past its length is not read).
// slots [B][max_frames][kFlacSlot] bytes, flen [B][max_frames], md5 [B][16]: scratch.  out: row b at out + b * out_bstride receives
// out_len[b] = 42 + the frames' bytes <= flac_stream_bound(len[b]); nothing past them is written.  max_len >= every len[b] (host copy).
// Three launches on `st`, in order: MD5 (a wave per row), frames (a workgroup per block and row), assembly.
void launch_flac_encode(const float* x, long x_bstride, const int* rows, const int* len, const int* rate, int B, int max_len, uint8_t* slots, int* flen,
                        uint8_t* md5, uint8_t* out, long out_bstride, int* out_len, hipStream_t st);

// The encoder with its scratch: rows in device memory -> streams in device memory.
class FlacEncoder {
public:
    // rows (nullable: stream b is row b), len, rate: host arrays [B] each; they go up in stream order (the member copy outlives the call)
    void encode(const float* d_x, long x_bstride, const std::vector<int>* rows, const std::vector<int>& len, const std::vector<int>& rate,
                uint8_t* d_out, long out_bstride, int* d_out_len, hipStream_t st) {
        const int B = (int)len.size();
        int max_len = 0;
        for (int b = 0; b < B; ++b) {
            AUR_REQUIRE(len[b] >= 1 && len[b] <= kFlacMaxSamples, "flac: 1 <= samples <= 2^24 per stream");
            AUR_REQUIRE(rate[b] >= 1 && rate[b] < kFlacMaxRate, "flac: 1 <= sample rate < 2^20");
            max_len = std::max(max_len, len[b]);
        }
        AUR_REQUIRE(out_bstride >= flac_stream_bound(max_len), "flac: output rows of at least 42 + frames * 8205 bytes");
        const size_t frames = (size_t)flac_frames(max_len);
        meta_.assign(len.begin(), len.end());
        meta_.insert(meta_.end(), rate.begin(), rate.end());
        if (rows) meta_.insert(meta_.end(), rows->begin(), rows->end());
        d_meta_.ensure(meta_.size() * 4);
        HIP_CHECK(hipMemcpyAsync(d_meta_.p, meta_.data(), meta_.size() * 4, hipMemcpyHostToDevice, st));
        d_slots_.ensure((size_t)B * frames * kFlacSlot);
        d_flen_.ensure((size_t)B * frames * 4);
        d_md5_.ensure((size_t)B * 16);
        launch_flac_encode(d_x, x_bstride, rows ? d_meta_.as<int>() + 2 * B : nullptr, d_meta_.as<int>(), d_meta_.as<int>() + B, B, max_len, d_slots_.as<uint8_t>(), d_flen_.as<int>(),
                           d_md5_.as<uint8_t>(), d_out, out_bstride, d_out_len, st);
    }

private:
    DevBuf d_meta_, d_slots_, d_flen_, d_md5_;
    std::vector<int> meta_;
};

}  // namespace aur
