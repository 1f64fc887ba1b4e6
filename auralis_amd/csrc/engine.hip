// Host runtime + C ABI (include/auralis_amd.h) of the MI355X-native XTTSv2 hot path.
//
// One Engine per GPU/process.  It owns the loaded weights, the continuous batcher (admission, the K/V block allocator, the sequences
// and their slots, the pipelined decode loop), the speaker table, the latent pool and the vocoder stage.  The three networks live apart
// from it: the GPT with its K/V pool, per-slot device state and the latent stash that replaces the reference's second GPT pass
// (XTTSv2.py:617-687; equivalence argued in SURVEY.md §7 and tested in tests/) in gpt_net.h, the vocoder in voc_net.h, conditioning in
// cond_net.h.  The reference's counterparts are vLLM's AsyncLLMEngine/scheduler/block manager (un-vendored, XTTSv2.py:198-232),
// HiddenStatesCollector (components/vllm/hidden_state_collector.py) and the asyncio.to_thread HiFi-GAN call (XTTSv2.py:804).
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "abi_internal.h"
#include "cond_net.h"
#include "flac_kernels.h"
#include "gpt_net.h"
#include "voc_net.h"

namespace aur {

thread_local std::string g_last_error;

constexpr int kProfileEvery = 64;   // profile mode default: every 64th decode step is followed by the per-kind replay batches (profile_replay)

// Pinned result block of one vocoder batch: the D2H copies land here and aur_result.wav / .latents point straight into
// it (no second host copy); the block returns to the pool when the last sequence of the batch is released.
struct PinBlock {
    PinBuf buf;
    int refs = 0;
};

enum class SeqState { WAITING, RUNNING, TOKENS_DONE, DONE, RELEASED };

struct Seq {
    uint64_t id = 0;
    SeqState state = SeqState::WAITING;
    std::vector<int> text_ids;
    int spk_row = -1;
    aur_seq_desc params{};
    int slot = -1;
    int n_prompt = 0;
    std::vector<int> blocks;
    std::vector<int32_t> tokens;
    std::atomic<int32_t> n_gen{0};    // tokens.size(), readable under mu_ alone while the driver thread appends (aur_get_load)
    const float* wav = nullptr;       // into `result_block`
    int n_samples = 0;
    const float* latents = nullptr;   // into `result_block` (aur_config.return_latents)
    int n_latent_rows = 0;
    const uint8_t* enc = nullptr;     // into `result_block` (aur_seq_desc.encoding)
    int64_t n_enc = 0;
    PinBlock* result_block = nullptr;
    int pool_idx = -1;   // latent-pool entry once the tokens are done (vocoder stage)
    bool shared_prefix = false;
    int error = 0;
    bool cancel = false;   // aur_cancel: stop decoding at the next step, skip the vocoder
};

class Engine {
public:
    Engine(const aur_config& c, int device) : cfg_(c), device_(device) {
        HIP_CHECK(hipSetDevice(device_));
        // GPT stream at the highest priority, vocoder stream at the lowest: when a vocoder batch overlaps the decode steps
        // of other sequences, the latency-bound decode kernels get the CUs first and the vocoder fills what is left
        int prio_lo = 0, prio_hi = 0;
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        HIP_CHECK(hipStreamCreateWithPriority(&st_, hipStreamDefault, prio_hi));   // blocking w.r.t. the null stream on purpose
        AUR_REQUIRE(c.n_layer >= 1 && c.n_layer <= 64, "n_layer in [1,64]");
        AUR_REQUIRE(c.max_seqs >= 1 && c.max_seqs <= 4096, "max_seqs in [1,4096]");
        if (cfg_.max_prefill_rows <= 0) cfg_.max_prefill_rows = 8192;
        if (cfg_.max_speakers <= 0) cfg_.max_speakers = 64;
        const int S = cfg_.max_seqs;
        n_blocks_ = (long)S * kMaxBlocks + 2L * cfg_.max_speakers;   // + 2 shared prefix blocks per speaker
        const bool kv_half = cfg_.kv_fp16 != 0;
        // paged_attention_kernel addresses a layer's pool with 32-bit byte offsets: 494 slots with the fp32 pool, 991 with fp16
        // (at 30 layers that is 120 GiB of K/V; HBM holds ~1000 slots' worth next to the weights)
        {
            const long cap = kv_half ? 2 * kMaxKvBlocksPerLayer + 1 : kMaxKvBlocksPerLayer;
            if (n_blocks_ > cap)
                throw InvalidArgument("requirement failed: K/V pool: a layer's pool must stay below 4 GiB; with max_speakers = " +
                                      std::to_string(cfg_.max_speakers) + (kv_half ? " and kv_fp16" : " and the fp32 pool") + " max_seqs <= " +
                                      std::to_string((cap - 2L * cfg_.max_speakers) / kMaxBlocks) + " (asked for " + std::to_string(S) + ")");
        }
        AUR_REQUIRE(!(cfg_.gpt_fp16 && cfg_.gemm_f32_exact), "gpt_fp16 and gemm_f32_exact exclude each other (the fp16-weight decode GEMMs "
                                                             "run on the split arithmetic)");
        GptLayout gl{cfg_.n_layer, S, n_blocks_, cfg_.gemm_f32_exact ? 0 : 1, cfg_.gpt_fp16 != 0, true, kv_half, cfg_.gelu_erf != 0, false};
        if (const char* e = getenv("AUR_GEMM_PRESPLIT")) gl.presplit = atoi(e) != 0; // 0: prompt-row GEMMs split their weights per tile instead of reading the planes packed at load time (A/B only)
        if (const char* e = getenv("AUR_SAMPLER_FULL_SORT")) gl.sampler_full_sort = atoi(e) != 0;
        gpt_.reset(new GptNet(w_, st_, gl));
        for (int b = (int)n_blocks_ - 1; b >= 0; --b) free_blocks_.push_back(b);
        spk_table_.ensure((size_t)cfg_.max_speakers * 32 * kHidden * sizeof(float));
        spk_emb_.ensure((size_t)cfg_.max_speakers * 512 * sizeof(float));
        voc_cond_.ensure((size_t)cfg_.max_speakers * kCondStride * sizeof(float));
        h_block_tables_.assign((size_t)(S + 1) * kMaxBlocks, 0);
        spk_info_.assign(cfg_.max_speakers, SpeakerInfo{});
        slot_owner_.assign(S, nullptr);
        HIP_CHECK(hipStreamCreateWithPriority(&st_voc_, hipStreamDefault, prio_lo));
        HIP_CHECK(hipEventCreateWithFlags(&ev_lat_, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&ev_voc_done_, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(ev_lat_, st_));
        latpool_.ensure((size_t)2 * S * kMaxLatRows * kHidden * sizeof(float));
        for (int i = 2 * S - 1; i >= 0; --i) latpool_free_.push_back(i);
        VocLayout lay{cfg_.vocoder_fp16 != 0, cfg_.vocoder_fp16 != 0, true};
        if (const char* e = getenv("AUR_XT_F16")) lay.halves = lay.halves && atoi(e) != 0;   // 0: fp32 ResBlock intermediates and residual stream (A/B only)
        if (const char* e = getenv("AUR_CONV_DMA")) lay.dma = atoi(e) != 0;   // 0: register-staged ResBlock convs (A/B only)
        voc_.reset(new HifiGan(w_, st_voc_, lay));
        if (const char* e = getenv("AUR_DECODE_PIPELINE")) pipeline_ = atoi(e) != 0;
        if (const char* e = getenv("AUR_HOST_TRACE")) host_trace_ = atoi(e) != 0;
        if (const char* e = getenv("AUR_TEST_FAIL_STEP")) fail_at_step_ = atoi(e);
        if (const char* e = getenv("AUR_TEST_FAIL_VOC")) fail_at_voc_ = atoi(e);

        for (StepEvents& ev : ev_step_) {
            HIP_CHECK(hipEventCreateWithFlags(&ev.readback, hipEventDisableTiming));
            HIP_CHECK(hipEventCreate(&ev.start));
            HIP_CHECK(hipEventCreate(&ev.end));
        }
        HIP_CHECK(hipEventCreate(&ev_a_));
        HIP_CHECK(hipEventCreate(&ev_b_));
        HIP_CHECK(hipStreamSynchronize(st_));
    }
    ~Engine() {
        (void)hipSetDevice(device_);
        (void)hipStreamSynchronize(st_);
        (void)hipStreamSynchronize(st_voc_);
        (void)hipEventDestroy(ev_a_);
        (void)hipEventDestroy(ev_b_);
        for (StepEvents& ev : ev_step_) {
            (void)hipEventDestroy(ev.readback);
            (void)hipEventDestroy(ev.start);
            (void)hipEventDestroy(ev.end);
        }
        if (comm_) (void)Rccl::get().CommDestroy(comm_);
        (void)hipEventDestroy(ev_lat_);
        (void)hipEventDestroy(ev_voc_done_);
        (void)hipStreamDestroy(st_voc_);
        (void)hipStreamDestroy(st_);
    }

    void use() { HIP_CHECK(hipSetDevice(device_)); }
    DbgCtx dbg_ctx() const {
        const GptLayout& g = gpt_->layout();
        return {device_, st_, st_voc_, g.prec, g.f16, g.presplit, gpt_->ksp_buf(), gpt_->ksp_cnt()};
    }

    // ------------------------------------------------------------------ weights
    void load(const aur_tensor_desc* t, size_t n) {
        use();
        std::lock_guard<std::mutex> gl(gpu_mu_);   // not while a step is running
        std::lock_guard<std::mutex> lk(mu_);       // submit() reads the table sizes under mu_
        for (size_t i = 0; i < n; ++i) {
            AUR_REQUIRE(t[i].name && t[i].data && t[i].numel > 0, "bad tensor desc");
            Tensor& dst = w_.map[t[i].name];
            if (!dst.buf) dst.buf.reset(new DevBuf());
            dst.buf->upload(t[i].data, (size_t)t[i].numel * sizeof(float));
            dst.numel = t[i].numel;
            dst.f16_eff = false;
        }
        voc_->unbind();
        gpt_->unbind();
        if (cfg_.gpt_fp16) gpt_->check_f16();
    }
    void ensure_gpt() { gpt_->bind(), voc_->bind(); }   // the layer tables out of what is loaded (no-ops once bound; load() unbinds)

    // ------------------------------------------------------------------ conditioning
    // Speaker table (caller holds mu_).  A row is pinned while any sequence submitted with it has not been delivered yet
    // (refs: aur_submit .. end of its vocoder batch, or its failure).  When the table is full the least recently used
    // unpinned voice is evicted; its two shared prefix KV blocks stay with the row and are overwritten by the newcomer.
    int speaker_row(uint64_t key, bool create) {
        auto it = spk_rows_.find(key);
        if (it != spk_rows_.end()) {
            spk_info_[it->second].last_use = ++spk_clock_;
            return it->second;
        }
        if (!create) return -1;
        int row = -1;
        if ((int)spk_rows_.size() < cfg_.max_speakers) {
            std::vector<char> used(cfg_.max_speakers, 0);
            for (auto& kv : spk_rows_) used[kv.second] = 1;
            for (int r = 0; r < cfg_.max_speakers && row < 0; ++r)
                if (!used[r]) row = r;
        } else {
            uint64_t victim = 0;
            for (auto& kv : spk_rows_) {
                const SpeakerInfo& si = spk_info_[kv.second];
                if (si.refs == 0 && (row < 0 || si.last_use < spk_info_[row].last_use)) {
                    row = kv.second;
                    victim = kv.first;
                }
            }
            if (row < 0) throw StateError("speaker table full: every registered voice has undelivered sequences (raise aur_config.max_speakers)");
            spk_rows_.erase(victim);
            spk_info_[row].ready = false;
        }
        spk_rows_[key] = row;
        spk_info_[row].last_use = ++spk_clock_;
        return row;
    }
    // ------------------------------------------------------------------ RCCL inside the boundary
    // The only exchange of the multi-GPU path is the speaker conditioning (133 120 B per voice).  RCCL is resolved at run time
    // (the copy PyTorch already loaded when there is one), so a single-GPU process never needs it.
    struct Rccl {
        typedef struct { char internal[128]; } UniqueId;
        int (*GetUniqueId)(UniqueId*) = nullptr;
        int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
        int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
        int (*CommDestroy)(void*) = nullptr;
        int (*CommCount)(void*, int*) = nullptr;
        int (*CommUserRank)(void*, int*) = nullptr;
        const char* (*GetErrorString)(int) = nullptr;
        static Rccl& get() {
            static Rccl r = [] {
                Rccl x;
                void* h = nullptr;
                for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"})
                    if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
                if (!h) throw StateError("RCCL (librccl.so) not found: multi-GPU conditioning broadcast unavailable");
                x.GetUniqueId = reinterpret_cast<decltype(x.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
                x.CommInitRank = reinterpret_cast<decltype(x.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
                x.Broadcast = reinterpret_cast<decltype(x.Broadcast)>(dlsym(h, "ncclBroadcast"));
                x.CommDestroy = reinterpret_cast<decltype(x.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
                x.CommCount = reinterpret_cast<decltype(x.CommCount)>(dlsym(h, "ncclCommCount"));
                x.CommUserRank = reinterpret_cast<decltype(x.CommUserRank)>(dlsym(h, "ncclCommUserRank"));
                x.GetErrorString = reinterpret_cast<decltype(x.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
                if (!x.GetUniqueId || !x.CommInitRank || !x.Broadcast || !x.CommDestroy) throw StateError("RCCL symbols missing");
                return x;
            }();
            return r;
        }
        void check(int rc, const char* what) const {
            if (rc != 0) throw StateError(std::string("RCCL ") + what + " failed: " + (GetErrorString ? GetErrorString(rc) : "?"));
        }
    };
    static void comm_unique_id(uint8_t* out) {
        Rccl::UniqueId id;
        Rccl::get().check(Rccl::get().GetUniqueId(&id), "ncclGetUniqueId");
        memcpy(out, id.internal, 128);
    }
    void comm_init(const uint8_t* id_bytes, int rank, int world) {
        std::lock_guard<std::mutex> gl(gpu_mu_);
        use();
        AUR_REQUIRE(world >= 1 && rank >= 0 && rank < world, "comm_init: rank / world");
        if (comm_) throw StateError("communicator already initialised");
        Rccl::UniqueId id;
        memcpy(id.internal, id_bytes, 128);
        Rccl::get().check(Rccl::get().CommInitRank(&comm_, world, id, rank), "ncclCommInitRank");
        comm_rank_ = rank;
        comm_world_ = world;
    }
    // collective: every rank of the communicator calls it; `root` must have the voice registered, the others receive it over
    // xGMI into a device buffer and register it from there (no host bounce)
    void broadcast_conditioning(uint64_t key, int root) {
        constexpr int kCond = 32 * kHidden, kTot = kCond + 512;
        {
            std::lock_guard<std::mutex> gl(gpu_mu_);
            use();
            if (!comm_) throw StateError("aur_comm_init has not been called");
            AUR_REQUIRE(root >= 0 && root < comm_world_, "broadcast_conditioning: root");
            bcast_buf_.ensure((size_t)kTot * sizeof(float));
            float* buf = bcast_buf_.as<float>();
            if (comm_rank_ == root) {
                int row;
                {
                    std::lock_guard<std::mutex> lk(mu_);
                    row = speaker_row(key, false);
                }
                if (row < 0) throw StateError("broadcast_conditioning: the root has no such speaker_key");
                HIP_CHECK(hipMemcpyAsync(buf, spk_table_.as<float>() + (long)row * kCond, (size_t)kCond * sizeof(float), hipMemcpyDeviceToDevice, st_));
                HIP_CHECK(hipMemcpyAsync(buf + kCond, spk_emb_.as<float>() + (long)row * 512, 512 * sizeof(float), hipMemcpyDeviceToDevice, st_));
            }
            Rccl::get().check(Rccl::get().Broadcast(buf, buf, (size_t)kTot, /*ncclFloat32*/ 7, root, comm_, st_), "ncclBroadcast");
            HIP_CHECK(hipStreamSynchronize(st_));
        }
        if (comm_rank_ != root) set_conditioning(key, bcast_buf_.as<float>(), bcast_buf_.as<float>() + kCond, true);
    }

    // what the communicator itself reports (not the values comm_init was called with)
    void comm_info(int32_t* n_ranks, int32_t* rank) {
        std::lock_guard<std::mutex> gl(gpu_mu_);
        *n_ranks = 0;
        *rank = -1;
        if (!comm_) return;
        AUR_REQUIRE(Rccl::get().CommCount && Rccl::get().CommUserRank, "RCCL: ncclCommCount / ncclCommUserRank missing");
        int n = 0, r = -1;
        Rccl::get().check(Rccl::get().CommCount(comm_, &n), "ncclCommCount");
        Rccl::get().check(Rccl::get().CommUserRank(comm_, &r), "ncclCommUserRank");
        *n_ranks = n;
        *rank = r;
    }
    // FNV-1a over the voice's conditioning as registered in device memory
    uint64_t conditioning_checksum(uint64_t key) {
        constexpr int kCond = 32 * kHidden;
        std::vector<float> h((size_t)kCond + 512);
        {
            std::lock_guard<std::mutex> gl(gpu_mu_);
            use();
            int row;
            {
                std::lock_guard<std::mutex> lk(mu_);
                row = speaker_row(key, false);
            }
            if (row < 0) throw InvalidArgument("conditioning_checksum: unknown speaker_key");
            HIP_CHECK(hipMemcpyAsync(h.data(), spk_table_.as<float>() + (long)row * kCond, (size_t)kCond * 4, hipMemcpyDeviceToHost, st_));
            HIP_CHECK(hipMemcpyAsync(h.data() + kCond, spk_emb_.as<float>() + (long)row * 512, 512 * 4, hipMemcpyDeviceToHost, st_));
            HIP_CHECK(hipStreamSynchronize(st_));
        }
        uint64_t x = 1469598103934665603ull;
        const unsigned char* b = reinterpret_cast<const unsigned char*>(h.data());
        for (size_t i = 0; i < h.size() * 4; ++i) {
            x ^= b[i];
            x *= 1099511628211ull;
        }
        return x;
    }

    bool has_conditioning(uint64_t key) {
        std::lock_guard<std::mutex> lk(mu_);
        return speaker_row(key, false) >= 0;
    }
    // Reference audio (mono float32, 22 050 Hz, host memory) -> gpt_cond_latent [32][1024], speaker_embedding [512] on the GPU
    // (cond_net.h).  Needs the "cond.*" tensors of weights.py: pack_conditioning.
    void compute_conditioning(const float* const* pcm, const int32_t* n_samples, int n_refs, const aur_cond_params& cp, float* out_cond,
                              float* out_spk) {
        std::lock_guard<std::mutex> gl(gpu_mu_);   // shares the GPT stream; not while a step is running
        use();
        if (!cond_net_) cond_net_.reset(new CondNet(w_, st_));
        AUR_REQUIRE(w_.has("cond.enc.init.w"), "conditioning weights not loaded (pack_conditioning)");
        CondParams p;
        p.max_ref_length = cp.max_ref_length;
        p.gpt_cond_len = cp.gpt_cond_len;
        p.gpt_cond_chunk_len = cp.gpt_cond_chunk_len;
        p.sound_norm_refs = cp.sound_norm_refs;
        AUR_REQUIRE(p.max_ref_length > 0 && p.gpt_cond_chunk_len > 0, "conditioning: lengths must be positive");
        std::vector<int> n(n_samples, n_samples + n_refs);
        cond_net_->run(pcm, n.data(), n_refs, p, out_cond, out_spk);
    }
    void set_conditioning(uint64_t key, const float* gpt_cond, const float* spk, bool device_ptrs) {
        std::lock_guard<std::mutex> gl(gpu_mu_);   // may be called while the driver thread is inside aur_step
        use();
        int row;
        {
            std::lock_guard<std::mutex> lk(mu_);
            row = speaker_row(key, true);
            if (spk_info_[row].refs != 0)
                throw StateError("speaker is in use by undelivered sequences: register the new voice under a new key");
        }
        const hipMemcpyKind kind = device_ptrs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        HIP_CHECK(hipMemcpyAsync(spk_table_.as<float>() + (long)row * 32 * kHidden, gpt_cond,
                                 32 * kHidden * sizeof(float), kind, st_));
        HIP_CHECK(hipMemcpyAsync(spk_emb_.as<float>() + (long)row * 512, spk, 512 * sizeof(float), kind, st_));
        // 1x1 conditioning convs of the vocoder on the speaker embedding (hifigan_decoder.py:243-251)
        float* dst = voc_cond_.as<float>() + (long)row * kCondStride;
        const float* g = spk_emb_.as<float>() + (long)row * 512;
        launch_gemv_rows(w_.W("voc.cond_layer.w", 512 * 512), w_.W("voc.cond_layer.b", 512), g, dst, 512, 512, 1, 0, 0, st_);
        int off = 512;
        for (int i = 0; i < 4; ++i) {
            const int C = kVocChans[i];
            const std::string p = "voc.conds." + std::to_string(i);
            launch_gemv_rows(w_.W(p + ".w", (int64_t)C * 512), w_.W(p + ".b", C), g, dst + off, C, 512, 1, 0, 0, st_);
            off += C;
        }
        HIP_CHECK(hipStreamSynchronize(st_));
        prefill_speaker_prefix(row);
    }
    // Prefix sharing: the first 32 prompt rows (speaker latents, XTTSv2.py:345) are identical for every sequence of a
    // speaker and, under causal attention, so are their K/V in every layer.  They are computed once per speaker into two
    // KV blocks (32 tokens = 2 blocks of 16) that every sequence's block table points at; a prompt prefill then only
    // processes the text rows + start token.  Results are bitwise those of the unshared path (row-independent kernels).
    void prefill_speaker_prefix(int row) {
        SpeakerInfo& si = spk_info_[row];
        si.ready = false;
        if (!w_.has("gpt.wte")) return;   // GPT weights not loaded yet: unshared path
        ensure_gpt();
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (si.blocks[0] < 0) {
                AUR_REQUIRE(free_blocks_.size() >= 2, "KV pool exhausted");
                for (int b = 0; b < 2; ++b) {
                    si.blocks[b] = free_blocks_.back();
                    free_blocks_.pop_back();
                }
            }
        }
        const int S = cfg_.max_seqs;
        std::vector<int4> desc;
        std::vector<int> row_slot(32, S), row_pos(32);
        for (int i = 0; i < 32; ++i) {
            desc.push_back(make_int4(0, i, row, 0));
            row_pos[i] = i;
        }
        h_block_tables_[(size_t)S * kMaxBlocks + 0] = si.blocks[0];
        h_block_tables_[(size_t)S * kMaxBlocks + 1] = si.blocks[1];
        gpt_->upload_block_tables(h_block_tables_);
        gpt_->prompt_rows(desc, row_slot, row_pos, spk_table_.as<float>());
        HIP_CHECK(hipStreamSynchronize(st_));
        si.ready = true;
    }

    // ------------------------------------------------------------------ submit / poll
    uint64_t submit(const aur_seq_desc& d) {
        AUR_REQUIRE(d.text_ids && d.n_text >= 1, "text_ids");
        AUR_REQUIRE(d.max_tokens >= 1 && d.max_tokens <= kMaxLatRows - 3, "max_tokens in [1,605]");
        const int n_prompt = 32 + d.n_text + 1;
        AUR_REQUIRE(n_prompt + d.max_tokens + 4 <= kMaxBlocks * kKvBlockTokens, "prompt + max_tokens exceeds max_model_len");
        AUR_REQUIRE(n_prompt <= cfg_.max_prefill_rows, "prompt longer than max_prefill_rows");
        AUR_REQUIRE(d.repetition_penalty > 0.f, "repetition_penalty > 0");
        AUR_REQUIRE(speed_valid(d.speed), "speed is 0 (unset) or in [0.5, 2.0]");
        AUR_REQUIRE(rate_class(d.sample_rate) >= 0, "sample_rate is 0 (unset) or one of 8000, 16000, 22050, 24000, 32000, 44100, 48000");
        AUR_REQUIRE(d.encoding == 0 || d.encoding == AUR_ENC_FLAC16, "encoding is 0 (none) or AUR_ENC_FLAC16");
        std::lock_guard<std::mutex> lk(mu_);
        {   // reject bad text ids / positions here, not in the middle of a batched prefill
            if (!w_.has("text_emb") || !w_.has("text_pos")) throw StateError("weights not loaded");
            const int vocab = (int)(w_.at("text_emb").numel / kHidden), npos = (int)(w_.at("text_pos").numel / kHidden);
            AUR_REQUIRE(d.n_text <= npos, "text longer than the text position table");
            for (int i = 0; i < d.n_text; ++i) AUR_REQUIRE(d.text_ids[i] >= 0 && d.text_ids[i] < vocab, "text id out of range");
        }
        const int row = speaker_row(d.speaker_key, false);
        AUR_REQUIRE(row >= 0, "unknown speaker_key (call aur_set_conditioning first)");
        spk_info_[row].refs++;
        auto s = std::make_unique<Seq>();
        s->id = next_id_++;
        s->text_ids.assign(d.text_ids, d.text_ids + d.n_text);
        s->spk_row = row;
        s->params = d;
        s->params.text_ids = nullptr;
        s->n_prompt = n_prompt;
        const uint64_t id = s->id;
        if (d.priority > 0) {   // aur_seq_desc.priority: behind the urgent sequences already waiting, in front of everything else
            auto it = waiting_.begin();
            while (it != waiting_.end() && (*it)->params.priority > 0) ++it;
            waiting_.insert(it, s.get());
        } else {
            waiting_.push_back(s.get());
        }
        seqs_[id] = std::move(s);
        return id;
    }

    size_t poll(aur_result* out, size_t cap) {
        std::lock_guard<std::mutex> lk(mu_);
        size_t n = 0;
        while (n < cap && !done_.empty()) {
            Seq* s = done_.front();
            done_.pop_front();
            aur_result& r = out[n++];
            r.seq_id = s->id;
            r.n_tokens = (int)s->tokens.size();
            r.tokens = s->tokens.data();
            r.n_samples = s->n_samples;
            r.wav = s->wav;
            r.n_latent_rows = s->n_latent_rows;
            r.latents = s->latents;
            r.error = s->error;
            r.sample_rate = s->params.sample_rate ? s->params.sample_rate : 24000;
            r.enc = s->enc;
            r.n_enc = s->n_enc;
        }
        return n;
    }
    void release(uint64_t id) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = seqs_.find(id);
        AUR_REQUIRE(it != seqs_.end(), "unknown seq_id");
        AUR_REQUIRE(it->second->state == SeqState::DONE, "sequence not finished");
        if (it->second->result_block) it->second->result_block->refs--;
        seqs_.erase(it);
    }

    // aur_cancel.  Takes only the queue lock: a WAITING sequence is dropped here; everything else is noted and handled by the driver
    // thread at the top of its next aur_step (process_cancels), so the caller -- the facade's event loop -- never waits for a step.
    void cancel(uint64_t id) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = seqs_.find(id);
        AUR_REQUIRE(it != seqs_.end(), "unknown seq_id");
        Seq* s = it->second.get();
        if (s->state == SeqState::WAITING) {
            waiting_.erase(std::remove(waiting_.begin(), waiting_.end(), s), waiting_.end());
            finish_cancelled(s);
        } else if (s->state == SeqState::RUNNING || s->state == SeqState::TOKENS_DONE) {
            if (!s->cancel) cancel_pending_.push_back(id);
        }
    }
    // (caller holds mu_; the sequence holds no slot, K/V block or pool entry any more)
    void finish_cancelled(Seq* s) {
        s->cancel = true;
        s->error = AUR_E_CANCELLED;
        s->wav = nullptr; s->n_samples = 0; s->latents = nullptr; s->n_latent_rows = 0; s->enc = nullptr; s->n_enc = 0;
        spk_info_[s->spk_row].refs--;
        s->state = SeqState::DONE;
        done_.push_back(s);
        finished_total_++;
    }
    // driver thread, inside aur_step (gpu_mu_ held): a running sequence gets max_tokens = 1 on the device -- the sampler then flags it
    // finished with the next token it draws, and finish_tokens() drops it instead of parking its latents; a sequence that waits in the
    // vocoder queue leaves it.  One already inside a vocoder batch is delivered normally.
    void process_cancels() {
        std::vector<uint64_t> ids;
        {
            std::lock_guard<std::mutex> lk(mu_);
            ids.swap(cancel_pending_);
        }
        for (uint64_t id : ids) {
            std::lock_guard<std::mutex> lk(mu_);
            auto it = seqs_.find(id);
            if (it == seqs_.end()) continue;
            Seq* s = it->second.get();
            if (s->state == SeqState::RUNNING && s->slot >= 0 && !s->cancel) {
                s->cancel = true;
                gpt_->limit_tokens(s->slot);
            } else if (s->state == SeqState::TOKENS_DONE) {
                auto q = std::find(voc_queue_.begin(), voc_queue_.end(), s);
                if (q != voc_queue_.end()) {
                    voc_queue_.erase(q);
                    if (s->pool_idx >= 0) latpool_free_.push_back(s->pool_idx);
                    s->pool_idx = -1;
                    finish_cancelled(s);
                }
            }
        }
    }

    // ------------------------------------------------------------------ one scheduler iteration
    // A failure inside a step (HIP error, exhausted pool) must not leave slots, KV blocks and pool entries half-updated:
    // every sequence that was in flight is failed (aur_result.error), its resources go back to the pools, and the
    // exception continues to the caller.  The engine stays usable if the device is.
    void step(int* n_live, int* n_finished_total) {
        std::lock_guard<std::mutex> gl(gpu_mu_);
        try {
            step_locked(n_live, n_finished_total);
        } catch (const InvalidArgument&) {
            fail_in_flight(AUR_E_INVALID);
            throw;
        } catch (const StateError&) {
            fail_in_flight(AUR_E_STATE);
            throw;
        } catch (...) {
            fail_in_flight(AUR_E_HIP);
            throw;
        }
    }
    void fail_in_flight(int code) {
        (void)hipStreamSynchronize(st_);
        (void)hipStreamSynchronize(st_voc_);
        (void)hipGetLastError();
        gpt_->reset_after_failure();
        infl_.on = false;
        just_finished_.clear();
        voc_->drop_events();
        std::lock_guard<std::mutex> lk(mu_);
        auto fail = [&](Seq* s) {
            for (int b : s->blocks) free_blocks_.push_back(b);
            s->blocks.clear();
            if (s->pool_idx >= 0) latpool_free_.push_back(s->pool_idx);
            s->pool_idx = -1;
            if (s->slot >= 0) slot_owner_[s->slot] = nullptr;
            s->slot = -1;
            s->error = code;
            s->wav = nullptr; s->n_samples = 0; s->latents = nullptr; s->n_latent_rows = 0; s->enc = nullptr; s->n_enc = 0;
            spk_info_[s->spk_row].refs--;
            s->state = SeqState::DONE;
            done_.push_back(s);
            finished_total_++;
        };
        for (Seq* s : slot_owner_)
            if (s) fail(s);
        for (Seq* s : voc_queue_) fail(s);
        voc_queue_.clear();
        // the vocoder batch, whether it had been launched completely (voc_active_) or the throw came from inside voc_launch
        // after the sequences had left the queue
        for (Seq* s : voc_batch_)
            if (s->state != SeqState::DONE) fail(s);
        if (voc_block_held_ && voc_block_) voc_block_->refs--;
        voc_block_held_ = false;
        voc_batch_.clear();
        voc_active_ = false;
        voc_split_rest_ = false;
    }
    void step_locked(int* n_live, int* n_finished_total) {
        use();
        ensure_gpt();
        if (fail_at_step_ > 0 && --fail_at_step_ == 0) {   // AUR_TEST_FAIL_STEP=n: fault injection for the recovery test
            throw HipError("injected failure (AUR_TEST_FAIL_STEP)");
        }
        bool worked = false;
        process_cancels();
        // back-pressure: every running sequence must be able to park its latents when it finishes
        while ((int)latpool_free_.size() < cfg_.max_seqs) {
            if (voc_active_)
                voc_poll(true);
            else if (!voc_queue_.empty())
                voc_launch();
            else
                break;
        }
        // 1. admission + prefill
        std::vector<Seq*> admitted;
        {
            std::lock_guard<std::mutex> lk(mu_);
            int rows = 0;
            // aur_config.admit_min_batch: a prefill pass costs ~150 launches whatever its rows; with a queue longer than the free
            // slots, wait until a group of slots is free (the decode step costs the same at 56 rows as at 64)
            int free_slots = 0;
            for (int i = 0; i < cfg_.max_seqs; ++i)
                if (!slot_owner_[i]) ++free_slots;
            // (default: an eighth of the slots -- the group size that balances the pass's fixed cost against the idle slot-steps grows
            // with the slot count: g* ~ slots * sqrt(2 * pass_ms / (step_ms * tokens per sequence)) ~ slots / 7 at 30 layers)
            const int group = std::min(cfg_.admit_min_batch > 0 ? cfg_.admit_min_batch : std::max(1, cfg_.max_seqs / 8), cfg_.max_seqs);
            // ... but never for long: with few finishes in sight the free slots would idle while requests wait (kAdmitHoldSteps decode
            // steps ~ 60 ms at 30 layers, then whatever fits is admitted)
            // aur_seq_desc.priority (latency-critical sequences: the head chunk of a stream somebody is waiting to hear).  While one of
            // them waits or runs, (1) it is admitted at once, whatever the group logic says; (2) the others are admitted only up to
            // `urgent_rows` running sequences -- a decode step's time grows with its rows (attention above all: 1.6 ms at 64 rows, ~3 ms
            // at 192 and 30 layers), and every step of the urgent sequence pays it -- and only in groups (a prefill pass in front of
            // every step would stall the urgent sequence's steps for the pass's ~4.5 ms of launches each time).
            int urgent_waiting = 0, n_running = cfg_.max_seqs - free_slots;
            bool urgent_running = false;
            for (Seq* q : waiting_) urgent_waiting += q->params.priority > 0 ? 1 : 0;
            for (int i = 0; i < cfg_.max_seqs; ++i)
                if (slot_owner_[i] && slot_owner_[i]->params.priority > 0 && slot_owner_[i]->state == SeqState::RUNNING) urgent_running = true;
            const bool urgent = urgent_waiting > 0 || urgent_running;
            // (default a quarter of the slots; measured on the long-form stream at 192 slots, profiles/r06_c5s_urgent_sweep.log: first chunk
            // 0.55 s / 32.2 M samples/s without a cap, 0.43 / 32.3 at 128 rows, 0.42 / 31.3 at 96, 0.33 / 31.5 at 64, 0.30 / 31.5 at 48)
            const int urgent_cap = std::min(cfg_.max_seqs, cfg_.urgent_rows > 0 ? cfg_.urgent_rows : std::max(1, cfg_.max_seqs / 4));
            const int n_plain = (int)waiting_.size() - urgent_waiting;
            const int free_eff = urgent ? std::max(0, std::min(free_slots, urgent_cap - n_running)) : free_slots;
            bool hold = free_slots < cfg_.max_seqs && free_eff < std::min(group, n_plain);
            // (an urgent sequence running beside a trickle of arrivals: wait for a group or kUrgentHoldSteps, not a pass per step)
            if (!hold && urgent_running && n_plain > 0 && n_plain < group && free_eff > 0) hold = true;
            if (hold && free_eff > 0 && ++admit_hold_steps_ > (urgent_running ? kUrgentHoldSteps : kAdmitHoldSteps)) hold = false;
            if (!hold) admit_hold_steps_ = 0;
            while (!waiting_.empty()) {
                Seq* s = waiting_.front();
                const bool s_urgent = s->params.priority > 0;
                if (!s_urgent && (hold || (urgent && n_running + (int)admitted.size() >= urgent_cap))) break;
                const SpeakerInfo& si = spk_info_[s->spk_row];
                s->shared_prefix = si.ready && share_prefix_now_;
                const int skip = s->shared_prefix ? 2 : 0;   // table entries 0,1 = the speaker's shared prefix blocks
                const int extra = cfg_.second_pass ? 4 : 0;   // second pass appends 4 stop tokens after the generated ones
                const int need = (s->n_prompt + s->params.max_tokens + extra + kKvBlockTokens - 1) / kKvBlockTokens - skip;
                int slot = -1;
                for (int i = 0; i < cfg_.max_seqs; ++i)
                    if (!slot_owner_[i]) {
                        slot = i;
                        break;
                    }
                const int n_rows = s->n_prompt - (s->shared_prefix ? 32 : 0);
                if (slot < 0 || (int)free_blocks_.size() < need || rows + n_rows > cfg_.max_prefill_rows) break;
                waiting_.pop_front();
                s->slot = slot;
                slot_owner_[slot] = s;
                for (int b = 0; b < skip; ++b) h_block_tables_[(size_t)slot * kMaxBlocks + b] = si.blocks[b];
                for (int b = 0; b < need; ++b) {
                    s->blocks.push_back(free_blocks_.back());
                    free_blocks_.pop_back();
                    h_block_tables_[(size_t)slot * kMaxBlocks + skip + b] = s->blocks.back();
                }
                s->state = SeqState::RUNNING;
                rows += n_rows;
                admitted.push_back(s);
            }
        }
        if (!admitted.empty()) {
            HIP_CHECK(hipEventRecord(ev_a_, st_));
            prefill(admitted);   // synchronises the stream before it returns
            HIP_CHECK(hipEventRecord(ev_b_, st_));
            HIP_CHECK(hipEventSynchronize(ev_b_));
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, ev_a_, ev_b_));
            stats_.gpt_ms += ms;
            stats_.prefill_ms += ms;
            stats_.prefill_batches++;
            worked = true;
        }
        // 2. decode step for every running sequence (GPU time is accounted per collected step inside decode)
        std::vector<int> active;
        for (int i = 0; i < cfg_.max_seqs; ++i)
            if (slot_owner_[i] && slot_owner_[i]->state == SeqState::RUNNING) active.push_back(i);
        if (!active.empty()) {
            HIP_CHECK(hipEventRecord(ev_a_, st_));
            decode_pipelined(active);
            worked = true;
        }
        {
            bool any_running = false;
            for (int i = 0; i < cfg_.max_seqs; ++i)
                if (slot_owner_[i] && slot_owner_[i]->state == SeqState::RUNNING) any_running = true;
            if (!any_running) drain_inflight();
        }
        if (worked) stats_.steps++;
        // 3. vocoder stage (asynchronous): finished sequences left their slots already (latents parked in the pool);
        //    one vocoder batch is in flight on its own stream while the next GPT steps run on the main stream.
        voc_poll(false);
        int running = 0;
        for (int i = 0; i < cfg_.max_seqs; ++i)
            if (slot_owner_[i]) ++running;
        size_t n_wait;
        {
            std::lock_guard<std::mutex> lk(mu_);
            n_wait = waiting_.size();
        }
        // aur_config.vocoder_min_batch: a vocoder pass of one utterance costs twice per utterance what a pass of eight does (and
        // slows the decode steps it runs beside); finished sequences wait for company, at most kVocHoldSteps steps
        const int minb = cfg_.vocoder_min_batch > 0 ? cfg_.vocoder_min_batch : std::max(1, cfg_.max_seqs / 16);
        // (the hold runs from the step the oldest queued sequence finished, also while another batch is in flight: reset only when
        // nothing waits, so a sequence queued behind an active batch is launched as soon as that batch is done once its hold is up)
        if (voc_queue_.empty()) voc_hold_steps_ = 0;
        else ++voc_hold_steps_;
        if (voc_queue_.empty()) voc_split_rest_ = false;   // (cancelled meanwhile)
        bool urgent_voc = false;   // an urgent sequence does not wait for company: its batch is whatever has finished with it
        for (Seq* q : voc_queue_) urgent_voc |= q->params.priority > 0;
        if (!voc_active_ && !voc_queue_.empty() &&
            ((int)voc_queue_.size() >= minb || urgent_voc || voc_split_rest_ || (running == 0 && n_wait == 0) || voc_hold_steps_ > kVocHoldSteps)) {
            voc_launch();
            voc_hold_steps_ = 0;
        }
        if (running == 0 && n_wait == 0 && voc_active_) voc_poll(true);   // nothing else to do: wait for the batch
        if (running == 0 && n_wait == 0 && !voc_active_ && !voc_queue_.empty()) {
            voc_launch();
            voc_poll(true);
        }
        {
            std::lock_guard<std::mutex> lk(mu_);
            int live = (int)waiting_.size() + (int)voc_queue_.size() + (voc_active_ ? (int)voc_batch_.size() : 0);
            for (int i = 0; i < cfg_.max_seqs; ++i)
                if (slot_owner_[i]) ++live;
            if (n_live) *n_live = live;
            if (n_finished_total) *n_finished_total = (int)finished_total_;
        }
    }

    // ------------------------------------------------------------------ standalone vocoder
    void vocode_host(const float* latents, const int* n_lat, const float* speed, const int* sample_rate, int B, int t_max, uint64_t key,
                     float* wav_out, int64_t wav_stride, int* n_samples_out) {
        use();
        voc_->bind();
        const int row = speaker_row(key, false);
        AUR_REQUIRE(row >= 0, "unknown speaker_key");
        AUR_REQUIRE(B >= 1 && t_max >= 1, "B, t_max");
        AUR_REQUIRE(!voc_active_, "vocoder stage busy");
        std::vector<int> nl(n_lat, n_lat + B), cond(B, row);
        std::vector<float> sp(B, 0.f);
        if (speed) sp.assign(speed, speed + B);
        std::vector<int> sr(B, 0);
        if (sample_rate) sr.assign(sample_rate, sample_rate + B);
        int max_samples = 0;
        for (int b = 0; b < B; ++b) {
            AUR_REQUIRE(nl[b] >= 1 && nl[b] <= t_max, "n_lat in [1,t_max]");
            AUR_REQUIRE(speed_valid(sp[b]), "speed is 0 (unset) or in [0.5, 2.0]");
            AUR_REQUIRE(rate_class(sr[b]) >= 0, "sample_rate is 0 (unset) or one of 8000, 16000, 22050, 24000, 32000, 44100, 48000");
            max_samples = std::max(max_samples, out_samples(nl[b], sp[b], sr[b]));
        }
        AUR_REQUIRE(wav_stride >= max_samples, "wav_stride too small");
        max_samples = (max_samples + 3) & ~3;   // the device rows: whole 16-byte stores (voc_launch)
        tmp_lat_.ensure((size_t)B * t_max * kHidden * sizeof(float));
        HIP_CHECK(hipMemcpyAsync(tmp_lat_.p, latents, (size_t)B * t_max * kHidden * sizeof(float),
                                 hipMemcpyHostToDevice, st_voc_));
        tmp_wav_.ensure((size_t)B * max_samples * sizeof(float));
        voc_->forward(B, nl, sp, sr, tmp_lat_.as<float>(), (long)t_max * kHidden, nullptr, cond, tmp_wav_.as<float>(), max_samples,
                      voc_cond_.as<float>(), cfg_.profile != 0);
        stats_.vocoder_batches++;
        HIP_CHECK(hipStreamSynchronize(st_voc_));
        voc_->collect(stats_);
        for (int b = 0; b < B; ++b) {
            const int ns = out_samples(nl[b], sp[b], sr[b]);
            HIP_CHECK(hipMemcpy(wav_out + (long)b * wav_stride, tmp_wav_.as<float>() + (long)b * max_samples,
                                (size_t)ns * sizeof(float), hipMemcpyDeviceToHost));
            if (n_samples_out) n_samples_out[b] = ns;
        }
    }

    // ------------------------------------------------------------------ standalone FLAC encoder (aur_encode_flac)
    void encode_flac(const float* const* x, const int32_t* n, const int32_t* rate, int B, uint8_t* out, int64_t out_stride, int64_t* out_lens) {
        std::lock_guard<std::mutex> gl(gpu_mu_);   // not while a step is running (shares the vocoder stream, in order behind a pass in flight)
        use();
        AUR_REQUIRE(B >= 1, "encode_flac: B >= 1");
        std::vector<int> len(n, n + B), sr(rate, rate + B);
        long max_n = 0;
        for (int b = 0; b < B; ++b) {
            AUR_REQUIRE(x[b], "encode_flac: null row");
            AUR_REQUIRE(len[b] >= 1 && len[b] <= kFlacMaxSamples, "encode_flac: 1 <= samples <= 2^24 per row");
            AUR_REQUIRE(sr[b] >= 1 && sr[b] < kFlacMaxRate, "encode_flac: 1 <= sample rate < 2^20");
            for (int i = 0; i < len[b]; ++i) AUR_REQUIRE(std::isfinite(x[b][i]), "encode_flac: samples must be finite");
            max_n = std::max(max_n, (long)len[b]);
        }
        const long bound = flac_stream_bound(max_n), ostride = (bound + 15) & ~15L, xstride = (max_n + 3) & ~3L;
        AUR_REQUIRE(out_stride >= bound, "encode_flac: out_stride must hold aur_flac_bound(longest row)");
        flac_x_.ensure((size_t)B * xstride * 4);
        flac_out_.ensure((size_t)B * ostride + (size_t)B * 4);
        for (int b = 0; b < B; ++b)
            HIP_CHECK(hipMemcpyAsync(flac_x_.as<float>() + (size_t)b * xstride, x[b], (size_t)len[b] * 4, hipMemcpyHostToDevice, st_voc_));
        int* d_len = reinterpret_cast<int*>(flac_out_.as<uint8_t>() + (size_t)B * ostride);
        flac_host_.encode(flac_x_.as<float>(), xstride, nullptr, len, sr, flac_out_.as<uint8_t>(), ostride, d_len, st_voc_);
        std::vector<int> got(B);
        HIP_CHECK(hipMemcpyAsync(got.data(), d_len, (size_t)B * 4, hipMemcpyDeviceToHost, st_voc_));
        HIP_CHECK(hipStreamSynchronize(st_voc_));
        for (int b = 0; b < B; ++b) {
            if (got[b] < kFlacHeader || got[b] > flac_stream_bound(len[b])) throw HipError("encode_flac: stream length out of range");
            HIP_CHECK(hipMemcpy(out + (size_t)b * out_stride, flac_out_.as<uint8_t>() + (size_t)b * ostride, (size_t)got[b], hipMemcpyDeviceToHost));
            out_lens[b] = got[b];
        }
    }

    void sync() {
        use();
        HIP_CHECK(hipStreamSynchronize(st_));
        HIP_CHECK(hipStreamSynchronize(st_voc_));
    }
    aur_stats stats() {
        std::lock_guard<std::mutex> lk(mu_);
        aur_stats s = stats_;
        s.kv_blocks_total = n_blocks_;
        s.kv_blocks_free = (int64_t)free_blocks_.size();
        s.result_blocks = (int64_t)result_blocks_.size();
        s.result_blocks_free = 0;
        s.result_block_bytes = 0;
        for (auto& b : result_blocks_) {
            if (b->refs == 0) s.result_blocks_free++;
            s.result_block_bytes += (int64_t)b->buf.bytes;
        }
        s.speakers = (int64_t)spk_rows_.size();
        s.sequences_tracked = (int64_t)seqs_.size();
        return s;
    }
    // aur_get_load.  Host only: the queue lock and nothing else -- no HIP call, no wait for a running step.  Everything read here is
    // written under mu_ (Seq::state, slot_owner_, seqs_) or atomic (Seq::n_gen); the vocoder queue and the token vectors, which the
    // driver thread changes without the lock, are not looked at.
    aur_load load_now() {
        std::lock_guard<std::mutex> lk(mu_);
        aur_load l{};
        for (auto& kv : seqs_) {
            const Seq& s = *kv.second;
            if (s.state == SeqState::WAITING) l.waiting++;
            else if (s.state == SeqState::RUNNING) l.running++;
            else if (s.state == SeqState::TOKENS_DONE) l.vocoding++;
            if (s.state == SeqState::WAITING || s.state == SeqState::RUNNING)
                l.token_budget += std::max(0, s.params.max_tokens - s.n_gen.load(std::memory_order_relaxed));
        }
        for (const Seq* s : slot_owner_)
            if (!s) l.free_slots++;
        return l;
    }
    void reset_stats() {
        std::lock_guard<std::mutex> lk(mu_);
        stats_ = aur_stats{};
    }
    void set_profile(int every) {
        std::lock_guard<std::mutex> gl(gpu_mu_);   // not while a step is running
        AUR_REQUIRE(every >= 0, "aur_set_profile: every >= 0");
        cfg_.profile = every > 0 ? 1 : 0;
        profile_every_ = every > 0 ? every : kProfileEvery;
        decode_step_count_ = 0;
    }

    // ------------------------------------------------------------------ debug entry points
    void dbg_prefill(const int* text_ids, int n_text, uint64_t key, float rep_penalty, float* lnf_rows_out,
                     float* logits_out) {
        use();
        ensure_gpt();
        AUR_REQUIRE(idle(), "dbg_prefill needs an idle engine");
        aur_seq_desc d{};
        d.text_ids = text_ids; d.n_text = n_text; d.speaker_key = key; d.temperature = 0.f; d.top_p = 1.f; d.top_k = -1;
        d.repetition_penalty = rep_penalty; d.max_tokens = 1; d.seed = 0; d.ignore_stop = 1;
        const uint64_t id = submit(d);
        {
            struct Restore {   // also when the step throws
                Engine& e;
                ~Restore() { e.share_prefix_now_ = true, e.gpt_->set_capture(false); }
            } restore{*this};
            gpt_->set_capture(true);
            share_prefix_now_ = false;
            step(nullptr, nullptr);
        }
        for (int guard = 0; guard < 1000 && seqs_.at(id)->state != SeqState::DONE; ++guard) step(nullptr, nullptr);
        Seq* s = seqs_.at(id).get();
        if (lnf_rows_out)
            HIP_CHECK(hipMemcpy(lnf_rows_out, gpt_->dbg_lnf(), (size_t)s->n_prompt * kHidden * 4, hipMemcpyDeviceToHost));
        if (logits_out) HIP_CHECK(hipMemcpy(logits_out, gpt_->dbg_logits(), (size_t)kMelVocab * 4, hipMemcpyDeviceToHost));
        aur_result r;
        while (poll(&r, 1) == 1) {
        }
        release(id);
    }
    void dbg_sample(const float* logits, int B, float temperature, float top_p, int top_k, float rep,
                    const uint8_t* seen, uint32_t seed, int step_idx, int* tokens_out) {
        use();
        AUR_REQUIRE(idle(), "dbg_sample needs an idle engine");
        AUR_REQUIRE(B >= 1 && B <= cfg_.max_seqs, "B <= max_seqs");
        gpt_->dbg_sample(logits, B, temperature, top_p, top_k, rep, seen, seed, step_idx, tokens_out);
    }

private:
    bool idle() {
        std::lock_guard<std::mutex> lk(mu_);
        if (!waiting_.empty() || !voc_queue_.empty() || voc_active_ || infl_.on) return false;
        for (auto* s : slot_owner_)
            if (s) return false;
        return true;
    }

    // the read-back of a sampler launch, once its copy has landed: appends the tokens (token | finished bit per row of `slots`),
    // notes the sequences that finished with theirs, returns the rows that drew one
    int append_tokens(const int* pin, const std::vector<int>& slots) {
        int rows = 0;
        for (size_t j = 0; j < slots.size(); ++j) {
            const int raw = pin[j];
            if (raw < 0) continue;   // ghost row of a sequence that had already finished
            Seq* s = slot_owner_[slots[j]];
            AUR_REQUIRE(s && s->state == SeqState::RUNNING, "token read-back for a slot without a running sequence");
            s->tokens.push_back(raw & ~kTokFinishedBit);
            s->n_gen.fetch_add(1, std::memory_order_relaxed);
            stats_.tokens_generated++;
            ++rows;
            if (raw & kTokFinishedBit) just_finished_.push_back(s);
        }
        return rows;
    }
    // sequences whose tokens completed in this step: (optional literal second pass) -> latent pool -> vocoder queue
    void retire_finished() {
        if (just_finished_.empty()) return;
        if (cfg_.second_pass) {
            std::vector<Seq*> wanted;
            for (Seq* s : just_finished_)
                if (!s->cancel) wanted.push_back(s);
            if (!wanted.empty()) second_pass(wanted);
        }
        for (Seq* s : just_finished_) finish_tokens(s);
        just_finished_.clear();
    }
    // A/B mode (aur_config.second_pass): the reference's get_model_logits (XTTSv2.py:617-687) restated on the GPU: one
    // prefill over [cond ; 1024 ; tokens ; 1025 x 4] with mel positions 0..N+4, collect ln_f rows of positions
    // n_cond .. n_cond+N-1 (i.e. drop the last 5), apply final_norm twice.  The sequence still owns its slot and KV
    // blocks, which are simply overwritten.  The default path (latent stash) never runs this.
    void second_pass(const std::vector<Seq*>& seqs) {
        std::vector<int4> desc;
        std::vector<int> row_slot, row_pos, lat_row0;
        for (Seq* s : seqs) {
            const int first = s->shared_prefix ? 32 : 0;
            const int n_cond = 32 + (int)s->text_ids.size();
            for (int i = first; i < 32; ++i) desc.push_back(make_int4(0, i, s->spk_row, 0));
            for (int i = 0; i < (int)s->text_ids.size(); ++i) desc.push_back(make_int4(1, s->text_ids[i], i, 0));
            lat_row0.push_back((int)desc.size());
            const int N = (int)s->tokens.size();
            for (int j = 0; j < N + 5; ++j) {
                const int id = (j == 0) ? kStartToken : (j <= N ? s->tokens[j - 1] : kStopToken);
                desc.push_back(make_int4(2, id, std::min(j, kMaxLatRows - 1), 0));   // trailing rows are dropped; keep wpe in range
            }
            for (int i = first; i < n_cond + N + 5; ++i) {
                row_slot.push_back(s->slot);
                row_pos.push_back(i);
            }
        }
        const int M = (int)row_slot.size();
        gpt_->prompt_rows(desc, row_slot, row_pos, spk_table_.as<float>());
        for (size_t k = 0; k < seqs.size(); ++k) {
            Seq* s = seqs[k];
            if (latpool_free_.empty()) throw StateError("latent pool exhausted");
            s->pool_idx = latpool_free_.back();
            latpool_free_.pop_back();
            gpt_->double_norm_rows(lat_row0[k], latpool_.as<float>() + (long)s->pool_idx * kMaxLatRows * kHidden, (int)s->tokens.size());
        }
        HIP_CHECK(hipStreamSynchronize(st_));
        stats_.prefill_rows += M;
    }
    void finish_tokens(Seq* s) {
        if (s->cancel) {   // aur_cancel: nobody wants the audio -- free slot and blocks, report it, no vocoder
            std::lock_guard<std::mutex> lk(mu_);
            for (int b : s->blocks) free_blocks_.push_back(b);
            s->blocks.clear();
            slot_owner_[s->slot] = nullptr;
            s->slot = -1;
            finish_cancelled(s);
            return;
        }
        // park the stashed latents in the pool (D2D on the main stream, ordered before any later prefill that reuses
        // the slot) and release slot + KV blocks at once: the vocoder stage no longer occupies a batcher slot
        if (s->pool_idx < 0) {   // (the second-pass mode has already written the pool entry)
            if (latpool_free_.empty()) throw StateError("latent pool exhausted");
            s->pool_idx = latpool_free_.back();
            latpool_free_.pop_back();
            const size_t n = s->tokens.size() * (size_t)kHidden * sizeof(float);
            HIP_CHECK(hipMemcpyAsync(latpool_.as<float>() + (long)s->pool_idx * kMaxLatRows * kHidden,
                                     gpt_->stash(s->slot), n, hipMemcpyDeviceToDevice, st_));
        }
        HIP_CHECK(hipEventRecord(ev_lat_, st_));
        std::lock_guard<std::mutex> lk(mu_);
        s->state = SeqState::TOKENS_DONE;   // (under the lock: aur_cancel reads the state from another thread)
        for (int b : s->blocks) free_blocks_.push_back(b);
        s->blocks.clear();
        slot_owner_[s->slot] = nullptr;
        s->slot = -1;
        voc_queue_.push_back(s);
    }
    void prefill(const std::vector<Seq*>& seqs) {
        std::vector<int4> desc;
        std::vector<int> row_slot, row_pos, sample_row, sample_slot, next_kvpos;
        std::vector<SlotInit> init;
        for (Seq* s : seqs) {
            const aur_seq_desc& p = s->params;
            init.push_back(SlotInit{s->slot, p.temperature, p.top_p, p.top_k, p.repetition_penalty, p.max_tokens,
                                    p.ignore_stop, p.seed, 0});
            const int first = s->shared_prefix ? 32 : 0;     // rows 0..31 live in the speaker's shared KV blocks
            for (int i = first; i < 32; ++i) desc.push_back(make_int4(0, i, s->spk_row, 0));
            for (int i = 0; i < (int)s->text_ids.size(); ++i) {
                const int id = s->text_ids[i];
                AUR_REQUIRE(gpt_->text_ok(id, i), "text id / position out of range");
                desc.push_back(make_int4(1, id, i, 0));
            }
            desc.push_back(make_int4(2, kStartToken, 0, 0));
            for (int i = first; i < s->n_prompt; ++i) {
                row_slot.push_back(s->slot);
                row_pos.push_back(i);
            }
            sample_row.push_back((int)row_slot.size() - 1);
            sample_slot.push_back(s->slot);
            next_kvpos.push_back(s->n_prompt);
        }
        const int M = (int)row_slot.size();
        gpt_->init_slots(init);
        gpt_->upload_block_tables(h_block_tables_);
        gpt_->prompt_rows(desc, row_slot, row_pos, spk_table_.as<float>());
        gpt_->capture_prompt_rows(M);   // (aur_dbg_prefill)
        stats_.prefill_rows += M;
        const int* pin = gpt_->sample_prompt(sample_row, sample_slot, next_kvpos);
        HIP_CHECK(hipStreamSynchronize(st_));
        append_tokens(pin, sample_slot);
        retire_finished();
    }
    // ---- pipelined decode (default): the step's kernel chain depends only on device-resident state, so step s+1 is
    // enqueued BEFORE the host waits for the token / finished-flag read-back of step s (otherwise the GPU idles for the
    // host round trip, ~80 us of a 2.8 ms step).  A sequence that turns out to have finished in step s rides along in
    // step s+1 as a ghost: the sampler leaves a finished slot untouched and reports token -1, its K/V write lands in
    // a block the sequence had reserved, and the GEMMs are bitwise batch-invariant, so the other rows are unaffected.
    struct InFlight {
        bool on = false;
        std::vector<int> slots;   // live slots at launch, in row order
        int buf = 0;              // read-back buffer / event index
        bool profiled = false;
    };
    InFlight launch_decode_step(const std::vector<int>& active) {
        InFlight f;
        f.on = true;
        f.slots = active;
        f.buf = rb_next_;
        rb_next_ ^= 1;
        f.profiled = cfg_.profile != 0 && (decode_step_count_++ % profile_every_ == 0);
        pin_rb_[f.buf].ensure(((size_t)cfg_.max_seqs * 2 + 16) * sizeof(int));
        // algorithmic bytes of this step: every live sequence's context (prompt + tokens so far, + 1 if the previous step is
        // still in flight) in K and V, all layers; the weights once
        double kv_tokens = 0.0;
        for (int slot : active) {
            const Seq* sq = slot_owner_[slot];
            kv_tokens += (double)(sq->n_prompt + (int)sq->tokens.size() + (infl_.on ? 1 : 0));
        }
        stats_.decode_kv_bytes += (cfg_.kv_fp16 ? 4.0 : 8.0) * kHidden * kv_tokens * cfg_.n_layer;
        stats_.decode_weight_bytes += (cfg_.gpt_fp16 ? 2.0 : 4.0) * cfg_.n_layer * 12.0 * kHidden * kHidden + 4.0 * kHidden * kMelVocab;
        gpt_->decode_step(active, f.profiled, kv_tokens, pin_rb_[f.buf].as<int>(), ev_step_[f.buf]);
        return f;
    }
    void collect_decode_step(InFlight& f) {
        HIP_CHECK(hipEventSynchronize(ev_step_[f.buf].readback));
        const int rows = append_tokens(pin_rb_[f.buf].as<int>(), f.slots);
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, ev_step_[f.buf].start, ev_step_[f.buf].end));
        stats_.gpt_ms += ms;
        stats_.decode_ms += ms;
        stats_.decode_steps++;
        stats_.decode_rows += rows;
        if (f.profiled) gpt_->collect_profile(stats_);
        f.on = false;
    }
    // launch the next step ahead of the read-back only if some sequence is certain to need it
    bool worth_speculating(const std::vector<int>& active, const InFlight& pending) const {
        if (!pipeline_ || cfg_.second_pass || debug_sync()) return false;
        for (int slot : active) {
            const Seq* s = slot_owner_[slot];
            const bool in_pending = std::find(pending.slots.begin(), pending.slots.end(), slot) != pending.slots.end();
            const int n_after = (int)s->tokens.size() + (in_pending ? 1 : 0);
            if (n_after < s->params.max_tokens) return true;
        }
        return false;
    }
    void decode_pipelined(const std::vector<int>& active) {
        if (!infl_.on) infl_ = launch_decode_step(active);
        InFlight next;
        const auto t0 = std::chrono::steady_clock::now();
        if (worth_speculating(active, infl_)) next = launch_decode_step(active);
        const auto t1 = std::chrono::steady_clock::now();
        collect_decode_step(infl_);
        const auto t2 = std::chrono::steady_clock::now();
        if (host_trace_) {
            ht_launch_ns_ += std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
            ht_wait_ns_ += std::chrono::duration_cast<std::chrono::nanoseconds>(t2 - t1).count();
            if (++ht_n_ % 256 == 0)
                fprintf(stderr, "[aur host trace] rows %zu: launch_decode_step %.1f us of host time per step, wait for the read-back %.1f us\n", active.size(),
                        ht_launch_ns_ / 256e3, ht_wait_ns_ / 256e3), ht_launch_ns_ = ht_wait_ns_ = 0;
        }
        retire_finished();
        infl_ = next;
    }
    void drain_inflight() {   // only ghosts can be left once no sequence is running
        if (infl_.on) collect_decode_step(infl_);
        retire_finished();
    }

    // ------------------------------------------------------------------ vocoder
    void voc_launch() {
        // The workspace is B x maxT and a slowed utterance is up to twice as long (aur_seq_desc.speed): a pass takes the longest prefix
        // of the queue with B * maxT <= max_seqs * frames_for(kMaxLatRows), today's worst case; a single utterance is always admissible
        // and the rest stays queued for the next pass.  (Batch invariance is bitwise, so results do not depend on where the cut falls.)
        const long cap = (long)cfg_.max_seqs * frames_for(kMaxLatRows);
        int B = 0, maxT = 0;
        while (B < (int)std::min(voc_queue_.size(), (size_t)cfg_.max_seqs)) {
            const Seq* q = voc_queue_[B];
            const int t = std::max(maxT, frames_for(stretched_rows((int)q->tokens.size(), q->params.speed)));
            if (B > 0 && (long)(B + 1) * t > cap) break;
            maxT = t;
            ++B;
        }
        voc_split_rest_ = B < (int)std::min(voc_queue_.size(), (size_t)cfg_.max_seqs);   // the rest goes as soon as the stage is free
        voc_batch_.assign(voc_queue_.begin(), voc_queue_.begin() + B);
        voc_queue_.erase(voc_queue_.begin(), voc_queue_.begin() + B);
        voc_nl_.resize(B);
        voc_speed_.resize(B);
        voc_rate_.resize(B);
        std::vector<int> rows(B), cond(B);
        // The result block's row stride: the longest utterance as it leaves, max_b n_out(b), in whole 16-byte stores.  At 24000 that is
        // maxT * 256 as ever; a pass at 48000 pins up to twice those bytes (aur_seq_desc.sample_rate), one at 8000 a third.
        voc_max_samples_ = 0;
        for (int b = 0; b < B; ++b) {
            voc_nl_[b] = (int)voc_batch_[b]->tokens.size();
            voc_speed_[b] = voc_batch_[b]->params.speed;
            voc_rate_[b] = voc_batch_[b]->params.sample_rate;
            voc_max_samples_ = std::max(voc_max_samples_, (out_samples(voc_nl_[b], voc_speed_[b], voc_rate_[b]) + 3) & ~3);
            rows[b] = voc_batch_[b]->pool_idx;
            cond[b] = voc_batch_[b]->spk_row;
        }
        {
            std::lock_guard<std::mutex> lk(mu_);
            voc_block_ = nullptr;
            for (auto& blk : result_blocks_)
                if (blk->refs == 0) voc_block_ = blk.get();
            if (!voc_block_) {
                result_blocks_.emplace_back(new PinBlock());
                voc_block_ = result_blocks_.back().get();
            }
            voc_block_->refs = 1;   // held by the in-flight batch
            voc_block_held_ = true;
        }
        if (fail_at_voc_ > 0 && --fail_at_voc_ == 0)   // AUR_TEST_FAIL_VOC=n: fault injection inside the n-th vocoder launch
            throw HipError("injected failure (AUR_TEST_FAIL_VOC)");
        // aur_seq_desc.encoding: the rows that also leave as FLAC streams.  Block layout: float rows | latents | streams (one row per
        // encoded utterance at voc_enc_stride_ = the longest one's bound, 42 + frames * 8205) | their lengths.  A pass without such a
        // row is what it was: same launches, same arguments, nothing allocated.
        voc_enc_rows_.clear();
        std::vector<int> enc_len, enc_rate;
        voc_enc_stride_ = 0;
        for (int b = 0; b < B; ++b)
            if (voc_batch_[b]->params.encoding) {
                voc_enc_rows_.push_back(b);
                enc_len.push_back(out_samples(voc_nl_[b], voc_speed_[b], voc_rate_[b]));
                enc_rate.push_back(voc_rate_[b] ? voc_rate_[b] : 24000);
                voc_enc_stride_ = std::max(voc_enc_stride_, (flac_stream_bound(enc_len.back()) + 15) & ~15L);
            }
        const size_t wav_bytes = (size_t)B * voc_max_samples_ * 4, lat_bytes = cfg_.return_latents ? (size_t)B * kMaxLatRows * kHidden * 4 : 0;
        const size_t n_enc = voc_enc_rows_.size(), enc_bytes = n_enc * (size_t)voc_enc_stride_;
        voc_block_->buf.ensure(wav_bytes + lat_bytes + enc_bytes + n_enc * 4);
        HIP_CHECK(hipStreamWaitEvent(st_voc_, ev_lat_, 0));   // latents parked by the main stream
        // The waveform goes straight into the pinned result block: conv_post (Cin -> 1, + tanh: 0.4 ms of HBM-bound work per 64
        // utterances) stores its samples over PCIe -- coalesced 1 KiB per workgroup -- instead of into device memory with one D2H copy
        // per sequence behind it (80 MB in 64 copies: 3.2 ms of the 64-utterance step with nothing to overlap, the batch's last
        // decode step being over).  hipHostMalloc memory is device-visible and coherent; the event below orders the host's reads.
        float* hw = voc_block_->buf.as<float>();
        float* hl = hw + (size_t)B * voc_max_samples_;
        // an encoded pass keeps the delivered waveform in device memory for the encoder; the float rows follow in one copy (same bits)
        float* wav_dst = hw;
        if (n_enc) {
            voc_dev_wav_.ensure(wav_bytes);
            wav_dst = voc_dev_wav_.as<float>();
        }
        voc_->forward(B, voc_nl_, voc_speed_, voc_rate_, latpool_.as<float>(), (long)kMaxLatRows * kHidden, &rows, cond, wav_dst, voc_max_samples_,
                      voc_cond_.as<float>(), cfg_.profile != 0);
        stats_.vocoder_batches++;
        if (n_enc) {
            HIP_CHECK(hipMemcpyAsync(hw, wav_dst, wav_bytes, hipMemcpyDeviceToHost, st_voc_));
            voc_dev_enc_.ensure(enc_bytes + n_enc * 4);
            uint8_t* d_enc = voc_dev_enc_.as<uint8_t>();
            flac_pass_.encode(wav_dst, voc_max_samples_, &voc_enc_rows_, enc_len, enc_rate, d_enc, voc_enc_stride_,
                              reinterpret_cast<int*>(d_enc + enc_bytes), st_voc_);
            HIP_CHECK(hipMemcpyAsync(reinterpret_cast<uint8_t*>(hw) + wav_bytes + lat_bytes, d_enc, enc_bytes + n_enc * 4, hipMemcpyDeviceToHost,
                                     st_voc_));
        }
        for (int b = 0; b < B && cfg_.return_latents; ++b)
            HIP_CHECK(hipMemcpyAsync(hl + (size_t)b * kMaxLatRows * kHidden,
                                     latpool_.as<float>() + (long)rows[b] * kMaxLatRows * kHidden,
                                     (size_t)voc_nl_[b] * kHidden * 4, hipMemcpyDeviceToHost, st_voc_));
        HIP_CHECK(hipEventRecord(ev_voc_done_, st_voc_));
        voc_active_ = true;
    }
    // finalize the in-flight vocoder batch if it has completed (or wait for it)
    void voc_poll(bool wait) {
        if (!voc_active_) return;
        if (wait) {
            HIP_CHECK(hipEventSynchronize(ev_voc_done_));
        } else {
            const hipError_t q = hipEventQuery(ev_voc_done_);
            if (q == hipErrorNotReady) return;
            HIP_CHECK(q);
        }
        voc_->collect(stats_);
        const int B = (int)voc_batch_.size();
        const float* hw = voc_block_->buf.as<float>();
        const float* hl = hw + (size_t)B * voc_max_samples_;
        const uint8_t* he = reinterpret_cast<const uint8_t*>(hw) + (size_t)B * voc_max_samples_ * 4 +
                            (cfg_.return_latents ? (size_t)B * kMaxLatRows * kHidden * 4 : 0);
        const int* he_len = reinterpret_cast<const int*>(he + voc_enc_rows_.size() * (size_t)voc_enc_stride_);
        // (before any sequence is handed its result: a throw here fails the whole batch like any other collect error)
        for (size_t i = 0; i < voc_enc_rows_.size(); ++i) {
            const int b = voc_enc_rows_[i];
            if (he_len[i] < kFlacHeader || he_len[i] > flac_stream_bound(out_samples(voc_nl_[b], voc_speed_[b], voc_rate_[b])))
                throw HipError("FLAC stream length out of range");
        }
        size_t ei = 0;
        for (int b = 0; b < B; ++b) {
            Seq* s = voc_batch_[b];
            const int ns = out_samples(voc_nl_[b], voc_speed_[b], voc_rate_[b]);   // delivered samples, at the sequence's rate
            s->wav = hw + (size_t)b * voc_max_samples_;
            s->n_samples = ns;
            if (cfg_.return_latents) {
                s->latents = hl + (size_t)b * kMaxLatRows * kHidden;
                s->n_latent_rows = voc_nl_[b];
            }
            stats_.samples_generated += ns;
            if (ei < voc_enc_rows_.size() && voc_enc_rows_[ei] == b) {
                s->enc = he + ei * (size_t)voc_enc_stride_;
                s->n_enc = he_len[ei];
                ++ei;
            }
            std::lock_guard<std::mutex> lk(mu_);
            s->result_block = voc_block_;
            voc_block_->refs++;
            latpool_free_.push_back(s->pool_idx);
            s->pool_idx = -1;
            spk_info_[s->spk_row].refs--;
            s->state = SeqState::DONE;
            done_.push_back(s);
            finished_total_++;
        }
        {
            std::lock_guard<std::mutex> lk(mu_);
            voc_block_->refs--;   // the batch's own hold
            voc_block_held_ = false;
        }
        voc_batch_.clear();
        voc_active_ = false;
    }

    aur_config cfg_;
    int device_;
    hipStream_t st_ = nullptr;
    hipEvent_t ev_a_ = nullptr, ev_b_ = nullptr;
    WeightTable w_;                     // what aur_load_weights has loaded; the three networks bind out of it
    std::unique_ptr<GptNet> gpt_;       // the GPT: layer tables, K/V pool, per-slot device state, forward chains, sampler, decode profile (gpt_net.h)
    int fail_at_step_ = 0;              // AUR_TEST_FAIL_STEP=n: throw inside the n-th aur_step (recovery test)
    int fail_at_voc_ = 0;               // AUR_TEST_FAIL_VOC=n: throw inside the n-th vocoder launch, after the batch left the queue
    bool voc_block_held_ = false;       // the vocoder batch holds a reference on voc_block_
    // K/V block allocator (the pool itself is GptNet's)
    long n_blocks_ = 0;
    std::vector<int> free_blocks_;
    std::vector<int> h_block_tables_;
    DevBuf spk_table_, spk_emb_, voc_cond_;
    std::map<uint64_t, int> spk_rows_;
    struct SpeakerInfo {
        int blocks[2] = {-1, -1};
        bool ready = false;
        int refs = 0;             // sequences submitted with this voice and not delivered yet
        uint64_t last_use = 0;    // LRU clock
    };
    uint64_t spk_clock_ = 0;
    std::vector<SpeakerInfo> spk_info_;
    bool share_prefix_now_ = true;    // dbg_prefill turns it off to return every prompt row
    std::mutex gpu_mu_;
    std::unique_ptr<CondNet> cond_net_;
    void* comm_ = nullptr;   // ncclComm_t
    int comm_rank_ = 0, comm_world_ = 1;
    DevBuf bcast_buf_;
    // vocoder stage
    hipStream_t st_voc_ = nullptr;
    hipEvent_t ev_lat_ = nullptr, ev_voc_done_ = nullptr;
    DevBuf latpool_;
    std::vector<int> latpool_free_;
    std::deque<Seq*> voc_queue_;
    std::vector<Seq*> voc_batch_;
    std::vector<int> voc_nl_;
    std::vector<float> voc_speed_;      // aur_seq_desc.speed of the batch's sequences
    std::vector<int> voc_rate_;         // aur_seq_desc.sample_rate of the batch's sequences
    bool voc_split_rest_ = false;       // the last pass left part of the queue behind because of the workspace bound
    int voc_max_samples_ = 0;
    std::vector<int> voc_enc_rows_;     // rows of the batch with aur_seq_desc.encoding, ascending
    long voc_enc_stride_ = 0;           // bytes per stream row of the batch's result block
    DevBuf voc_dev_wav_, voc_dev_enc_;  // an encoded pass: the delivered waveform and the streams in device memory
    FlacEncoder flac_pass_, flac_host_; // the vocoder pass's encoder and aur_encode_flac's (each with its scratch)
    DevBuf flac_x_, flac_out_;          // aur_encode_flac's device copies
    bool voc_active_ = false;
    std::vector<std::unique_ptr<PinBlock>> result_blocks_;   // pool; a block is free when refs == 0 (guarded by mu_)
    PinBlock* voc_block_ = nullptr;                          // block of the in-flight vocoder batch
    InFlight infl_;                     // decode step launched but not yet collected
    PinBuf pin_rb_[2];                  // token read-backs of the two steps that can be in flight, and their events
    StepEvents ev_step_[2];
    int rb_next_ = 0;
    bool host_trace_ = false;           // AUR_HOST_TRACE=1: host time of enqueueing a decode step vs waiting for the previous one (stderr, every 256 steps)
    long ht_launch_ns_ = 0, ht_wait_ns_ = 0, ht_n_ = 0;
    bool pipeline_ = true;              // AUR_DECODE_PIPELINE=0: wait for every read-back before launching the next step
    std::unique_ptr<HifiGan> voc_;      // the vocoder's forward graph, weights tables, workspace and profile events (voc_net.h)
    DevBuf tmp_lat_, tmp_wav_;          // vocode_host's device copies
    int profile_every_ = kProfileEvery;
    long decode_step_count_ = 0;
    // sequences
    std::mutex mu_;
    uint64_t next_id_ = 1;
    std::unordered_map<uint64_t, std::unique_ptr<Seq>> seqs_;
    std::deque<Seq*> waiting_, done_;
    std::vector<uint64_t> cancel_pending_;   // aur_cancel requests for sequences past the waiting queue (guarded by mu_)
    static constexpr int kAdmitHoldSteps = 32;   // longest hold of an admissible request by aur_config.admit_min_batch, in aur_steps
    static constexpr int kUrgentHoldSteps = 8;   // ... while an urgent sequence runs (arrivals are grouped, not kept waiting long)
    int admit_hold_steps_ = 0;
    static constexpr int kVocHoldSteps = 16;     // longest wait of a finished sequence for a fuller vocoder batch, in aur_steps (~30 ms)
    int voc_hold_steps_ = 0;
    std::vector<Seq*> slot_owner_;
    std::vector<Seq*> just_finished_;
    int64_t finished_total_ = 0;
    aur_stats stats_{};
};

}  // namespace aur

// ================================================================================================ C ABI
struct aur_engine {
    aur::Engine impl;
    aur_engine(const aur_config& c, int dev) : impl(c, dev) {}
};

aur::DbgCtx aur::dbg_ctx(const aur_engine* e) { return e->impl.dbg_ctx(); }

// Device binding.  HIP's current device belongs to the calling THREAD, and one process may hold engines on several devices driven from
// several threads (a driver thread per engine, the event loop, whichever thread drops a result lease).  Every entry point that can reach
// a HIP call therefore goes through bound(): it binds the calling thread to the engine's device before anything else runs.  The others
// are host-only -- they take mu_ and make no HIP call -- and bind nothing: aur_has_conditioning, aur_comm_info, aur_submit,
// aur_poll_finished, aur_release, aur_cancel, aur_get_stats, aur_reset_stats, aur_get_load, aur_set_profile.  aur_engine_create and
// aur_engine_destroy bind in the constructor / destructor, aur_step at the top of step_locked (inside its failure handling); the
// aur_dbg_* harness binds in its own use() (dbg_harness.hip).
template <class F>
static int bound(aur_engine* e, F&& f) {
    return guarded([&] {
        e->impl.use();
        f();
    });
}

extern "C" {

const char* aur_last_error(void) { return aur::g_last_error.c_str(); }
int aur_version(void) { return 1; }

int aur_engine_create(const aur_config* cfg, int device_id, aur_engine** out) {
    CHECK_PTR(cfg);
    CHECK_PTR(out);
    *out = nullptr;
    return guarded([&] {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
            throw aur::StateError("no HIP device visible: the MI355X path has no CPU fallback");
        AUR_REQUIRE(device_id >= 0 && device_id < n, "device_id out of range");
        *out = new aur_engine(*cfg, device_id);
    });
}
int aur_engine_destroy(aur_engine* e) {
    CHECK_PTR(e);
    return guarded([&] { delete e; });
}
int aur_load_weights(aur_engine* e, const aur_tensor_desc* t, size_t n) {
    CHECK_PTR(e);
    CHECK_PTR(t);
    return bound(e, [&] { e->impl.load(t, n); });
}
int aur_set_conditioning(aur_engine* e, uint64_t key, const float* gpt_cond, const float* spk) {
    CHECK_PTR(e);
    CHECK_PTR(gpt_cond);
    CHECK_PTR(spk);
    return bound(e, [&] { e->impl.set_conditioning(key, gpt_cond, spk, false); });
}
int aur_set_conditioning_device(aur_engine* e, uint64_t key, const float* d_gpt_cond, const float* d_spk) {
    CHECK_PTR(e);
    CHECK_PTR(d_gpt_cond);
    CHECK_PTR(d_spk);
    return bound(e, [&] { e->impl.set_conditioning(key, d_gpt_cond, d_spk, true); });
}
int aur_has_conditioning(aur_engine* e, uint64_t key, int32_t* out) {
    CHECK_PTR(e);
    CHECK_PTR(out);
    return guarded([&] { *out = e->impl.has_conditioning(key) ? 1 : 0; });
}
int aur_comm_unique_id(uint8_t* out128) {
    CHECK_PTR(out128);
    return guarded([&] { aur::Engine::comm_unique_id(out128); });
}
int aur_comm_init(aur_engine* e, const uint8_t* id128, int32_t rank, int32_t world) {
    CHECK_PTR(e);
    CHECK_PTR(id128);
    return bound(e, [&] { e->impl.comm_init(id128, rank, world); });
}
int aur_broadcast_conditioning(aur_engine* e, uint64_t key, int32_t root) {
    CHECK_PTR(e);
    return bound(e, [&] { e->impl.broadcast_conditioning(key, root); });
}
int aur_comm_info(aur_engine* e, int32_t* n_ranks, int32_t* rank) {
    CHECK_PTR(e);
    CHECK_PTR(n_ranks);
    CHECK_PTR(rank);
    return guarded([&] { e->impl.comm_info(n_ranks, rank); });
}
int aur_conditioning_checksum(aur_engine* e, uint64_t key, uint64_t* out) {
    CHECK_PTR(e);
    CHECK_PTR(out);
    return bound(e, [&] { *out = e->impl.conditioning_checksum(key); });
}
int aur_compute_conditioning(aur_engine* e, const float* const* pcm, const int32_t* n_samples, int32_t n_refs, const aur_cond_params* p,
                             float* out_gpt_cond, float* out_spk_emb) {
    CHECK_PTR(e);
    CHECK_PTR(pcm);
    CHECK_PTR(n_samples);
    CHECK_PTR(p);
    CHECK_PTR(out_gpt_cond);
    CHECK_PTR(out_spk_emb);
    return bound(e, [&] { e->impl.compute_conditioning(pcm, n_samples, n_refs, *p, out_gpt_cond, out_spk_emb); });
}
int64_t aur_flac_bound(int64_t n_samples) { return n_samples < 0 ? 0 : aur::flac_stream_bound(n_samples); }
int aur_encode_flac(aur_engine* e, const float* const* x, const int32_t* n, const int32_t* rate, int32_t B, uint8_t* out, int64_t out_stride,
                    int64_t* out_lens) {
    CHECK_PTR(e);
    CHECK_PTR(x);
    CHECK_PTR(n);
    CHECK_PTR(rate);
    CHECK_PTR(out);
    CHECK_PTR(out_lens);
    return bound(e, [&] { e->impl.encode_flac(x, n, rate, B, out, out_stride, out_lens); });
}
int aur_submit(aur_engine* e, const aur_seq_desc* seq, uint64_t* seq_id) {
    CHECK_PTR(e);
    CHECK_PTR(seq);
    CHECK_PTR(seq_id);
    return guarded([&] { *seq_id = e->impl.submit(*seq); });
}
int aur_step(aur_engine* e, int32_t* n_live, int32_t* n_finished_total) {
    CHECK_PTR(e);
    // (binds first thing inside, in step_locked, where a failure fails what was in flight)
    return guarded([&] { e->impl.step(n_live, n_finished_total); });
}
int aur_poll_finished(aur_engine* e, aur_result* out, size_t cap, size_t* n) {
    CHECK_PTR(e);
    CHECK_PTR(out);
    CHECK_PTR(n);
    return guarded([&] { *n = e->impl.poll(out, cap); });
}
int aur_release(aur_engine* e, uint64_t seq_id) {
    CHECK_PTR(e);
    return guarded([&] { e->impl.release(seq_id); });
}
int aur_cancel(aur_engine* e, uint64_t seq_id) {
    CHECK_PTR(e);
    return guarded([&] { e->impl.cancel(seq_id); });
}
int aur_vocode(aur_engine* e, const float* latents, const int32_t* n_lat, int32_t B, int32_t t_max,
               uint64_t speaker_key, float* wav_out, int64_t wav_stride, int32_t* n_samples_out) {
    return aur_vocode_speed(e, latents, n_lat, nullptr, B, t_max, speaker_key, wav_out, wav_stride, n_samples_out);
}
int aur_vocode_speed(aur_engine* e, const float* latents, const int32_t* n_lat, const float* speed, int32_t B, int32_t t_max,
                     uint64_t speaker_key, float* wav_out, int64_t wav_stride, int32_t* n_samples_out) {
    return aur_vocode_rate(e, latents, n_lat, speed, nullptr, B, t_max, speaker_key, wav_out, wav_stride, n_samples_out);
}
int aur_vocode_rate(aur_engine* e, const float* latents, const int32_t* n_lat, const float* speed, const int32_t* sample_rate, int32_t B,
                    int32_t t_max, uint64_t speaker_key, float* wav_out, int64_t wav_stride, int32_t* n_samples_out) {
    CHECK_PTR(e);
    CHECK_PTR(latents);
    CHECK_PTR(n_lat);
    CHECK_PTR(wav_out);
    return bound(e, [&] { e->impl.vocode_host(latents, n_lat, speed, sample_rate, B, t_max, speaker_key, wav_out, wav_stride, n_samples_out); });
}
int aur_sync(aur_engine* e) {
    CHECK_PTR(e);
    return bound(e, [&] { e->impl.sync(); });
}
int aur_get_stats(aur_engine* e, aur_stats* out) {
    CHECK_PTR(e);
    CHECK_PTR(out);
    return guarded([&] { *out = e->impl.stats(); });
}
int aur_get_load(aur_engine* e, aur_load* out) {
    CHECK_PTR(e);
    CHECK_PTR(out);
    return guarded([&] { *out = e->impl.load_now(); });
}
int aur_reset_stats(aur_engine* e) {
    CHECK_PTR(e);
    return guarded([&] { e->impl.reset_stats(); });
}
int aur_set_profile(aur_engine* e, int32_t every) {
    CHECK_PTR(e);
    return guarded([&] { e->impl.set_profile(every); });
}
int aur_dbg_prefill(aur_engine* e, const int32_t* text_ids, int32_t n_text, uint64_t speaker_key, float repetition_penalty,
                    float* lnf_rows_out, float* logits_out) {
    CHECK_PTR(e);
    CHECK_PTR(text_ids);
    return bound(e, [&] { e->impl.dbg_prefill(text_ids, n_text, speaker_key, repetition_penalty, lnf_rows_out, logits_out); });
}
int aur_dbg_sample(aur_engine* e, const float* logits, int32_t B, float temperature, float top_p, int32_t top_k,
                   float repetition_penalty, const uint8_t* seen, uint32_t seed, int32_t step, int32_t* tokens_out) {
    CHECK_PTR(e);
    CHECK_PTR(logits);
    CHECK_PTR(tokens_out);
    return bound(e, [&] { e->impl.dbg_sample(logits, B, temperature, top_p, top_k, repetition_penalty, seen, seed, step, tokens_out); });
}

}  // extern "C"
