// The XTTSv2 GPT on the GPU (kernels: gpt_kernels.h; host rules shared with the kernel test harness: gpt_host.h): the layer tables bound
// out of the loaded weights, the paged K/V pool, the per-slot state of the continuous batcher, the row workspace, the prompt-row and
// decode forward chains, the sampling tail and the decode profile.  GptNet launches on the GPT stream and knows nothing about a
// sequence: which slot, block or row belongs to whom, and when to wait for a read-back, is the engine's business (engine.hip).
#pragma once
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/auralis_amd.h"
#include "gpt_host.h"

namespace aur {

constexpr int kMaxLatRows = 608;
constexpr int kMelVocab = 1026;
constexpr int kHeadPad = 1088;         // mel_head columns padded to a multiple of 64
constexpr int kStartToken = 1024, kStopToken = 1025;
constexpr int kProj2Slabs = 4;   // split-K slabs of the prompt-row MLP projection (forward_rows)

struct GptLayout {
    int n_layer, max_seqs;
    long n_blocks;     // K/V blocks of a layer's pool
    int prec;          // GemmRowsArgs.prec of every decode GEMM (aur_config.gemm_f32_exact)
    bool f16;          // aur_config.gpt_fp16: the four per-layer decode GEMMs run with prec 2 on fp16 copies
    bool presplit;     // prompt-row GEMMs read their weights as the three bf16 planes packed at load time (launch_pack_wsplit)
    bool kv_half;      // aur_config.kv_fp16
    bool gelu_erf;
    bool sampler_full_sort;   // AUR_SAMPLER_FULL_SORT=1: disable the sampler's top-k fast path (A/B)
};
// what a decode step records on the stream: around its kernels (timing) and behind its token read-back
struct StepEvents { hipEvent_t start = nullptr, end = nullptr, readback = nullptr; };

class GptNet {
public:
    GptNet(WeightTable& w, hipStream_t st, GptLayout lay) : w_(w), st_(st), lay_(lay) {
        const int S = lay_.max_seqs;
        kv_layer_stride_ = lay_.n_blocks * kKvBlockElems;
        kv_.ensure((size_t)lay_.n_layer * kv_layer_stride_ * (lay_.kv_half ? 2 : 4));
        for (DevBuf* b : {&slot_tok_, &slot_pos_, &slot_kvpos_, &slot_ngen_, &slot_finished_, &temperature_, &top_p_, &top_k_, &rep_,
                          &max_tokens_, &ignore_stop_, &seed_})
            b->zeros((size_t)S * sizeof(int), st_);
        block_tables_.zeros((size_t)(S + 1) * kMaxBlocks * sizeof(int), st_);   // row S: pseudo-slot used to prefill a speaker prefix
        seen_.zeros((size_t)S * kSeenStride, st_);
        latents_.ensure((size_t)S * kMaxLatRows * kHidden * sizeof(float));
        zero_bias_.zeros(4096 * sizeof(float), st_);
        ksp_buf_.ensure((size_t)kGemmKspTiles * 16 * 256 * sizeof(float));   // K-split partial tiles of the small-M mlp projection
        ksp_cnt_.zeros((size_t)kGemmKspTiles * sizeof(unsigned), st_);
    }
    ~GptNet() { for (auto& e : gemm_events_) (void)hipEventDestroy(e.a), (void)hipEventDestroy(e.b); }   // (not copyable: the buffers are not)
    const GptLayout& layout() const { return lay_; }
    float* ksp_buf() const { return ksp_buf_.as<float>(); }
    unsigned* ksp_cnt() const { return ksp_cnt_.as<unsigned>(); }
    bool text_ok(int id, int pos) const { return id >= 0 && id < text_vocab_ && pos < text_positions_; }   // text_emb / text_pos have the row

    // ------------------------------------------------------------------ weights
    // The four linears of a GPT layer, in the order the decode chain runs them: tensor name (.w / .b) under the layer's prefix, the
    // LayerNorm in front of it (folded into its decode operand) or none, and its shape.
    struct LinearSpec { const char *name, *ln; int K, N; };
    static constexpr LinearSpec kLinears[4] = {{"attn.c_attn", "ln_1", kHidden, 3 * kHidden}, {"attn.c_proj", nullptr, kHidden, kHidden},
                                               {"mlp.c_fc", "ln_2", kHidden, 4 * kHidden}, {"mlp.c_proj", nullptr, 4 * kHidden, kHidden}};
    static std::string layer_prefix(int i) { return "gpt.h." + std::to_string(i) + "."; }
    // aur_config.gpt_fp16: once every per-layer matrix and its LayerNorm gain are loaded, a matrix the rule rejects (not finite, or
    // beyond the fp16 range after folding) fails the load that completed the set, before anything is converted
    void check_f16() {
        auto has = [&](const std::string& n, int64_t numel) { return w_.has(n) && w_.at(n).numel == numel; };
        for (int i = 0; i < lay_.n_layer; ++i)
            for (const LinearSpec& m : kLinears)   // not complete yet (or misshapen: bind reports that)
                if (!has(layer_prefix(i) + m.name + ".w", (int64_t)m.K * m.N) || (m.ln && !has(layer_prefix(i) + m.ln + ".w", m.K))) return;
        DevBuf dbad, scratch;
        dbad.zeros(sizeof(int), st_);
        scratch.ensure((size_t)4 * kHidden * kHidden * 2);
        for (int i = 0; i < lay_.n_layer; ++i)
            for (const LinearSpec& m : kLinears)
                launch_pack_wt16_f16(w_.W(layer_prefix(i) + m.name + ".w"), m.N, m.ln ? w_.W(layer_prefix(i) + m.ln + ".w") : nullptr, nullptr,
                                     scratch.p, dbad.as<int>(), m.K, m.N, st_);
        int bad = 0;
        HIP_CHECK(hipMemcpyAsync(&bad, dbad.p, sizeof(int), hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipStreamSynchronize(st_));
        if (bad) throw InvalidArgument("gpt_fp16: a per-layer GPT linear is not finite or leaves the fp16 range after LayerNorm folding");
    }
    // the layer tables and packed operands out of the loaded weights (a missing or misshapen one throws); unbind() after a load, the
    // next step binds again
    void unbind() { bound_ = false; }
    void bind() {
        if (bound_) return;
        layers_.clear();
        packed_.clear();
        const int H = kHidden;
        // aur_config.gpt_fp16: fp16 decode operands by the rule of launch_pack_wt16_f16; the matrices themselves are replaced by W'' in
        // place, so the prompt-row GEMMs (their pre-split planes are taken afterwards) and second_pass run on the same effective
        // weights.  Converting W'' again gives the same bits.
        DevBuf dbad;   // (never read: check_f16 has checked before anything is converted)
        if (lay_.f16) {
            check_f16();
            dbad.ensure(sizeof(int));
        }
        for (int i = 0; i < lay_.n_layer; ++i) {
            const std::string p = layer_prefix(i);
            layers_.emplace_back();
            for (int k = 0; k < 4; ++k) {
                const LinearSpec& m = kLinears[k];
                const std::string wn = p + m.name + ".w", gn = m.ln ? p + m.ln + ".w" : "";
                Linear& L = layers_.back().lin[k];
                L.K = m.K; L.N = m.N;
                L.w = w_.W(wn, (int64_t)m.K * m.N); L.b = w_.W(p + m.name + ".b", m.N);
                L.lnw = m.ln ? w_.W(gn, m.K) : nullptr; L.lnb = m.ln ? w_.W(p + m.ln + ".b", m.K) : nullptr;
                if (lay_.f16 && m.ln && w_.at(wn).f16_eff && !w_.at(gn).f16_eff)
                    throw StateError("gpt_fp16: " + gn + " was loaded again after " + wn + " was converted with the previous "
                                     "one; load " + wn + " again as well");
                L.op = prepare_decode_operand(lay_.f16 ? 2 : lay_.prec, L.w, m.N, L.lnw, L.lnb, L.b, m.K, m.N, w_.at(wn).d(), dbad.as<int>(),
                                              fold_scratch_, packed_, st_);
                if (lay_.f16) w_.at(wn).f16_eff = true;
                if (lay_.f16 && m.ln) w_.at(gn).f16_eff = true;
                L.split = nullptr;
                if (lay_.prec == 1 && lay_.presplit) {
                    packed_.emplace_back(new DevBuf());
                    packed_.back()->ensure((size_t)3 * m.K * m.N * 2);
                    launch_pack_wsplit(L.w, m.N, packed_.back()->p, m.K, m.N, st_);
                    L.split = packed_.back()->p;
                }
            }
        }
        wte_ = w_.W("gpt.wte", (int64_t)kMelVocab * H);
        wpe_ = w_.W("gpt.wpe", (int64_t)kMaxLatRows * H);
        lnfw_ = w_.W("gpt.ln_f.w", H); lnfb_ = w_.W("gpt.ln_f.b", H);
        fnw_ = w_.W("final_norm.w", H); fnb_ = w_.W("final_norm.b", H);
        headT_ = w_.W("mel_head.wT", (int64_t)H * kHeadPad);
        headb_ = w_.W("mel_head.b", kHeadPad);
        thead_ = prepare_decode_operand(lay_.prec, headT_, kHeadPad, nullptr, nullptr, nullptr, H, kHeadPad, nullptr, nullptr, fold_scratch_,
                                        packed_, st_).Wt;
        HIP_CHECK(hipStreamSynchronize(st_));
        fold_scratch_.release();
        text_emb_ = w_.W("text_emb");
        text_pos_ = w_.W("text_pos");
        text_vocab_ = (int)(w_.at("text_emb").numel / H);
        text_positions_ = (int)(w_.at("text_pos").numel / H);
        bound_ = true;
    }

    // ------------------------------------------------------------------ per-slot state
    void init_slots(const std::vector<SlotInit>& init) {
        i_init_.ensure(init.size() * sizeof(SlotInit));
        HIP_CHECK(hipMemcpyAsync(i_init_.p, init.data(), init.size() * sizeof(SlotInit), hipMemcpyHostToDevice, st_));
        launch_init_slots(i_init_.as<SlotInit>(), (int)init.size(), slot_tok_.as<int>(), slot_pos_.as<int>(), slot_kvpos_.as<int>(),
                          slot_ngen_.as<int>(), slot_finished_.as<int>(), temperature_.as<float>(), top_p_.as<float>(), top_k_.as<int>(),
                          rep_.as<float>(), max_tokens_.as<int>(), ignore_stop_.as<int>(), seed_.as<unsigned>(), seen_.as<unsigned char>(),
                          kStartToken, st_);
    }
    void upload_block_tables(const std::vector<int>& h) { HIP_CHECK(hipMemcpyAsync(block_tables_.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, st_)); }   // [max_seqs + 1][kMaxBlocks]
    const float* stash(int slot) const { return latents_.as<float>() + (long)slot * kMaxLatRows * kHidden; }   // row n: the latent of the slot's n-th generated token
    // max_tokens = 1 on the device: the sampler flags the slot finished with the next token it draws
    void limit_tokens(int slot) { HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(max_tokens_.as<int>() + slot), 1, 1, st_)); }
    // after a failed step (the stream has drained)
    void reset_after_failure() {
        (void)hipMemsetAsync(ksp_cnt_.p, 0, (size_t)kGemmKspTiles * sizeof(unsigned), st_);   // an aborted K-split launch may have left tickets behind
        last_active_.clear();
        n_gemm_events_ = 0;
    }

    // ------------------------------------------------------------------ prompt rows
    // Prefill, speaker prefix, literal second pass: embeds the rows desc[m] (launch_embed_prompt; spk_table: the kind-0 rows' source)
    // at (row_slot[m], row_pos[m]) and runs them through the blocks.  Leaves the ln_f rows in the workspace (sample_prompt,
    // double_norm_rows, capture_prompt_rows read them).
    void prompt_rows(const std::vector<int4>& desc, const std::vector<int>& row_slot, const std::vector<int>& row_pos, const float* spk_table) {
        const int M = (int)row_slot.size();
        last_active_.clear();   // the prompt rows reuse the index buffers of the decode chain
        ensure_rows(M);
        HIP_CHECK(hipMemcpyAsync(i_desc_.p, desc.data(), (size_t)M * sizeof(int4), hipMemcpyHostToDevice, st_));
        HIP_CHECK(hipMemcpyAsync(i_row_slot_.p, row_slot.data(), (size_t)M * 4, hipMemcpyHostToDevice, st_));
        HIP_CHECK(hipMemcpyAsync(i_row_pos_.p, row_pos.data(), (size_t)M * 4, hipMemcpyHostToDevice, st_));
        launch_embed_prompt(i_desc_.as<int4>(), spk_table, text_emb_, text_pos_, wte_, wpe_, h_.as<float>(), M, st_);
        forward_rows(M, upload_qblocks(row_slot, row_pos));
    }
    // final_norm -> latent stash -> mel_head GEMM -> fused sampler on rows sample_row of the prompt rows, for slots sample_slot, whose
    // K/V position becomes next_kvpos.  Returns the pinned tokens (token | finished bit), valid once the stream has been synchronised.
    const int* sample_prompt(const std::vector<int>& sample_row, const std::vector<int>& sample_slot, const std::vector<int>& next_kvpos) {
        const int Ms = (int)sample_slot.size();
        pin_.ensure(((size_t)lay_.max_seqs * 2 + 16) * sizeof(int));
        sample_upload(sample_slot);
        HIP_CHECK(hipMemcpyAsync(i_sample_row_.p, sample_row.data(), (size_t)Ms * 4, hipMemcpyHostToDevice, st_));
        HIP_CHECK(hipMemcpyAsync(i_next_kvpos_.p, next_kvpos.data(), (size_t)Ms * 4, hipMemcpyHostToDevice, st_));
        launch_final_norm(xn_.as<float>(), i_sample_row_.as<int>(), i_sample_slot_.as<int>(), fnw_, fnb_, ybuf_.as<float>(),
                          latents_.as<float>(), (long)kMaxLatRows * kHidden, slot_ngen_.as<int>(), kMaxLatRows, Ms, 1e-5f, st_);
        launch_gemm_tile(ybuf_.as<float>(), kHidden, headT_, P2_.as<float>(), Ms, kHeadPad, kHidden, st_, nullptr, lay_.prec);
        launch_sampler(sampler_args(P2_.as<float>(), Ms, kHeadPad, headb_, i_next_kvpos_.as<int>()), st_);
        HIP_CHECK(hipMemcpyAsync(pin_.p, i_out_tok_.p, (size_t)Ms * 4, hipMemcpyDeviceToHost, st_));   // token | finished bit
        return pin_.as<int>();
    }
    // literal second pass: dst[0 .. n) = final_norm(final_norm(.)) of the ln_f rows [first_row, first_row + n)
    void double_norm_rows(int first_row, float* dst, int n) { launch_double_norm_rows(xn_.as<float>() + (long)first_row * kHidden, dst, n, fnw_, fnb_, 1e-5f, st_); }

    // ------------------------------------------------------------------ decode
    // One decode step for the live slots `active` (row order): embed -> 30 x (QKV GEMM, attention, proj, FC, proj2) -> final norms ->
    // head GEMM -> sampler, 154 launches that depend only on device-resident state (hipGraph replay of the chain was measured within
    // noise in round 2: the launches are already back to back), then the token read-back into `pin` ([rows]: token | finished bit,
    // -1 for a ghost row).  Waits for nothing unless the set of slots changed (index upload).  profiled: the replay batches follow
    // the read-back (collect_profile); kv_tokens: the sum of the rows' context lengths, for their accounting.
    void decode_step(const std::vector<int>& active, bool profiled, double kv_tokens, int* pin, const StepEvents& ev) {
        const int M = (int)active.size();
        if (active != last_active_) {
            ensure_rows(M);
            HIP_CHECK(hipMemcpyAsync(i_row_slot_.p, active.data(), (size_t)M * 4, hipMemcpyHostToDevice, st_));
            sample_upload(active);
            HIP_CHECK(hipStreamSynchronize(st_));   // pageable sources: the vectors may change before the copies run
        }
        HIP_CHECK(hipEventRecord(ev.start, st_));
        launch_embed_decode(i_row_slot_.as<int>(), slot_tok_.as<int>(), slot_pos_.as<int>(), wte_, wpe_, h_.as<float>(), M, st_,
                            rows_cap_ / 16, stats_.as<float2>(), row_meta_.as<int>(), slot_kvpos_.as<int>(),
                            block_tables_.as<int>(), kMaxBlocks);
        forward_decode(M);
        sample_kernels_decode(M);
        HIP_CHECK(hipEventRecord(ev.end, st_));
        // (the sampler writing the tokens straight into the pinned block instead of this 256-byte copy: 621.3 vs 621.8 ms per bench
        // step, 1.193 vs 1.194 ms per single-utterance decode step -- the copy is not on the critical path of the pipelined loop)
        HIP_CHECK(hipMemcpyAsync(pin, i_out_tok_.p, (size_t)M * 4, hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipEventRecord(ev.readback, st_));
        if (profiled) profile_replay(M, kv_tokens);   // behind the read-back: the step's tokens do not wait for it
        last_active_ = active;
    }
    // books the replay batches of the profiled steps since the last call
    void collect_profile(aur_stats& stats) {
        // the replay batches sit behind the step's token read-back on the stream (and, with the pipelined decode, the next step's
        // batches may already be queued behind them): wait for the last one recorded
        if (n_gemm_events_) HIP_CHECK(hipEventSynchronize(gemm_events_[n_gemm_events_ - 1].b));
        const float ovh = n_gemm_events_ ? event_pair_overhead_ms() : 0.f;
        if (n_gemm_events_) stats.event_pair_overhead_ms = ovh;
        for (size_t i = 0; i < n_gemm_events_; ++i) {
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, gemm_events_[i].a, gemm_events_[i].b));
            const ProfEvent& ev = gemm_events_[i];
            if (ev.kind == 5) {
                stats.attn_ms += ms; stats.attn_bytes += ev.bytes; stats.attn_launches += ev.count;
                continue;
            }
            if (ev.kind >= 0 && ev.kind < 5) {
                stats.gemm_kind_ms[ev.kind] += ms; stats.gemm_kind_bytes[ev.kind] += ev.bytes;
                stats.gemm_kind_flops[ev.kind] += ev.flops; stats.gemm_kind_launches[ev.kind] += ev.count;
            }
            stats.gemm_ms_raw += ms;
            stats.gemm_ms += std::max(0.f, ms - ovh);   // one pair per batch of ev.count launches
            stats.gemm_flops += ev.flops; stats.gemm_bytes += ev.bytes; stats.gemm_launches += ev.count;
        }
        n_gemm_events_ = 0;
    }

    // ------------------------------------------------------------------ debug entry points (aur_dbg_prefill, aur_dbg_sample)
    // capture on: the sampler keeps its penalised logits, capture_prompt_rows the ln_f rows
    void set_capture(bool on) { if (on) dbg_logits_.ensure((size_t)kMelVocab * 4); dbg_capture_ = on; }
    void capture_prompt_rows(int M) {
        if (!dbg_capture_) return;
        dbg_lnf_.ensure((size_t)M * kHidden * 4);
        HIP_CHECK(hipMemcpyAsync(dbg_lnf_.p, xn_.p, (size_t)M * kHidden * 4, hipMemcpyDeviceToDevice, st_));
    }
    const void* dbg_lnf() const { return dbg_lnf_.p; }
    const void* dbg_logits() const { return dbg_logits_.p; }
    void dbg_sample(const float* logits, int B, float temperature, float top_p, int top_k, float rep, const uint8_t* seen, uint32_t seed,
                    int step_idx, int* tokens_out) {
        std::vector<SlotInit> init(B);
        std::vector<int> slots(B);
        for (int b = 0; b < B; ++b) {
            init[b] = SlotInit{b, temperature, top_p, top_k, rep, 1 << 30, 1, seed + (unsigned)b, step_idx};
            slots[b] = b;
        }
        init_slots(init);
        if (seen) {
            for (int b = 0; b < B; ++b)
                HIP_CHECK(hipMemcpyAsync(seen_.as<unsigned char>() + (long)b * kSeenStride, seen + (long)b * kMelVocab,
                                         kMelVocab, hipMemcpyHostToDevice, st_));
        } else {
            HIP_CHECK(hipMemsetAsync(seen_.p, 0, (size_t)B * kSeenStride, st_));
        }
        DevBuf dl;
        dl.ensure((size_t)B * kMelVocab * 4);
        HIP_CHECK(hipMemcpyAsync(dl.p, logits, (size_t)B * kMelVocab * 4, hipMemcpyHostToDevice, st_));
        i_sample_slot_.ensure(B * 4);
        i_out_tok_.ensure(B * 4);
        HIP_CHECK(hipMemcpyAsync(i_sample_slot_.p, slots.data(), B * 4, hipMemcpyHostToDevice, st_));
        launch_sampler(sampler_args(dl.as<float>(), B, kMelVocab, zero_bias_.as<float>(), nullptr), st_);
        HIP_CHECK(hipStreamSynchronize(st_));
        HIP_CHECK(hipMemcpy(tokens_out, i_out_tok_.p, B * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b)
            if (tokens_out[b] >= 0) tokens_out[b] &= ~kTokFinishedBit;
    }

private:
    struct Linear {   // one entry of kLinears in one layer
        const float *w, *b;       // the loaded [K][N] matrix (aur_config.gpt_fp16: W'' once bind has run) and bias
        const float *lnw, *lnb;   // gain and shift of the LayerNorm in front of it, or null
        int K, N;
        DecodeOperand op;    // decode-regime GEMM (gemm_rows_kernel): packed weights, c1, effective bias (prepare_decode_operand)
        const void* split;   // prefill-regime GEMM: the three bf16 planes of launch_pack_wsplit (only the split arithmetic uses them)
    };
    enum { kQkv, kProj, kFc, kProj2 };   // indices into kLinears / LayerW::lin, = the GEMM kind of the decode profile
    struct LayerW { Linear lin[4]; };
    void* kv_layer(int l) const { return (char*)kv_.p + (size_t)l * kv_layer_stride_ * (lay_.kv_half ? 2 : 4); }
    void ensure_rows(int M) {
        if (M <= rows_cap_) return;
        last_active_.clear();   // buffers move: the row indices have to be uploaded again
        const int cap = (std::max(M, 64) + 63) / 64 * 64;   // whole 64-row groups: the decode chain keeps its rows packed (pk_off)
        for (DevBuf* b : {&ybuf_, &h_, &xn_, &qbuf_, &att_}) b->ensure((size_t)cap * kHidden * 4);
        stats_.ensure((size_t)cap * 64 * sizeof(float2));
        row_meta_.ensure((size_t)cap * kRowMetaStride * sizeof(int));
        // embed_decode writes entries [0, kRowMetaBt + max_blocks) of the live rows only; the look-ahead entries behind them and the rows
        // >= M of the last tile are READ (their values discarded by selects): defined zeros, not whatever the allocation held
        HIP_CHECK(hipMemsetAsync(row_meta_.p, 0, (size_t)cap * kRowMetaStride * sizeof(int), st_));
        act_.ensure((size_t)cap * 4 * kHidden * 4);
        P_.ensure((size_t)cap * 4096 * 4);   // one GEMM output slab (prefill)
        for (DevBuf* b : {&i_row_slot_, &i_row_pos_}) b->ensure((size_t)cap * 4);
        i_desc_.ensure((size_t)cap * sizeof(int4));
        rows_cap_ = cap;
    }
    // uploads the query blocks of a batch of prompt rows (prompt_qblocks) for forward_rows and returns their number
    int upload_qblocks(const std::vector<int>& row_slot, const std::vector<int>& row_pos) {
        h_qblk_ = prompt_qblocks(row_slot, row_pos);
        i_qblk_.ensure(h_qblk_.size() * sizeof(int2));
        HIP_CHECK(hipMemcpyAsync(i_qblk_.p, h_qblk_.data(), h_qblk_.size() * sizeof(int2), hipMemcpyHostToDevice, st_));
        return (int)h_qblk_.size();
    }
    // Prompt rows (prefill, speaker prefix, literal second pass): explicit row positions, LDS-tiled GEMMs in the configured arithmetic
    // (lay_.prec: bf16 x 3 split by default, exact-f32 MFMA under aur_config.gemm_f32_exact; k ascending for every M => a prompt's rows do not depend on what else was admitted), separate LayerNorm launches.
    void forward_rows(int M, int n_qblk) {
        float *h = h_.as<float>(), *xn = xn_.as<float>(), *P = P_.as<float>();
        const int* bt = block_tables_.as<int>();
        const int *d_row_slot = i_row_slot_.as<int>(), *d_row_pos = i_row_pos_.as<int>();
        const bool kv_half = lay_.kv_half;
        // P = X @ (one linear of the layer), or what `epi` makes of it
        auto gemm = [&](const float* X, const Linear& L, const GemmGelu* epi, int slabs) {
            launch_gemm_tile(X, L.K, L.w, P, M, L.N, L.K, st_, epi, lay_.prec, slabs, L.split);
        };
        launch_rows_ln(nullptr, 0, nullptr, h, layers_[0].lin[kQkv].lnw, layers_[0].lin[kQkv].lnb, xn, M, 1e-5f, st_);
        for (int l = 0; l < lay_.n_layer; ++l) {
            const Linear* L = layers_[l].lin;
            void* kvl = kv_layer(l);
            if (lay_.prec == 1) {   // bias, q rows and the K / V page writes in the GEMM's epilogue (27.50 vs 27.62 ms per prefill)
                GemmGelu qe{L[kQkv].b, nullptr, 0};
                qe.qbuf = qbuf_.as<float>(); qe.kv_layer = kvl; qe.row_slot = d_row_slot; qe.row_pos = d_row_pos; qe.block_tables = bt;
                qe.max_blocks = kMaxBlocks; qe.kv_half = kv_half ? 1 : 0;
                gemm(xn, L[kQkv], &qe, 1);
            } else {
                gemm(xn, L[kQkv], nullptr, 1);
                launch_qkv_epilogue(P, 1, L[kQkv].b, qbuf_.as<float>(), kvl, d_row_slot, d_row_pos, slot_kvpos_.as<int>(), bt, kMaxBlocks, M, st_, kv_half);
            }
            launch_prompt_attention(qbuf_.as<float>(), kvl, i_qblk_.as<int2>(), n_qblk, d_row_slot, d_row_pos, bt, kMaxBlocks, att_.as<float>(), st_, kv_half);
            // (two K-slabs for this GEMM -- 576 workgroups instead of 288 on 256 CUs: 27.55-27.68 vs 27.82 ms per prefill, four slabs
            // 27.83-27.93: not worth another slab sum)
            gemm(att_.as<float>(), L[kProj], nullptr, 1);
            launch_rows_ln(P, 1, L[kProj].b, h, L[kFc].lnw, L[kFc].lnb, xn, M, 1e-5f, st_);
            const GemmGelu ge{L[kFc].b, act_.as<float>(), lay_.gelu_erf ? 1 : 0};
            gemm(xn, L[kFc], &ge, 1);
            // K = 4096 against N = 1024: four K-slabs (4x the workgroups of a GEMM that otherwise fills one round of CUs with
            // 256 dependent k-steps); rows_ln sums them in a fixed order
            gemm(act_.as<float>(), L[kProj2], nullptr, kProj2Slabs);
            const bool last = (l + 1 == lay_.n_layer);
            launch_rows_ln(P, kProj2Slabs, L[kProj2].b, h, last ? lnfw_ : layers_[l + 1].lin[kQkv].lnw, last ? lnfb_ : layers_[l + 1].lin[kQkv].lnb,
                           xn, M, 1e-5f, st_);
        }
    }
    // the four GEMM launches of layer l exactly as forward_decode issues them; `redirect` sends every output to the profile scratch
    GemmRowsArgs decode_gemm_args(int l, int kind, int M, bool redirect) {
        const Linear& L = layers_[l].lin[kind];
        const int mtt = rows_cap_ / 16;   // h, att, act are packed rows (pk_off) with this many 16-row tiles
        float* h = h_.as<float>();
        GemmRowsArgs a{};
        a.M = M; a.prec = lay_.f16 ? 2 : lay_.prec; a.xmt = mtt;
        a.ksp_buf = ksp_buf_.as<float>(); a.ksp_cnt = ksp_cnt_.as<unsigned>();
        a.Wt = L.op.Wt; a.N = L.N; a.K = L.K; a.bias = L.op.bias; a.ln_c1 = L.op.c1;
        if (kind == kQkv) {
            a.eps = 1e-5f; a.X = h; a.stats_in = stats_.as<float2>(); a.out = redirect ? prof_q_.as<float>() : qbuf_.as<float>(); a.ldo = kHidden;
            a.kv_layer = redirect ? prof_kv_.p : kv_layer(l); a.kv_half = lay_.kv_half ? 1 : 0; a.row_meta = row_meta_.as<int>();
        } else if (kind == kProj) {
            a.X = att_.as<float>();
            a.out = redirect ? prof_h_.as<float>() : h; a.omt = mtt; a.stats_out = redirect ? prof_stats_.as<float2>() : stats_.as<float2>();
        } else if (kind == kFc) {
            a.eps = 1e-5f; a.X = h; a.stats_in = stats_.as<float2>(); a.out = redirect ? prof_act_.as<float>() : act_.as<float>(); a.omt = mtt;
            a.gelu_erf = lay_.gelu_erf ? 1 : 0;
        } else {
            a.X = act_.as<float>();
            a.out = redirect ? prof_h_.as<float>() : h; a.omt = mtt;
            // (ln_f computes its own statistics in final_rows_kernel)
            if (l + 1 < lay_.n_layer) a.stats_out = redirect ? prof_stats_.as<float2>() : stats_.as<float2>();
        }
        return a;
    }
    static constexpr bool kKindLn[4] = {true, false, true, false};   // launch_gemm_rows' ln and epi of the four kinds
    static constexpr GemmRowsEpi kKindEpi[4] = {kEpiQkv, kEpiResidual, kEpiBiasGelu, kEpiResidual};
    // One decode step through the blocks: 5 launches per layer (QKV GEMM with LN1 folded and KV page write, attention,
    // proj GEMM + residual, FC GEMM with LN2 folded + gelu, proj2 GEMM + residual), no split-K slabs in HBM.  Leaves the
    // residual stream in h_ (ln_f is applied by final_rows_kernel).
    void forward_decode(int M) {
        const int mtt = rows_cap_ / 16;
        for (int l = 0; l < lay_.n_layer; ++l)
            for (int kind = 0; kind < 4; ++kind) {
                launch_gemm_rows(decode_gemm_args(l, kind, M, false), kKindLn[kind], kKindEpi[kind], st_);
                if (kind == 0)
                    launch_paged_attention(qbuf_.as<float>(), kv_layer(l), row_meta_.as<int>(), kMaxBlocks, att_.as<float>(), M, st_, mtt, lay_.kv_half);
            }
    }
    GemmRowsArgs head_gemm_args(int Ms, bool redirect) {
        GemmRowsArgs a{};
        a.M = Ms; a.prec = lay_.prec; a.X = ybuf_.as<float>(); a.xmt = rows_cap_ / 16; a.Wt = thead_; a.N = kHeadPad; a.K = kHidden; a.bias = headb_;
        a.out = redirect ? prof_act_.as<float>() : P2_.as<float>(); a.ldo = kHeadPad;
        return a;
    }
    SamplerArgs sampler_args(const float* P, int Ms, int Npad, const float* bias, const int* next_kvpos) {
        SamplerArgs a{};
        a.P = P; a.S = 1; a.Ms = Ms; a.Npad = Npad; a.V = kMelVocab; a.bias = bias;
        a.sample_slot = i_sample_slot_.as<int>();
        a.next_kvpos = next_kvpos;
        a.seen = seen_.as<unsigned char>();
        a.slot_tok = slot_tok_.as<int>(); a.slot_pos = slot_pos_.as<int>(); a.slot_kvpos = slot_kvpos_.as<int>();
        a.slot_ngen = slot_ngen_.as<int>(); a.slot_finished = slot_finished_.as<int>();
        a.temperature = temperature_.as<float>(); a.top_p = top_p_.as<float>(); a.top_k = top_k_.as<int>();
        a.rep_penalty = rep_.as<float>(); a.max_tokens = max_tokens_.as<int>(); a.ignore_stop = ignore_stop_.as<int>();
        a.seed = seed_.as<unsigned>();
        a.out_tok = i_out_tok_.as<int>();
        a.dbg_logits = dbg_capture_ ? dbg_logits_.as<float>() : nullptr;
        a.stop_token = kStopToken;
        a.force_full_sort = lay_.sampler_full_sort ? 1 : 0;
        return a;
    }
    // the sampling tail's buffers for the rows of `sample_slot`, and their slots on the device (the decode tail's rows are the live
    // sequences in order and need no more; kept apart from the kernels, which depend on device-resident state only)
    void sample_upload(const std::vector<int>& sample_slot) {
        const int Ms = (int)sample_slot.size();
        for (DevBuf* b : {&i_sample_row_, &i_sample_slot_, &i_next_kvpos_, &i_out_tok_}) b->ensure((size_t)std::max(Ms, 64) * 4);
        ybuf_.ensure((size_t)std::max(Ms, 64) * kHidden * 4);
        P2_.ensure((size_t)std::max(Ms, 64) * kHeadPad * 4);
        HIP_CHECK(hipMemcpyAsync(i_sample_slot_.p, sample_slot.data(), (size_t)Ms * 4, hipMemcpyHostToDevice, st_));
    }
    // decode tail of the gemm_rows chain: rows are the live sequences in order (sample_row = identity), h_ holds the
    // residual stream: ln_f + final_norm (+ second final_norm into the latent stash) -> mel_head GEMM (+ bias) -> sampler
    void sample_kernels_decode(int Ms) {
        const int mtt = rows_cap_ / 16;
        launch_final_rows(h_.as<float>(), mtt, i_sample_slot_.as<int>(), lnfw_, lnfb_, fnw_, fnb_, ybuf_.as<float>(),
                          latents_.as<float>(), (long)kMaxLatRows * kHidden, slot_ngen_.as<int>(), kMaxLatRows, Ms, 1e-5f, st_);
        launch_gemm_rows(head_gemm_args(Ms, false), false, kEpiBias, st_);
        launch_sampler(sampler_args(P2_.as<float>(), Ms, kHeadPad, zero_bias_.as<float>(), nullptr), st_);
    }
    // Profile mode, decode chain.  A HIP-event pair around ONE 5-12 us launch adds 2-5 us to what it measures (the pair serialises
    // the launch processing), so the per-kernel numbers of the bench line come from REPLAY BATCHES instead: after a profiled decode
    // step the step's own launches are issued once more, kind by kind -- the QKV GEMM of every layer back
    // to back between one event pair, then every layer's attention, proj, FC, proj2, then the head -- on the step's real operands
    // (each layer's weights, the live rows, the real contexts) with the OUTPUTS redirected to scratch buffers (the residual
    // stream, K/V pages and latents of the sequences are not touched).  One pair per n_layer launches: the interval is the
    // launch-to-launch period a kernel-trace reports per kernel.  Algorithmic bytes of a GEMM launch: weights once + the activation
    // rows once + the output tile once (the residual epilogue reads and writes it).
    ProfEvent& prof_event(int kind, double flops, double bytes, int count) {
        ProfEvent& ev = next_event(gemm_events_, n_gemm_events_);
        ev.kind = kind; ev.flops = flops; ev.bytes = bytes; ev.count = count;
        return ev;
    }
    static double gemm_alg_bytes(const GemmRowsArgs& a, GemmRowsEpi epi) {
        return (a.prec == 2 ? 2.0 : 4.0) * a.K * a.N + 4.0 * ((double)a.M * a.K + (double)a.M * a.N * (epi == kEpiResidual ? 2.0 : 1.0));
    }
    void profile_replay(int M, double kv_tokens) {
        const int mtt = rows_cap_ / 16, nl = lay_.n_layer;
        const bool kv_half = lay_.kv_half;
        // (the residual replays READ their output scratch -- out += ... -- so a freshly allocated buffer is defined once)
        auto scratch = [&](DevBuf& buf, size_t n) {
            const void* before = buf.p;
            buf.ensure(n);
            if (buf.p != before) HIP_CHECK(hipMemsetAsync(buf.p, 0, n, st_));
        };
        scratch(prof_q_, (size_t)rows_cap_ * kHidden * 4);
        scratch(prof_h_, (size_t)rows_cap_ * kHidden * 4);
        scratch(prof_stats_, (size_t)rows_cap_ * 64 * sizeof(float2));
        scratch(prof_act_, (size_t)rows_cap_ * 4 * kHidden * 4);
        prof_kv_.ensure((size_t)kv_layer_stride_ * (kv_half ? 2 : 4));
        for (int kind = 0; kind < 4; ++kind) {
            const bool ln = kKindLn[kind];
            const GemmRowsEpi epi = kKindEpi[kind];
            const GemmRowsArgs a0 = decode_gemm_args(0, kind, M, true);
            ProfEvent& ev = prof_event(kind, nl * 2.0 * a0.M * a0.N * a0.K, nl * gemm_alg_bytes(a0, epi), nl);
            HIP_CHECK(hipEventRecord(ev.a, st_));
            for (int l = 0; l < nl; ++l) launch_gemm_rows(decode_gemm_args(l, kind, M, true), ln, epi, st_);
            HIP_CHECK(hipEventRecord(ev.b, st_));
            if (kind == 0) {   // attention of every layer: the step's q rows against each layer's real K/V pages
                ProfEvent& ea = prof_event(5, nl * 4.0 * kHidden * kv_tokens, nl * ((kv_half ? 4.0 : 8.0) * kHidden * kv_tokens + 8.0 * kHidden * M), nl);
                HIP_CHECK(hipEventRecord(ea.a, st_));
                for (int l = 0; l < nl; ++l)
                    launch_paged_attention(qbuf_.as<float>(), kv_layer(l), row_meta_.as<int>(), kMaxBlocks, prof_h_.as<float>(), M, st_, mtt, kv_half);
                HIP_CHECK(hipEventRecord(ea.b, st_));
            }
        }
        {   // the mel head has one weight matrix: its replays are L2 / Infinity-Cache warm after the first (1 launch in 152)
            const GemmRowsArgs a0 = head_gemm_args(M, true);
            ProfEvent& ev = prof_event(4, nl * 2.0 * a0.M * a0.N * a0.K, nl * gemm_alg_bytes(a0, kEpiBias), nl);
            HIP_CHECK(hipEventRecord(ev.a, st_));
            for (int l = 0; l < nl; ++l) launch_gemm_rows(a0, false, kEpiBias, st_);
            HIP_CHECK(hipEventRecord(ev.b, st_));
        }
    }
    // Fixed cost of one HIP-event pair on an otherwise busy stream: recording events between back-to-back short
    // kernels serialises their launch processing, which inflates a ~12 us kernel by ~3 us.  Measured once as the
    // median elapsed time of 64 empty pairs and subtracted from every sampled GEMM interval (reported in aur_stats).
    float event_pair_overhead_ms() {
        if (event_overhead_ms_ >= 0.f) return event_overhead_ms_;
        std::vector<hipEvent_t> ev(128);
        for (auto& e : ev) HIP_CHECK(hipEventCreate(&e));
        for (int i = 0; i < 64; ++i) {
            HIP_CHECK(hipEventRecord(ev[2 * i], st_));
            HIP_CHECK(hipEventRecord(ev[2 * i + 1], st_));
        }
        HIP_CHECK(hipStreamSynchronize(st_));
        std::vector<float> d(64);
        for (int i = 0; i < 64; ++i) HIP_CHECK(hipEventElapsedTime(&d[i], ev[2 * i], ev[2 * i + 1]));
        for (auto& e : ev) (void)hipEventDestroy(e);
        std::sort(d.begin(), d.end());
        event_overhead_ms_ = d[32];
        return event_overhead_ms_;
    }

    WeightTable& w_;
    hipStream_t st_;
    const GptLayout lay_;
    bool bound_ = false;
    std::vector<LayerW> layers_;
    std::vector<std::unique_ptr<DevBuf>> packed_;   // pack_wt16 copies (decode GEMM layout)
    DevBuf fold_scratch_;                           // load-time scratch of launch_fold_ln
    const float* thead_ = nullptr;
    const float *wte_ = nullptr, *wpe_ = nullptr, *lnfw_ = nullptr, *lnfb_ = nullptr, *fnw_ = nullptr, *fnb_ = nullptr,
                *headT_ = nullptr, *headb_ = nullptr, *text_emb_ = nullptr, *text_pos_ = nullptr;
    int text_vocab_ = 0, text_positions_ = 0;
    DevBuf kv_;   // the paged K/V pool, [n_layer][n_blocks] blocks
    long kv_layer_stride_ = 0;   // in elements
    // per-slot device state
    DevBuf slot_tok_, slot_pos_, slot_kvpos_, slot_ngen_, slot_finished_, temperature_, top_p_, top_k_, rep_, max_tokens_,
        ignore_stop_, seed_, block_tables_, seen_, latents_;
    DevBuf zero_bias_, i_init_;
    DevBuf ksp_buf_, ksp_cnt_;   // GemmRowsArgs::ksp_buf / ksp_cnt
    // row workspace of the forward chains (prompt rows and decode rows share it)
    int rows_cap_ = 0;
    DevBuf h_, xn_, qbuf_, att_, act_, P_, P2_, ybuf_, stats_, row_meta_;   // row_meta: per-row K/V addressing of the current decode step   // stats: LayerNorm partials of the packed residual stream [rows][64] float2
    DevBuf i_row_slot_, i_row_pos_, i_desc_, i_sample_row_, i_sample_slot_, i_next_kvpos_, i_out_tok_, i_qblk_;
    std::vector<int2> h_qblk_;   // query blocks of the prompt rows in flight (launch_prompt_attention)
    PinBuf pin_;                 // sample_prompt's read-back
    std::vector<int> last_active_;      // live slots whose row indices are resident in the decode chain's index buffers
    DevBuf dbg_lnf_, dbg_logits_;
    bool dbg_capture_ = false;
    std::vector<ProfEvent> gemm_events_;
    size_t n_gemm_events_ = 0;
    DevBuf prof_q_, prof_h_, prof_stats_, prof_act_, prof_kv_;   // output scratch of profile_replay
    float event_overhead_ms_ = -1.f;
};

}  // namespace aur
