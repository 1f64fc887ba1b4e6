/* auralis_amd.h — C ABI of the MI355X-native XTTSv2 generate_speech() hot path.
 *
 * Drop-in boundary for astramind-ai/Auralis (v0.2.8.post2).  The reference has no native code: its
 * engine plugin is the Python class XTTSv2Engine (src/auralis/models/xttsv2/XTTSv2.py:39) behind
 * BaseAsyncTTSEngine (src/auralis/models/base.py:57).  Each entry point below replaces the Python/vLLM
 * mechanism cited next to it; the ctypes binding a maintainer would add is shown in INTEGRATION.md and
 * shipped as auralis_amd/_lib.py.
 *
 * Conventions: every function returns 0 on success or a negative AUR_E_* code; the message of the last
 * failure on the calling thread is aur_last_error().  No exception crosses the boundary.  Handles are
 * opaque and owned by the library.  Pointers passed in are caller-owned HOST pointers borrowed for the
 * duration of the call unless the name says _device.  All floating-point tensors are fp32, row-major.
 * Threading: one driver thread per engine calls aur_step(); aur_submit()/aur_poll_finished()/
 * aur_release() may be called from other threads (internally serialised).
 */
#ifndef AURALIS_AMD_H
#define AURALIS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AUR_OK 0
#define AUR_E_INVALID (-1)   /* bad argument / unknown id / shape mismatch */
#define AUR_E_HIP (-2)       /* HIP runtime or kernel failure */
#define AUR_E_STATE (-3)     /* call not valid in the current state (e.g. weights not loaded) */
#define AUR_E_NOMEM (-4)
#define AUR_E_CANCELLED (-5) /* aur_result.error of a sequence that was cancelled with aur_cancel */

typedef struct aur_engine aur_engine;

/* Engine geometry.  Replaces the AsyncEngineArgs built in XTTSv2Engine.init_vllm_engine
 * (XTTSv2.py:198-232: max_model_len 1047, max_num_seqs = concurrency, block size 16). */
typedef struct aur_config {
    int32_t n_layer;          /* GPT blocks (30 for XTTSv2; tests may use fewer) */
    int32_t max_seqs;         /* concurrent sequences (continuous-batching slots).  A layer's K/V pool is addressed with 32-bit byte
                                 offsets, so max_seqs * 66 + 2 * max_speakers blocks must stay <= 32767 (fp32 pool; 65535 with
                                 kv_fp16): 494 / 991 slots at the default 64 speakers; aur_engine_create reports the limit it computed */
    int32_t max_prefill_rows; /* cap on prompt rows prefetched in one step (0 = default 8192) */
    int32_t max_speakers;     /* speaker-conditioning table entries (0 = default 64) */
    int32_t vocoder_min_batch;/* finished sequences wait until this many are ready for one vocoder pass -- at most 16 steps (~30 ms) counted
                                 from the step the oldest waiting one finished, plus, when a vocoder pass is already in flight, the rest of
                                 that pass (one pass at a time) -- and not at all when nothing else runs or waits.  0 = default
                                 max_seqs / 16 (4 at 64 slots); 1 = vocode at once */
    int32_t profile;          /* 1 = profile mode from the start (see aur_set_profile; every 64th decode step) */
    int32_t vocoder_fp16;     /* 1 = HiFi-GAN convs on fp16-input / fp32-accumulate MFMA (needs the voc16.* tensors);
                                 0 = exact-f32 MFMA parity mode */
    int32_t second_pass;      /* 1 = A/B mode: recompute the latents with the reference's literal second GPT pass
                                 (XTTSv2.py:617-687) instead of the decode-time stash */
    int32_t return_latents;   /* 1 = also copy each sequence's vocoder input latents to the host (aur_result.latents; parity
                                 tests).  0 = audio and tokens only, as the reference's TTSOutput (saves ~1.1 MB of D2H
                                 and host copies per 280-token utterance) */
    int32_t kv_fp16;          /* 1 = throughput mode: the paged K/V pool holds fp16 (rounded to nearest on write; scores, softmax
                                 and P.V stay fp32), which halves the bytes the decode attention streams.  NOT the parity mode:
                                 greedy ids can differ from the fp32 reference after a near-tie (measured rate: DESIGN.md §4).
                                 0 (default) = fp32 K/V, bit-exact contract */
    int32_t gemm_f32_exact;   /* arithmetic of BOTH GEMM regimes (decode rows: gemm_rows_kernel; prompt rows: gemm_tile_split_kernel /
                                 gemm_tile_kernel): 0 (default) = every fp32 operand is split exactly into three bf16 terms and a product
                                 runs as six bf16 MFMAs with fp32 accumulation (the accuracy of an fp32 dot product at 2.7x less
                                 matrix-pipe time); 1 = v_mfma_f32_*_f32, bitwise an fp32 fma chain.  The speaker-conditioning networks
                                 always use the exact-f32 kernels */
    int32_t gelu_erf;         /* MLP activation: 0 = tanh form ("gelu_new", what checkpoint_converter.py:197 writes), 1 = erf form
                                 ("gelu", the XTTSGPTConfig class default, xttsv2_gpt_config.py:184); from the checkpoint's
                                 gpt/config.json "activation_function" */
    int32_t admit_min_batch;  /* continuous batching under saturation: while MORE sequences wait than slots are free (and something
                                 is running), hold admission until this many slots are free, so that one prefill pass (a fixed
                                 ~4.5 ms of launches at 30 layers, whatever the rows) serves that many prompts.  A request that finds
                                 a free slot and no longer queue than free slots is admitted at once, as the reference's vLLM scheduler
                                 does (two_phase_scheduler.py:168-236 hands every request straight to it).  A hold ends after 32 steps (~60 ms) whatever is
                                 free by then.  0 = default max_seqs / 8 (8 at 64 slots); 1 = never hold */
    int32_t urgent_rows;      /* running sequences the engine fills up to while a latency-critical sequence (aur_seq_desc.priority > 0)
                                 waits or runs.  0 = default max_seqs / 4; max_seqs = no cap */
    int32_t gpt_fp16;         /* 1 = the four per-layer GPT linears (attn.c_attn, attn.c_proj, mlp.c_fc, mlp.c_proj) stay in HBM as
                                 fp16 for the decode GEMMs (half their bytes); every product is still computed to fp32 accuracy, so
                                 the mode is the exact model on the effective weights W'' defined here:
                                   c_proj pairs:  f = fp16_rne(W), W'' = f;
                                   c_attn with ln_1, c_fc with ln_2 (gain g, bias b): f[k][n] = fp16_rne(fp32(g[k] * W[k][n])),
                                   W''[k][n] = fp32(f[k][n] / g[k]) (fp16_rne(W[k][n]) where g[k] == 0); the decode GEMM streams f.
                                 The prompt-row GEMMs and second_pass run on W'' too (the engine keeps W'' in place of W).  The rule
                                 is idempotent: an engine loaded with W'' computes bitwise what one loaded with W does.  A matrix
                                 that is not finite or leaves the fp16 range after folding makes aur_load_weights fail with
                                 AUR_E_INVALID; gpt_fp16 together with gemm_f32_exact makes aur_engine_create fail with
                                 AUR_E_INVALID.  0 (default) = fp32 weights, bit-exact contract */
} aur_config;

/* One named fp32 tensor.  Names are the packed names produced by auralis_amd/weights.py from the
 * reference's on-disk keys (checkpoint_converter.py:225-284; loaders XTTSv2.py:288-301,
 * vllm_mm_gpt.py:714-733). */
typedef struct aur_tensor_desc {
    const char* name;
    const float* data;
    int64_t numel;
} aur_tensor_desc;

/* One sequence = one <=250-char text chunk.  Replaces TokensPrompt + ExtendedSamplingParams built in
 * XTTSv2Engine.get_generation_context (XTTSv2.py:727-756) and the text embedding of
 * prepare_text_tokens_async (XTTSv2.py:506-543). */
typedef struct aur_seq_desc {
    const int32_t* text_ids;  /* BPE ids incl. [START]/[STOP] (XTTSv2.py:520-521) */
    int32_t n_text;
    uint64_t speaker_key;     /* conditioning previously registered with aur_set_conditioning */
    float temperature;        /* < 1e-5 => greedy (vLLM _SAMPLING_EPS) */
    float top_p;
    int32_t top_k;            /* <= 0 disables */
    float repetition_penalty; /* hijack.py:49-88 semantics, 1.0 disables */
    int32_t max_tokens;       /* gpt_max_audio_tokens (605) */
    uint32_t seed;            /* per-sequence noise stream (new surface; reference has none) */
    int32_t ignore_stop;      /* 1 = fixed-length mode for timing (stop id does not end the sequence) */
    int32_t encoding;         /* 0 = none; AUR_ENC_FLAC16 = also encode the delivered waveform (after speed and sample_rate, at the delivered
                                 rate) to a 16-bit FLAC stream on the GPU behind the vocoder: aur_result.enc / n_enc, the bytes aur_encode_flac
                                 gives for aur_result.wav.  Anything else makes aur_submit fail with AUR_E_INVALID.  New surface; tokens,
                                 latents and wav do not depend on it.  Such a pass pins about half as many host bytes again */
    int32_t priority;         /* 0 = normal; > 0 = latency-critical (the chunk a listener is waiting for: the head of a stream; the
                                 reference has no counterpart, its streaming latency is whatever vLLM's FIFO gives,
                                 tests/integration/stream_ttfb.py:24-37).  It is admitted in front of the normal queue and at once,
                                 vocoded as soon as its tokens are done, and while it waits or runs the engine admits normal
                                 sequences only up to aur_config.urgent_rows running ones (a decode step's time grows with its
                                 rows).  Results do not depend on it */
    int32_t sample_rate;      /* output sample rate in Hz (new surface, like speed; the reference's counterpart is TTSOutput.resample,
                                 torchaudio.functional.resample over the finished waveform on the host).  0 = unset = 24000, the vocoder's
                                 own rate; otherwise one of 8000, 16000, 22050, 24000, 32000, 44100, 48000, anything else makes aur_submit
                                 fail with AUR_E_INVALID.  The rule is torchaudio's Hann-windowed sinc, lowpass_filter_width 6, rolloff
                                 0.99: for 24000:rate reduced by their gcd to orig:new, base = min(orig, new) * 0.99,
                                 width = ceil(6 orig / base), c[p][k] = sinc(pi t) cos^2(pi t / 12) base / orig with
                                 t = clamp((-p / new + (k - width) / orig) base, -6, 6), k in [0, 2 width + orig), and output sample
                                 j new + p = sum_k c[p][k] xpad[j orig + k], xpad the 24 kHz waveform behind `width` zeros and followed
                                 by zeros; n samples become ceil(n new / orig).  Computed on the GPU behind the vocoder in fp32 (one fma
                                 chain per sample), after speed.  Decoding does not depend on it: tokens, aur_result.latents and
                                 n_latent_rows are unchanged.  A result at 48000 pins twice the host bytes of one at 24000 */
    float speed;              /* speaking rate (new surface, like seed and priority; the reference's counterpart is a phase vocoder over
                                 the finished waveform, TTSOutput.change_speed).  0 = unset = 1.0; otherwise 0.5 <= speed <= 2.0, anything
                                 else (or a non-finite value) makes aur_submit fail with AUR_E_INVALID.  The XTTS inference(speed=) rule:
                                 the GPT latents are linearly interpolated along time by ls = 1 / speed ahead of the vocoder, as
                                 F.interpolate(latents^T, scale_factor=ls, mode="linear") does -- n rows become
                                 L0' = max(1, floor(n * ls)) rows (ls = 1.0 / (double)speed), and the vocoder synthesises
                                 256 * floor(4 L0' * 24000 / 22050) samples at unchanged pitch.  Decoding does not depend on it:
                                 tokens, aur_result.latents and n_latent_rows are those of speed 1 */
} aur_seq_desc;
#define AUR_ENC_FLAC16 1

/* Finished sequence.  Pointers stay valid until aur_release(seq_id).  Replaces the RequestOutput consumed at
 * XTTSv2.py:785 and the TTSOutput array built at XTTSv2.py:804-811. */
typedef struct aur_result {
    uint64_t seq_id;
    int32_t n_tokens;
    const int32_t* tokens;    /* mel token ids, stop id included when emitted */
    int32_t n_samples;
    const float* wav;         /* mono PCM in [-1, 1] at `sample_rate` (a resampled waveform can overshoot the range by the filter's ripple) */
    int32_t n_latent_rows;
    const float* latents;     /* [n_tokens][1024] vocoder input (final_norm applied twice), may be NULL */
    int32_t error;            /* 0 or AUR_E_* if this sequence failed */
    const uint8_t* enc;       /* aur_seq_desc.encoding: the encoded stream of wav (n_enc bytes), valid until aur_release; else NULL */
    int64_t n_enc;
    int32_t sample_rate;      /* of wav, in Hz: aur_seq_desc.sample_rate, 24000 when that was 0 */
} aur_result;

typedef struct aur_stats {
    int64_t steps;                 /* aur_step calls that did work */
    int64_t prefill_rows;          /* prompt rows processed */
    int64_t decode_rows;           /* decode rows processed (one per live sequence per step) */
    int64_t tokens_generated;
    int64_t samples_generated;     /* as delivered, at each sequence's output rate */
    int64_t vocoder_batches;
    /* profile == 1 only: HIP-event time of the MFMA conv launches of the vocoder */
    int64_t conv_launches;
    double conv_ms;
    double conv_flops;             /* algorithmic FLOPs of those launches */
    double conv_bytes;             /* algorithmic (layer-granular) HBM bytes of those launches */
    int64_t gemm_launches;         /* profile mode: decode GEMM launches timed in the replay batches (aur_set_profile) */
    double gemm_ms;                /* event time of the batches minus one event-pair overhead per batch */
    double gemm_ms_raw;            /* event time of the batches */
    double event_pair_overhead_ms; /* measured cost of one empty HIP-event pair */
    double gemm_flops;
    double gemm_bytes;             /* algorithmic: weights once + activations + slabs */
    double vocoder_ms;             /* whole vocoder batches (interp .. conv_post), event-timed */
    double gpt_ms;                 /* prefill + decode + sampling, event-timed per step */
    int64_t kv_blocks_total;
    int64_t kv_blocks_free;
    /* profile mode, per-kernel splits.  GEMM kinds: 0 qkv, 1 attn proj, 2 fc, 3 mlp proj, 4 mel head.  After a profiled decode
     * step its launches are replayed kind by kind, the n_layer launches of one kind back to back between ONE HIP-event pair
     * (outputs redirected to scratch): *_ms are those intervals, *_launches the launches inside them.  Bytes are ALGORITHMIC
     * (weights + activations in + activations out, fp32 as stored; attention: K and V rows of every live sequence's whole
     * context + q + out). */
    int64_t gemm_kind_launches[5];
    double gemm_kind_ms[5];
    double gemm_kind_bytes[5];
    double gemm_kind_flops[5];
    int64_t attn_launches;
    double attn_ms;
    double attn_bytes;
    /* every decode step (not sampled): event time and algorithmic bytes of the whole step */
    int64_t decode_steps;
    double decode_ms;              /* embed .. sampler of the decode steps (gpt_ms = decode_ms + prefill_ms) */
    double prefill_ms;
    double decode_weight_bytes;    /* block + head weights, once per step, fp32 as stored */
    double decode_kv_bytes;        /* K/V rows read by attention, all layers, fp32 as stored */
    /* vocoder conv launches by class (profile mode): 0..3 = ResBlock convs of the 256- / 128- / 64- / 32-channel stage,
     * 4 = conv_pre and the four polyphase transposed convs.  The stages are bounded differently (the wide ones by the fp16
     * matrix pipe and LDS, the narrow ones by HBM), so the bench reports a roofline per class. */
    int64_t conv_class_launches[5];
    double conv_class_ms[5];
    double conv_class_bytes[5];
    double conv_class_flops[5];
    int64_t prefill_batches;       /* prefill passes (one per aur_step that admitted sequences; aur_config.admit_min_batch groups them) */
    /* resource gauges (not reset by aur_reset_stats): what a soak test watches next to hipMemGetInfo (the reference's only resource
     * assertion is tests/integration/memory_leak.py:42-51, VRAM delta over 100 generate_speech calls) */
    int64_t result_blocks;         /* pinned result blocks the engine has allocated (one per vocoder batch in flight or undelivered) */
    int64_t result_blocks_free;    /* ... of which no sequence holds a reference (reusable by the next vocoder batch) */
    int64_t result_block_bytes;    /* pinned host bytes of all result blocks */
    int64_t speakers;              /* voices registered in the speaker table (<= aur_config.max_speakers) */
    int64_t sequences_tracked;     /* sequences the engine still holds (waiting, running, vocoding, or finished and not yet released) */
} aur_stats;

/* What an engine has on its hands right now: what a dispatcher over several engines (one per GPU) places work by. */
typedef struct aur_load {
    int32_t waiting;               /* submitted, no slot yet */
    int32_t running;               /* decoding in a slot */
    int32_t vocoding;              /* tokens done, waiting for or inside a vocoder batch */
    int32_t free_slots;            /* of aur_config.max_seqs */
    int64_t token_budget;          /* sum over waiting and running sequences of max_tokens - tokens generated so far: an upper bound on
                                      the decode work still ahead of the engine */
} aur_load;

const char* aur_last_error(void);
int aur_version(void);

int aur_engine_create(const aur_config* cfg, int device_id, aur_engine** out);
int aur_engine_destroy(aur_engine* e);

/* Upload packed weights (may be called several times; later names overwrite earlier ones). */
int aur_load_weights(aur_engine* e, const aur_tensor_desc* tensors, size_t n);

/* Register/replace the conditioning of one speaker: gpt_cond_latent [32][1024] and speaker embedding
 * [512] (outputs of XTTSv2Engine.get_conditioning_latents, XTTSv2.py:409-468).  Also precomputes the
 * vocoder's 1x1 conditioning convs (hifigan_decoder.py:243-251) for this speaker on the GPU. */
int aur_set_conditioning(aur_engine* e, uint64_t speaker_key, const float* gpt_cond, const float* spk_emb);
/* Same with DEVICE pointers (e.g. the receive buffer of an RCCL broadcast). */
int aur_set_conditioning_device(aur_engine* e, uint64_t speaker_key, const float* d_gpt_cond,
                                const float* d_spk_emb);

/* RCCL inside the boundary (the reference has no counterpart: it forwards tensor_parallel_size to vLLM,
 * XTTSv2.py:214-215).  One engine per GPU per process; the only exchange of the utterance-sharded path is the speaker
 * conditioning.  aur_comm_unique_id: rank 0 creates the 128-byte id and the launcher hands it to every rank (any channel);
 * aur_comm_init: collective, builds the communicator of this engine; aur_broadcast_conditioning: collective, the voice
 * registered on `root` is sent with ONE ncclBroadcast of 133 120 bytes over xGMI and registered on the other ranks from the
 * device receive buffer (same effect as aur_set_conditioning_device there).  RCCL is loaded at run time (dlopen). */
int aur_comm_unique_id(uint8_t* out128);
int aur_comm_init(aur_engine* e, const uint8_t* id128, int32_t rank, int32_t world_size);
int aur_broadcast_conditioning(aur_engine* e, uint64_t speaker_key, int32_t root);
/* What the communicator itself reports (ncclCommCount / ncclCommUserRank): *n_ranks = 0 before aur_comm_init. */
int aur_comm_info(aur_engine* e, int32_t* n_ranks, int32_t* rank);
/* 64-bit FNV-1a checksum over the registered conditioning of a voice as it sits in device memory (gpt_cond_latent [32][1024]
 * then speaker embedding [512], fp32 bytes): lets the ranks of a job verify that a broadcast delivered identical bytes. */
int aur_conditioning_checksum(aur_engine* e, uint64_t speaker_key, uint64_t* out);

/* *out = 1 if speaker_key is registered (and marks it most recently used), else 0.  The table holds
 * aur_config.max_speakers voices; when it is full, registering a new key evicts the least recently used voice that has
 * no undelivered sequences (replaces the reference's unbounded per-request conditioning, XTTSv2.py:409-468: callers
 * re-register an evicted voice). */
int aur_has_conditioning(aur_engine* e, uint64_t speaker_key, int32_t* out);

/* Speaker conditioning from reference audio on the GPU (replaces XTTSv2Engine.get_conditioning_latents,
 * models/xttsv2/XTTSv2.py:409-468, with get_speaker_embedding :312-328 and get_gpt_cond_latents :349-407 underneath:
 * ResNet-SE speaker encoder, ConditioningEncoder, PerceiverResampler and their mel front-ends).
 * pcm[r]: n_samples[r] mono float32 samples of reference r at 22 050 Hz in HOST memory (decoding / resampling of the files is
 * the loader's job, as in the reference's load_audio).  Outputs (host): gpt_cond_latent [32][1024], speaker embedding [512],
 * ready for aur_set_conditioning.  Needs the "cond.*" tensors (auralis_amd/weights.py: pack_conditioning). */
typedef struct aur_cond_params {
    int32_t max_ref_length;      /* seconds of each reference that are used (reference default 30) */
    int32_t gpt_cond_len;        /* seconds of the concatenated references that feed the latents (default 6) */
    int32_t gpt_cond_chunk_len;  /* seconds per chunk (default 6) */
    int32_t sound_norm_refs;     /* 1: each reference scaled to 0.75 of its peak */
} aur_cond_params;
int aur_compute_conditioning(aur_engine* e, const float* const* pcm, const int32_t* n_samples, int32_t n_refs,
                             const aur_cond_params* params, float* out_gpt_cond, float* out_spk_emb);

/* Queue a sequence (replaces llm_engine.generate, XTTSv2.py:752). */
int aur_submit(aur_engine* e, const aur_seq_desc* seq, uint64_t* seq_id);

/* One continuous-batching iteration: admit + prefill waiting sequences, one decode step for every live
 * sequence, fused sampling, and vocoding of sequences that finished (replaces vLLM's engine step, the
 * second pass of get_model_logits XTTSv2.py:617-687 and the HiFi-GAN call XTTSv2.py:804).
 * n_live = sequences still waiting/decoding/vocoding after the step. */
int aur_step(aur_engine* e, int32_t* n_live, int32_t* n_finished_total);

int aur_poll_finished(aur_engine* e, aur_result* out, size_t cap, size_t* n);
int aur_release(aur_engine* e, uint64_t seq_id);
/* Stop a sequence nobody is waiting for any more (a streaming consumer that disconnected; the reference has no counterpart: its
 * chunks decode to the end, two_phase_scheduler.py:279-291 only stops scheduling new ones).  A sequence still waiting for a slot is
 * dropped at once; a running one stops within two decode steps and is NOT vocoded; one whose tokens are done but whose vocoder batch has
 * not been launched is dropped; one already being vocoded (or finished) is left alone.  A cancelled sequence is reported by
 * aur_poll_finished like any other, with error = AUR_E_CANCELLED, the tokens generated so far and no audio; it still needs
 * aur_release.  Thread-safe, does not wait for a running aur_step.  No other sequence's output changes. */
int aur_cancel(aur_engine* e, uint64_t seq_id);

/* Standalone vocoder (HifiDecoder.forward, hifigan_decoder.py:776-802) for parity tests and for callers
 * that bring their own latents: latents [B][t_max][1024], n_lat[B] valid rows each; wav_out [B][wav_stride]. */
int aur_vocode(aur_engine* e, const float* latents, const int32_t* n_lat, int32_t B, int32_t t_max,
               uint64_t speaker_key, float* wav_out, int64_t wav_stride, int32_t* n_samples_out);
/* Same with a speaking rate per utterance, speed[B] (aur_seq_desc.speed: 0 = unset = 1.0, else in [0.5, 2.0]); utterance b yields
 * 256 * floor(4 L0' * 24000 / 22050) samples, L0' = max(1, floor(n_lat[b] / speed[b])), and wav_stride must hold the longest.
 * speed == NULL is aur_vocode (which forwards here).  New surface; the reference has no counterpart. */
int aur_vocode_speed(aur_engine* e, const float* latents, const int32_t* n_lat, const float* speed, int32_t B, int32_t t_max,
                     uint64_t speaker_key, float* wav_out, int64_t wav_stride, int32_t* n_samples_out);
/* Same with an output sample rate per utterance, sample_rate[B] (aur_seq_desc.sample_rate: 0 = unset = 24000, else a supported rate);
 * utterance b yields ceil(n new / orig) samples of the n that aur_vocode_speed yields, and wav_stride must hold the longest.
 * sample_rate == NULL is aur_vocode_speed (which forwards here); speed == NULL as there. */
int aur_vocode_rate(aur_engine* e, const float* latents, const int32_t* n_lat, const float* speed, const int32_t* sample_rate, int32_t B,
                    int32_t t_max, uint64_t speaker_key, float* wav_out, int64_t wav_stride, int32_t* n_samples_out);

/* FLAC on the GPU: B finished float waveforms x[b] (n[b] mono samples in HOST memory, rate[b] Hz) -> B complete 16-bit FLAC streams,
 * byte for byte what the host writer gives (auralis_amd/api/flac.py: flac.encode(codecs._to_int(x, 2), rate, 16)): samples clamped
 * to [-1, 1], * 32767 in fp32, converted toward zero; 4096-sample blocks; CONSTANT, VERBATIM or FIXED (order 0..4) subframes with
 * partitioned Rice codes; MD5 of the PCM in STREAMINFO.  Replaces torchaudio.save(format="flac") of TTSOutput.to_bytes (output.py:119-187).
 * Stream b goes to out + b * out_stride (out_lens[b] bytes; nothing past them is written); out_stride must hold
 * aur_flac_bound(max n[b]).  1 <= n[b] <= 2^24, 1 <= rate[b] < 2^20 and the samples finite, anything else is AUR_E_INVALID.  Takes
 * the GPU between steps, as aur_compute_conditioning does.  aur_flac_bound(n) = 42 + ceil(n / 4096) * 8205. */
int64_t aur_flac_bound(int64_t n_samples);
int aur_encode_flac(aur_engine* e, const float* const* x, const int32_t* n, const int32_t* rate, int32_t B, uint8_t* out, int64_t out_stride,
                    int64_t* out_lens);

int aur_sync(aur_engine* e);
int aur_get_stats(aur_engine* e, aur_stats* out);
int aur_reset_stats(aur_engine* e);
/* Host only: takes the engine's submission lock and nothing else -- no HIP call, no synchronisation, does not wait for a running
 * aur_step.  Safe from any thread at any time.  New surface; the reference has no counterpart. */
int aur_get_load(aur_engine* e, aur_load* out);
/* Profile mode at run time (new surface; the reference has no counterpart): every > 0 -- HIP events around every vocoder conv
 * launch, and after every `every`-th decode step the per-kind replay batches described at aur_stats.gemm_kind_*; 0 = off (the
 * configuration the parity tests run).  Results of the sequences are the same either way. */
int aur_set_profile(aur_engine* e, int32_t every);

/* ---- per-kernel entry points used by the parity tests (host pointers) ------------------------------- */
/* Prefill-regime GEMM (gemm_tile_split_kernel, or gemm_tile_kernel under aur_config.gemm_f32_exact: the kernel every prompt-row
 * linear of vLLM's GPT2Block runs on here, vllm_mm_gpt.py:757-761 at M = prompt rows): out[M][N] = X[M][K] @ W[K][N]. */
int aur_dbg_gemm(aur_engine* e, const float* X, const float* W, float* out, int32_t M, int32_t N, int32_t K);
/* The same launcher with everything its callers vary (tests/test_gpu_prefill_kernels.py).  X [M][ldx], ldx >= K; W [K][N]; `slabs`
 * K slabs of K / slabs consecutive k each.  epi 0: out [slabs][M][N], slab s = X[:, s K/slabs : (s+1) K/slabs] @ the matching rows of W.
 * epi 1 (one slab, bias [N]): out [M][N] = gelu(X @ W + bias), erf != 0 the erf form (HF "gelu"), else the tanh form ("gelu_new"):
 * the FC linear and activation of GPT2MLP.  exact != 0 runs gemm_tile_kernel (exact-f32 MFMA) whatever the engine's arithmetic is, as
 * the speaker-conditioning network does; otherwise the engine's mode, pre-split weight planes included.  The device output starts as
 * NaN words, so an element no workgroup wrote comes back as NaN. */
int aur_dbg_gemm_tile(aur_engine* e, const float* X, int32_t ldx, const float* W, const float* bias, float* out, int32_t M, int32_t N,
                      int32_t K, int32_t slabs, int32_t epi, int32_t erf, int32_t exact);
/* The QKV linear of prompt rows with its epilogue (GPT2Attention.c_attn and vLLM's K/V cache write, vllm_mm_gpt.py:757-761).
 * X [M][1024], W [1024][3072], bias [3072]; row m is token row_pos[m] of sequence row_seq[m].  q_out [M][1024] = (X @ W + bias)[:, :1024];
 * columns 1024..2047 / 2048..3071 of row m go to k_inout / v_inout [n_seq][ctx_max][1024] at [row_seq[m]][row_pos[m]], through a paged
 * pool (16-token blocks) built from those arrays and read back whole: every other element returns as it came.  kv_half: the fp16 pool
 * (the arrays' values must be fp16-representable to return unchanged; written values are rounded to nearest).  fused != 0: in the
 * GEMM's epilogue (AUR_E_INVALID under aur_config.gemm_f32_exact), else the plain GEMM followed by qkv_epilogue_kernel.
 * *stray_out = pool words that belong to no token of a context (the empty block 0, the tail of a last block) and came back non-zero. */
int aur_dbg_qkv_rows(aur_engine* e, const float* X, const float* W, const float* bias, const int32_t* row_seq, const int32_t* row_pos,
                     int32_t M, int32_t n_seq, int32_t ctx_max, int32_t fused, int32_t kv_half, float* q_out, float* k_inout, float* v_inout,
                     int64_t* stray_out);
/* rows_ln_kernel with K slabs: h_inout[M][1024] += sum_s P[s] + bias (P [S][M][1024], S in 0..16; S = 0: h unchanged, P and bias
 * unused), out [M][1024] = LayerNorm(h_inout; gamma, beta, eps 1e-5): the residual add and ln_2 / next ln_1 behind a prompt-row linear. */
int aur_dbg_rows_ln(aur_engine* e, const float* P, int32_t S, const float* bias, float* h_inout, const float* gamma, const float* beta,
                    float* out, int32_t M);
/* Decode-regime GEMM (gemm_rows_kernel: full-K workgroups, fused LayerNorm prologue and bias / gelu / residual epilogue;
 * replaces one GPT2Block linear of vLLM's GPT2Attention / GPT2MLP at M = live sequences, vllm_mm_gpt.py:757-761):
 * out[M][N] = epi(LN?(X[M][K]) @ W[K][N] + bias), epi 0 = bias, 1 = bias + gelu_new, 2 = out += (.. + bias).
 * ln != 0 applies LayerNorm(gamma, beta, eps 1e-5) to the rows of X first (K must be 1024).  K in {1024, 4096}.
 * Follows the engine's mode: under aur_config.gpt_fp16 W is converted by that rule (fp16 copy, effective weights W'') and the
 * kernel runs its fp16-weight arithmetic, as for the four per-layer GEMMs; aur_dbg_gemm_rows_ksplit_stress likewise. */
int aur_dbg_gemm_rows(aur_engine* e, const float* X, const float* W, const float* bias, const float* gamma,
                      const float* beta, float* out, int32_t M, int32_t N, int32_t K, int32_t epi, int32_t ln);
/* Stress of the decode GEMM's K-split form (the K = 4096 -> 1024 projection at M <= 32 live sequences, same reference linear): `iters`
 * back-to-back launches that ALTERNATE between two pseudo-random operand sets (activations and residual), so that consecutive
 * launches publish different partial tiles and a stale read cannot return the right bits, while a second stream streams 256 MiB
 * per launch through the chip for the whole test; each result is compared bitwise on the device with the unsplit kernel's result on
 * the matching operands; *mismatches_out = differing 32-bit words over all launches (0 = the cross-workgroup hand-off held every time). */
int aur_dbg_gemm_rows_ksplit_stress(aur_engine* e, int32_t M, int32_t iters, int64_t* mismatches_out);
/* The kernels' cross-lane helpers (lane_xor<J>, wave_sum, wave_max: DPP and gfx950 lane swaps, csrc/common.h) against the wavefront
 * shuffles they replace, on `blocks` workgroups of pseudo-random words; *mismatches_out = results that differ bitwise (0 expected).
 * Test support: the reference has no counterpart (its reductions are torch's). */
int aur_dbg_lane_xor_selftest(aur_engine* e, int32_t blocks, int64_t* mismatches_out);
/* The decode attention kernel alone (models/xttsv2/components/vllm_mm_gpt.py:757-761: GPT2Attention over vLLM's paged K/V).
 * q [M][1024]; row m attends ctx[m] >= 1 cached tokens whose keys / values are k, v [M][ctx_max][1024] (16 heads x 64 inside a token);
 * the first `shared` tokens (0, 16 or 32; <= every ctx[m]) are taken from row 0 and live in blocks every row's table points to, as the
 * speaker prefix does.  kv_half: the fp16 pool (values rounded to nearest on the way in).  out [M][1024].  Test support. */
int aur_dbg_paged_attention(aur_engine* e, const float* q, const float* k, const float* v, const int32_t* ctx, int32_t M,
                            int32_t ctx_max, int32_t shared, int32_t kv_half, float* out);
/* The prompt-row (prefill) attention kernel alone.  n_seq sequences with keys / values k, v [n_seq][ctx_max][1024]; M query rows
 * q [M][1024], row m belongs to sequence row_seq[m] and sits at position row_pos[m] (it attends that sequence's tokens 0..row_pos[m]);
 * consecutive rows of one sequence with positions ascending by one form the kernel's query blocks (cut every 32 rows), exactly as the
 * engine's prefill builds them.  The first `shared` tokens (0, 16 or 32) are sequence 0's and live in blocks every table points to.
 * out [M][1024].  Test support. */
int aur_dbg_prompt_attention(aur_engine* e, const float* q, const float* k, const float* v, const int32_t* row_seq, const int32_t* row_pos,
                             int32_t M, int32_t n_seq, int32_t ctx_max, int32_t shared, int32_t kv_half, float* out);
/* out[M][1024] = LayerNorm(h) rows */
int aur_dbg_layernorm(aur_engine* e, const float* h, const float* gamma, const float* beta, float* out,
                      int32_t M);
/* Generic masked conv on packed weights: x [B][Cin][L]; out [B][Cout][L*max(1,ups_s)]; see vocoder_kernels.h */
int aur_dbg_conv1d(aur_engine* e, const float* x, const float* wp, const float* bias, const float* res,
                   float* out, const int32_t* lens, int32_t B, int32_t Cin, int32_t Mtot, int32_t Cout,
                   int32_t L, int32_t KS, int32_t DIL, int32_t padl, float slope, int32_t ups_s, int32_t ups_p);
/* Same on the fp16-input MFMA kernel; wp16 = packed halves [Mtot/MT][Cin/16][KS][MT][16] (auralis_amd/weights.py). */
int aur_dbg_conv1d_f16(aur_engine* e, const float* x, const void* wp16, const float* bias, const float* res,
                       float* out, const int32_t* lens, int32_t B, int32_t Cin, int32_t Mtot, int32_t Cout,
                       int32_t L, int32_t KS, int32_t DIL, int32_t padl, float slope, int32_t ups_s, int32_t ups_p);
/* ---- the vocoder's kernels one at a time (tests/test_gpu_vocoder_kernels.py) --------------------------
 * Every tensor is a plain row-major fp32 host array [B][C][L]; where the kernel under test wants the interleaved halves layout
 * [B][C/16][L][16] the harness converts on the way in and out (exact when the values are fp16-representable).  L, the row stride, is
 * the longest utterance of `lens` (times ups_s on the output side), as in the engine.  Output tensors are IN/OUT: the caller's content
 * (a sentinel) is uploaded first, so that what the kernel leaves alone comes back unchanged.  Every device output buffer sits between
 * two 4 KiB guards filled with `guard_value`; *guard_changed = 32-bit guard words that no longer hold it (0 expected). */
/* One ConvArgs launch (csrc/vocoder_kernels.h).  variant 0: launch_conv1d, fp32 tensors, w = packed floats [Mtot/MT][Cin][KS][MT].
 * variant 1 / 2: launch_conv1d_f16 on interleaved halves, w = packed halves [Mtot/MT][Cin/16][KS][MT][16]; 1 = register staging (no
 * zero page), 2 = with the zero page (the LDS-DMA kernel for 64-row tiles).  Their tensor flags are the engine's: x_f16 always (x is
 * stored activated; `slope` is ignored), and for KS >= 3 res_f16 with a residual, mrf_f16 with an MRF mode, out_act_f16 in modes 0 and
 * 3; for KS == 2 (the transposed convs) out_act_f16.  x [B][Cin][L]; res (NULL: none), mrf (modes 1..3), out (modes 0 and 3)
 * [B][Cout][L * max(1, ups_s)]; cond (NULL: none) [cond_rows][cond_stride], utterance b adds row cond_row[b].  Arguments the
 * launchers refuse come back as AUR_E_INVALID. */
int aur_dbg_conv1d_args(aur_engine* e, int32_t variant, const float* x, const void* w, const float* bias, const float* cond,
                        const int32_t* cond_row, int32_t cond_rows, int32_t cond_stride, const float* res, float* mrf, float* out,
                        const int32_t* lens, int32_t B, int32_t Cin, int32_t Mtot, int32_t Cout, int32_t L, int32_t KS, int32_t DIL,
                        int32_t padl, float slope, int32_t ups_s, int32_t ups_p, int32_t mrf_mode, float out_slope, float res_unact,
                        float guard_value, int64_t* guard_changed);
/* One fused ResBlock round (RoundArgs, resblock_round_f16_kernel) on the activated stream y [B][C][L], C in {64, 32}; w1 / w2 packed
 * halves [C/16][KS][C][16], b1 / b2 [C].  mrf_mode 0 writes out; 1 and 2 update mrf; 3 reads mrf and writes out (RoundArgs::e_out,
 * activated with e_slope).  Passing the array of y as out hands the launcher one device tensor for both, which it refuses. */
int aur_dbg_resblock_round_f16(aur_engine* e, const float* y, const void* w1, const void* w2, const float* b1, const float* b2,
                               float* mrf, float* out, const int32_t* lens, int32_t B, int32_t C, int32_t L, int32_t KS, int32_t DIL,
                               int32_t mrf_mode, float e_slope, float guard_value, int64_t* guard_changed);
/* The two chained interpolations (interp2_kernel, or interp2_h_kernel when out_f16).  lat [R][n_max][C]; utterance b reads n_lat[b]
 * rows of lat[lat_row[b]] (lat_row NULL: b) and owns frames_for(n_lat[b]) = floor(4 n * 24000 / 22050) positions of
 * z [B][C][Lz], Lz = the longest of them. */
int aur_dbg_interp2(aur_engine* e, const float* lat, const int32_t* lat_row, const int32_t* n_lat, int32_t R, int32_t n_max, int32_t B,
                    int32_t C, int32_t Lz, int32_t out_f16, float* z, float guard_value, int64_t* guard_changed);
/* The same with the speed stretch in front (interp3_kernel / interp3_h_kernel): speed[B] as aur_seq_desc.speed; utterance b owns
 * frames_for(max(1, floor(n_lat[b] / speed[b]))) positions of z. */
int aur_dbg_interp3(aur_engine* e, const float* lat, const int32_t* lat_row, const int32_t* n_lat, const float* speed, int32_t R,
                    int32_t n_max, int32_t B, int32_t C, int32_t Lz, int32_t out_f16, float* z, float guard_value, int64_t* guard_changed);
/* conv_post + tanh (conv_post_kernel): x [B][Cin][L] (x_f16_act: the activated halves form, `slope` unused), w [Cin][7], wav [B][L]. */
int aur_dbg_conv_post(aur_engine* e, const float* x, const float* w, const int32_t* lens, int32_t B, int32_t Cin, int32_t L, float slope,
                      int32_t x_f16_act, float* wav, float guard_value, int64_t* guard_changed);
/* The output-rate resampler alone (resample_out_kernel): x [B][L] 24 kHz rows of which lens[b] >= 1 samples count (what a row holds
 * past them must not matter), rate[b] as aur_seq_desc.sample_rate; utterance b owns ceil(lens[b] new / orig) samples of out [B][Lout],
 * Lout = the longest of them.  In / out sentinel and guards as above. */
int aur_dbg_resample_out(aur_engine* e, const float* x, const int32_t* lens, const int32_t* rate, int32_t B, int32_t L, float* out,
                         int32_t Lout, float guard_value, int64_t* guard_changed);
/* The FLAC kernels alone (flac_md5_kernel, flac_frame_kernel, flac_assemble_kernel): x [B][stride] rows of which lens[b] >= 1 samples
 * count (what a row holds past them must not matter), rates[b] Hz.  out [B][out_stride] bytes is IN/OUT (the caller's content is
 * uploaded first, so that what the kernels leave alone comes back unchanged) and sits between two guards on the device; a changed guard
 * is AUR_E_HIP.  out_lens[b] = bytes of stream b; out_stride >= aur_flac_bound(max lens). */
int aur_dbg_flac_encode(aur_engine* e, const float* x, const int32_t* lens, const int32_t* rates, int32_t B, int64_t stride, uint8_t* out,
                        int64_t out_stride, int32_t* out_lens);
/* Prefill one prompt and return ln_f rows [n_rows][1024] and the penalised logits [1026] of the last row. */
int aur_dbg_prefill(aur_engine* e, const int32_t* text_ids, int32_t n_text, uint64_t speaker_key,
                    float repetition_penalty, float* lnf_rows_out, float* logits_out);
/* Run the fused sampler on given logits rows [B][1026] (greedy if temperature < 1e-5). */
int aur_dbg_sample(aur_engine* e, const float* logits, int32_t B, float temperature, float top_p, int32_t top_k,
                   float repetition_penalty, const uint8_t* seen /*[B][1026] or NULL*/, uint32_t seed,
                   int32_t step, int32_t* tokens_out);

#ifdef __cplusplus
}
#endif
#endif /* AURALIS_AMD_H */
