// The HiFi-GAN vocoder on the GPU (kernels: vocoder_kernels.h; HifiganGenerator.forward, hifigan_decoder.py:228-260) and the host rules of
// its launches: how a launch's tensors are stored, the shapes of a stage, what a launch costs.  HifiGan::forward and the kernel test
// harness (dbg_harness.hip) fill their ConvArgs / RoundArgs through the same functions, so that the kernel tests exercise the engine's rules.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/auralis_amd.h"
#include "dev_buf.h"
#include "vocoder_kernels.h"

namespace aur {

// The four upsampling stages: stride and taps of the transposed conv, channels behind it.  A stage's three ResBlocks: taps; the
// dilations of a ResBlock's three rounds.
constexpr int kVocRates[4] = {8, 8, 2, 2}, kVocKern[4] = {16, 16, 4, 4}, kVocChans[4] = {256, 128, 64, 32};
constexpr int kResTaps[3] = {3, 7, 11}, kResDil[3] = {1, 3, 5};
constexpr long kCondStride = 1024;   // floats per speaker row of the conditioning table: cond_layer's 512, then conds.0 .. 3 (kVocChans)

// How the vocoder keeps its activations.  f16: the fp16-MFMA kernels (aur_config.vocoder_fp16).  halves: stage inputs, the residual
// stream, the c1 -> c2 intermediate and the MRF sum are interleaved halves in HBM (ConvArgs; AUR_XT_F16=0: fp32).  dma: the LDS-DMA
// staged kernels, which read a zero page for positions outside an utterance (AUR_CONV_DMA=0: register-staged).
struct VocLayout { bool f16 = false, halves = false, dma = false; };
// what a ConvArgs launch is: conv_pre, a stage's transposed conv, the first and the residual conv of a ResBlock round
enum class VocRole { Pre, Ups, C1, C2 };

// The storage of every tensor of a ConvArgs launch.  mrf_mode: ConvArgs::mrf_mode (non-zero on the residual conv of a ResBlock's last
// round).  stored_slope: the leaky-ReLU slope a halves output is stored with, its reader's (0.1; 0.01 for the last stage's MRF mean,
// which feeds conv_post).
inline void conv_storage(ConvArgs& a, VocLayout lay, VocRole role, int mrf_mode, float stored_slope, const void* zero_page) {
    const bool h = lay.halves, resblock = role == VocRole::C1 || role == VocRole::C2;
    a.mrf_mode = mrf_mode;
    // z leaves the interpolation as halves only for the LDS-DMA kernel (round 5: conv_pre register-staged spilled 32 VGPRs)
    a.x_f16 = role == VocRole::Pre ? h && lay.dma : h;
    a.zeros = (lay.dma && (resblock || h)) ? zero_page : nullptr;
    // stage inputs (conv_pre's output, the transposed convs', the MRF mean), the c1 -> c2 intermediate and the stream after rounds 0
    // and 1 are stored the way their reader stages them, fp16(lrelu(., stored_slope)); the running MRF sum is plain halves
    a.out_act_f16 = h && (mrf_mode == 0 || mrf_mode == 3);
    a.out_slope = a.out_act_f16 ? stored_slope : 0.f;
    a.mrf_f16 = h && mrf_mode != 0;
    a.res_f16 = h && role == VocRole::C2;   // the residual is read back from the activated stream and the activation undone
    a.res_unact = a.res_f16 ? 1.0f / 0.1f : 0.f;
}
// A fused ResBlock round's outputs: rounds 0 and 1 (mode 0) write the next stream; a ResBlock's last round folds the MRF sum and, in
// mode 3, writes the stage's mean as fp16(lrelu(., e_slope)).
inline void round_outputs(RoundArgs& a, int mrf_mode, void* stream_out, void* mrf, void* e_out, float e_slope) {
    a.mrf_mode = mrf_mode;
    if (mrf_mode == 0) a.out = stream_out;
    else a.mrf = mrf, a.e_out = e_out, a.e_slope = e_slope;
}

// The shapes of `role`'s launch in stage i (conv_pre: i unused), its input mul positions per frame, on a workspace of T frames per
// utterance, the longest utterance maxT.  KS, DIL: a ResBlock conv's taps and dilation.  conv_pre takes the 1024 latent channels to 512;
// a transposed conv runs as a 2-tap polyphase conv over virtual channels co*s + r.
inline void conv_geometry(ConvArgs& a, VocRole role, int i, int mul, long T, int maxT, int KS = 0, int DIL = 1) {
    const bool pre = role == VocRole::Pre, ups = role == VocRole::Ups;
    const int C = pre ? 512 : kVocChans[i], Cin = pre ? 1024 : !ups ? C : i ? kVocChans[i - 1] : 512, s = ups ? kVocRates[i] : 0;
    const long Lin = T * mul, Lout = ups ? Lin * s : Lin;
    a.len_mul = mul; a.max_len = maxT * mul;
    a.Cin = Cin; a.Cout = C; a.Mtot = ups ? C * s : C;
    a.x_stride = Lin; a.x_bstride = Cin * Lin; a.o_stride = Lout; a.o_bstride = C * Lout;
    a.ups_s = s; a.ups_p = ups ? (kVocKern[i] - s) / 2 : 0;
    a.padl = pre ? 3 : ups ? 1 : (KS - 1) / 2 * DIL;
    a.slope = pre ? 1.0f : 0.1f;
}
inline void round_geometry(RoundArgs& a, int i, int mul, long T, int maxT) {
    a.len_mul = mul; a.max_len = maxT * mul; a.C = kVocChans[i]; a.stride = T * mul; a.bstride = a.C * a.stride;
}

// What a profiled launch is booked as; totT: frames of the batch.  kind: the class of the per-stage roofline (aur_stats.conv_class_*),
// ResBlock convs by channel count (256 / 128 / 64 / 32 -> 0..3), everything else (conv_pre, the four transposed convs) -> 4.
inline void conv_cost(ProfEvent& e, const ConvArgs& a, int KS, double totT) {
    const double tot_in = totT * a.len_mul, tot_out = a.ups_s ? tot_in * a.ups_s : tot_in;
    e.kind = (a.ups_s == 0 && a.Cin == a.Cout) ? (a.Cout == 256 ? 0 : a.Cout == 128 ? 1 : a.Cout == 64 ? 2 : a.Cout == 32 ? 3 : 4) : 4;
    // bytes in the dtype each tensor is actually stored in (the c1 -> c2 intermediate may be fp16)
    const double mrf_b = a.mrf_f16 ? 2.0 : 4.0, o_b = a.out_act_f16 ? 2.0 : 4.0;
    const double out_b = a.mrf_mode == 0 ? o_b : a.mrf_mode == 1 ? mrf_b : a.mrf_mode == 2 ? 2.0 * mrf_b : mrf_b + o_b;
    e.flops = 2.0 * a.Cin * KS * a.Mtot * tot_in;
    e.bytes = (a.x_f16 ? 2.0 : 4.0) * a.Cin * tot_in + a.Cout * tot_out * (out_b + (a.res ? (a.res_f16 ? 2.0 : 4.0) : 0.0));
}
inline void round_cost(ProfEvent& e, const RoundArgs& a, int KS, double totT) {
    const double tot = totT * a.len_mul;
    // stream in, then: stream out (mode 0) | running sum out (1) | in and out (2) | running sum in, stage output out (3)
    const double io = a.mrf_mode == 0 ? 2.0 : a.mrf_mode == 1 ? 2.0 : 4.0;
    e.kind = a.C == 64 ? 2 : 3; e.flops = 2.0 * (2.0 * a.C * KS * a.C * tot) /* conv1 + conv2 */; e.bytes = a.C * tot * (2.0 + io);
}

// samples utterance b of a pass leaves: the vocoder's 256 per frame at 24 kHz, then the output rate (0 = unset = 24000)
inline int out_samples(int n_lat, float speed, int sample_rate) {
    return (int)resampled_len((long)frames_for(stretched_rows(n_lat, speed)) * 256, rate_class(sample_rate));
}

class HifiGan {
public:
    // (on the engine's device: the resampler's table, no weight of the checkpoint, goes up here)
    HifiGan(WeightTable& w, hipStream_t st, VocLayout lay) : W_(w), st_(st), lay_(lay) { v_rtab_.upload(resample_table()); }
    ~HifiGan() {   // (not copyable: the workspace buffers are not)
        for (auto& e : events_) (void)hipEventDestroy(e.a), (void)hipEventDestroy(e.b);
    }

    // the layer tables out of the loaded weights (a missing one throws); unbind() after a load, the next forward binds again
    void bind() {
        if (bound_) return;
        auto layer = [&](const std::string& n) {
            return ConvLayer{W_.W("voc." + n + ".wp"), W_.W("voc." + n + ".bias"), lay_.f16 ? W_.W("voc16." + n + ".wp") : nullptr};
        };
        pre_ = layer("conv_pre");
        for (int i = 0; i < 4; ++i) {
            ups_[i] = layer("ups." + std::to_string(i));
            for (int j = 0; j < 3; ++j)
                for (int c = 0; c < 3; ++c) {
                    const std::string p = "rb." + std::to_string(i * 3 + j) + ".", n = "." + std::to_string(c);
                    c1_[i][j][c] = layer(p + "c1" + n), c2_[i][j][c] = layer(p + "c2" + n);
                }
        }
        post_ = W_.W("voc.conv_post.w");
        bound_ = true;
    }
    void unbind() { bound_ = false; }

    // latents: d_lat + lat_row[b]*lat_bstride (lat_row nullable => b); wav: d_wav + b*wav_bstride; speed[b] as aur_seq_desc.speed;
    // rate[b] as aur_seq_desc.sample_rate (a supported rate or 0), utterance b leaves out_samples(n_lat[b], speed[b], rate[b]) samples;
    // condt: the conditioning table, row cond_row[b] of kCondStride floats.  profile: every conv launch between an event pair (collect)
    void forward(int B, const std::vector<int>& n_lat, const std::vector<float>& speed, const std::vector<int>& rate, const float* d_lat,
                 long lat_bstride, const std::vector<int>* lat_row, const std::vector<int>& cond_row, float* d_wav, long wav_bstride,
                 const float* condt, bool profile) {
        bind();
        profile_ = profile;
        meta_.assign(7 * (size_t)B, 0);
        int maxT = 0;
        double totT = 0;   // frames of the batch
        bool stretched = false;   // some utterance's speed changes its row count: the three-stage kernel
        bool resampled = false;   // some utterance leaves at another rate than the vocoder's 24000: conv_post stages, resample_out_kernel
        long max_out = 0;         // stores
        for (int b = 0; b < B; ++b) {
            const int l0 = stretched_rows(n_lat[b], speed[b]);
            const float r0 = stretch_ratio(speed[b]);
            meta_[b] = n_lat[b];
            meta_[B + b] = frames_for(l0);
            meta_[2 * B + b] = cond_row[b];
            meta_[3 * B + b] = lat_row ? (*lat_row)[b] : b;
            meta_[4 * B + b] = l0;
            std::memcpy(&meta_[5 * B + b], &r0, 4);
            meta_[6 * B + b] = rate_class(rate[b]);
            AUR_REQUIRE(meta_[6 * B + b] >= 0, "sample_rate is 0 (unset) or one of 8000, 16000, 22050, 24000, 32000, 44100, 48000");
            stretched |= l0 != n_lat[b];
            resampled |= meta_[6 * B + b] != 0;
            max_out = std::max(max_out, resampled_len((long)meta_[B + b] * 256, meta_[6 * B + b]));
            maxT = std::max(maxT, meta_[B + b]);
            totT += meta_[B + b];
        }
        v_meta_.ensure(meta_.size() * 4);
        HIP_CHECK(hipMemcpyAsync(v_meta_.p, meta_.data(), meta_.size() * 4, hipMemcpyHostToDevice, st_));
        const int *d_nlat = v_meta_.as<int>(), *d_len = d_nlat + B, *d_cond = d_nlat + 2 * B, *d_latrow = d_nlat + 3 * B;
        const bool h = lay_.halves;
        const size_t T = (size_t)maxT, Bz = (size_t)B;
        v_z_.ensure(Bz * 1024 * T * 4);
        v_s0_.ensure(Bz * 512 * T * 4);
        for (auto* b : {&v_B_, &v_D_, &v_E_}) b->ensure(Bz * 8192 * T * 4);
        if (!v_zero_.p) v_zero_.zeros(256, st_);
        // the residual stream, activated halves or fp32: S0 the stage input (the transposed conv's output, shared by the stage's three
        // ResBlocks), S1 the value after rounds 0 / 1; the fused rounds ping-pong S1 and S2 (neighbouring tiles read each other's halo)
        for (auto* b : {&v_S0_, &v_S1_}) b->ensure(Bz * 8192 * T * (h ? 2 : 4));
        if (h) v_S2_.ensure(Bz * 8192 * T * 2);
        const size_t whole = n_events_;   // the pair around the whole forward (aur_stats.vocoder_ms)
        next_event(events_, n_events_).kind = -1;
        HIP_CHECK(hipEventRecord(events_[whole].a, st_));
        const bool z_f16 = h && lay_.dma;   // as conv_pre reads it (conv_storage): on the LDS-DMA kernel like every other wide conv
        // (a batch in which every utterance keeps its rows -- speed 1, or a stretch that floors back to n_lat -- is the two-stage kernel's)
        if (stretched)
            launch_interp3(d_lat, lat_bstride, d_latrow, d_nlat, d_nlat + 4 * B, reinterpret_cast<const float*>(d_nlat + 5 * B), d_len,
                           v_z_.as<float>(), (long)T, (long)(1024 * T), 1024, B, maxT, st_, z_f16);
        else
            launch_interp2(d_lat, lat_bstride, d_latrow, d_nlat, d_len, v_z_.as<float>(), (long)T, (long)(1024 * T), 1024, B, maxT, st_, z_f16);
        // one conv launch; cond_off >= 0: + the 1x1 conditioning conv of the speaker embedding, precomputed per speaker at that offset
        int mul = 1;   // positions per frame of the running stage
        auto conv = [&](VocRole role, int i, const ConvLayer& l, const void* x, void* out, long cond_off, int KS, int DIL, int mrf_mode = 0,
                        float stored_slope = 0.1f, const void* res = nullptr, void* mrf = nullptr) {
            ConvArgs a{};
            a.base_len = d_len; a.B = B;
            a.x = static_cast<const float*>(x); a.out = static_cast<float*>(out);
            a.res = static_cast<const float*>(res); a.mrf = static_cast<float*>(mrf);
            a.wp = l.wp; a.wp16 = l.wp16; a.bias = l.bias;
            if (cond_off >= 0) a.cond = condt + cond_off, a.cond_row = d_cond, a.cond_stride = kCondStride;
            conv_geometry(a, role, i, mul, (long)T, maxT, KS, DIL);
            conv_storage(a, lay_, role, mrf_mode, stored_slope, v_zero_.p);
            timed([&](ProfEvent& e) { conv_cost(e, a, KS, totT); }, [&] { lay_.f16 ? launch_conv1d_f16(a, KS, DIL, st_) : launch_conv1d(a, KS, DIL, st_); });
        };
        void *S0 = v_S0_.p, *S1 = v_S1_.p, *S2 = v_S2_.p, *Bb = v_B_.p, *D = v_D_.p, *E = v_E_.p;
        conv(VocRole::Pre, 0, pre_, v_z_.p, v_s0_.p, 0, 7, 1);   // (+ cond_layer)
        long cond_off = 512;
        for (int i = 0; i < 4; ++i) {
            const float mean_slope = (i == 3) ? 0.01f : 0.1f;   // the last stage's MRF mean feeds conv_post
            conv(VocRole::Ups, i, ups_[i], i ? E : v_s0_.p, S0, cond_off, 2, 1);
            cond_off += kVocChans[i], mul *= kVocRates[i];
            // the 64- and 32-channel stages (HBM-bound as two launches per round): one fused launch per ResBlock round (RoundArgs)
            const bool fused = h && lay_.dma && kVocChans[i] <= 64;
            for (int j = 0; j < 3; ++j)
                for (int c = 0; c < 3; ++c) {
                    const int KS = kResTaps[j], DIL = kResDil[c];
                    const int mode = c < 2 ? 0 : j + 1;   // a ResBlock's last round goes into the MRF sum D, the third ResBlock's into the mean E
                    const ConvLayer &l1 = c1_[i][j][c], &l2 = c2_[i][j][c];
                    if (fused) {
                        RoundArgs ra{};
                        ra.y = (c == 0) ? S0 : (c == 1) ? S1 : S2;
                        ra.w1 = l1.wp16; ra.w2 = l2.wp16; ra.b1 = l1.bias; ra.b2 = l2.bias;
                        ra.base_len = d_len; ra.B = B; ra.zeros = v_zero_.p;
                        round_geometry(ra, i, mul, (long)T, maxT);
                        round_outputs(ra, mode, (c == 0) ? S1 : S2, D, E, mean_slope);
                        timed([&](ProfEvent& e) { round_cost(e, ra, KS, totT); }, [&] { launch_resblock_round_f16(ra, KS, DIL, st_); });
                        continue;
                    }
                    // the first conv stages the stream as is; the residual conv reads it back and updates S1, in place from round 1 on
                    const void* r = (c == 0) ? S0 : S1;
                    conv(VocRole::C1, i, l1, r, Bb, -1, KS, DIL);
                    conv(VocRole::C2, i, l2, Bb, mode ? E : S1, -1, KS, 1, mode, mode ? mean_slope : 0.1f, r, mode ? D : nullptr);
                }
        }
        // (a batch in which every utterance leaves at 24000 is what it was: conv_post stores into d_wav, same launches, same arguments)
        float* post_out = d_wav;
        long post_bstride = wav_bstride;
        if (resampled) {   // conv_post stores into a device staging buffer [B][maxT * 256], allocated on the first such pass
            v_wav_.ensure(Bz * T * 256 * 4);
            post_out = v_wav_.as<float>(), post_bstride = (long)T * 256;
        }
        launch_conv_post(static_cast<const float*>(E), post_, post_out, d_len, 256, 32, (long)T * 256, (long)32 * T * 256, post_bstride, 0.01f,
                         B, maxT * 256, st_, h);
        if (resampled)
            launch_resample_out(post_out, post_bstride, d_len, 256, d_nlat + 6 * B, v_rtab_.as<int>(), d_wav, wav_bstride, B, max_out, st_);
        HIP_CHECK(hipEventRecord(events_[whole].b, st_));
    }

    // a finished forward's events into the vocoder fields of the statistics (the caller has waited for the stream)
    void collect(aur_stats& s) {
        for (size_t i = 0; i < n_events_; ++i) {
            const ProfEvent& c = events_[i];
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, c.a, c.b));
            if (c.kind < 0) {
                s.vocoder_ms += ms;
            } else {
                s.conv_ms += ms; s.conv_flops += c.flops; s.conv_bytes += c.bytes; s.conv_launches++;
                s.conv_class_ms[c.kind] += ms; s.conv_class_flops[c.kind] += c.flops; s.conv_class_bytes[c.kind] += c.bytes;
                s.conv_class_launches[c.kind]++;
            }
        }
        n_events_ = 0;
    }
    void drop_events() { n_events_ = 0; }   // after a forward that failed, whose events may never complete

private:
    struct ConvLayer { const float *wp = nullptr, *bias = nullptr; const void* wp16 = nullptr; };
    // `launch`, between the next event pair of the pool and booked as `cost` fills it in when the forward profiles
    template <class Cost, class Launch>
    void timed(Cost&& cost, Launch&& launch) {
        if (!profile_) return launch();
        ProfEvent& ev = next_event(events_, n_events_);
        cost(ev);
        HIP_CHECK(hipEventRecord(ev.a, st_));
        launch();
        HIP_CHECK(hipEventRecord(ev.b, st_));
    }

    WeightTable& W_;
    hipStream_t st_;
    VocLayout lay_;
    bool bound_ = false, profile_ = false;
    ConvLayer pre_, ups_[4], c1_[4][3][3], c2_[4][3][3];
    const float* post_ = nullptr;
    DevBuf v_meta_, v_z_, v_s0_, v_S0_, v_S1_, v_S2_, v_B_, v_D_, v_E_, v_zero_;
    DevBuf v_wav_, v_rtab_;   // output rates other than 24000: conv_post's staging buffer, resample_table() on the device
    std::vector<int> meta_;   // host copy of v_meta_ (member: the async H2D copy must not outlive its source)
    std::vector<ProfEvent> events_;   // of the forward in flight: the pair around all of it, then one per profiled launch
    size_t n_events_ = 0;
};

}  // namespace aur
