// Kernel test harness: the aur_dbg_* entry points of include/auralis_amd.h that run ONE kernel on host arrays (tests/test_gpu_kernels.py,
// test_gpu_prefill_kernels.py, test_gpu_vocoder_kernels.py, test_gpu_resample.py, test_gpu_flac.py, test_gpu_gpt.py, test_gpu_gpt_fp16.py).  They take from the engine its streams, its arithmetic mode and
// the K-split scratch (DbgCtx) and nothing else, and the host rules of a launch from where the engine takes them: gpt_host.h (the decode
// GEMMs' operands) and voc_net.h (the storage of a vocoder conv's tensors); aur_dbg_prefill and aur_dbg_sample drive real engine state
// and live in engine.hip.
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "abi_internal.h"
#include "flac_kernels.h"
#include "gpt_host.h"
#include "voc_net.h"

namespace aur {

// Background HBM / L2 traffic on a second stream (aur_dbg_gemm_rows_ksplit_stress).  Every workgroup streams a 64 KiB-aligned share
// of `src` (>= 32 KiB per CU per launch, the guide's "uneven load" rule for cross-workgroup hand-off tests) and leaves one partial
// sum per workgroup so that the loads cannot be dropped.
__global__ __launch_bounds__(256) void stress_load_kernel(const float4* __restrict__ src, float* __restrict__ sink, long n_vec) {
    float acc = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_vec; i += (long)gridDim.x * 256) {
        const float4 v = src[i];
        acc += v.x + v.y + v.z + v.w;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) atomicAdd(sink + blockIdx.x, acc);
}

static DbgCtx use(const aur_engine* e) {
    const DbgCtx c = dbg_ctx(e);
    HIP_CHECK(hipSetDevice(c.device));
    return c;
}
static void download(void* dst, const DevBuf& src, size_t n, hipStream_t st) {
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipMemcpy(dst, src.p, n, hipMemcpyDeviceToHost));
}
// one 8-byte mismatch counter: zeroed on `st`, read back once `st` has drained
static void zero_count(DevBuf& d, hipStream_t st) { d.zeros(8, st); }
static long long read_count(const DevBuf& d, hipStream_t st) {
    unsigned long long bad = 0;
    HIP_CHECK(hipMemcpyAsync(&bad, d.p, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return (long long)bad;
}

// Paged K/V pool ([block][K|V][head][token in block][64], gpt_kernels.hip: kv_offset) of n_seq contexts from row-major
// k, v [n_seq][ctx_max][1024], as halves when `half`.  Block 0 stays empty (what a table entry past a sequence's blocks names), the
// `shared` leading tokens of every context are sequence 0's and live in blocks 1.., every sequence has ceil(ctx_max / 16) entries of
// its own behind them.  table[sq * stride + b] receives the block tables; n_tok[sq] (null: ctx_max) tokens of a context are stored.
static void upload_kv_pool(const float* k, const float* v, int n_seq, int ctx_max, int shared, const int* n_tok, bool half, int* table,
                           int stride, DevBuf& dpool) {
    const int n_shared = shared / kKvBlockTokens, per_seq = (ctx_max + kKvBlockTokens - 1) / kKvBlockTokens;
    std::vector<float> pool((size_t)(1 + n_shared + (long)n_seq * per_seq) * kKvBlockElems, 0.f);
    for (int sq = 0; sq < n_seq; ++sq) {
        int* bt = table + (size_t)sq * stride;
        for (int b = 0; b < per_seq; ++b) bt[b] = b < n_shared ? 1 + b : 1 + n_shared + sq * per_seq + b;
        for (int t = 0; t < (n_tok ? n_tok[sq] : ctx_max); ++t) {
            const int src = t < shared ? 0 : sq;
            for (int kvi = 0; kvi < 2; ++kvi) {
                const float* row = (kvi ? v : k) + ((size_t)src * ctx_max + t) * kHidden;
                for (int h = 0; h < kHeads; ++h)
                    std::memcpy(&pool[((((size_t)bt[t / kKvBlockTokens] * 2 + kvi) * kHeads + h) * kKvBlockTokens + t % kKvBlockTokens) * kHeadDim],
                                row + h * kHeadDim, kHeadDim * sizeof(float));
            }
        }
    }
    if (half)
        dpool.upload(std::vector<_Float16>(pool.begin(), pool.end()));
    else
        dpool.upload(pool);
}

// The pool of upload_kv_pool (shared = 0, every context ctx_max tokens) back into k, v [n_seq][ctx_max][1024], halves widened exactly.
// Returns the pool words that belong to no token of a context (block 0, the tail of every last block) and are no longer zero.
static long long download_kv_pool(const DevBuf& dpool, int n_seq, int ctx_max, bool half, const int* table, int stride, float* k, float* v) {
    const int per_seq = (ctx_max + kKvBlockTokens - 1) / kKvBlockTokens;
    std::vector<float> pool((size_t)(1 + (long)n_seq * per_seq) * kKvBlockElems);
    if (half) {
        std::vector<_Float16> hp(pool.size());
        HIP_CHECK(hipMemcpy(hp.data(), dpool.p, hp.size() * 2, hipMemcpyDeviceToHost));
        std::copy(hp.begin(), hp.end(), pool.begin());
    } else {
        HIP_CHECK(hipMemcpy(pool.data(), dpool.p, pool.size() * 4, hipMemcpyDeviceToHost));
    }
    for (int sq = 0; sq < n_seq; ++sq) {
        const int* bt = table + (size_t)sq * stride;
        for (int t = 0; t < ctx_max; ++t)
            for (int kvi = 0; kvi < 2; ++kvi) {
                float* row = (kvi ? v : k) + ((size_t)sq * ctx_max + t) * kHidden;
                for (int h = 0; h < kHeads; ++h) {
                    float* src = &pool[((((size_t)bt[t / kKvBlockTokens] * 2 + kvi) * kHeads + h) * kKvBlockTokens + t % kKvBlockTokens) * kHeadDim];
                    std::memcpy(row + h * kHeadDim, src, kHeadDim * sizeof(float));
                    std::memset(src, 0, kHeadDim * sizeof(float));   // what is left non-zero below belongs to no token
                }
            }
    }
    long long stray = 0;
    for (const float& w : pool) {
        uint32_t bits;
        std::memcpy(&bits, &w, 4);
        stray += bits != 0;
    }
    return stray;
}

// ---- the vocoder's kernels on host arrays [B][C][L] (aur_dbg_conv1d_args, _resblock_round_f16, _interp2, _conv_post) ----
constexpr size_t kGuardBytes = 4096;

// [B][C][L] floats -> interleaved halves [B][C/16][L][16] (ConvArgs) and back
static std::vector<_Float16> to_halves(const float* src, int B, int C, long L) {
    std::vector<_Float16> h((size_t)B * C * L);
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c)
            for (long t = 0; t < L; ++t) h[(((size_t)b * (C / 16) + c / 16) * L + t) * 16 + c % 16] = (_Float16)src[((size_t)b * C + c) * L + t];
    return h;
}
static void from_halves(const _Float16* h, float* dst, int B, int C, long L) {
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c)
            for (long t = 0; t < L; ++t) dst[((size_t)b * C + c) * L + t] = (float)h[(((size_t)b * (C / 16) + c / 16) * L + t) * 16 + c % 16];
}

// A device tensor [B][C][L] (floats, or interleaved halves) between two guards of kGuardBytes that hold `guard`
struct GuardedBuf {
    DevBuf d;
    int B = 0, C = 0;
    long L = 0;
    bool half = false;
    float guard = 0.f;
    size_t data_bytes() const { return (size_t)B * C * L * (half ? 2 : 4); }
    void* data() const { return d.as<char>() + kGuardBytes; }
    template <class T>
    void put(const std::vector<T>& body) {   // guard | body | guard
        std::vector<T> img(2 * kGuardBytes / sizeof(T) + body.size(), (T)guard);
        std::copy(body.begin(), body.end(), img.begin() + kGuardBytes / sizeof(T));
        d.upload(img);
    }
    void upload(const float* host, int B_, int C_, long L_, bool half_, float guard_) {
        B = B_; C = C_; L = L_; half = half_; guard = guard_;
        AUR_REQUIRE(!half || C % 16 == 0, "dbg: interleaved halves need whole 16-channel chunks");
        if (half) put(to_halves(host, B, C, L));
        else put(std::vector<float>(host, host + (size_t)B * C * L));
    }
    // the tensor back into `host`; returns the 32-bit guard words that changed
    template <class T>
    long long get(float* host) {
        const size_t ng = kGuardBytes / sizeof(T), n = (size_t)B * C * L;
        std::vector<T> img(2 * ng + n);
        HIP_CHECK(hipMemcpy(img.data(), d.p, img.size() * sizeof(T), hipMemcpyDeviceToHost));
        std::vector<T> ref(ng, (T)guard);
        long long bad = 0;
        for (const T* g : {img.data(), img.data() + ng + n})
            for (size_t i = 0; i < kGuardBytes; i += 4) bad += std::memcmp((const char*)g + i, (const char*)ref.data() + i, 4) != 0;
        if constexpr (std::is_same<T, float>::value) std::copy(img.begin() + ng, img.begin() + ng + n, host);
        else from_halves(img.data() + ng, host, B, C, L);
        return bad;
    }
    long long download(float* host, hipStream_t st) {
        HIP_CHECK(hipStreamSynchronize(st));
        return half ? get<_Float16>(host) : get<float>(host);
    }
};

static void check_lens(const int* lens, int B, int L, const char* what) {
    AUR_REQUIRE(B >= 1 && L >= 1, what);
    for (int b = 0; b < B; ++b) AUR_REQUIRE(lens[b] >= 1 && lens[b] <= L, what);
    AUR_REQUIRE(*std::max_element(lens, lens + B) == L, what);   // the row stride is the longest utterance, as in the engine
}

// aur_dbg_conv1d_args' variant as the engine's storage layout: 0 the fp32 vocoder, 1 / 2 interleaved halves, register / LDS-DMA staged
static VocLayout variant_layout(int variant) { return {variant != 0, variant != 0, variant == 2}; }

// One ConvArgs launch on host arrays [B][C][L], every tensor stored as the engine stores it under `lay` in the role the arguments
// name (conv_storage, voc_net.h): ups_s > 0 a transposed conv, a residual the second conv of a ResBlock round, anything else the
// first.  mrf and out go between guards of guard_value; returns the guard words that changed.
static long long run_conv(const DbgCtx& c, VocLayout lay, const float* x, const void* w, const float* bias, const float* cond, const int* cond_row,
                          int cond_rows, int cond_stride, const float* res, float* mrf, float* out, const int* lens, int B, int Cin, int Mtot,
                          int Cout, int L, int KS, int DIL, int padl, float slope, int ups_s, int ups_p, int mrf_mode, float out_slope,
                          float guard_value) {
    const long Lout = (long)L * std::max(1, ups_s);
    DevBuf dx, dw, db, dc, dcr, dr, dl, dz;
    GuardedBuf gm, go;
    if (lay.halves) {
        AUR_REQUIRE(Cin % 16 == 0, "dbg_conv1d_args: interleaved halves need whole 16-channel chunks");
        dx.upload(to_halves(x, B, Cin, L));
        if (res) {
            AUR_REQUIRE(Cout % 16 == 0, "dbg_conv1d_args: interleaved halves need whole 16-channel chunks");
            dr.upload(to_halves(res, B, Cout, Lout));
        }
    } else {
        dx.upload(x, (size_t)B * Cin * L * 4);
        if (res) dr.upload(res, (size_t)B * Cout * Lout * 4);
    }
    dw.upload(w, (size_t)Mtot * Cin * KS * (lay.f16 ? 2 : 4));
    dl.upload(lens, (size_t)B * 4);
    if (bias) db.upload(bias, (size_t)Cout * 4);
    if (cond) {
        dc.upload(cond, (size_t)cond_rows * cond_stride * 4);
        dcr.upload(cond_row, (size_t)B * 4);
    }
    if (lay.dma) dz.zeros(256, c.st);
    ConvArgs a{};
    a.x = dx.as<float>();
    a.wp = dw.as<float>();
    a.wp16 = lay.f16 ? dw.p : nullptr;
    a.bias = db.as<float>();
    a.cond = dc.as<float>(); a.cond_row = dcr.as<int>(); a.cond_stride = cond_stride;
    a.res = dr.as<float>();
    a.base_len = dl.as<int>();
    a.len_mul = 1;
    a.Cin = Cin; a.Mtot = Mtot; a.Cout = Cout;
    a.x_stride = L; a.o_stride = Lout;
    a.x_bstride = (long)Cin * L; a.o_bstride = (long)Cout * Lout;
    a.padl = padl; a.slope = slope; a.ups_s = ups_s; a.ups_p = ups_p;
    a.max_len = *std::max_element(lens, lens + B);
    a.B = B;
    conv_storage(a, lay, ups_s > 0 ? VocRole::Ups : res ? VocRole::C2 : VocRole::C1, mrf_mode, out_slope, dz.p);
    if (mrf_mode != 0) {
        gm.upload(mrf, B, Cout, Lout, a.mrf_f16 != 0, guard_value);
        a.mrf = reinterpret_cast<float*>(gm.data());
    }
    if (mrf_mode == 0 || mrf_mode == 3) {
        go.upload(out, B, Cout, Lout, a.out_act_f16 != 0, guard_value);
        a.out = reinterpret_cast<float*>(go.data());
    }
    if (lay.f16)
        launch_conv1d_f16(a, KS, DIL, c.st);
    else
        launch_conv1d(a, KS, DIL, c.st);
    long long bad = 0;
    if (mrf_mode != 0) bad += gm.download(mrf, c.st);
    if (mrf_mode == 0 || mrf_mode == 3) bad += go.download(out, c.st);
    return bad;
}
// aur_dbg_conv1d / _f16: the same launch on fp32 tensors (f16: fp16 weights and MFMA) without conditioning or MRF, into a zeroed output
static void run_conv_plain(const aur_engine* e, bool f16, const float* x, const void* w, const float* bias, const float* res, float* out,
                           const int* lens, int B, int Cin, int Mtot, int Cout, int L, int KS, int DIL, int padl, float slope, int ups_s, int ups_p) {
    std::fill(out, out + (size_t)B * Cout * L * std::max(1, ups_s), 0.f);
    run_conv(use(e), {f16, false, false}, x, w, bias, nullptr, nullptr, 0, 0, res, nullptr, out, lens, B, Cin, Mtot, Cout, L, KS, DIL, padl, slope,
             ups_s, ups_p, 0, 0.f, 0.f);
}

}  // namespace aur

using namespace aur;

extern "C" {

// prefill-regime GEMM (gemm_tile_kernel / gemm_tile_split_kernel, the arithmetic the engine was configured with) on host data: out = X @ W
int aur_dbg_gemm(aur_engine* e, const float* X, const float* W, float* out, int32_t M, int32_t N, int32_t K) {
    CHECK_PTR(e);
    return guarded([&] {
        const DbgCtx c = use(e);
        DevBuf dx, dw, dp, ds;
        dx.upload(X, (size_t)M * K * 4);
        dw.upload(W, (size_t)K * N * 4);
        dp.ensure((size_t)M * N * 4);
        if (c.prec == 1 && c.presplit && N % 128 == 0) {   // the pre-split weight operand, as the engine prepares it for the prompt-row GEMMs
            ds.ensure((size_t)3 * K * N * 2);
            launch_pack_wsplit(dw.as<float>(), N, ds.p, K, N, c.st);
        }
        launch_gemm_tile(dx.as<float>(), K, dw.as<float>(), dp.as<float>(), M, N, K, c.st, nullptr, c.prec, 1, ds.p);
        download(out, dp, (size_t)M * N * 4, c.st);
    });
}
// The prefill-regime launcher with everything the engine and cond_net.h vary: ldx, K slabs, the bias + GELU epilogue, exact-f32 on a
// split-arithmetic engine.  epi 0: out [slabs][M][N] raw slabs; epi 1: out [M][N] = gelu(X @ W + bias).  The output starts as NaN words.
int aur_dbg_gemm_tile(aur_engine* e, const float* X, int32_t ldx, const float* W, const float* bias, float* out, int32_t M, int32_t N,
                      int32_t K, int32_t slabs, int32_t epi, int32_t erf, int32_t exact) {
    CHECK_PTR(e);
    CHECK_PTR(X);
    CHECK_PTR(W);
    CHECK_PTR(out);
    return guarded([&] {
        const DbgCtx c = use(e);
        AUR_REQUIRE(M >= 1 && M <= 8192 && N >= 64 && K >= 16 && ldx >= K, "dbg_gemm_tile: 1..8192 rows, N >= 64, K >= 16, ldx >= K");
        AUR_REQUIRE(epi == 0 || (epi == 1 && bias && slabs == 1), "dbg_gemm_tile: epi 0, or 1 with a bias and one slab");
        AUR_REQUIRE(slabs >= 1 && slabs <= 16, "dbg_gemm_tile: 1..16 slabs");
        const int prec = exact ? 0 : c.prec;
        const size_t n_out = (size_t)(epi ? 1 : slabs) * M * N * 4;
        DevBuf dx, dw, db, dp, da, ds;
        dx.upload(X, (size_t)M * ldx * 4);
        dw.upload(W, (size_t)K * N * 4);
        if (bias) db.upload(bias, (size_t)N * 4);
        DevBuf& dout = epi ? da : dp;
        dp.ensure((size_t)slabs * M * N * 4);
        dout.ensure(n_out);
        HIP_CHECK(hipMemsetAsync(dout.p, 0xFF, n_out, c.st));
        if (prec == 1 && c.presplit && N % 128 == 0) {   // as aur_dbg_gemm
            ds.ensure((size_t)3 * K * N * 2);
            launch_pack_wsplit(dw.as<float>(), N, ds.p, K, N, c.st);
        }
        const GemmGelu ge{db.as<float>(), da.as<float>(), erf ? 1 : 0};
        launch_gemm_tile(dx.as<float>(), ldx, dw.as<float>(), dp.as<float>(), M, N, K, c.st, epi ? &ge : nullptr, prec, slabs, ds.p);
        download(out, dout, n_out, c.st);
    });
}
// The QKV GEMM of prompt rows with its epilogue (bias, q rows, K / V into the paged pool at (row_seq[m], row_pos[m])): fused != 0 in the
// GEMM's own epilogue (split arithmetic only), else the plain GEMM and qkv_epilogue_kernel with explicit positions -- forward_rows' two
// forms.  The pool is built from k_inout / v_inout and read back whole; *stray_out: download_kv_pool.
int aur_dbg_qkv_rows(aur_engine* e, const float* X, const float* W, const float* bias, const int32_t* row_seq, const int32_t* row_pos,
                     int32_t M, int32_t n_seq, int32_t ctx_max, int32_t fused, int32_t kv_half, float* q_out, float* k_inout, float* v_inout,
                     int64_t* stray_out) {
    CHECK_PTR(e);
    CHECK_PTR(X);
    CHECK_PTR(W);
    CHECK_PTR(bias);
    CHECK_PTR(row_seq);
    CHECK_PTR(row_pos);
    CHECK_PTR(q_out);
    CHECK_PTR(k_inout);
    CHECK_PTR(v_inout);
    CHECK_PTR(stray_out);
    return guarded([&] {
        const DbgCtx c = use(e);
        AUR_REQUIRE(M >= 1 && M <= 8192 && n_seq >= 1 && n_seq <= 64 && ctx_max >= 1 && ctx_max <= kMaxBlocks * kKvBlockTokens,
                    "dbg_qkv_rows: 1..8192 rows, 1..64 sequences, context 1..1056");
        AUR_REQUIRE(!fused || c.prec == 1, "dbg_qkv_rows: the fused epilogue needs the split arithmetic");
        for (int m = 0; m < M; ++m)
            AUR_REQUIRE(row_seq[m] >= 0 && row_seq[m] < n_seq && row_pos[m] >= 0 && row_pos[m] < ctx_max, "dbg_qkv_rows: row_seq / row_pos out of range");
        constexpr int N = 3 * kHidden, K = kHidden;
        std::vector<int> bt((size_t)n_seq * kMaxBlocks, 0);
        DevBuf dx, dw, db, dpool, dbt, drs, drp, dp, dq, ds;
        upload_kv_pool(k_inout, v_inout, n_seq, ctx_max, 0, nullptr, kv_half != 0, bt.data(), kMaxBlocks, dpool);
        dx.upload(X, (size_t)M * K * 4);
        dw.upload(W, (size_t)K * N * 4);
        db.upload(bias, (size_t)N * 4);
        dbt.upload(bt);
        drs.upload(row_seq, (size_t)M * 4);
        drp.upload(row_pos, (size_t)M * 4);
        dp.ensure((size_t)M * N * 4);
        dq.ensure((size_t)M * kHidden * 4);
        HIP_CHECK(hipMemsetAsync(dq.p, 0xFF, (size_t)M * kHidden * 4, c.st));
        if (c.prec == 1 && c.presplit) {   // as aur_dbg_gemm
            ds.ensure((size_t)3 * K * N * 2);
            launch_pack_wsplit(dw.as<float>(), N, ds.p, K, N, c.st);
        }
        if (fused) {
            GemmGelu qe{db.as<float>(), nullptr, 0};
            qe.qbuf = dq.as<float>(); qe.kv_layer = dpool.p; qe.row_slot = drs.as<int>(); qe.row_pos = drp.as<int>(); qe.block_tables = dbt.as<int>();
            qe.max_blocks = kMaxBlocks; qe.kv_half = kv_half ? 1 : 0;
            launch_gemm_tile(dx.as<float>(), K, dw.as<float>(), dp.as<float>(), M, N, K, c.st, &qe, c.prec, 1, ds.p);
        } else {
            launch_gemm_tile(dx.as<float>(), K, dw.as<float>(), dp.as<float>(), M, N, K, c.st, nullptr, c.prec, 1, ds.p);
            launch_qkv_epilogue(dp.as<float>(), 1, db.as<float>(), dq.as<float>(), dpool.p, drs.as<int>(), drp.as<int>(), nullptr, dbt.as<int>(),
                                kMaxBlocks, M, c.st, kv_half != 0);
        }
        download(q_out, dq, (size_t)M * kHidden * 4, c.st);
        *stray_out = download_kv_pool(dpool, n_seq, ctx_max, kv_half != 0, bt.data(), kMaxBlocks, k_inout, v_inout);
    });
}
// rows_ln_kernel with slabs: h[M][1024] += sum of the S slabs P[S][M][1024] + bias (S > 0), out = LayerNorm(h)
int aur_dbg_rows_ln(aur_engine* e, const float* P, int32_t S, const float* bias, float* h_inout, const float* gamma, const float* beta,
                    float* out, int32_t M) {
    CHECK_PTR(e);
    CHECK_PTR(h_inout);
    CHECK_PTR(gamma);
    CHECK_PTR(beta);
    CHECK_PTR(out);
    return guarded([&] {
        const DbgCtx c = use(e);
        AUR_REQUIRE(M >= 1 && M <= 8192 && S >= 0 && S <= 16, "dbg_rows_ln: 1..8192 rows, 0..16 slabs");
        AUR_REQUIRE(S == 0 || (P && bias), "dbg_rows_ln: slabs need P and bias");
        const size_t n = (size_t)M * kHidden * 4;
        DevBuf dp, dbi, dh, dg, db, dout;
        if (S > 0) {
            dp.upload(P, (size_t)S * n);
            dbi.upload(bias, kHidden * 4);
        }
        dh.upload(h_inout, n);
        dg.upload(gamma, kHidden * 4);
        db.upload(beta, kHidden * 4);
        dout.ensure(n);
        launch_rows_ln(dp.as<float>(), S, dbi.as<float>(), dh.as<float>(), dg.as<float>(), db.as<float>(), dout.as<float>(), M, 1e-5f, c.st);
        download(out, dout, n, c.st);
        HIP_CHECK(hipMemcpy(h_inout, dh.p, n, hipMemcpyDeviceToHost));
    });
}
// decode-regime GEMM on host data: out = epi(LN?(X) @ W + bias); W is the plain [K][N] matrix, made the kernel's operand on the device
// by the routine the engine uses at load time (prepare_decode_operand).  epi: 0 bias, 1 bias + gelu_new, 2 out += (X @ W + bias).
int aur_dbg_gemm_rows(aur_engine* e, const float* X, const float* W, const float* bias, const float* gamma, const float* beta,
                      float* out, int32_t M, int32_t N, int32_t K, int32_t epi, int32_t ln) {
    CHECK_PTR(e);
    CHECK_PTR(X);
    CHECK_PTR(W);
    CHECK_PTR(out);
    return guarded([&] {
        const DbgCtx c = use(e);
        AUR_REQUIRE(epi >= 0 && epi <= 2, "dbg_gemm_rows: epi in {0,1,2}");
        AUR_REQUIRE(!ln || (gamma && beta), "dbg_gemm_rows: LN needs gamma and beta");
        const int mtt = (M + 63) / 64 * 4;                      // 16-row tiles of the packed activation buffers
        const bool out_packed = (epi == kEpiBiasGelu || epi == kEpiResidual);
        std::vector<float> hx((size_t)mtt * 16 * K, 0.f), ho((size_t)mtt * 16 * N, 0.f);
        for (int m = 0; m < M; ++m)
            for (int k = 0; k < K; ++k) hx[pk_off(m, k, mtt)] = X[(size_t)m * K + k];
        for (int m = 0; m < M; ++m)
            for (int n = 0; n < N; ++n) ho[out_packed ? pk_off(m, n, mtt) : (size_t)m * N + n] = out[(size_t)m * N + n];
        DevBuf dx, dw, db, dg, dbe, dout, dst, dsc, dbad;
        dx.upload(hx);
        dw.upload(W, (size_t)K * N * 4);
        dout.upload(ho);
        if (bias) db.upload(bias, (size_t)N * 4);
        else if (!ln) db.zeros((size_t)N * 4, c.st);   // the kernel loads its bias unconditionally
        if (ln) {
            // LayerNorm partials per 16-column tile, as the residual-stream producers emit them (GemmRowsArgs)
            std::vector<float2> hs((size_t)mtt * 16 * 64, make_float2(0.f, 0.f));
            for (int m = 0; m < M; ++m)
                for (int t = 0; t < 64; ++t) {
                    float sm = 0.f, m2 = 0.f;
                    for (int i = 0; i < 16; ++i) sm += X[(size_t)m * K + 16 * t + i];
                    const float mu = sm * (1.0f / 16.0f);
                    for (int i = 0; i < 16; ++i) {
                        const float d = X[(size_t)m * K + 16 * t + i] - mu;
                        m2 += d * d;
                    }
                    hs[(size_t)m * 64 + t] = make_float2(mu, m2);
                }
            dst.upload(hs);
            dg.upload(gamma, (size_t)K * 4);
            dbe.upload(beta, (size_t)K * 4);
        }
        GemmRowsArgs a{};
        a.prec = c.gpt_fp16 ? 2 : c.prec;
        dbad.zeros(sizeof(int), c.st);
        std::vector<std::unique_ptr<DevBuf>> keep;
        const DecodeOperand op = prepare_decode_operand(a.prec, dw.as<float>(), N, dg.as<float>(), dbe.as<float>(), db.as<float>(), K, N, nullptr,
                                                        dbad.as<int>(), dsc, keep, c.st);
        int bad = 0;
        HIP_CHECK(hipMemcpyAsync(&bad, dbad.p, sizeof(int), hipMemcpyDeviceToHost, c.st));
        HIP_CHECK(hipStreamSynchronize(c.st));
        AUR_REQUIRE(!bad, "dbg_gemm_rows: gpt_fp16 rejects these weights (not finite, or beyond the fp16 range after folding)");
        a.X = dx.as<float>(); a.xmt = mtt; a.Wt = op.Wt; a.bias = op.bias; a.ln_c1 = op.c1; a.M = M; a.N = N; a.K = K;
        a.eps = 1e-5f;
        if ((long)((M + 15) / 16) * (N / 16) <= kGemmKspTiles) { a.ksp_buf = c.ksp_buf; a.ksp_cnt = c.ksp_cnt; }
        a.stats_in = dst.as<float2>();
        a.out = dout.as<float>(); a.ldo = N; a.omt = mtt;
        launch_gemm_rows(a, ln, (GemmRowsEpi)epi, c.st);
        download(ho.data(), dout, ho.size() * 4, c.st);
        for (int m = 0; m < M; ++m)
            for (int n = 0; n < N; ++n) out[(size_t)m * N + n] = ho[out_packed ? pk_off(m, n, mtt) : (size_t)m * N + n];
    });
}
// Stress of the K-split projection's cross-workgroup protocol (gemm_rows_kernel.inc, KSP: write-through partial tiles, drained
// vmcnt, device-scope ticket, sc0 sc1 read-back by the last arriver, counter reset for the next launch): `iters` back-to-back
// launches of the K = 4096 -> 1024 residual GEMM at M rows, no host synchronisation in between, on two alternating operand
// sets and beside a second stream that streams 256 MiB per launch, each compared word for word on the device with the UNSPLIT
// kernel's result on the matching operands.  A visibility bug shows up as a non-zero count.
int aur_dbg_gemm_rows_ksplit_stress(aur_engine* e, int32_t M, int32_t iters, int64_t* mismatches_out) {
    CHECK_PTR(e);
    CHECK_PTR(mismatches_out);
    return guarded([&] {
        const DbgCtx c = use(e);
        const int K = 4 * kHidden, N = kHidden;
        AUR_REQUIRE(M >= 1 && M <= 32 && iters >= 1, "ksplit stress: the split is used for M <= 32 rows");
        AUR_REQUIRE(gemm_rows_shape(M, N, K, false).ksp > 1, "ksplit stress: the policy does not split at this M");
        // TWO operand sets, alternated launch by launch: consecutive launches publish DIFFERENT partial tiles into ksp_buf, so a
        // last arriver that read a stale partial (the previous launch's, left in a cache the sc0 sc1 read-back failed to bypass, or
        // a ticket that ran ahead of its data) produces the wrong words -- on identical operands it would have produced the right ones.
        const int mtt = 4;
        const size_t nx = (size_t)mtt * 16 * K, nh = (size_t)mtt * 16 * N;
        std::vector<float> hx(2 * nx), hw((size_t)K * N), hb(N), hh(2 * nh);
        unsigned sd = 12345u + (unsigned)M;
        auto rnd = [&] { sd = sd * 1664525u + 1013904223u; return (float)(sd >> 8) * (1.0f / 8388608.0f) - 1.0f; };
        for (auto& v : hx) v = rnd();
        for (auto& v : hw) v = 0.05f * rnd();
        for (auto& v : hb) v = 0.1f * rnd();
        for (auto& v : hh) v = rnd();
        DevBuf dx, dw, db, dh0, dh, dref, dcnt, dload, dsink, dsc, dbad;
        dx.upload(hx);
        dw.upload(hw);
        db.upload(hb);
        dh0.upload(hh);
        dh.ensure(nh * 4);
        dref.ensure(hh.size() * 4);
        zero_count(dcnt, c.st);
        GemmRowsArgs a{};
        a.prec = c.gpt_fp16 ? 2 : c.prec;   // aur_config.gpt_fp16: the fp16 decode copy and arithmetic of the per-layer GEMMs
        dbad.ensure(sizeof(int));
        std::vector<std::unique_ptr<DevBuf>> keep;
        const DecodeOperand op = prepare_decode_operand(a.prec, dw.as<float>(), N, nullptr, nullptr, db.as<float>(), K, N, nullptr, dbad.as<int>(),
                                                        dsc, keep, c.st);
        a.xmt = mtt; a.omt = mtt; a.Wt = op.Wt; a.M = M; a.N = N; a.K = K; a.bias = op.bias;
        // references: no scratch -> the UNSPLIT kernel, one per operand set
        HIP_CHECK(hipMemcpyAsync(dref.p, dh0.p, hh.size() * 4, hipMemcpyDeviceToDevice, c.st));
        for (int s = 0; s < 2; ++s) {
            a.X = dx.as<float>() + s * nx; a.out = dref.as<float>() + s * nh;
            launch_gemm_rows(a, false, kEpiResidual, c.st);
        }
        // background load on the low-priority stream for the whole test: 256 MiB streamed per launch by 1024 workgroups (256 KiB
        // each), a launch enqueued for every second split launch (~50 us of traffic against ~25 us per iteration), so that the
        // split kernel's workgroups start unevenly and its partials, tickets and read-backs share L2 and the fabric with other traffic
        const size_t load_bytes = (size_t)256 << 20;
        dload.zeros(load_bytes, c.st_lo);
        dsink.zeros(1024 * 4, c.st_lo);
        HIP_CHECK(hipStreamSynchronize(c.st));
        a.ksp_buf = c.ksp_buf; a.ksp_cnt = c.ksp_cnt;
        auto split_launch = [&](int s) {
            HIP_CHECK(hipMemcpyAsync(dh.p, dh0.as<float>() + s * nh, nh * 4, hipMemcpyDeviceToDevice, c.st));
            a.X = dx.as<float>() + s * nx; a.out = dh.as<float>();
            launch_gemm_rows(a, false, kEpiResidual, c.st);
        };
        for (int i = 0; i < iters; ++i) {
            const int s = i & 1;
            if ((i & 1) == 0)
                hipLaunchKernelGGL(stress_load_kernel, dim3(1024), dim3(256), 0, c.st_lo, dload.as<float4>(), dsink.as<float>(), (long)(load_bytes / 16));
            if (i % 3 == 2) {   // two split launches on DIFFERENT data with nothing between them but the residual copy: the counter reset
                split_launch(s ^ 1);   // and the scratch reuse are on the path; only the second one is checked
            }
            split_launch(s);
            launch_count_mismatch(dh.p, dref.as<float>() + s * nh, (long)nh, dcnt.as<unsigned long long>(), c.st);
        }
        HIP_CHECK(hipGetLastError());
        *mismatches_out = read_count(dcnt, c.st);
        HIP_CHECK(hipStreamSynchronize(c.st_lo));
    });
}
int aur_dbg_lane_xor_selftest(aur_engine* e, int32_t blocks, int64_t* mismatches_out) {
    CHECK_PTR(e);
    CHECK_PTR(mismatches_out);
    return guarded([&] {
        const DbgCtx c = use(e);
        AUR_REQUIRE(blocks >= 1 && blocks <= 4096, "lane_xor selftest: 1..4096 workgroups");
        DevBuf dcnt;
        zero_count(dcnt, c.st);
        launch_lane_xor_selftest(0x9E3779B9u, blocks, dcnt.as<unsigned long long>(), c.st);
        *mismatches_out = read_count(dcnt, c.st);
    });
}
int aur_dbg_paged_attention(aur_engine* e, const float* q, const float* k, const float* v, const int32_t* ctx, int32_t M, int32_t ctx_max,
                            int32_t shared, int32_t kv_half, float* out) {
    CHECK_PTR(e);
    CHECK_PTR(q);
    CHECK_PTR(k);
    CHECK_PTR(v);
    CHECK_PTR(ctx);
    CHECK_PTR(out);
    return guarded([&] {
        const DbgCtx c = use(e);
        AUR_REQUIRE(M >= 1 && M <= 256 && ctx_max >= 1 && ctx_max <= kMaxBlocks * kKvBlockTokens, "dbg_paged_attention: 1..256 rows, context 1..1056");
        AUR_REQUIRE(shared == 0 || shared == 16 || shared == 32, "dbg_paged_attention: shared prefix of 0, 16 or 32 tokens");
        for (int m = 0; m < M; ++m)
            AUR_REQUIRE(ctx[m] >= 1 && ctx[m] <= ctx_max && ctx[m] >= shared, "dbg_paged_attention: ctx[m] in [max(1, shared), ctx_max]");
        std::vector<int> rm((size_t)M * kRowMetaStride, 0);
        DevBuf dq, dpool, drm, dout;
        upload_kv_pool(k, v, M, ctx_max, shared, ctx, kv_half != 0, &rm[kRowMetaBt], kRowMetaStride, dpool);
        for (int m = 0; m < M; ++m) {
            int* r = &rm[(size_t)m * kRowMetaStride];
            r[0] = ctx[m] - 1;
            r[1] = m;
            r[kRowMetaWblk] = r[kRowMetaBt + (ctx[m] - 1) / kKvBlockTokens];
        }
        dq.upload(q, (size_t)M * kHidden * 4);
        drm.upload(rm);
        dout.ensure((size_t)M * kHidden * 4);
        launch_paged_attention(dq.as<float>(), dpool.p, drm.as<int>(), kMaxBlocks, dout.as<float>(), M, c.st, 0, kv_half != 0);
        download(out, dout, (size_t)M * kHidden * 4, c.st);
    });
}
int aur_dbg_prompt_attention(aur_engine* e, const float* q, const float* k, const float* v, const int32_t* row_seq, const int32_t* row_pos,
                             int32_t M, int32_t n_seq, int32_t ctx_max, int32_t shared, int32_t kv_half, float* out) {
    CHECK_PTR(e);
    CHECK_PTR(q);
    CHECK_PTR(k);
    CHECK_PTR(v);
    CHECK_PTR(row_seq);
    CHECK_PTR(row_pos);
    CHECK_PTR(out);
    return guarded([&] {
        const DbgCtx c = use(e);
        AUR_REQUIRE(M >= 1 && M <= 8192 && n_seq >= 1 && n_seq <= 64 && ctx_max >= 1 && ctx_max <= kMaxBlocks * kKvBlockTokens,
                    "dbg_prompt_attention: 1..8192 rows, 1..64 sequences, context 1..1056");
        AUR_REQUIRE(shared == 0 || shared == 16 || shared == 32, "dbg_prompt_attention: shared prefix of 0, 16 or 32 tokens");
        std::vector<int> bt((size_t)n_seq * kMaxBlocks, 0), rs(row_seq, row_seq + M), rp(row_pos, row_pos + M);
        DevBuf dq, dpool, dbt, drs, drp, dqb, dout;
        upload_kv_pool(k, v, n_seq, ctx_max, shared, nullptr, kv_half != 0, bt.data(), kMaxBlocks, dpool);
        for (int m = 0; m < M; ++m)
            AUR_REQUIRE(rs[m] >= 0 && rs[m] < n_seq && rp[m] >= 0 && rp[m] < ctx_max, "dbg_prompt_attention: row_seq / row_pos out of range");
        const std::vector<int2> qblk = prompt_qblocks(rs, rp);
        dqb.upload(qblk);
        dq.upload(q, (size_t)M * kHidden * 4);
        dbt.upload(bt);
        drs.upload(rs);
        drp.upload(rp);
        dout.ensure((size_t)M * kHidden * 4);
        launch_prompt_attention(dq.as<float>(), dpool.p, dqb.as<int2>(), (int)qblk.size(), drs.as<int>(), drp.as<int>(), dbt.as<int>(), kMaxBlocks,
                                dout.as<float>(), c.st, kv_half != 0);
        download(out, dout, (size_t)M * kHidden * 4, c.st);
    });
}
int aur_dbg_layernorm(aur_engine* e, const float* h, const float* gamma, const float* beta, float* out, int32_t M) {
    CHECK_PTR(e);
    return guarded([&] {
        const DbgCtx c = use(e);
        DevBuf dh, dg, db, dout;
        dh.upload(h, (size_t)M * kHidden * 4);
        dg.upload(gamma, kHidden * 4);
        db.upload(beta, kHidden * 4);
        dout.ensure((size_t)M * kHidden * 4);
        launch_rows_ln(nullptr, 0, nullptr, dh.as<float>(), dg.as<float>(), db.as<float>(), dout.as<float>(), M, 1e-5f, c.st);
        download(out, dout, (size_t)M * kHidden * 4, c.st);
    });
}
int aur_dbg_conv1d(aur_engine* e, const float* x, const float* wp, const float* bias, const float* res, float* out,
                   const int32_t* lens, int32_t B, int32_t Cin, int32_t Mtot, int32_t Cout, int32_t L, int32_t KS,
                   int32_t DIL, int32_t padl, float slope, int32_t ups_s, int32_t ups_p) {
    CHECK_PTR(e);
    return guarded([&] { run_conv_plain(e, false, x, wp, bias, res, out, lens, B, Cin, Mtot, Cout, L, KS, DIL, padl, slope, ups_s, ups_p); });
}
int aur_dbg_conv1d_f16(aur_engine* e, const float* x, const void* wp16, const float* bias, const float* res, float* out,
                       const int32_t* lens, int32_t B, int32_t Cin, int32_t Mtot, int32_t Cout, int32_t L, int32_t KS,
                       int32_t DIL, int32_t padl, float slope, int32_t ups_s, int32_t ups_p) {
    CHECK_PTR(e);
    return guarded([&] { run_conv_plain(e, true, x, wp16, bias, res, out, lens, B, Cin, Mtot, Cout, L, KS, DIL, padl, slope, ups_s, ups_p); });
}
// One ConvArgs launch as the engine would fill it (run_conv).  The storage flags come from conv_storage, so two arguments only carry what
// the engine's rule leaves open: out_slope is used where the output is stored as activated halves, and res_unact is not read at all (a
// halves residual is un-activated with the engine's 1 / 0.1).
int aur_dbg_conv1d_args(aur_engine* e, int32_t variant, const float* x, const void* w, const float* bias, const float* cond,
                        const int32_t* cond_row, int32_t cond_rows, int32_t cond_stride, const float* res, float* mrf, float* out,
                        const int32_t* lens, int32_t B, int32_t Cin, int32_t Mtot, int32_t Cout, int32_t L, int32_t KS, int32_t DIL,
                        int32_t padl, float slope, int32_t ups_s, int32_t ups_p, int32_t mrf_mode, float out_slope, float res_unact,
                        float guard_value, int64_t* guard_changed) {
    CHECK_PTR(e);
    CHECK_PTR(x);
    CHECK_PTR(w);
    CHECK_PTR(lens);
    CHECK_PTR(guard_changed);
    return guarded([&] {
        const DbgCtx c = use(e);
        AUR_REQUIRE(variant >= 0 && variant <= 2, "dbg_conv1d_args: variant in {0,1,2}");
        AUR_REQUIRE(mrf_mode >= 0 && mrf_mode <= 3 && Cin >= 1 && Cout >= 1 && Mtot >= 1 && KS >= 1 && ups_s >= 0, "dbg_conv1d_args: shapes");
        AUR_REQUIRE(Mtot == Cout * std::max(1, ups_s), "dbg_conv1d_args: Mtot = Cout * max(1, ups_s) virtual channels");
        AUR_REQUIRE(ups_s == 0 || (mrf_mode == 0 && !res), "dbg_conv1d_args: no residual or MRF on a transposed conv");
        AUR_REQUIRE(mrf_mode == 0 || mrf, "dbg_conv1d_args: the MRF modes need mrf");
        AUR_REQUIRE((mrf_mode == 1 || mrf_mode == 2) || out, "dbg_conv1d_args: modes 0 and 3 need out");
        check_lens(lens, B, L, "dbg_conv1d_args: 1 <= lens[b] <= L = max(lens)");
        if (cond) {
            AUR_REQUIRE(cond_row && cond_rows >= 1 && cond_stride >= Cout, "dbg_conv1d_args: cond needs cond_row and cond_stride >= Cout");
            for (int b = 0; b < B; ++b) AUR_REQUIRE(cond_row[b] >= 0 && cond_row[b] < cond_rows, "dbg_conv1d_args: cond_row out of range");
        }
        const bool half = variant != 0;
        // on halves KS == 2 is the transposed convs (out_act_f16 alone): a plain k = 2 conv would read a halves residual as floats
        AUR_REQUIRE(!half || KS != 2 || ups_s > 0, "dbg_conv1d_args: KS == 2 on interleaved halves is a transposed conv (ups_s > 0)");
        *guard_changed = run_conv(c, variant_layout(variant), x, w, bias, cond, cond_row, cond_rows, cond_stride, res, mrf, out, lens, B, Cin, Mtot,
                                  Cout, L, KS, DIL, padl, slope, ups_s, ups_p, mrf_mode, out_slope, guard_value);
    });
}
int aur_dbg_resblock_round_f16(aur_engine* e, const float* y, const void* w1, const void* w2, const float* b1, const float* b2,
                               float* mrf, float* out, const int32_t* lens, int32_t B, int32_t C, int32_t L, int32_t KS, int32_t DIL,
                               int32_t mrf_mode, float e_slope, float guard_value, int64_t* guard_changed) {
    CHECK_PTR(e);
    CHECK_PTR(y);
    CHECK_PTR(w1);
    CHECK_PTR(w2);
    CHECK_PTR(b1);
    CHECK_PTR(b2);
    CHECK_PTR(lens);
    CHECK_PTR(guard_changed);
    return guarded([&] {
        const DbgCtx c = use(e);
        AUR_REQUIRE((C == 64 || C == 32) && KS >= 1 && mrf_mode >= 0 && mrf_mode <= 3, "dbg_resblock_round: 64 or 32 channels, mode 0..3");
        AUR_REQUIRE(mrf_mode == 0 || mrf, "dbg_resblock_round: the MRF modes need mrf");
        AUR_REQUIRE((mrf_mode == 1 || mrf_mode == 2) || out, "dbg_resblock_round: modes 0 and 3 need out");
        check_lens(lens, B, L, "dbg_resblock_round: 1 <= lens[b] <= L = max(lens)");
        const size_t wbytes = (size_t)C * C * KS * 2;
        DevBuf dw1, dw2, db1, db2, dl, dz;
        GuardedBuf gy, gm, go;   // y between guards too: with out == y it is the output tensor the launcher is handed
        gy.upload(y, B, C, L, true, guard_value);
        dw1.upload(w1, wbytes);
        dw2.upload(w2, wbytes);
        db1.upload(b1, (size_t)C * 4);
        db2.upload(b2, (size_t)C * 4);
        dl.upload(lens, (size_t)B * 4);
        dz.zeros(256, c.st);
        RoundArgs a{};
        a.y = gy.data();
        a.w1 = dw1.p; a.w2 = dw2.p; a.b1 = db1.as<float>(); a.b2 = db2.as<float>();
        a.base_len = dl.as<int>(); a.len_mul = 1;
        a.stride = L; a.bstride = (long)C * L;
        a.C = C;
        a.B = B; a.max_len = L;
        a.zeros = dz.p;
        const bool has_out = mrf_mode == 0 || mrf_mode == 3, aliased = has_out && out == y;
        if (mrf_mode != 0) gm.upload(mrf, B, C, L, true, guard_value);
        if (has_out && !aliased) go.upload(out, B, C, L, true, guard_value);
        void* dout = !has_out ? nullptr : aliased ? gy.data() : go.data();
        round_outputs(a, mrf_mode, dout, mrf_mode != 0 ? gm.data() : nullptr, dout, e_slope);
        launch_resblock_round_f16(a, KS, DIL, c.st);
        long long bad = 0;
        if (mrf_mode != 0) bad += gm.download(mrf, c.st);
        if (has_out) bad += (aliased ? gy : go).download(out, c.st);
        *guard_changed = bad;
    });
}
int aur_dbg_interp2(aur_engine* e, const float* lat, const int32_t* lat_row, const int32_t* n_lat, int32_t R, int32_t n_max, int32_t B,
                    int32_t C, int32_t Lz, int32_t out_f16, float* z, float guard_value, int64_t* guard_changed) {
    CHECK_PTR(e);
    CHECK_PTR(lat);
    CHECK_PTR(n_lat);
    CHECK_PTR(z);
    CHECK_PTR(guard_changed);
    return guarded([&] {
        const DbgCtx c = use(e);
        AUR_REQUIRE(R >= 1 && n_max >= 1 && B >= 1 && C >= 8 && C % 8 == 0, "dbg_interp2: shapes (channels in whole groups of 8)");
        std::vector<int> len(B);
        for (int b = 0; b < B; ++b) {
            AUR_REQUIRE(n_lat[b] >= 1 && n_lat[b] <= n_max, "dbg_interp2: 1 <= n_lat[b] <= n_max");
            AUR_REQUIRE(lat_row ? (lat_row[b] >= 0 && lat_row[b] < R) : b < R, "dbg_interp2: lat_row out of range");
            len[b] = frames_for(n_lat[b]);
        }
        check_lens(len.data(), B, Lz, "dbg_interp2: Lz = frames_for(max n_lat)");
        DevBuf dlat, drow, dn, dl;
        GuardedBuf gz;
        dlat.upload(lat, (size_t)R * n_max * C * 4);
        if (lat_row) drow.upload(lat_row, (size_t)B * 4);
        dn.upload(n_lat, (size_t)B * 4);
        dl.upload(len);
        gz.upload(z, B, C, Lz, out_f16 != 0, guard_value);
        launch_interp2(dlat.as<float>(), (long)n_max * C, drow.as<int>(), dn.as<int>(), dl.as<int>(), reinterpret_cast<float*>(gz.data()), Lz,
                       (long)C * Lz, C, B, Lz, c.st, out_f16 != 0);
        *guard_changed = gz.download(z, c.st);
    });
}
int aur_dbg_interp3(aur_engine* e, const float* lat, const int32_t* lat_row, const int32_t* n_lat, const float* speed, int32_t R,
                    int32_t n_max, int32_t B, int32_t C, int32_t Lz, int32_t out_f16, float* z, float guard_value, int64_t* guard_changed) {
    CHECK_PTR(e);
    CHECK_PTR(lat);
    CHECK_PTR(n_lat);
    CHECK_PTR(speed);
    CHECK_PTR(z);
    CHECK_PTR(guard_changed);
    return guarded([&] {
        const DbgCtx c = use(e);
        AUR_REQUIRE(R >= 1 && n_max >= 1 && B >= 1 && C >= 8 && C % 8 == 0, "dbg_interp3: shapes (channels in whole groups of 8)");
        std::vector<int> len(B), l0(B);
        std::vector<float> r0(B);
        for (int b = 0; b < B; ++b) {
            AUR_REQUIRE(n_lat[b] >= 1 && n_lat[b] <= n_max, "dbg_interp3: 1 <= n_lat[b] <= n_max");
            AUR_REQUIRE(lat_row ? (lat_row[b] >= 0 && lat_row[b] < R) : b < R, "dbg_interp3: lat_row out of range");
            AUR_REQUIRE(speed_valid(speed[b]), "dbg_interp3: speed 0 (unset) or in [0.5, 2]");
            l0[b] = stretched_rows(n_lat[b], speed[b]);
            r0[b] = stretch_ratio(speed[b]);
            len[b] = frames_for(l0[b]);
        }
        check_lens(len.data(), B, Lz, "dbg_interp3: Lz = frames_for(max stretched rows)");
        DevBuf dlat, drow, dn, dl0, dr0, dl;
        GuardedBuf gz;
        dlat.upload(lat, (size_t)R * n_max * C * 4);
        if (lat_row) drow.upload(lat_row, (size_t)B * 4);
        dn.upload(n_lat, (size_t)B * 4);
        dl0.upload(l0);
        dr0.upload(r0);
        dl.upload(len);
        gz.upload(z, B, C, Lz, out_f16 != 0, guard_value);
        launch_interp3(dlat.as<float>(), (long)n_max * C, drow.as<int>(), dn.as<int>(), dl0.as<int>(), dr0.as<float>(), dl.as<int>(),
                       reinterpret_cast<float*>(gz.data()), Lz, (long)C * Lz, C, B, Lz, c.st, out_f16 != 0);
        *guard_changed = gz.download(z, c.st);
    });
}
int aur_dbg_conv_post(aur_engine* e, const float* x, const float* w, const int32_t* lens, int32_t B, int32_t Cin, int32_t L, float slope,
                      int32_t x_f16_act, float* wav, float guard_value, int64_t* guard_changed) {
    CHECK_PTR(e);
    CHECK_PTR(x);
    CHECK_PTR(w);
    CHECK_PTR(lens);
    CHECK_PTR(wav);
    CHECK_PTR(guard_changed);
    return guarded([&] {
        const DbgCtx c = use(e);
        AUR_REQUIRE(Cin >= 1, "dbg_conv_post: shapes");
        check_lens(lens, B, L, "dbg_conv_post: 1 <= lens[b] <= L = max(lens)");
        DevBuf dx, dw, dl;
        GuardedBuf gw;
        if (x_f16_act) {
            AUR_REQUIRE(Cin % 16 == 0, "dbg_conv_post: interleaved halves need whole 16-channel chunks");
            dx.upload(to_halves(x, B, Cin, L));
        } else {
            dx.upload(x, (size_t)B * Cin * L * 4);
        }
        dw.upload(w, (size_t)Cin * 7 * 4);
        dl.upload(lens, (size_t)B * 4);
        gw.upload(wav, B, 1, L, false, guard_value);
        launch_conv_post(dx.as<float>(), dw.as<float>(), reinterpret_cast<float*>(gw.data()), dl.as<int>(), 1, Cin, L, (long)Cin * L, L, slope,
                         B, L, c.st, x_f16_act != 0);
        *guard_changed = gw.download(wav, c.st);
    });
}
int aur_dbg_resample_out(aur_engine* e, const float* x, const int32_t* lens, const int32_t* rate, int32_t B, int32_t L, float* out,
                         int32_t Lout, float guard_value, int64_t* guard_changed) {
    CHECK_PTR(e);
    CHECK_PTR(x);
    CHECK_PTR(lens);
    CHECK_PTR(rate);
    CHECK_PTR(out);
    CHECK_PTR(guard_changed);
    return guarded([&] {
        const DbgCtx c = use(e);
        check_lens(lens, B, L, "dbg_resample_out: 1 <= lens[b] <= L = max(lens)");
        std::vector<int> cls(B), n_out(B);
        for (int b = 0; b < B; ++b) {
            cls[b] = rate_class(rate[b]);
            AUR_REQUIRE(cls[b] >= 0, "dbg_resample_out: rate 0 (unset) or one of 8000, 16000, 22050, 24000, 32000, 44100, 48000");
            n_out[b] = (int)resampled_len(lens[b], cls[b]);
        }
        check_lens(n_out.data(), B, Lout, "dbg_resample_out: Lout = the longest output");
        // the kernel stages with 16-byte loads: rows of whole float4s on the device, as the engine's staging buffer has them
        const long Ld = (L + 3) & ~3L;
        std::vector<float> xd((size_t)B * Ld, 0.f);
        for (int b = 0; b < B; ++b) std::copy(x + (size_t)b * L, x + (size_t)(b + 1) * L, xd.begin() + (size_t)b * Ld);
        DevBuf dx, dl, dc, dt;
        GuardedBuf go;
        dx.upload(xd);
        dl.upload(lens, (size_t)B * 4);
        dc.upload(cls);
        dt.upload(resample_table());
        go.upload(out, B, 1, Lout, false, guard_value);
        launch_resample_out(dx.as<float>(), Ld, dl.as<int>(), 1, dc.as<int>(), dt.as<int>(), reinterpret_cast<float*>(go.data()), Lout, B, Lout,
                            c.st);
        *guard_changed = go.download(out, c.st);
    });
}
int aur_dbg_flac_encode(aur_engine* e, const float* x, const int32_t* lens, const int32_t* rates, int32_t B, int64_t stride, uint8_t* out,
                        int64_t out_stride, int32_t* out_lens) {
    CHECK_PTR(e);
    CHECK_PTR(x);
    CHECK_PTR(lens);
    CHECK_PTR(rates);
    CHECK_PTR(out);
    CHECK_PTR(out_lens);
    return guarded([&] {
        const DbgCtx c = use(e);
        AUR_REQUIRE(B >= 1 && stride >= 1, "dbg_flac_encode: shapes");
        for (int b = 0; b < B; ++b) AUR_REQUIRE(lens[b] >= 1 && lens[b] <= stride, "dbg_flac_encode: 1 <= lens[b] <= stride");
        // guard | out rows (the caller's bytes) | guard
        const uint8_t guard = 0xA5;
        const size_t body = (size_t)B * out_stride;
        std::vector<uint8_t> img(2 * kGuardBytes + body, guard);
        std::memcpy(img.data() + kGuardBytes, out, body);
        DevBuf dx, dout, dlen;
        dx.upload(x, (size_t)B * stride * 4);
        dout.upload(img);
        dlen.ensure((size_t)B * 4);
        FlacEncoder enc;
        enc.encode(dx.as<float>(), stride, nullptr, std::vector<int>(lens, lens + B), std::vector<int>(rates, rates + B), dout.as<uint8_t>() + kGuardBytes,
                   out_stride, dlen.as<int>(), c.st_lo);
        download(img.data(), dout, img.size(), c.st_lo);
        HIP_CHECK(hipMemcpy(out_lens, dlen.p, (size_t)B * 4, hipMemcpyDeviceToHost));
        std::memcpy(out, img.data() + kGuardBytes, body);
        for (size_t i = 0; i < kGuardBytes; ++i)
            if (img[i] != guard || img[kGuardBytes + body + i] != guard) throw HipError("dbg_flac_encode: a guard byte around the output rows changed");
    });
}

}  // extern "C"
