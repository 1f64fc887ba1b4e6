// Kernel test harness: the aur_dbg_* entry points of include/auralis_amd.h that run ONE kernel on host arrays (tests/test_gpu_kernels.py,
// test_gpu_gpt.py, test_gpu_gpt_fp16.py).  They take from the engine its streams, its arithmetic mode and the K-split scratch (DbgCtx)
// and nothing else; aur_dbg_prefill and aur_dbg_sample drive real engine state and live in engine.hip.
#include <algorithm>
#include <cstring>

#include "abi_internal.h"
#include "gpt_host.h"
#include "vocoder_kernels.h"

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

static void dbg_conv1d(const aur_engine* e, const float* x, const void* wp, const float* bias, const float* res, float* out, const int* lens,
                       int B, int Cin, int Mtot, int Cout, int L, int KS, int DIL, int padl, float slope, int ups_s, int ups_p, bool f16) {
    const DbgCtx c = use(e);
    const int Lout = L * std::max(1, ups_s);
    const size_t n_out = (size_t)B * Cout * Lout * 4;
    DevBuf dx, dw, db, dr, dout, dl;
    dx.upload(x, (size_t)B * Cin * L * 4);
    dw.upload(wp, (size_t)Mtot * Cin * KS * (f16 ? 2 : 4));
    dl.upload(lens, (size_t)B * 4);
    dout.zeros(n_out, c.st);
    if (bias) db.upload(bias, (size_t)Cout * 4);
    if (res) dr.upload(res, n_out);
    ConvArgs a{};
    a.x = dx.as<float>();
    a.wp = dw.as<float>();
    a.wp16 = dw.p;
    a.bias = db.as<float>();
    a.res = dr.as<float>();
    a.out = dout.as<float>();
    a.base_len = dl.as<int>();
    a.len_mul = 1;
    a.Cin = Cin; a.Mtot = Mtot; a.Cout = Cout;
    a.x_stride = L; a.o_stride = Lout;
    a.x_bstride = (long)Cin * L; a.o_bstride = (long)Cout * Lout;
    a.padl = padl; a.slope = slope; a.ups_s = ups_s; a.ups_p = ups_p;
    a.max_len = *std::max_element(lens, lens + B);
    a.B = B;
    if (f16)
        launch_conv1d_f16(a, KS, DIL, c.st);
    else
        launch_conv1d(a, KS, DIL, c.st);
    download(out, dout, n_out, c.st);
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
    return guarded([&] { dbg_conv1d(e, x, wp, bias, res, out, lens, B, Cin, Mtot, Cout, L, KS, DIL, padl, slope, ups_s, ups_p, false); });
}
int aur_dbg_conv1d_f16(aur_engine* e, const float* x, const void* wp16, const float* bias, const float* res, float* out,
                       const int32_t* lens, int32_t B, int32_t Cin, int32_t Mtot, int32_t Cout, int32_t L, int32_t KS,
                       int32_t DIL, int32_t padl, float slope, int32_t ups_s, int32_t ups_p) {
    CHECK_PTR(e);
    return guarded([&] { dbg_conv1d(e, x, wp16, bias, res, out, lens, B, Cin, Mtot, Cout, L, KS, DIL, padl, slope, ups_s, ups_p, true); });
}

}  // extern "C"
