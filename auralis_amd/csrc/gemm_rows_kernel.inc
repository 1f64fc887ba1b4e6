// Body of the decode-regime GEMM kernel (see gpt_kernels.h).  Included by gpt_kernels.hip (the product instantiation) and by
// tools/gemm_bench.hip (a second instantiation with the tile loads and MFMAs compiled out: the fixed cost of a launch).  The
// includer sits inside namespace aur and defines
//     AUR_GR_NAME      the kernel template's name
//     AUR_GR_LAUNCH    the name of the host launcher (signature of launch_gemm_rows, gpt_kernels.h) defined at the end of this file
//     AUR_GR_NO_DATA   0: the kernel;  1: the same launch without its weight / activation tile loads and without its MFMAs
//     AUR_GR_LN_EARLY  (optional, default 0) 0: the rows' LayerNorm partials are requested behind the first tile loads and combined
//                      after the last MFMA; 1: they are the first request of the launch and are combined while the tile loads are in
//                      flight.  Same box, same run (tools/gemm_bench.sh with GEMM_BENCH_VARIANT, profiles/r05_gemm_bench_ln_early_ab.log):
//                      chain of 30 layers 33.0-33.3 us per layer with 1, 33.1 with 0; QKV 7.81 / 8.05, FC 9.2-9.3 / 9.1 -- neutral:
//                      the combination is 0.1 us of DPP arithmetic and the wave that finishes its MFMAs first hides it.
#ifndef AUR_GR_LN_EARLY
#define AUR_GR_LN_EARLY 0
#endif
//
// What a launch waits for before its first weight byte is on the way (round 5; DESIGN section 3 item 7).  Until round 4 the kernel
// took one by-value GemmRowsArgs, and hipcc sinks every kernel-argument fetch to its first use: the ISA had three to four
// DEPENDENT scalar round trips to the kernarg segment (s_load -> s_waitcnt lgkmcnt(0) -> s_load ...) in front of the first
// global_load_dwordx4.  Now
//   * everything the tile addresses need (Wt, X, M, N, xmt) and the epilogue inputs that can be requested at once (bias, c1, the
//     residual element, the rows' LayerNorm partials) are the LEADING SCALAR ARGUMENTS -- 14 dwords (the four small integers packed
//     into two), which the build's -amdgpu-kernarg-preload-count=16 has the command processor place in SGPRs before the wave starts
//     (.amdhsa_user_sgpr_kernarg_preload_length 14): no fetch at all.  K is not an argument: it is 1024 * KCH;
//   * the rest (GemmRowsTail) is read in ONE burst behind the first chunk's tile loads and pinned there by an asm statement, so it
//     costs one scalar round trip that runs under the tile loads instead of in front of them;
//   * no branch sits between the loads (bias is required; the launcher checks), so the counted waits of the MFMA blocks stay exact.
// tests/test_isa_prologue.py holds the compiled kernel to this: no s_waitcnt lgkmcnt in front of the first tile load.
template <int MT, int KCH, bool LN, int EPI, int NW, int NTL = 1, int PREC = 0, bool NT = false, int KSP = 1>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(1, NW == 16 ? 4 : (NW == 8 ? 6 : (KSP > 1 ? 2 : 8)))))
void AUR_GR_NAME(const float* __restrict__ Wt_, const float* X_, const float* bias, const float* ln_c1, float* out, const float2* stats_in,
                 unsigned mn, unsigned mts, GemmRowsTail tl) {
    // (five pointers and the LayerNorm statistics pointer fill 12 of the 14 preloaded dwords; the four small integers share two:
    // mn = M | (column tiles of the grid = N / (16 NTL)) << 16, mts = xmt | omt << 16)
    const int M = (int)(mn & 0xffffu), n_tiles = (int)(mn >> 16), xmt = (int)(mts & 0xffffu), omt = (int)(mts >> 16);
    // (amdgpu_waves_per_eu: without the cap hipcc schedules for 8 waves per SIMD — 64 VGPRs — and gets there by issuing the tile
    // loads two at a time between the MFMAs: 5-7 dependent memory round trips per launch instead of one.  A 16-wave workgroup
    // occupies 4 waves per SIMD anyway.)
    // NTL = 16-column tiles per workgroup (each wave keeps MT x NTL accumulator tiles): the activation rows a CU pulls through
    // its L1 are shared by NTL column tiles; the K order of every output element is the same for every NTL (bitwise equal)
    static_assert(!LN || KCH == 1, "LN prologue needs the whole row in one chunk");
    static_assert(NW == 4 || NW == 8 || NW == 16, "waves per workgroup");
    static_assert(KSP == 1 || (!LN && MT == 1 && NTL == 1 && NW * KSP == 16), "K split: 16 slices, one 16 x 16 tile, no LayerNorm fold");
    constexpr int K = 1024 * KCH;
    constexpr int NB = 64 / (NW * KSP);   // 16-deep K blocks per wave per 1024-deep chunk
    constexpr bool kData = !(AUR_GR_NO_DATA);
    __shared__ __attribute__((aligned(16))) float red[NW][MT * NTL * 256];
    __shared__ float rs[LN ? 16 * MT : 1][2];   // (mean, rstd) of the workgroup's rows
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wg = KSP > 1 ? (int)blockIdx.z * NW + w : w;   // this wave's K-slice among the NW * KSP slices
    // workgroup -> (column tile, row group) = (blockIdx.x, blockIdx.y).  Workgroups are dealt to the 8 XCDs round-robin in dispatch
    // order (x fastest) and the grid's x extent is a multiple of 8, so every row group (and every K part) of a column tile lands on
    // XCD x % 8: the tile's weights leave HBM once and the other groups hit them in that XCD's L2; the whole grid is resident at
    // once (one workgroup per CU), so they also run at the same time.  (Until round 5 the pair was decoded from a linear id with an
    // integer division by the runtime number of row groups -- thirty instructions of the 86 a wave executed, out of an instruction
    // cache that is COLD at every launch, before its first tile load; DESIGN section 3 item 7.)
    const int ntile = blockIdx.x, mgrp = blockIdx.y;
    // (the grid is padded to a multiple of 8 column tiles: the mel head has 68, and with the plain order its four row
    // groups landed on four XCDs and pulled the weights from HBM four times: PMC 18.7 MB per launch for 4.5 MB of weights)
    if (ntile >= n_tiles) return;
    const int n0 = ntile * 16 * NTL, m0 = mgrp * 16 * MT;
    // 16-byte pieces of one packed 16-column tile: a float4 per lane and K block (pack_wt16), or for PREC 2 eight fp16 per lane and
    // K-block pair (pack_wt16_f16: the same 8 values the PREC 1 split takes from the float4s of blocks 2p, 2p + 1)
    constexpr long wt_tile = PREC == 2 ? (long)(K >> 5) * 64 : (long)(K >> 4) * 64;
    const f32x4* wt = reinterpret_cast<const f32x4*>(Wt_) + (long)ntile * NTL * wt_tile + lane;
    // packed rows: the float4 of lane `lane` for (16-row tile t, K block kb) is at ((kb * xmt + t) * 64 + lane); rows >= M of
    // the last tiles are allocated but undefined: their products stay in their own (never stored) output rows
    const f32x4* xp = reinterpret_cast<const f32x4*>(X_) + (long)(mgrp * MT) * 64 + lane;
    // K = 4096: two chunk buffers (the loads run one 1024-deep chunk ahead of the MFMAs).  Three buffers measured slower
    // (13.6 vs 12.3 us at M = 64).
    constexpr int NBUF = (KCH > 1) ? 2 : 1;
    static_assert(PREC >= 0 && PREC <= 2 && NB % 2 == 0, "arithmetic; PREC 1 / 2 take K blocks in pairs");
    constexpr int NBW = PREC == 2 ? NB / 2 : NB;   // weight pieces per wave and chunk
    f32x4 bf[NBUF][NTL][NBW], af[NBUF][MT][NB];
    // loads in K-block order (for PREC 1 and 2 in pairs of blocks; PREC 2: the pair's weight piece with the first block): the MFMAs
    // of block b need exactly the first (b + 1) / NB of the chunk's loads, and loads return in order
    auto load_chunk = [&](int c, int buf) {
        const int kb0 = c * 64 + NB * wg;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (PREC != 2 || !(b & 1)) {
                const int bw = PREC == 2 ? b >> 1 : b;
                const long off = PREC == 2 ? (long)((kb0 + b) >> 1) * 64 : (long)(kb0 + b) * 64;
#pragma unroll
                for (int t = 0; t < NTL; ++t) {
                    if constexpr (NT) bf[buf][t][bw] = __builtin_nontemporal_load(&wt[t * wt_tile + off]);
                    else bf[buf][t][bw] = wt[t * wt_tile + off];
                }
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) af[buf][mt][b] = xp[((long)(kb0 + b) * xmt + mt) * 64];
            if (PREC == 0 || (b & 1)) __builtin_amdgcn_sched_barrier(0);   // (hipcc reorders the loads among themselves otherwise)
        }
        // nothing below may move above this line and no load above may sink below it (hipcc otherwise sinks the tile loads
        // under the LayerNorm barrier and next to their first use)
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    // LayerNorm is folded into the weights (launch_fold_ln): the MFMAs run on the raw rows, nothing in front of them waits
    // for the statistics or for the other waves, and the epilogue applies  y = rstd * (x W' - mean * c1) + c2.  The partials
    // of the rows this wave will combine (rows w, w + NW, ...; lane t holds column tile t) are requested with the epilogue inputs,
    // behind the first tile loads (stats_in is preloaded; AUR_GR_LN_EARLY above: in front of them measured the same).
    constexpr int RPW = LN ? (16 * MT + NW - 1) / NW : 1;   // rows per wave
    float2 pt[RPW];
    auto load_pt = [&] {
#pragma unroll
        for (int u = 0; u < RPW; ++u) pt[u] = stats_in[(long)(m0 + min(w + NW * u, 16 * MT - 1)) * 64 + lane];
    };
    auto combine_pt = [&](float eps_) {   // Chan's combination of the 64 tile partials of a row, fixed order (one DPP wave reduction each)
#pragma unroll
        for (int u = 0; u < RPW; ++u) {
            const int rr = w + NW * u;
            const float mu = wave_sum_dpp(pt[u].x) * (1.0f / 64.0f);
            const float d = pt[u].x - mu;
            const float m2 = wave_sum_dpp(fmaf(16.0f * d, d, pt[u].y));
            if (lane == 0 && rr < 16 * MT) {
                rs[rr][0] = mu;
                rs[rr][1] = 1.0f / sqrtf(m2 * (1.0f / 1024.0f) + eps_);
            }
        }
    };
    if (LN && AUR_GR_LN_EARLY) load_pt();
    // The tile loads go out next: with a cold instruction cache every line of code in front of them is a miss the whole chip waits for.
    if constexpr (kData) load_chunk(0, 0);
    // Epilogue inputs that need nothing but the preloaded arguments next: one output element per thread (e = tid), so its bias, c1,
    // residual value and (LN) the row statistics it will combine are known now.  They arrive under the operands instead of costing
    // dependent memory round trips after the reduction.
    constexpr int NE = MT * NTL * 256;
    static_assert(NE <= 64 * NW, "one output element per thread");
    const int e = min(tid, NE - 1);
    const int ect = (e >> 8) / MT, emt = (e >> 8) - ect * MT;
    const int em = m0 + 16 * emt + 4 * ((e & 63) >> 4) + ((e >> 6) & 3), en = n0 + 16 * ect + (e & 15);
    const float ebias = bias[en];
    float ec1 = 0.f;
    if (LN) ec1 = ln_c1[en];
    float* eptr = nullptr;
    float eres = 0.f;
    if (EPI == kEpiResidual) {
        eptr = out + pk_off(em, en, omt);
        eres = *eptr;
    }
    if (LN && !AUR_GR_LN_EARLY) load_pt();
    __builtin_amdgcn_sched_barrier(0);
    // ---- the rest of the arguments: one burst of scalar loads, one wait, under the tile loads
    // (inputs only: a pointer that comes OUT of an asm statement has lost its address space, and the loads through it compile to
    // FLAT loads, after which every counted wait becomes vmcnt(0))
    float2* const stats_out = tl.stats_out;
    const int* const row_meta = tl.row_meta;
    void* const kv_layer = tl.kv_layer;
    float* const ksp_buf = tl.ksp_buf;
    unsigned* const ksp_cnt = tl.ksp_cnt;
    const float eps = tl.eps;
    const int ldo = tl.ldo, kv_half = tl.kv_half, gelu_erf_form = tl.gelu_erf;
    asm volatile("; GemmRowsTail resident" ::"s"(stats_out), "s"(row_meta), "s"(kv_layer), "s"(ksp_buf), "s"(ksp_cnt), "s"(eps),
                 "s"(ldo), "s"(kv_half), "s"(gelu_erf_form));
    f32x4 acc[MT][NTL], lo[PREC ? MT : 1][PREC ? NTL : 1];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int t = 0; t < NTL; ++t) {
            acc[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (PREC) lo[mt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    int epos = 0, eblk = 0;
    if (EPI == kEpiQkv) {   // where this thread's K / V element goes (embed_decode_kernel's dense per-row table)
        epos = row_meta[(long)em * kRowMetaStride];
        eblk = row_meta[(long)em * kRowMetaStride + kRowMetaWblk];
    }
    __builtin_amdgcn_sched_barrier(0);
    if (LN && AUR_GR_LN_EARLY) {   // under the tile loads
        combine_pt(eps);
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (kData) {
#pragma unroll
        for (int c = 0; c < KCH; ++c) {
            const int cur = c % NBUF;
            // (NBUF == 1: chunk 0 is already in flight; round 2 re-issued it here, which made the loads above dead and put the
            // real ones behind the LayerNorm barrier: one extra memory round trip per LN launch)
            if (NBUF > 1 && c + NBUF - 1 < KCH) load_chunk(c + NBUF - 1, (c + NBUF - 1) % NBUF);
            if (!LN) __builtin_amdgcn_sched_barrier(0);   // the next chunks' loads are issued before this chunk's MFMAs
#pragma unroll
            for (int b = 0; b < NB; b += (PREC ? 2 : 1)) {
                if constexpr (PREC == 0) {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int t = 0; t < NTL; ++t)
#pragma unroll
                            for (int mt = 0; mt < MT; ++mt)
                                acc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[cur][mt][b][s], bf[cur][t][b][s], acc[mt][t], 0, 0, 0);
                } else if constexpr (PREC == 2) {
                    bf16x8 ah[MT], am[MT], al[MT];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) split3_bf16(af[cur][mt][b], af[cur][mt][b + 1], ah[mt], am[mt], al[mt]);
#pragma unroll
                    for (int t = 0; t < NTL; ++t) {
                        bf16x8 wh, wl;
                        split2_f16(bf[cur][t][b >> 1], wh, wl);
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
                            lo[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[mt], wl, lo[mt][t], 0, 0, 0);
                            lo[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[mt], wh, lo[mt][t], 0, 0, 0);
                            lo[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], wl, lo[mt][t], 0, 0, 0);
                            lo[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[mt], wh, lo[mt][t], 0, 0, 0);
                            acc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], wh, acc[mt][t], 0, 0, 0);
                        }
                    }
                } else {
                    bf16x8 ah[MT], am[MT], al[MT];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) split3_bf16(af[cur][mt][b], af[cur][mt][b + 1], ah[mt], am[mt], al[mt]);
#pragma unroll
                    for (int t = 0; t < NTL; ++t) {
                        bf16x8 bh, bm, bl;
                        split3_bf16(bf[cur][t][b], bf[cur][t][b + 1], bh, bm, bl);
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
                            lo[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], bl, lo[mt][t], 0, 0, 0);
                            lo[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[mt], bh, lo[mt][t], 0, 0, 0);
                            lo[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[mt], bm, lo[mt][t], 0, 0, 0);
                            lo[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], bm, lo[mt][t], 0, 0, 0);
                            lo[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[mt], bh, lo[mt][t], 0, 0, 0);
                            acc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[mt], bh, acc[mt][t], 0, 0, 0);
                        }
                    }
                }
                // keep the blocks in load order: hipcc otherwise hoists the LayerNorm arithmetic of every block in front of the
                // first MFMA, which then waits for (almost) the whole tile
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if (LN && !AUR_GR_LN_EARLY) combine_pt(eps);
    // D layout: row = 4*(lane>>4) + r, col = lane&15
#pragma unroll
    for (int t = 0; t < NTL; ++t)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                red[w][(t * MT + mt) * 256 + r * 64 + lane] = PREC ? acc[mt][t][r] + lo[mt][t][r] : acc[mt][t][r];
    __syncthreads();
    if constexpr (KSP > 1) {
        // publish this workgroup's NW partial tiles (thread e: element e of every one of them), take a ticket; only the last
        // arriver goes on.  red[] is reused for the ticket: every wave has read its elements before the barrier below.
        // Ordering: the partials are write-through (sc0 sc1) stores, drained by vmcnt(0) in every thread; the barrier makes that hold
        // for the whole workgroup before thread 0 takes the ticket (a device-scope read-modify-write, performed past the XCD's L2);
        // the last arriver's read-back is issued behind its own barrier with sc0 sc1 loads, which no stale line of this CU's L1 or
        // this XCD's L2 can serve (MI355X_MICROARCH.md, inter-workgroup visibility).  The ticket itself stays RELAXED: an agent-scope
        // release / acquire would add an L2 write-back and an L2 invalidate per workgroup, which is what the explicit cache-policy
        // bits are there to avoid.  tests/test_gpu_kernels.py::test_gemm_rows_ksplit_stress hammers the protocol.
        const int tile = mgrp * n_tiles + ntile;
        float* pb = ksp_buf + ((long)tile * 16 + (long)blockIdx.z * NW) * 256;
        {
            const int ww = tid >> 6, l4 = (tid & 63) * 4;   // one float4 (elements l4 .. l4 + 3 of partial ww) per thread
            store_sc1(pb + ww * 256 + l4, *reinterpret_cast<const f32x4*>(&red[ww][l4]));
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) reinterpret_cast<unsigned*>(&rs[0][0])[0] = __hip_atomic_fetch_add(ksp_cnt + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (reinterpret_cast<const unsigned*>(&rs[0][0])[0] != KSP - 1) return;
        if (tid == 0) __hip_atomic_store(ksp_cnt + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
    }
    if (tid < NE) {
        float t;
        if constexpr (KSP > 1) {
            const float* pa = ksp_buf + (long)(mgrp * n_tiles + ntile) * 16 * 256 + e;
            float pv[16];
#pragma unroll
            for (int ww = 0; ww < 16; ++ww) pv[ww] = load_sc1(pa + ww * 256);
            // (the loads are asm: the wait must name their destinations, or the sums below may be scheduled in front of it)
            asm volatile("s_waitcnt vmcnt(0)"
                         : "+v"(pv[0]), "+v"(pv[1]), "+v"(pv[2]), "+v"(pv[3]), "+v"(pv[4]), "+v"(pv[5]), "+v"(pv[6]), "+v"(pv[7]), "+v"(pv[8]),
                           "+v"(pv[9]), "+v"(pv[10]), "+v"(pv[11]), "+v"(pv[12]), "+v"(pv[13]), "+v"(pv[14]), "+v"(pv[15])
                         :
                         : "memory");
            t = pv[0];
#pragma unroll
            for (int ww = 1; ww < 16; ++ww) t += pv[ww];
        } else {
            t = red[0][e];
#pragma unroll
            for (int ww = 1; ww < NW; ++ww) t += red[ww][e];
        }
        const bool ok = em < M;
        if (LN) t = rs[em - m0][1] * (t - rs[em - m0][0] * ec1);
        t += ebias;
        if (EPI == kEpiBias) {
            if (ok) out[(long)em * ldo + en] = t;
        } else if (EPI == kEpiBiasGelu) {
            if (ok) out[pk_off(em, en, omt)] = gelu_erf_form ? gelu_erf(t) : gelu_new(t);
        } else if (EPI == kEpiResidual) {
            const float v = eres + t;
            if (ok) *eptr = v;   // (rows >= M of the last tile are allocated)
            if (stats_out) {   // LayerNorm partials of this 16-column tile: the 16 lanes of a row are adjacent
                // the butterfly x += x[lane ^ 8], ^ 4, ^ 2, ^ 1 over the row's 16 lanes (= one DPP row; whole waves run this) as four
                // v_add_f32_dpp each instead of eight dependent ds_bpermute round trips at the very end of the launch: rotation by 8
                // is lane ^ 8; after it the values are invariant under ^ 8, so the rotation by 4 delivers x[lane ^ 4]; ^ 2 and ^ 1 are
                // quad permutations.  The shuffles' operand pairs in the shuffles' order: the same bits.
#define AUR_ROW16_SUM(x)                                                                                          \
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xF, 0xF, false)); /* row_ror:8 */ \
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x124, 0xF, 0xF, false)); /* row_ror:4 */ \
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xF, 0xF, false));  /* quad_perm [2,3,0,1] */ \
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, false));  /* quad_perm [1,0,3,2] */
                float sm = v;
                AUR_ROW16_SUM(sm)
                const float mu = sm * (1.0f / 16.0f);
                const float d = v - mu;
                float m2 = d * d;
                AUR_ROW16_SUM(m2)
#undef AUR_ROW16_SUM
                if (ok && (e & 15) == 0) stats_out[(long)em * 64 + ntile * NTL + ect] = make_float2(mu, m2);
            }
        } else if (ok) {
            const int u = en / kHidden, d = en - u * kHidden;
            if (u == 0) {
                out[(long)em * kHidden + d] = t;
            } else {
                const long off = kv_offset(eblk, u - 1, d / kHeadDim, epos % kKvBlockTokens) + d % kHeadDim;
                if (kv_half) reinterpret_cast<_Float16*>(kv_layer)[off] = (_Float16)t;
                else reinterpret_cast<float*>(kv_layer)[off] = t;
            }
        }
    }
}

// ---- host side: shape dispatch (the policy itself is gemm_rows_shape, gpt_kernels.hip) --------------------------------------
#define AUR_GR_CAT2(a, b) a##b
#define AUR_GR_CAT(a, b) AUR_GR_CAT2(a, b)
#define AUR_GR_ARGS(a, n_tiles) (a).Wt, (a).X, (a).bias, (a).ln_c1, (a).out, (a).stats_in, (unsigned)(a).M | ((unsigned)(n_tiles) << 16), \
                                (unsigned)(a).xmt | ((unsigned)(a).omt << 16), tail(a)
struct AUR_GR_CAT(AUR_GR_LAUNCH, _dispatch) {
    // the kernel's leading scalar arguments are the ones it needs before its first tile load; this is the rest
    static GemmRowsTail tail(const GemmRowsArgs& a) {
        return GemmRowsTail{a.stats_out, a.row_meta, a.kv_layer, a.ksp_buf, a.ksp_cnt, a.eps, a.ldo, a.kv_half, a.gelu_erf};
    }
    // Workgroup shapes: 16 waves, K-slice 64 per wave (K = 4096 needs two chunk buffers: at most 32 rows per workgroup).  The A/B
    // shapes of rounds 3-4 (8 waves, wider tiles) are gone from the source; their measurements are in DESIGN section 7.
    template <int KCH, bool LN, int EPI, int PREC, bool NT>
    static void mt(const GemmRowsArgs& a, int mt_, int nw, hipStream_t st, int ntl) {
        const int n_tiles = a.N / (16 * ntl);
        const int n_grp = (a.M + 16 * mt_ - 1) / (16 * mt_);
        const dim3 grid((unsigned)((n_tiles + 7) / 8 * 8), (unsigned)n_grp);   // x: whole groups of 8 column tiles (one per XCD; surplus workgroups exit), y: row groups
        AUR_REQUIRE(a.N % (16 * ntl) == 0, "gemm_rows: N is not a multiple of the workgroup's column tile");
#define AUR_GR(MT_, NW_, NTL_)                                                                                                  \
    if (mt_ == MT_ && nw == NW_ && ntl == NTL_) {                                                                               \
        hipLaunchKernelGGL((AUR_GR_NAME<MT_, KCH, LN, EPI, NW_, NTL_, PREC, NT>), grid, dim3(64 * NW_), 0, st, AUR_GR_ARGS(a, n_tiles)); \
        return;                                                                                                                 \
    }
        AUR_GR(1, 16, 1)
        if constexpr (!NT && KCH == 1 && LN) {
            AUR_GR(1, 16, 2)
            AUR_GR(1, 16, 3)
            AUR_GR(2, 16, 2)
        }
#undef AUR_GR
        throw InvalidArgument("gemm_rows: no kernel for this (rows, waves, column tiles) workgroup shape");
    }
    // K = 4096, K split over kGemmKsp workgroups of 4 waves per 16 x 16 output tile (M <= 32 rows)
    template <int PREC>
    static void ksp(const GemmRowsArgs& a, GemmRowsEpi epi, hipStream_t st) {
        static_assert(kGemmKsp == 4, "16 K-slices = 4 workgroups of 4 waves");
        AUR_REQUIRE(a.K == 4096 && a.N % 16 == 0 && a.ksp_buf && a.ksp_cnt, "gemm_rows K split: K == 4096 and the partial-tile scratch");
        const int n_tiles = a.N / 16, n_grp = (a.M + 15) / 16;
        const dim3 grid((unsigned)((n_tiles + 7) / 8 * 8), (unsigned)n_grp, kGemmKsp);   // z: the K parts of a tile (same XCD as the tile)
        if (epi == kEpiResidual) hipLaunchKernelGGL((AUR_GR_NAME<1, 4, false, kEpiResidual, 4, 1, PREC, true, kGemmKsp>), grid, dim3(256), 0, st, AUR_GR_ARGS(a, n_tiles));
        else if (epi == kEpiBias) hipLaunchKernelGGL((AUR_GR_NAME<1, 4, false, kEpiBias, 4, 1, PREC, true, kGemmKsp>), grid, dim3(256), 0, st, AUR_GR_ARGS(a, n_tiles));
        else throw InvalidArgument("gemm_rows K split: bias or residual epilogue");
    }
    template <int PREC, bool NT>
    static void prec(const GemmRowsArgs& b, bool ln, GemmRowsEpi epi, const GemmRowsShape& s, hipStream_t st) {
        if (ln && epi == kEpiQkv) mt<1, true, kEpiQkv, PREC, NT>(b, s.mt, s.nw, st, s.ntl);
        else if (ln && epi == kEpiBiasGelu) mt<1, true, kEpiBiasGelu, PREC, NT>(b, s.mt, s.nw, st, s.ntl);
        else if (ln && epi == kEpiBias) mt<1, true, kEpiBias, PREC, NT>(b, s.mt, s.nw, st, s.ntl);
        else if (!ln && epi == kEpiResidual && b.K == 1024) mt<1, false, kEpiResidual, PREC, NT>(b, s.mt, s.nw, st, s.ntl);
        else if (!ln && epi == kEpiResidual && b.K == 4096) mt<4, false, kEpiResidual, PREC, NT>(b, s.mt, s.nw, st, s.ntl);
        else if (!ln && epi == kEpiBias && b.K == 1024) mt<1, false, kEpiBias, PREC, NT>(b, s.mt, s.nw, st, s.ntl);
        else if (!ln && epi == kEpiBias && b.K == 4096) mt<4, false, kEpiBias, PREC, NT>(b, s.mt, s.nw, st, s.ntl);
        else throw InvalidArgument("launch_gemm_rows: unsupported (ln, epilogue, K) combination");
    }
};

void AUR_GR_LAUNCH(const GemmRowsArgs& a, bool ln, GemmRowsEpi epi, hipStream_t st) {
    using D = AUR_GR_CAT(AUR_GR_LAUNCH, _dispatch);
    AUR_REQUIRE(a.N % 16 == 0 && (a.K == 1024 || a.K == 4096) && a.M >= 1 && a.xmt >= 4 * ((a.M + 63) / 64), "gemm_rows: shape");
    AUR_REQUIRE(a.M < 65536 && a.N / 16 < 65536 && a.xmt < 65536 && a.omt >= 0 && a.omt < 65536 && (a.M + 15) / 16 < 65536,
                "gemm_rows: sizes are passed as 16-bit fields, row groups as grid.y");
    AUR_REQUIRE((epi != kEpiBiasGelu && epi != kEpiResidual) || a.omt >= (a.M + 15) / 16, "gemm_rows: packed output rows");
    AUR_REQUIRE(!ln || (a.K == 1024 && a.stats_in && a.ln_c1 && a.bias), "gemm_rows: a LayerNorm-folded GEMM needs K == 1024, the row statistics, c1 and c2");
    AUR_REQUIRE(!a.stats_out || (epi == kEpiResidual && a.N == 1024), "gemm_rows: statistics are emitted for 1024-wide residual rows");
    AUR_REQUIRE(a.bias, "gemm_rows: bias is required (the kernel loads it unconditionally; pass zeros for none)");
    AUR_REQUIRE(epi != kEpiQkv || (a.row_meta && a.kv_layer), "gemm_rows: the QKV epilogue needs the step's row_meta table and the K/V pool");
    GemmRowsShape s = gemm_rows_shape(a.M, a.N, a.K, ln);
    trace_launch("gemm_rows_kernel");
    AUR_REQUIRE(a.prec >= 0 && a.prec <= 2, "gemm_rows: prec is 0 (exact f32 MFMA), 1 (bf16 x 3 split) or 2 (fp16 weights)");
    if (s.ksp > 1 && !(a.ksp_buf && a.ksp_cnt)) s = GemmRowsShape{1, 16, 1, a.M <= 16, 1};   // no scratch given: the unsplit kernel (same bits)
    if (s.ksp > 1) {
        AUR_REQUIRE((long)((a.M + 15) / 16) * (a.N / 16) <= kGemmKspTiles, "gemm_rows K split: more output tiles than the scratch holds");
        if (a.prec == 2) D::template ksp<2>(a, epi, st);
        else if (a.prec == 1) D::template ksp<1>(a, epi, st);
        else D::template ksp<0>(a, epi, st);
        HIP_CHECK(hipGetLastError());
        return;
    }
    if (a.prec == 2) {
        if (s.nt) D::template prec<2, true>(a, ln, epi, s, st);
        else D::template prec<2, false>(a, ln, epi, s, st);
    } else if (a.prec == 1) {
        if (s.nt) D::template prec<1, true>(a, ln, epi, s, st);
        else D::template prec<1, false>(a, ln, epi, s, st);
    } else {
        if (s.nt) D::template prec<0, true>(a, ln, epi, s, st);
        else D::template prec<0, false>(a, ln, epi, s, st);
    }
    HIP_CHECK(hipGetLastError());
}
#undef AUR_GR_ARGS
#undef AUR_GR_CAT
#undef AUR_GR_CAT2
