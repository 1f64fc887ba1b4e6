// Host-side rules of the GPT path that the engine and the kernel test harness (dbg_harness.hip) share, so that the kernel tests
// exercise the code the engine runs.
#pragma once
#include <memory>
#include <vector>

#include "dev_buf.h"
#include "gpt_kernels.h"

namespace aur {

constexpr int kMaxBlocks = 66;   // block-table entries per sequence: ceil(1047 / 16)

// What a decode GEMM (launch_gemm_rows) reads of one linear: GemmRowsArgs::Wt, ln_c1 and bias.
struct DecodeOperand {
    const float* Wt = nullptr;     // packed weights (prec 2: the fp16 words)
    const float* c1 = nullptr;     // LayerNorm folded in: c1, else null
    const float* bias = nullptr;   // LayerNorm folded in: c2, else the bias that was passed
};
// How a row-major [K][ldw] matrix becomes that operand, on the device, once per load.  prec: GemmRowsArgs::prec (2 = fp16 weights,
// aur_config.gpt_fp16).  gamma / beta: the LayerNorm in front of the linear, folded into the weights and the two epilogue vectors
// (launch_fold_ln, launch_fold_ln_f16), or null (launch_pack_wt16, launch_pack_wt16_f16).  prec 2 only: Weff receives the effective
// weights W'' (may be W itself, or null) and *bad is set when the fp16 rule rejects the matrix.  The buffers made are appended to
// `keep`; `scratch` is launch_fold_ln's workspace, the caller's to release once the stream has drained.
inline DecodeOperand prepare_decode_operand(int prec, const float* W, int ldw, const float* gamma, const float* beta, const float* bias,
                                            int K, int N, float* Weff, int* bad, DevBuf& scratch,
                                            std::vector<std::unique_ptr<DevBuf>>& keep, hipStream_t st) {
    auto buf = [&](size_t n) {
        keep.emplace_back(new DevBuf());
        keep.back()->ensure(n);
        return keep.back().get();
    };
    DevBuf* wt = buf((size_t)K * N * (prec == 2 ? 2 : sizeof(float)));
    DecodeOperand o;
    o.Wt = wt->as<float>();
    o.bias = bias;
    if (gamma) {
        float* v = buf((size_t)2 * N * sizeof(float))->as<float>();
        if (prec == 2) {
            launch_fold_ln_f16(W, ldw, gamma, beta, bias, Weff, wt->p, v, v + N, bad, K, N, st);
        } else {
            scratch.ensure((size_t)K * N * sizeof(float));
            launch_fold_ln(W, ldw, gamma, beta, bias, scratch.as<float>(), wt->as<float>(), v, v + N, K, N, st);
        }
        o.c1 = v;
        o.bias = v + N;
    } else if (prec == 2) {
        launch_pack_wt16_f16(W, ldw, nullptr, Weff, wt->p, bad, K, N, st);
    } else {
        launch_pack_wt16(W, ldw, wt->as<float>(), K, N, st);
    }
    return o;
}

// Query blocks of a batch of prompt rows for launch_prompt_attention: runs of consecutive rows of one slot with positions
// ascending by one, cut every 32 rows (from the run's first row: a sequence's blocks do not depend on what else is in the batch).
inline std::vector<int2> prompt_qblocks(const std::vector<int>& row_slot, const std::vector<int>& row_pos) {
    std::vector<int2> qblk;
    const int M = (int)row_slot.size();
    for (int m = 0; m < M;) {
        int n = 1;
        while (m + n < M && n < 32 && row_slot[m + n] == row_slot[m] && row_pos[m + n] == row_pos[m] + n) ++n;
        qblk.push_back(make_int2(m, n));
        m += n;
    }
    return qblk;
}

}  // namespace aur
