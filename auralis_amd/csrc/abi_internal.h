// What the translation units that define extern "C" entry points of include/auralis_amd.h share and the header does not export:
// the mapping of exception types to AUR_E_* codes, and the engine state the kernel test harness (dbg_harness.hip) runs on (the host
// rules of a launch it shares with the engine's networks, gpt_net.h and voc_net.h, are gpt_host.h's and voc_net.h's).
#pragma once
#include <new>
#include <string>

#include "../../include/auralis_amd.h"
#include "common.h"

namespace aur {

extern thread_local std::string g_last_error;   // one object for the library (engine.hip); aur_last_error() reports it

// By value: the harness touches no sequence, slot, K/V pool or batcher state.
struct DbgCtx {
    int device;
    hipStream_t st, st_lo;   // the GPT stream and the low-priority (vocoder) stream
    int prec;                // GemmRowsArgs::prec of the engine's configuration (aur_config.gemm_f32_exact)
    bool gpt_fp16, presplit; // aur_config.gpt_fp16; AUR_GEMM_PRESPLIT
    float* ksp_buf;          // GemmRowsArgs::ksp_buf / ksp_cnt
    unsigned* ksp_cnt;
};
__attribute__((visibility("hidden"))) DbgCtx dbg_ctx(const aur_engine* e);   // not part of the library's interface

}  // namespace aur

template <class F>
static int guarded(F&& f) {
    try {
        f();
        return AUR_OK;
    } catch (const aur::InvalidArgument& e) {
        aur::g_last_error = e.what();
        return AUR_E_INVALID;
    } catch (const aur::StateError& e) {
        aur::g_last_error = e.what();
        return AUR_E_STATE;
    } catch (const aur::HipError& e) {
        aur::g_last_error = e.what();
        return AUR_E_HIP;
    } catch (const std::bad_alloc&) {
        aur::g_last_error = "out of host memory";
        return AUR_E_NOMEM;
    } catch (const std::exception& e) {
        aur::g_last_error = e.what();
        return AUR_E_HIP;
    }
}
#define CHECK_PTR(p)                                    \
    if (!(p)) {                                         \
        aur::g_last_error = "null argument: " #p;       \
        return AUR_E_INVALID;                           \
    }
