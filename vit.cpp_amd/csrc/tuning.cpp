// tuning.cpp -- per-device launch state: the Tuning table and the one-time bring-up of every kernel family on a device.
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <mutex>
#include <vector>

#include "kernels.h"

namespace vitx {

// ------------------------------------------------------------------------------------------------
// Per-device launch state (see Tuning in kernels.h).
// ------------------------------------------------------------------------------------------------
static hipError_t prepare_device_kernels(const Tuning &t) {
    hipError_t e = prepare_gemm(t);
    if (e == hipSuccess) e = prepare_patch_embed();
    if (e == hipSuccess) e = prepare_attention();
    if (e == hipSuccess) e = prepare_attention_text();
    if (e == hipSuccess) e = prepare_dense();
    if (e == hipSuccess) e = prepare_depth();
    return e;
}

const Tuning *tuning_for_device(int device) {
    static std::mutex mu;
    static std::vector<std::unique_ptr<Tuning>> table;      // one entry per device, never moved or freed
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if ((size_t)device < table.size() && table[device]) return table[device].get();
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return nullptr;
    if (cur != device && hipSetDevice(device) != hipSuccess) return nullptr;
    std::unique_ptr<Tuning> t(new Tuning());
    t->device = device;
    if (hipDeviceGetAttribute(&t->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || t->n_cu <= 0) t->n_cu = 256;
    if (hipDeviceGetAttribute(&t->n_xcd, hipDeviceAttributeNumberOfXccs, device) != hipSuccess || t->n_xcd <= 0) { (void)hipGetLastError(); t->n_xcd = 0; }      // unknown: no LayerNorm fusion
#ifdef VITX_LAB      // the laboratory build (tools/) reads its experiment switches from the environment; the product library reads none of them
    auto env_int = [](const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; };
    if (const char *e = getenv("VITX_GEMM_CFG")) t->gemm_cfg = !strcmp(e, "pp") ? 1 : atoi(e);
    t->gemm_split = env_int("VITX_GEMM_SPLIT", 0);
    t->gemm_balance = env_int("VITX_GEMM_BALANCE", 1);
    t->group_m = env_int("VITX_GROUP_M", 0);
    t->skinny_tiles = env_int("VITX_SKINNY_TILES", 128);
    t->pp_flags = env_int("VITX_PP_FLAGS", 0);
    t->gemm_dbg = env_int("VITX_GEMM_DBG", 0);
    t->attn_kernel = env_int("VITX_ATTN_KERNEL", 0);
    t->attn_grid = env_int("VITX_ATTN_GRID", 0);
#endif
    const hipError_t e = prepare_device_kernels(*t);
    if (cur != device) (void)hipSetDevice(cur);
    if (e != hipSuccess) return nullptr;
    if ((size_t)device >= table.size()) table.resize(device + 1);
    table[device] = std::move(t);
    return table[device].get();
}

}  // namespace vitx
