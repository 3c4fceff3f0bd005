#include "common.h"

#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>

static thread_local char g_err[512] = "ok";

void di2p_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* di2p_last_error(void) { return g_err; }
extern "C" int di2p_version(void) { return 9; }

namespace {
struct OptDef { const char* name; const char* env; long long def; };
const OptDef kOpts[DI2P_OPT_COUNT] = {
#define DI2P_OPT_DEF(ID, NAME, ENV, DEF) {NAME, ENV, DEF},
    DI2P_OPTIONS(DI2P_OPT_DEF)
#undef DI2P_OPT_DEF
};
long long g_opt[DI2P_OPT_COUNT];
std::once_flag g_opt_once;
void opts_init() {
    for (int i = 0; i < DI2P_OPT_COUNT; ++i) {
        const char* e = getenv(kOpts[i].env);
        g_opt[i] = e ? atoll(e) : kOpts[i].def;
    }
}
}  // namespace

int di2p_cu_count() {
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int n = cached[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

int di2p_allow_dynamic_lds(const void* kernel, size_t bytes, const char* who) {
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) return 0;
    di2p_set_error("%s: %zu bytes of dynamic LDS refused: %s", who, bytes, hipGetErrorString(e));
    (void)hipGetLastError();
    return -1;
}

long long di2p_opt(int id) {
    std::call_once(g_opt_once, opts_init);
    return g_opt[id];
}

// name = lower-case knob name ("conv_nosplit", "solver_nocull", ...).  Returns 0, or -1 for an unknown name.
extern "C" int di2p_set_option(const char* name, long long value) {
    std::call_once(g_opt_once, opts_init);
    for (int i = 0; i < DI2P_OPT_COUNT; ++i)
        if (name && strcmp(name, kOpts[i].name) == 0) { g_opt[i] = value; return 0; }
    di2p_set_error("di2p_set_option: unknown option");
    return -1;
}

extern "C" long long di2p_get_option(const char* name) {
    std::call_once(g_opt_once, opts_init);
    for (int i = 0; i < DI2P_OPT_COUNT; ++i)
        if (name && strcmp(name, kOpts[i].name) == 0) return g_opt[i];
    return -1;
}
