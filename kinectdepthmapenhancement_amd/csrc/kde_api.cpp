// kde_api.cpp — the library-wide part of the extern "C" surface of libkde_hip.so (include/kde_hip.h): the error
// message, the version and the device entry points.  The handle objects live in kde_api_<class>.cpp, one file per
// family of reference classes; what those files share is kde_handles.h.
#include "kde_internal.h"

#include <algorithm>

namespace kde {

// ---- errors ---------------------------------------------------------------------------------------
static thread_local char g_err[512] = "no error";

int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#ifdef KDE_STAGE_HOOKS
StageCtl g_stage = {nullptr, nullptr, nullptr, nullptr, 0};
size_t g_stage_cache_bytes = kCacheBytes;
uint64_t g_stage_streaming[kCacheSites] = {};
#endif

}  // namespace kde

using namespace kde;

#ifdef KDE_STAGE_HOOKS
// include/kde_test_hooks.h: exists only in tools/hooks/libkde_hip_stage.so
extern "C" int kde_stage_set(float* jbf_avg_dev, float* ers_avg_dev, float* ers_dev_dev, unsigned* counters_dev, int force_full_rules)
{
    g_stage.jbf_avg = jbf_avg_dev;
    g_stage.ers_avg = ers_avg_dev;
    g_stage.ers_dev = ers_dev_dev;
    g_stage.counters = counters_dev;
    g_stage.force_full_rules = force_full_rules;
    return KDE_OK;
}

extern "C" int kde_stage_set_cache_bytes(size_t bytes)
{
    g_stage_cache_bytes = bytes;
    return KDE_OK;
}

extern "C" int kde_stage_streaming_launches(uint64_t* counts, int n)
{
    KDE_REQUIRE(n >= 0 && n <= (int)kCacheSites && (counts || n == 0), "kde_stage_streaming_launches: n=%d outside 0..%d, or null counts",
                n, (int)kCacheSites);
    for (int i = 0; i < n; i++) counts[i] = g_stage_streaming[i];
    std::fill(g_stage_streaming, g_stage_streaming + kCacheSites, (uint64_t)0);
    return KDE_OK;
}
#endif

// =====================================================================================================
// library
// =====================================================================================================
extern "C" int kde_abi_version(void) { return KDE_ABI_VERSION; }
extern "C" const char* kde_last_error_string(void) { return g_err; }

extern "C" int kde_device_count(int* count)
{
    KDE_REQUIRE(count, "kde_device_count: null argument");
    KDE_HIP_TRY(hipGetDeviceCount(count));
    return KDE_OK;
}

extern "C" int kde_set_device(int device)
{
    KDE_HIP_TRY(hipSetDevice(device));
    return KDE_OK;
}

extern "C" int kde_device_info(char* arch_buf, size_t arch_cap, int* cu_count)
{
    int dev = 0;
    KDE_HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    KDE_HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (arch_buf && arch_cap) snprintf(arch_buf, arch_cap, "%s", prop.gcnArchName);
    if (cu_count) *cu_count = prop.multiProcessorCount;
    return KDE_OK;
}

extern "C" int kde_device_pci_bus_id(char* buf, size_t cap)
{
    KDE_REQUIRE(buf && cap >= 13, "kde_device_pci_bus_id: a buffer of at least 13 bytes is required");
    int dev = 0;
    KDE_HIP_TRY(hipGetDevice(&dev));
    KDE_HIP_TRY(hipDeviceGetPCIBusId(buf, (int)std::min<size_t>(cap, 64), dev));
    return KDE_OK;
}

