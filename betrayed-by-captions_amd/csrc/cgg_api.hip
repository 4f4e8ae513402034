// Library-level entry points of libcgg_hip.so: version, thread-local error string, and the one place that
// raises a kernel's dynamic-LDS limit.
#include "cgg_common.h"

#include <map>
#include <mutex>

static thread_local char g_cgg_err[512] = "";

void cgg_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_cgg_err, sizeof(g_cgg_err), fmt, ap);
  va_end(ap);
}

// Largest dynamic-LDS limit granted so far, per (device, kernel host address). Host memory only: nothing
// to set up at cgg_init, and a lookup is legal under stream capture.
static std::mutex g_lds_mu;
static std::map<const void*, size_t> g_lds_granted[CGG_MAX_DEVICES];

int cgg_raise_dynamic_lds(const void* kernel, size_t bytes, const char* who) {
  if (bytes <= 64 * 1024) return CGG_OK;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  const bool tabled = dev >= 0 && dev < CGG_MAX_DEVICES;   // an untabled device sets the attribute every time
  std::lock_guard<std::mutex> lock(g_lds_mu);
  if (tabled) {
    auto it = g_lds_granted[dev].find(kernel);
    if (it != g_lds_granted[dev].end() && it->second >= bytes) return CGG_OK;
  }
  hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  CGG_REQUIRE(e == hipSuccess, (int)e, "%s: cannot raise dynamic LDS to %zu: %s", who, bytes, hipGetErrorString(e));
  if (tabled) g_lds_granted[dev][kernel] = bytes;
  return CGG_OK;
}

// The most dynamic LDS one workgroup may ask for on the current device; without a device, gfx950's 160 KiB (the only
// target this library is built for), so that a gate can be evaluated where nothing can be launched.
extern "C" int64_t cgg_dynamic_lds_limit(void) {
  int dev = -1, v = 0;
  if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess &&
      v > 0)
    return v;
  return 160 * 1024;
}

extern "C" int cgg_version(void) { return CGG_VERSION; }

extern "C" const char* cgg_last_error_string(void) { return g_cgg_err; }
