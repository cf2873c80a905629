// rt_query_emu.cpp — TEST TOOLING: the ray-query body (raytrace_amd/csrc/rt_query.h over rt_trace.h)
// compiled for the host (RT_HOST_EMU), so the device kernel's logic can be checked against
// tests/query_ref.py and closed forms without a GPU and compared with the device field for field.
// Never linked into librt_amd.so.
#define RT_HOST_EMU 1
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt.h"
#include "../../raytrace_amd/csrc/rt_internal.h"
#include "../../raytrace_amd/csrc/rt_kernel_class.h"

namespace rt_emu {
thread_local long long counters[4];
}

#define RT_F64 0
#include "../../raytrace_amd/csrc/rt_trace.h"
#include "../../raytrace_amd/csrc/rt_query.h"
namespace qemu32 {
#include "query_body.h"
}
#undef RT_F64
#define RT_F64 1
#include "../../raytrace_amd/csrc/rt_trace.h"
#include "../../raytrace_amd/csrc/rt_query.h"
namespace qemu64 {
#include "query_body.h"
}

namespace {
thread_local std::string g_err;
}

extern "C" {
const char* rt_query_emu_last_error(void) { return g_err.c_str(); }

// n rays against scene sc (f64 = 0: the FP32 kernel's body; 1: the binary64 one), as rt_scene_cast;
// *variant receives the scene's kernel variant code (rt_internal.h RT_VAR_*)
int rt_query_emu(const rt_scene* sc, const rt_ray* rays, rt_hit* hits, long long n, int flags, int f64, int* variant) {
  HostScene H;
  if (int rc = rt_host_build_scene(sc, H, g_err)) return rc;
  if (variant) *variant = rt_host_variant(H);
  return f64 ? qemu64::cast(H, rays, hits, n, flags, g_err) : qemu32::cast(H, rays, hits, n, flags, g_err);
}
}
