// rt_list_emu.cpp — TEST TOOLING: the per-pixel path body (raytrace_amd/csrc/rt_list.h over
// rt_trace.h) compiled for the host (RT_HOST_EMU), so the pixel-list kernel's logic can be compared
// with the render's lane loops (tests/kernel_emu) bit for bit without a GPU.  Never linked into
// librt_amd.so.
#define RT_HOST_EMU 1
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt.h"
#include "../../raytrace_amd/csrc/rt_adaptive.h"
#include "../../raytrace_amd/csrc/rt_internal.h"
#include "../../raytrace_amd/csrc/rt_kernel_class.h"

namespace rt_emu {
thread_local long long counters[4];
}

#define RT_F64 0
#include "../../raytrace_amd/csrc/rt_trace.h"
#include "../../raytrace_amd/csrc/rt_list.h"
namespace lemu32 {
#include "list_body.h"
}
#undef RT_F64
#define RT_F64 1
#include "../../raytrace_amd/csrc/rt_trace.h"
#include "../../raytrace_amd/csrc/rt_list.h"
namespace lemu64 {
#include "list_body.h"
}

namespace {
thread_local std::string g_err;
}

extern "C" {
const char* rt_list_emu_last_error(void) { return g_err.c_str(); }

// The mean image of samples [0, counts[p]) of every tile pixel p of the frame (cs, ex) of scene sc:
// counts holds one uint32 per tile pixel; out tile pixels x 3 doubles (f64 = 1) or floats.
// cs->samples_per_pixel is validated and otherwise not read.
int rt_list_emu(const rt_camera_settings* cs, const rt_scene* sc, uint64_t seed, const rt_exec* ex, const uint32_t* counts,
                void* out, int f64) {
  HostScene H;
  if (int rc = rt_host_build_scene(sc, H, g_err)) return rc;
  return f64 ? lemu64::render(H, cs, seed, ex, counts, (double*)out, g_err)
             : lemu32::render(H, cs, seed, ex, counts, (float*)out, g_err);
}
}
