// rt_radiance_emu.cpp — TEST TOOLING: the radiance-query body (raytrace_amd/csrc/rt_radiance.h over
// rt_trace.h) compiled for the host (RT_HOST_EMU), so the kernel's logic can be compared with the
// per-pixel path body (tests/list_emu) and with closed forms bit for bit without a GPU.  Never
// linked into librt_amd.so.
#define RT_HOST_EMU 1
#include <cmath>
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
#include "../../raytrace_amd/csrc/rt_radiance.h"
namespace remu32 {
#include "radiance_body.h"
}
#undef RT_F64
#define RT_F64 1
#include "../../raytrace_amd/csrc/rt_trace.h"
#include "../../raytrace_amd/csrc/rt_radiance.h"
namespace remu64 {
#include "radiance_body.h"
}

namespace {
thread_local std::string g_err;
}

extern "C" {
const char* rt_radiance_emu_last_error(void) { return g_err.c_str(); }

// rt_scene_radiance on the host: n rays, n_samples each, into work (n x 7 words with f64, n x 4
// without: include/rt.h's workspace layout less the cursor) and out
int rt_radiance_emu(const rt_camera_settings* cs, const rt_scene* sc, uint64_t seed, const rt_path_ray* rays, int64_t n,
                    int32_t n_samples, int32_t flags, unsigned long long* work, rt_radiance* out, int f64) {
  rt_exec ex{};
  if (int rc = rt_host_radiance_check(sc, &ex, cs, rays, out, n, n_samples, flags, g_err)) return rc;
  HostScene H;
  if (int rc = rt_host_build_scene(sc, H, g_err)) return rc;
  return f64 ? remu64::radiance(H, cs, seed, rays, n, n_samples, flags, work, out, g_err)
             : remu32::radiance(H, cs, seed, rays, n, n_samples, flags, work, out, g_err);
}

// rt_scene_camera_rays on the host: height x width records
int rt_radiance_emu_camera_rays(const rt_camera_settings* cs, const rt_scene* sc, uint64_t seed, int32_t sample,
                                rt_path_ray* rays, int f64) {
  HostScene H;
  if (int rc = rt_host_build_scene(sc, H, g_err)) return rc;
  return f64 ? remu64::camera_rays(H, cs, seed, sample, rays, g_err) : remu32::camera_rays(H, cs, seed, sample, rays, g_err);
}
}
