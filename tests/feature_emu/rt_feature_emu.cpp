// rt_feature_emu.cpp — TEST TOOLING: the first-hit feature body (raytrace_amd/csrc/rt_features.h
// over rt_trace.h) compiled for the host (RT_HOST_EMU), so the device kernel's logic can be checked
// against the FP64 oracle without a GPU and compared with the device word for word.  Never linked
// into librt_amd.so.
#define RT_HOST_EMU 1
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt.h"
#include "../../raytrace_amd/csrc/rt_denoise.h"
#include "../../raytrace_amd/csrc/rt_internal.h"
#include "../../raytrace_amd/csrc/rt_kernel_class.h"

namespace rt_emu {
thread_local long long counters[4];
}

#define RT_F64 0
#include "../../raytrace_amd/csrc/rt_trace.h"
#include "../../raytrace_amd/csrc/rt_features.h"
namespace femu32 {
#include "feature_body.h"
}
#undef RT_F64
#define RT_F64 1
#include "../../raytrace_amd/csrc/rt_trace.h"
#include "../../raytrace_amd/csrc/rt_features.h"
namespace femu64 {
#include "feature_body.h"
}

namespace {
thread_local std::string g_err;
}

extern "C" {
const char* rt_feature_emu_last_error(void) { return g_err.c_str(); }

// The feature words of samples [0, n_feat) of every tile pixel of the frame (cs, ex) of scene sc:
// out holds tile pixels x 8 int64 (f64 = 0, the FP32 kernel's words) or x 16 (f64 = 1), zeroed here.
int rt_feature_emu(const rt_camera_settings* cs, const rt_scene* sc, uint64_t seed, const rt_exec* ex, int n_feat,
                   long long* out, int f64) {
  HostScene H;
  if (int rc = rt_host_build_scene(sc, H, g_err)) return rc;
  return f64 ? femu64::features(H, cs, seed, ex, n_feat, out, g_err) : femu32::features(H, cs, seed, ex, n_feat, out, g_err);
}
}
