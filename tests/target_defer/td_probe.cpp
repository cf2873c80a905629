// td_probe.cpp — TEST TOOLING (tests/test_target_defer.py): what the host decides about the
// deferred redirect pdf of a render (rt_build.cpp rt_host_render_params), and the layout of
// KernelParams.  Host code only; never linked into librt_amd.so.
#include <cstddef>
#include <string>

#include "../../include/rt.h"
#include "../../raytrace_amd/csrc/rt_internal.h"
#include "../../raytrace_amd/csrc/rt_kernel_class.h"
#include "kp_members.h"

namespace {
thread_local std::string g_err;

// out[0] = KernelParams::target_defer, out[1] = target_rec, for the kernel class the scene runs
template <class R>
int target_match(const HostScene& H, const rt_camera_settings* cs, int* out) {
  KernelParamsT<R> P;
  rt_exec ex = {};
  ex.n_shards = 1;
  ex.row_block = 4;
  if (int rc = rt_host_render_params(H, rt_host_variant(H), rt_host_records<R>(H), cs, 0, &ex, LaunchInputs(), P, g_err))
    return rc;
  out[0] = P.target_defer;
  out[1] = P.target_rec;
  return RT_OK;
}
// byte offsets of KernelParamsT<R>'s members in declaration order (kp_members.h), then its size
template <class R>
int params_offsets(long long* out, const char** names, int n) {
  using KP = KernelParamsT<R>;
  int k = 0;
#define RT_TD_KP_ONE(m)                  \
  if (k < n) {                           \
    out[k] = (long long)offsetof(KP, m); \
    if (names) names[k] = #m;            \
  }                                      \
  ++k;
  RT_TD_KP_MEMBERS(RT_TD_KP_ONE)
#undef RT_TD_KP_ONE
  if (k < n) {
    out[k] = (long long)sizeof(KP);
    if (names) names[k] = "sizeof";
  }
  return k + 1;
}
}  // namespace

extern "C" {
const char* rt_td_last_error(void) { return g_err.c_str(); }
// f64 = 1: the binary64 records
int rt_td_target_match(const rt_camera_settings* cs, const rt_scene* sc, int f64, int* out) {
  HostScene H;
  int rc = rt_host_build_scene(sc, H, g_err);
  if (rc) return rc;
  return f64 ? target_match<double>(H, cs, out) : target_match<float>(H, cs, out);
}
// returns the number of entries (members + 1); fills at most n of out / names (names may be null)
int rt_td_params_offsets(int f64, long long* out, const char** names, int n) {
  return f64 ? params_offsets<double>(out, names, n) : params_offsets<float>(out, names, n);
}
}
