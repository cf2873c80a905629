// td_probe.cpp — TEST TOOLING (tests/test_target_defer.py): what the host decides about the
// deferred redirect pdf of a render (rt_build.cpp rt_host_match_target), and the layout of
// KernelParams.  Host code only; never linked into librt_amd.so.
#include <cstddef>
#include <string>

#include "../../include/rt.h"
#include "../../raytrace_amd/csrc/rt_internal.h"
#include "../../raytrace_amd/csrc/rt_kernel_class.h"

namespace {
thread_local std::string g_err;

// out[0] = KernelParams::target_defer, out[1] = target_rec, for the kernel class the scene runs
template <class R>
int target_match(const HostScene& H, const rt_camera_settings* cs, int* out) {
  KernelParamsT<R> P = {};
  rt_exec ex = {};
  ex.n_shards = 1;
  ex.row_block = 4;
  if (int rc = rt_host_make_params(cs, 0, &ex, P, g_err)) return rc;
  const int variant = rt_host_variant(H.flat, H.n_media, H.noise, H.full_mats, H.uv_tex, H.n_instances > 0, H.leaf_kind,
                                      rt_host_media_late(H), H.max_depth > 1 ? H.max_depth : 1);
  rt_host_match_target(H, variant, P);
  out[0] = P.target_defer;
  out[1] = P.target_rec;
  return RT_OK;
}
// byte offsets of KernelParamsT<R>'s members in declaration order, then its size
#define RT_TD_KP_MEMBERS(X)                                                                                            \
  X(nodes) X(prims) X(prim_shade) X(prim_uv) X(mats) X(texs) X(motions) X(uvframes) X(texels) X(perlin_perm)          \
  X(perlin_grad) X(flat_recs) X(boxes) X(instances) X(out) X(status) X(accum) X(nanflag) X(counter) X(chunk)          \
  X(n_chunks) X(n_items) X(big_chunk) X(n_big_chunks) X(big_items) X(small_start) X(div_big) X(div_small) X(agg_big)  \
  X(agg_small) X(pool_shift) X(stack_depth) X(lds_nodes) X(trav_exit_pct) X(leaf_exit_pct) X(n_prims) X(surface_root) \
  X(surface_prefix) X(n_media) X(n_targets) X(rem_prob) X(media) X(flat_sets) X(targets) X(cam) X(key0) X(key1)       \
  X(n_shards) X(shard) X(row_block) X(tile_rows) X(out_frame_rows) X(div_width) X(div_block) X(sample0)               \
  X(target_defer) X(target_rec) X(cam_defocus)
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
