// rt_radiance.h — one radiance query of ONE precision (include/rt.h rt_scene_radiance): included
// after rt_trace.h of the same RT_F64, includes rt_lane.h itself (no include guard, as rt_trace.h's
// per-precision part), by rt_radiance.hip / rt_radiance64_nl.hip for the device and by
// tests/radiance_emu for the host (RT_HOST_EMU).  A translation unit includes this file OR one of
// rt_list.h, rt_features.h and rt_query.h per precision.
//
// path_from_ray is rt_list.h path_sample with the camera call replaced by the caller's ray: sample
// `sample` of Philox stream `stream` (counter word 0, where a render puts the global pixel id) from
// a GIVEN ray to the event that ends it.  The camera draws of a render sit under events of their own
// (RT_EV_CAMERA0 / 1), so a path that starts from the ray camera_ray made for (pixel, sample), with
// stream = pixel, consumes exactly the words the render's path consumes after its camera ray: the
// radiance of that ray is the render's sample, word for word (camera_ray_record writes such rays).
// What differs from rt_query.h's ray: the media events are included, random numbers are drawn and the
// hit is shaded.  self_gid / self_inst are -1: the ray leaves no leaf.

#include "../../include/rt.h"
#include "rt_adaptive.h"
#include "rt_lane.h"  // (per precision, like this file: no include guard, included by exactly one body header)

namespace RT_NS {

// a ray the kernel can trace: finite fields, a direction that is not zero, time in [0, 1]
RT_FN bool path_ray_ok(const rt_path_ray& q) {
  const double inf = __builtin_huge_val();
  const bool finite = fabs(q.origin[0]) < inf && fabs(q.origin[1]) < inf && fabs(q.origin[2]) < inf && fabs(q.dir[0]) < inf &&
                      fabs(q.dir[1]) < inf && fabs(q.dir[2]) < inf;  // (a NaN fails every compare)
  const bool dir = q.dir[0] != 0.0 || q.dir[1] != 0.0 || q.dir[2] != 0.0;
  return finite && dir && q.time >= 0.0 && q.time <= 1.0;
}

// The per-lane record prologue: the ray of a well-formed record (path_ray_ok) as rt_query.h's, by
// the same function (rt_lane.h lane_ray_begin); RT_RADIANCE_UNIT_DIR: the direction's bits as they
// stand
RT_FN void path_ray_begin(const rt_path_ray& q, int flags, RayCtx& R) {
  lane_ray_begin(q.origin, q.dir, q.time, (flags & RT_RADIANCE_UNIT_DIR) != 0, R);
}

// One evaluation of rayColor max_depth time ray (Ray.hs:174-224) added to A.  R0: path_ray_begin's
// ray (not modified: every sample of the record starts from it).  THE SEGMENT LOOP IS rt_list.h
// path_sample's, kept as a second copy because the shared form — path_sample split at its camera
// call into the camera ray and a `path_segments(P0, prims, W, R, pix, sample, A, bad, overflow)` that
// both would call — would change rt_list.h, whose kernels' code must stay as it is (the convention
// of rt_trace.h lane_loop_lockstep and its copies).  A change to one loop is a change to both;
// tests/test_radiance_host.py holds them together bit for bit.
template <int kVar, int kTex, int kMedia, bool kMats, bool kInst, int kLeaf>
RT_FN void path_from_ray(const KernelParams& P0, const real* prims_, const Trav& W, const RayCtx& R0, uint32_t stream,
                         int sample, Acc& A, bool& bad, int& overflow) {
  constexpr bool kFlat = kVar == RT_VAR_FLAT;
  // the deferred redirect pdf of the diffuse flat classes (lane_loop_lockstep kDefer)
  constexpr bool kDefer = kFlat && kMedia == 0 && !kMats;
  const cfp prims = cf(prims_);
  const uint32_t pix = stream;
  RayCtx R = R0;
  f3 T = mk3(RL(1.), RL(1.), RL(1.));
  real apdf = RL(1.);
  int seg = 0;
  for (;;) {
    const KernelParams& P = RT_KARGS(P0);
    f3 L = mk3(RL(0.), RL(0.), RL(0.));
    bool ended;
    if constexpr (kDefer) {
      const SegEvent E = segment_events<kVar, kMedia, false, kLeaf>(P0, prims, W, R, pix, sample, seg, overflow, &apdf);
      // the throughput over the whole mixture pdf, once the surface query has added the target's term
      if (P.target_defer) T = (seg == 0 ? RL(1.) : RT_RCP(apdf)) * T;
      ended = shade<kTex, kMats, false>(P, prims, pix, sample, seg, E.t, E.prim, E.medium, R, L, T, -1, &apdf);
    } else {
      const SegEvent E = segment_events<kVar, kMedia, kInst, kLeaf>(P0, prims, W, R, pix, sample, seg, overflow);
      ended = shade<kTex, kMats, kInst>(P, prims, pix, sample, seg, E.t, E.prim, E.medium, R, L, T, E.inst);
    }
    if (ended) {  // (R, T and apdf are indeterminate from here: shade's invariant)
      acc_sample(A, L, bad);
      return;
    }
  }
}

// Samples sample0 + [k0, k1) of record q summed into A; false (A untouched) for a malformed record.
// A frame without depth (max_recursion_depth <= 0) has black samples, as rayColor 0 is.
template <int kVar, int kTex, int kMedia, bool kMats, bool kInst, int kLeaf>
RT_FN bool path_record(const KernelParams& P, const Trav& W, const rt_path_ray& q, int flags, int k0, int k1, Acc& A, bool& bad,
                       int& overflow) {
  if (!path_ray_ok(q)) return false;
  if (P.cam.max_depth <= 0) return true;
  RayCtx R0;
  path_ray_begin(q, flags, R0);
  for (int k = k0; k < k1; ++k)
    path_from_ray<kVar, kTex, kMedia, kMats, kInst, kLeaf>(P, P.prims, W, R0, q.stream, (int)(q.sample0 + (uint32_t)k), A, bad,
                                                            overflow);
  return true;
}

// ---- the workspace (include/rt.h): per ray RT_ACC_WORDS(real) 64-bit sum words in the film state's
// order (the high words of R, G, B; binary64: then the low words), then one 64-bit word whose low
// half is the NaN flag and whose high half is the ray's sample count
constexpr int kRadWords = (int)RT_ACC_WORDS(real) + 1;
RT_FN unsigned long long rad_count_word(uint32_t n) { return (unsigned long long)n << 32; }

// The resolve of one ray: rt_render_kernel.h rt_resolve_kernel's operation sequence with the ray's
// own count (rt_adaptive.h rt_adaptive_resolve*), so a ray that holds N samples resolves as a film
// pixel that holds N; a flagged ray is NaN as a flagged pixel, a ray without samples 0
RT_FN void radiance_resolve(const unsigned long long* w, bool ok, rt_radiance& o) {
  const uint32_t flag = (uint32_t)w[kRadWords - 1], n = (uint32_t)(w[kRadWords - 1] >> 32);
  o.samples = n;
  o.status = !ok ? -1 : flag ? 2 : 1;
  for (int c = 0; c < 3; ++c) {
#if RT_F64
    const double v = n ? rt_adaptive_resolve64((long long)w[c], w[3 + c], n) : 0.0;
#else
    const double v = n ? (double)rt_adaptive_resolve32((long long)w[c], n) : 0.0;
#endif
    o.rgb[c] = !ok ? 0.0 : flag ? __builtin_nan("") : v;
  }
}

// The camera-ray body: the ray the render makes for sample `sample` of global pixel pix (gy = pix /
// width) as a record — the class's own function, as rt_list.h path_sample chooses it; origin and unit
// direction widened to binary64 (exact), time = u01(time word), stream = pix, sample0 = sample
template <bool kFlat>
RT_FN void camera_ray_record(const KernelParams& P0, uint32_t pix, int gy, int px, int sample, rt_path_ray& q) {
  RayCtx R;
  ray_clear(R);
  {
    const KernelParams& P = RT_KARGS(P0);
    if constexpr (kFlat)
      camera_ray_flat(P, pix, sample, (uint32_t)gy << 16 | (uint32_t)px, R);
    else
      camera_ray(P, pix, sample, ~0u, R);
  }
  q.origin[0] = (double)R.o.x, q.origin[1] = (double)R.o.y, q.origin[2] = (double)R.o.z;
  q.dir[0] = (double)R.d.x, q.dir[1] = (double)R.d.y, q.dir[2] = (double)R.d.z;
  q.time = (double)u01(R.time_w);
  q.stream = pix;
  q.sample0 = (uint32_t)sample;
}

}  // namespace RT_NS
