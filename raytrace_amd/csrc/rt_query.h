// rt_query.h — one ray query of ONE precision (include/rt.h rt_scene_cast): included after rt_trace.h
// of the same RT_F64, includes rt_lane.h itself (no include guard, as rt_trace.h's per-precision
// part), by rt_query.hip / rt_query64.hip / rt_query64_bvh.hip for the device and by tests/query_emu
// for the host (RT_HOST_EMU).
//
// query_ray turns one rt_ray into one rt_hit against the scene's surface set, by the query a
// render's segment runs (rt_lane.h lane_query, with its any-hit stop) and the render's hit
// information (rt_trace.h surface_info_world).  What differs from a camera ray: the ray is the
// caller's (normalised in binary64 before it is converted to the kernel's precision), its time word is floor(time 2^24) << 8 (u01 of it is the time the
// kernel sees, rt_trace.h u01), tmin stands where kTmin does, and tmax enters as the initial Closest
// ({tmax, 0, -1, -1}; FP32: the key hit_key(tmax, 0)), so a candidate needs t < tmax strictly — no
// leaf's key order is below 0.  self_gid / self_inst are -1: a query ray leaves no leaf.  Media are
// not queried (their events are random draws keyed by pixel and sample).
#include "../../include/rt.h"
#include "rt_lane.h"  // (per precision, like this file: no include guard, included by exactly one body header)

namespace RT_NS {

// a ray the kernel can trace: finite fields, a direction that is not zero, 0 <= tmin < tmax, time in [0, 1]
RT_FN bool query_ray_ok(const rt_ray& q) {
  const double s = q.origin[0] + q.origin[1] + q.origin[2] + q.dir[0] + q.dir[1] + q.dir[2] + q.tmin + q.time;
  const bool finite = fabs(s) < __builtin_huge_val() && fabs(q.origin[0]) < __builtin_huge_val() &&
                      fabs(q.origin[1]) < __builtin_huge_val() && fabs(q.origin[2]) < __builtin_huge_val() &&
                      fabs(q.dir[0]) < __builtin_huge_val() && fabs(q.dir[1]) < __builtin_huge_val() &&
                      fabs(q.dir[2]) < __builtin_huge_val();
  const bool dir = q.dir[0] != 0.0 || q.dir[1] != 0.0 || q.dir[2] != 0.0;
  return finite && dir && q.tmin >= 0.0 && q.tmax > q.tmin && q.time >= 0.0 && q.time <= 1.0;  // (a NaN tmax fails)
}

// kVar, kInst, kLeaf: the scene's kernel class (rt_kernel_class.h), the fields a surface hit sees.
// prim_mat: the material index of every primitive (rt_internal.h HostScene::prim_mat).
template <int kVar, bool kInst, int kLeaf>
RT_FN void query_ray(const KernelParams& P0, const real* prims_, const int* prim_mat, const Trav& W, const rt_ray& q,
                     int flags, rt_hit& H, int& overflow) {
  constexpr bool kFlat = kVar == RT_VAR_FLAT;
  H = rt_hit{};
  H.instance = -1;
  H.material = -1;
  H.leaf = -1;
  if (!query_ray_ok(q)) {
    H.hit = -1;
    return;
  }
  const cfp prims = cf(prims_);
  const bool any = (flags & RT_QUERY_ANY_HIT) != 0;
  RayCtx R;
  lane_ray_begin(q.origin, q.dir, q.time, false, R);  // (shared with a radiance query's rays, rt_radiance.h)
  const real tmin = (real)q.tmin, tmax = (real)q.tmax;
  Closest C = no_hit();
  C.t = tmax;
#if !RT_F64
  const unsigned long long key0 = hit_key(tmax, 0);
  C.key = key0;
#endif
  if constexpr (!kFlat) prep_ray(R);
  // any-hit: a BVH traversal ends at the first accepted hit
  lane_query<kVar, kInst, kLeaf>(P0, prims, W, R, RT_KARGS(P0).surface_root, 0, tmin, C, overflow, any);
  bool hit = C.prim >= 0;
  if constexpr (kFlat) {
#if RT_F64
    hit = C.t < tmax;  // every accepted candidate is below tmax
    C.prim = C.ord;    // slot = primitive index (rt_trace.h closest_flat)
#else
    hit = C.key < key0;
#endif
  }
  if (!hit) {
    H.t = __builtin_huge_val();
    return;
  }
  H.hit = 1;
  H.t = (double)C.t;
  if (any) return;
  const KernelParams& P = RT_KARGS(P0);
  const int best = C.prim, best_inst = kInst ? C.inst : -1;
#if RT_F64
  H.leaf = C.ord;
#else
  H.leaf = (int)(uint32_t)C.key;
#endif
  H.instance = best_inst;
  int mat = ldci(prim_mat, best);
  const bool need_uv = (flags & RT_QUERY_UV) != 0;
  if constexpr (kInst) {
    if (best_inst >= 0) {  // a placement's own material overrides its leaves' (rt_trace.h hit_material)
      const int im = inst_rec(P, best_inst)->material;
      if (im >= 0) mat = im;
    }
  }
  HitInfo h = surface_info_world<kInst>(P, prims, best, best_inst, R, C.t, need_uv);
  // a sphere's (p - c) / r is unit up to the hit point's rounding over r (eps |p| / r, many eps for
  // a small sphere far from the origin): the record's normal is re-normalised
  h.n = unit(h.n);
  H.material = mat;
  H.front = h.front ? 1 : 0;
  H.point[0] = (double)h.p.x, H.point[1] = (double)h.p.y, H.point[2] = (double)h.p.z;
  H.normal[0] = (double)h.n.x, H.normal[1] = (double)h.n.y, H.normal[2] = (double)h.n.z;
  H.uv[0] = (double)h.u, H.uv[1] = (double)h.v;
}

}  // namespace RT_NS
