// rt_lane.h — what the one-lane kernels share, for ONE precision: included after rt_trace.h of the same
// RT_F64 (no include guard, as rt_trace.h's per-precision part) by rt_list.h, rt_features.h,
// rt_query.h and rt_radiance.h themselves — a translation unit includes one of the four per precision.  Their kernels
// give a lane one thing to run to completion (a pixel's samples, a pixel's first hits, a ray, a ray's paths)
// instead of interleaving a work queue's paths as the render's lane loops do.
//
//   lane_query      one closest-hit query over a set, run by one lane from start to end
//   segment_events  one path segment's events: the surface query, then the media in the class's mode
//   lane_ray_begin  a caller's ray record as the ray a lane traces (the query and radiance kernels)
// both the render's functions in the render's order (rt_trace.h lane_loop_lockstep for the flat
// classes, lane_loop_bvh for the others), so that a pixel's path, its first hit and a query's hit
// are the render's bit for bit; and the three launchers' shape.

namespace RT_NS {

// One closest-hit query over a set: the flat sets through closest<true>; a BVH set by its start
// (the surface prefix for set 0, the generic test for a medium set that is a single leaf of a leaf
// class) and trav_round until done.  C enters as the bound a candidate has to beat (no_hit(), or a
// ray query's tmax) and leaves as the hit.  any: stop at the first accepted hit (rt_query.h's
// any-hit; the literal false elsewhere).  The kernel arguments are re-read (rt_trace.h RT_KARGS).
template <int kVar, bool kInst, int kLeaf>
RT_FN void lane_query(const KernelParams& P0, cfp prims, const Trav& W, RayCtx& R, int root, int set, real tmin, Closest& C,
                      int& overflow, bool any = false) {
  const KernelParams& P = RT_KARGS(P0);
  if constexpr (kVar == RT_VAR_FLAT) {
    closest<true>(P, prims, root, set, R, tmin, C, W, &overflow);
  } else {
    TravState S;
    trav_begin(S, root, tmin);
    S.C = C;
    if (set == 0) {
      prefix_hits<kInst>(P, prims, R, tmin, S.C);
    } else if (kLeaf != 0 && S.node == RT_EMPTY_ROOT) {
      test_leaf_generic<kInst>(P, R, S);
    }
    while (!trav_done(S) && !(any && S.C.prim >= 0)) trav_round<kInst, kLeaf>(P, R, S, W, overflow RT_PROF_NULLARG);
    C = S.C;
  }
}

// A caller's ray (include/rt.h rt_ray, rt_path_ray) as the ray a lane traces: the origin and the
// direction converted to the kernel's precision and the time as the render's Philox word,
// floor(time 2^24) << 8 (u01 of it is the time the kernel sees; a time of 1 is 1 - 2^-24).  The
// direction is dir / |dir| in binary64, scaled by its largest component first (no overflow or
// underflow of the squares); unit: the caller says it is unit already, its bits are used as they
// stand.  The fields are finite, the direction is not zero and the time lies in [0, 1] (the callers'
// own checks).  R is ray_clear'ed otherwise: the ray leaves no leaf.
RT_FN void lane_ray_begin(const double (&o)[3], const double (&d)[3], double time, bool unit, RayCtx& R) {
  ray_clear(R);
  R.o = mk3((real)o[0], (real)o[1], (real)o[2]);
  if (unit) {
    R.d = mk3((real)d[0], (real)d[1], (real)d[2]);
  } else {
    const double m = fmax(fmax(fabs(d[0]), fabs(d[1])), fabs(d[2]));
    const double dx = d[0] / m, dy = d[1] / m, dz = d[2] / m;
    const double il = 1.0 / sqrt(dx * dx + dy * dy + dz * dz);
    R.d = mk3((real)(dx * il), (real)(dy * il), (real)(dz * il));
  }
  const double tw = floor(time * 16777216.0);
  R.time_w = (uint32_t)(tw > 16777215.0 ? 16777215.0 : tw) << 8;
}

// the event that ends a segment: a surface hit (prim, inst; t), a medium event (medium >= 0; t) or neither
struct SegEvent {
  real t;
  int prim, inst, medium;
};
// Segment seg of sample `sample` of pixel pix along R (prep_ray is run here): the surface query, then
// the segment's medium events with the render's Philox words (kMedia 1: media_chain over lane_query;
// 2: media_events_late).  apdf given (the diffuse flat classes of a path, rt_trace.h
// lane_loop_lockstep's kDefer): the surface query is closest_flat<true>, which adds the redirect
// target's term to *apdf.
template <int kVar, int kMedia, bool kInst, int kLeaf, class... Defer>
RT_FN SegEvent segment_events(const KernelParams& P0, cfp prims, const Trav& W, RayCtx& R, uint32_t pix, int sample, int seg,
                              int& overflow, Defer... apdf) {
  const KernelParams& P = RT_KARGS(P0);
  if constexpr (kVar != RT_VAR_FLAT) prep_ray(R);
  Closest C = no_hit();
  if constexpr (sizeof...(Defer) > 0)
    closest_flat<true>(P, 0, R, kTmin, C, apdf...);
  else
    lane_query<kVar, kInst, kLeaf>(P0, prims, W, R, P.surface_root, 0, kTmin, C, overflow, false);
  SegEvent E{C.t, C.prim, -1, -1};
  if constexpr (kInst) E.inst = C.inst;
  if constexpr (kMedia == 2) {
    media_events_late<kInst>(P, prims, R, pix, sample, seg, E.prim, E.t, E.t, E.medium);
  } else if constexpr (kMedia == 1) {
    media_chain(P, prims, R, pix, sample, seg, C, E.t, E.medium, [&](int root, int set, real tmin, Closest& Cm) {
      lane_query<kVar, kInst, kLeaf>(P0, prims, W, R, root, set, tmin, Cm, overflow, false);
    });
  }
  return E;
}

// ---- the launchers' shape (rt_list_kernel.h, rt_features_kernel.h, rt_query_kernel.h)
constexpr int kLaneBlock = 64;         // one wave per workgroup: nothing is shared across one but a claimed id
constexpr int kLaneResident = 131072;  // 256 CUs x 8 waves x 64 lanes: the lanes that fill the device
// dynamic LDS of a workgroup: the BVH classes' traversal stacks, [stack_depth + 1][64] ints as the
// render kernels lay them out (Trav{smem + lane, kLaneBlock}); no staged nodes (lds_nodes = 0)
inline size_t lane_stack_bytes(int variant, int stack_depth) {
  return rt_class_of(RT_F64, variant).var == RT_VAR_FLAT ? 0 : (size_t)(stack_depth + 1) * kLaneBlock * sizeof(int);
}

}  // namespace RT_NS
