// rt_list.h — one whole path of ONE precision, per lane: included after rt_trace.h of the same
// RT_F64 (no include guard, as rt_trace.h's per-precision part), by rt_list.hip / rt_list64_nl.hip for
// the device and by tests/list_emu for the host (RT_HOST_EMU).
//
// The render kernels' lane loops (rt_trace.h lane_loop_lockstep, lane_loop_flat_ring, lane_loop_bvh)
// interleave the paths of a work queue's items; they take a pixel from the shard formula and a
// sample range from one sample0 (open_item).  An adaptive film pass (rt_adaptive.h) renders a LIST
// of pixels, each from its own first sample, so it needs the path as a function of (pixel, sample):
// path_sample runs sample `sample` of global pixel `pix` from the camera to the event that ends it
// and adds its radiance to an Acc — the render's Philox key and events, the same functions in the
// same order per segment as the class's lane loop (rt_features.h feature_sample is this segment 0):
//   camera_ray_flat / camera_ray + prep_ray
//   per segment: the surface query (flat: closest<true>, or closest_flat<true> with the deferred
//     redirect pdf in the diffuse flat classes, as lane_loop_lockstep; BVH: trav_begin, prefix_hits /
//     test_leaf_generic and trav_round until done), the media in the class's mode (1: the query chain,
//     2: media_events_late), then shade
// so a pixel's sums over samples [a, b) are the render's, word for word.  shade's invariant holds:
// after it returns true nothing reads R, T or the self ids.

namespace RT_NS {

template <int kVar, int kTex, int kMedia, bool kMats, bool kInst, int kLeaf>
RT_FN void path_sample(const KernelParams& P0, const real* prims_, const Trav& W, uint32_t pix, uint32_t pxgy, int sample,
                       Acc& A, bool& bad, int& overflow) {
  constexpr bool kFlat = kVar == RT_VAR_FLAT;
  // the deferred redirect pdf of the diffuse flat classes (lane_loop_lockstep kDefer)
  constexpr bool kDefer = kFlat && kMedia == 0 && !kMats;
  const cfp prims = cf(prims_);
  RayCtx R;
  R.o = R.d = mk3(RL(0.), RL(0.), RL(0.));
#if RT_NODE_F32
  R.idir = R.off0 = R.off1 = f3n{0.f, 0.f, 0.f};
#else
  R.idir = R.oidir = R.o;
#endif
  R.time_w = 0u;
  R.self_gid = -1;
  R.self_inst = -1;
  {
    const KernelParams& P = RT_KARGS(P0);  // (re-read per phase, as the lane loops: rt_trace.h RT_KARGS)
    if constexpr (kFlat)
      camera_ray_flat(P, pix, sample, pxgy, R);
    else
      camera_ray(P, pix, sample, ~0u, R);
  }
  f3 T = mk3(RL(1.), RL(1.), RL(1.));
  real apdf = RL(1.);
  int seg = 0;
  // one closest-hit query over a set (rt_features.h feature_sample's)
  auto query = [&](int root, int set, real tmin, Closest& C) {
    const KernelParams& P = RT_KARGS(P0);
    if constexpr (kFlat) {
      closest<true>(P, prims, root, set, R, tmin, C, W, &overflow);
    } else {
      TravState S;
      trav_begin(S, root, tmin);
      if (set == 0) {
        prefix_hits<kInst>(P, prims, R, tmin, S.C);
      } else if (kLeaf != 0 && S.node == RT_EMPTY_ROOT) {
        test_leaf_generic<kInst>(P, R, S);
      }
      while (!trav_done(S)) trav_round<kInst, kLeaf>(P, R, S, W, overflow RT_PROF_NULLARG);
      C = S.C;
    }
  };
  for (;;) {
    const KernelParams& P = RT_KARGS(P0);
    if constexpr (!kFlat) prep_ray(R);
    Closest C = no_hit();
    if constexpr (kDefer) {
      closest_flat<true>(P, 0, R, kTmin, C, &apdf);
      if (P.target_defer) T = (seg == 0 ? RL(1.) : RT_RCP(apdf)) * T;
    } else {
      query(P.surface_root, 0, kTmin, C);
    }
    real tbest = C.t;
    const int best = C.prim;
    int best_inst = -1;
    if constexpr (kInst) best_inst = C.inst;
    int hit_medium = -1;
    if constexpr (kMedia == 2) {
      media_events_late<kInst>(P, prims, R, pix, sample, seg, best, tbest, tbest, hit_medium);
    } else if constexpr (kMedia == 1) {
      // constantMedium (Geometry.hs:306-328), the order of lane_loop_lockstep
      for (int m = 0; m < P.n_media; ++m) {
        const DevMedium& M = P.media[m];
        Closest C1 = no_hit();
        if (M.alias_surface) {
          C1.t = C.t;
          C1.prim = C.prim;
        } else {
          query(M.root, m + 1, kTmin, C1);
        }
        if (C1.prim < 0) continue;
        const real t1 = C1.t;
        real lo, hi;
        if (prim_front(P, prims, C1.prim, R, t1)) {
          if (!(t1 < tbest)) continue;
          Closest C2 = no_hit();
          query(M.root, m + 1, t1, C2);
          if (C2.prim < 0) continue;
          lo = t1;
          hi = C2.t;
        } else {
          lo = kTmin;
          hi = t1;
        }
        medium_event(P, m, pix, sample, seg, lo, hi, tbest, hit_medium);
      }
    }
    f3 L = mk3(RL(0.), RL(0.), RL(0.));
    bool ended;
    if constexpr (kDefer)
      ended = shade<kTex, kMats, false>(P, prims, pix, sample, seg, tbest, best, hit_medium, R, L, T, -1, &apdf);
    else
      ended = shade<kTex, kMats, kInst>(P, prims, pix, sample, seg, tbest, best, hit_medium, R, L, T, best_inst);
    if (ended) {  // (R, T and apdf are indeterminate from here: shade's invariant)
      acc_sample(A, L, bad);
      return;
    }
  }
}

// Samples [s0, s1) of tile pixel tp (the rt_exec row interleave of rt_trace.h open_item) summed into
// A.  A shard's padding row and a render without depth have none, as open_item: false
template <int kVar, int kTex, int kMedia, bool kMats, bool kInst, int kLeaf>
RT_FN bool path_pixel(const KernelParams& P, const Trav& W, int tp, int s0, int s1, Acc& A, bool& bad, int& overflow) {
  const int width = P.cam.width;
  const int tr = (int)fast_div((uint32_t)tp, P.div_width);
  const int px = tp - tr * width;
  const int tb = (int)fast_div((uint32_t)tr, P.div_block);
  const int gy = (tb * P.n_shards + P.shard) * P.row_block + (tr - tb * P.row_block);
  if (gy >= P.cam.height || P.cam.max_depth <= 0) return false;
  const uint32_t pix = (uint32_t)(gy * width + px), pxgy = (uint32_t)gy << 16 | (uint32_t)px;
  for (int s = s0; s < s1; ++s) path_sample<kVar, kTex, kMedia, kMats, kInst, kLeaf>(P, P.prims, W, pix, pxgy, s, A, bad, overflow);
  return true;
}

}  // namespace RT_NS
