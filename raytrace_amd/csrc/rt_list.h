// rt_list.h — one whole path of ONE precision, per lane: included after rt_trace.h of the same
// RT_F64, includes rt_lane.h itself (no include guard, as rt_trace.h's per-precision part), by rt_list.hip /
// rt_list64_nl.hip for the device and by tests/list_emu for the host (RT_HOST_EMU).
//
// The render kernels' lane loops (rt_trace.h lane_loop_lockstep, lane_loop_flat_ring, lane_loop_bvh)
// interleave the paths of a work queue's items; they take a pixel from the shard formula and a
// sample range from one sample0 (open_item).  An adaptive film pass (rt_adaptive.h) renders a LIST
// of pixels, each from its own first sample, so it needs the path as a function of (pixel, sample):
// path_sample runs sample `sample` of global pixel `pix` from the camera to the event that ends it
// and adds its radiance to an Acc — the render's Philox key, camera_ray_flat / camera_ray, then per
// segment the events (rt_lane.h segment_events; in the diffuse flat classes with the deferred
// redirect pdf, as lane_loop_lockstep) and shade — so a pixel's sums over samples [a, b) are the
// render's, word for word.  shade's invariant holds: after it returns true nothing reads R, T or the
// self ids.

#include "rt_lane.h"  // (per precision, like this file: no include guard, included by exactly one body header)

namespace RT_NS {

template <int kVar, int kTex, int kMedia, bool kMats, bool kInst, int kLeaf>
RT_FN void path_sample(const KernelParams& P0, const real* prims_, const Trav& W, uint32_t pix, uint32_t pxgy, int sample,
                       Acc& A, bool& bad, int& overflow) {
  constexpr bool kFlat = kVar == RT_VAR_FLAT;
  // the deferred redirect pdf of the diffuse flat classes (lane_loop_lockstep kDefer)
  constexpr bool kDefer = kFlat && kMedia == 0 && !kMats;
  const cfp prims = cf(prims_);
  RayCtx R;
  ray_clear(R);
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

// Samples [s0, s1) of tile pixel tp (rt_trace.h tile_pixel) summed into A.  A shard's padding row and
// a render without depth have none, as open_item: false
template <int kVar, int kTex, int kMedia, bool kMats, bool kInst, int kLeaf>
RT_FN bool path_pixel(const KernelParams& P, const Trav& W, int tp, int s0, int s1, Acc& A, bool& bad, int& overflow) {
  int gy;
  uint32_t pix, pxgy;
  tile_pixel(P, tp, gy, pix, pxgy);
  if (gy >= P.cam.height || P.cam.max_depth <= 0) return false;
  for (int s = s0; s < s1; ++s) path_sample<kVar, kTex, kMedia, kMats, kInst, kLeaf>(P, P.prims, W, pix, pxgy, s, A, bad, overflow);
  return true;
}

}  // namespace RT_NS
