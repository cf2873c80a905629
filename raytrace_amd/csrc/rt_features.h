// rt_features.h — the first-hit feature sample of ONE precision: included after rt_trace.h of the
// same RT_F64, includes rt_lane.h itself (no include guard, as rt_trace.h's per-precision part), by
// rt_features.hip / rt_features64_nl.hip for the device and by tests/feature_emu for the host
// (RT_HOST_EMU).
//
// feature_sample traces the primary ray of (pixel, sample) — rt_trace.h camera_ray, the render's
// Philox key and events — to its first event: segment 0 of rt_lane.h segment_events, with no
// deferred pdf.  It adds 8 words (rt_denoise.h RT_FEAT_WORDS):
//   albedo RGB  the hit material's texture at the hit's (point, uv); dielectric 1, pitchBlack 0;
//               the phase material's texture in a medium; the background of the ray on a miss
//   normal xyz  the unit normal facing the ray, as the materials see it; 0 in a medium or on a miss
//   depth, hits the hit's t and 1; nothing on a miss
// each real in the render's fixed point (rt_trace.h acc_add / to_fixed): FP32 one word in units of
// 2^-32; binary64 that word and a second one with the next 32 bits, as the render's own sums
// (rt_internal.h RT_ACC_WORDS).  A pixel's words: 8 high words, then (binary64) 8 low words, the
// last of them unused.  A non-finite value adds nothing.  Integer sums: the order of the samples
// does not matter.

#include "rt_lane.h"  // (per precision, like this file: no include guard, included by exactly one body header)

namespace RT_NS {

struct FeatAcc {
  long long w[8];
#if RT_F64
  unsigned long long lo[8];
#endif
};

// word k += the render's fixed-point words of x; a non-finite value adds nothing
RT_FN void feat_add(FeatAcc& A, int k, real x) {
#if RT_F64
  if (!(RABS(x) < RL(1.0e9))) return;
  fixed_words_add(x, A.w[k], A.lo[k]);
#else
  bool bad = false;
  A.w[k] += to_fixed(x, bad);
#endif
}

// The classes' template arguments that matter here: the set representation (flat / BVH), the
// texture level, the media mode, instancing and the leaf class (rt_kernel_class.h KernelClass; the
// material set and the workgroup size change nothing a first hit sees).
template <int kVar, int kTex, int kMedia, bool kInst, int kLeaf>
RT_FN void feature_sample(const KernelParams& P0, const real* prims_, const Trav& W, uint32_t pix, uint32_t pxgy, int sample,
                          FeatAcc& A, int& overflow) {
  const cfp prims = cf(prims_);
  RayCtx R;
  ray_clear(R);
  {
    // (the kernel arguments re-read per phase, as the render's lane loops do: rt_trace.h RT_KARGS)
    const KernelParams& P = RT_KARGS(P0);
    if constexpr (kVar == RT_VAR_FLAT)
      camera_ray_flat(P, pix, sample, pxgy, R);
    else
      camera_ray(P, pix, sample, ~0u, R);
  }
  const SegEvent E = segment_events<kVar, kMedia, kInst, kLeaf>(P0, prims, W, R, pix, sample, 0, overflow);
  const KernelParams& P = RT_KARGS(P0);
  const bool miss = E.medium < 0 && E.prim < 0;
  f3 tex = mk3(RL(0.), RL(0.), RL(0.)), n = tex;
  if (miss) {
    tex = background(P, R.d);
  } else {  // the material and the hit, as shade_event reads them
    const RT_CAS DevMaterial* Mp = hit_material<kInst>(P, E.prim, E.inst, E.medium);
    const int kind = Mp->kind;
    const bool need_tex = kTex > 0 && !Mp->tex_const && kind != RT_MAT_PITCH_BLACK && kind != RT_MAT_DIELECTRIC;
    HitInfo h;
    if (E.medium >= 0) {
      h.p = R.o + E.t * R.d;
      h.u = h.v = RL(0.);
    } else {
      h = surface_info_world<kInst>(P, prims, E.prim, E.inst, R, E.t, need_tex);
      n = h.n;
    }
    tex = f3{Mp->c0[0], Mp->c0[1], Mp->c0[2]};
    if (need_tex) tex = eval_texture<kTex == 2>(P, Mp->tex, h.u, h.v, h.p);
    if (kind == RT_MAT_DIELECTRIC) tex = mk3(RL(1.), RL(1.), RL(1.));
    if (kind == RT_MAT_PITCH_BLACK) tex = mk3(RL(0.), RL(0.), RL(0.));
  }
  feat_add(A, 0, tex.x);
  feat_add(A, 1, tex.y);
  feat_add(A, 2, tex.z);
  if (!miss) {
    feat_add(A, 3, n.x);
    feat_add(A, 4, n.y);
    feat_add(A, 5, n.z);
    feat_add(A, 6, E.t);
    A.w[7] += 1;
  }
}

// The samples [s0, s1) of tile pixel tp (rt_trace.h tile_pixel; a shard's padding rows have none)
// summed into A; false for a padding row
template <int kVar, int kTex, int kMedia, bool kInst, int kLeaf>
RT_FN bool feature_pixel(const KernelParams& P, const Trav& W, int tp, int s0, int s1, FeatAcc& A, int& overflow) {
  int gy;
  uint32_t pix, pxgy;
  tile_pixel(P, tp, gy, pix, pxgy);
  if (gy >= P.cam.height) return false;
  for (int s = s0; s < s1; ++s) feature_sample<kVar, kTex, kMedia, kInst, kLeaf>(P, P.prims, W, pix, pxgy, s, A, overflow);
  return true;
}

}  // namespace RT_NS
