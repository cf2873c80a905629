// rt_features.h — the first-hit feature sample of ONE precision: included after rt_trace.h of the
// same RT_F64 (no include guard, as rt_trace.h's per-precision part), by rt_features.hip /
// rt_features64_nl.hip for the device and by tests/feature_emu for the host (RT_HOST_EMU).
//
// feature_sample traces the primary ray of (pixel, sample) — rt_trace.h camera_ray, the render's
// Philox key and events — to its first event exactly as the render's segment 0 finds it: the
// surface query (the flat sets, or the prefix and trav_round with the class's instancing and leaf
// flags), then the segment's medium events with the render's own Philox words (the query chain or
// media_events_late, by the class's media mode).  It adds 8 words (rt_denoise.h RT_FEAT_WORDS):
//   albedo RGB  the hit material's texture at the hit's (point, uv); dielectric 1, pitchBlack 0;
//               the phase material's texture in a medium; the background of the ray on a miss
//   normal xyz  the unit normal facing the ray, as the materials see it; 0 in a medium or on a miss
//   depth, hits the hit's t and 1; nothing on a miss
// each real in the render's fixed point (rt_trace.h acc_add / to_fixed): FP32 one word in units of
// 2^-32; binary64 that word and a second one with the next 32 bits, as the render's own sums
// (rt_internal.h RT_ACC_WORDS).  A pixel's words: 8 high words, then (binary64) 8 low words, the
// last of them unused.  A non-finite value adds nothing.  Integer sums: the order of the samples
// does not matter.

namespace RT_NS {

struct FeatAcc {
  long long w[8];
#if RT_F64
  unsigned long long lo[8];
#endif
};

// word k += the render's fixed-point words of x
RT_FN void feat_add(FeatAcc& A, int k, real x) {
#if RT_F64
  if (!(RABS(x) < RL(1.0e9))) return;  // (rt_trace.h acc_add: non-finite)
  const real xs = x * RL(4294967296.0);
  const real fl = RFLOOR(xs);
  A.w[k] += (long long)fl;
  A.lo[k] += (unsigned long long)(unsigned)((xs - fl) * RL(4294967296.0));
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
  constexpr bool kFlat = kVar == RT_VAR_FLAT;
  const cfp prims = cf(prims_);
  RayCtx R;
  R.o = R.d = mk3(RL(0.), RL(0.), RL(0.));
#if RT_NODE_F32
  R.idir = R.off0 = R.off1 = f3n{0.f, 0.f, 0.f};
#else
  R.idir = R.oidir = R.o;
#endif
  R.time_w = 0u;
  // (the kernel arguments re-read per phase, as the render's lane loops do: rt_trace.h RT_KARGS)
  const KernelParams& P = RT_KARGS(P0);
  if constexpr (kFlat) {
    camera_ray_flat(P, pix, sample, pxgy, R);
  } else {
    camera_ray(P, pix, sample, ~0u, R);
    prep_ray(R);
  }
  // one closest-hit query over a set, as the render's lane loops run it (rt_trace.h closest_flat;
  // lane_loop_bvh: the surface prefix first, a single-leaf medium set by the generic test)
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
  Closest C = no_hit();
  query(P.surface_root, 0, kTmin, C);
  real tbest = C.t;
  const int best = C.prim, best_inst = C.inst;
  int hit_medium = -1;
  if constexpr (kMedia == 2) {
    media_events_late<kInst>(P, prims, R, pix, sample, 0, best, tbest, tbest, hit_medium);
  } else if constexpr (kMedia == 1) {
    // constantMedium (Geometry.hs:306-328), the order of rt_trace.h lane_loop_lockstep
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
      medium_event(P, m, pix, sample, 0, lo, hi, tbest, hit_medium);
    }
  }
  const bool miss = hit_medium < 0 && best < 0;
  f3 tex = mk3(RL(0.), RL(0.), RL(0.)), n = tex;
  if (miss) {  // cs_background (rt_trace.h shade_event)
    const KernelParams& P = RT_KARGS(P0);
    tex = ld3(P.cam.bg0);
    if (P.cam.bg_kind == 1) {
      const real a = RL(0.5) * (R.d.y + RL(1.0));
      tex = (RL(1.0) - a) * tex + a * ld3(P.cam.bg1);
    }
  } else {  // the material and the hit, as shade_event reads them
    const KernelParams& P = RT_KARGS(P0);
    const RT_CAS DevMaterial* Mp = hit_medium >= 0 ? (const RT_CAS DevMaterial*)P.mats + P.media[hit_medium].material
                                                   : (const RT_CAS DevMaterial*)P.prim_shade + best;
    if constexpr (kInst) {
      if (hit_medium < 0 && best_inst >= 0) {
        const int im = inst_rec(P, best_inst)->material;
        if (im >= 0) Mp = (const RT_CAS DevMaterial*)P.mats + im;
      }
    }
    const int kind = Mp->kind;
    const bool need_tex = kTex > 0 && !Mp->tex_const && kind != RT_MAT_PITCH_BLACK && kind != RT_MAT_DIELECTRIC;
    HitInfo h;
    if (hit_medium >= 0) {
      h.p = R.o + tbest * R.d;
      h.u = h.v = RL(0.);
    } else {
      bool in_object = false;
      if constexpr (kInst) {
        if (best_inst >= 0) {  // hit information in object space, point and normal back to world
          const RT_CAS DevInstance* I = inst_rec(P, best_inst);
          RayCtx Ro = R;
          Ro.o = inst_to_object(I, R.o, true);
          Ro.d = inst_to_object(I, R.d, false);
          h = surface_info(P, prims, best, Ro, tbest, need_tex);
          h.p = R.o + tbest * R.d;
          h.n = inst_rotate(I, h.n);
          in_object = true;
        }
      }
      if (!in_object) h = surface_info(P, prims, best, R, tbest, need_tex);
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
    feat_add(A, 6, tbest);
    A.w[7] += 1;
  }
}

// The samples [s0, s1) of tile pixel tp (the rt_exec row interleave of rt_trace.h open_item; a
// shard's padding rows have none) summed into A; false for a padding row
template <int kVar, int kTex, int kMedia, bool kInst, int kLeaf>
RT_FN bool feature_pixel(const KernelParams& P, const Trav& W, int tp, int s0, int s1, FeatAcc& A, int& overflow) {
  const int width = P.cam.width;
  const int tr = (int)fast_div((uint32_t)tp, P.div_width);
  const int px = tp - tr * width;
  const int tb = (int)fast_div((uint32_t)tr, P.div_block);
  const int gy = (tb * P.n_shards + P.shard) * P.row_block + (tr - tb * P.row_block);
  if (gy >= P.cam.height) return false;
  const uint32_t pix = (uint32_t)(gy * width + px), pxgy = (uint32_t)gy << 16 | (uint32_t)px;
  for (int s = s0; s < s1; ++s) feature_sample<kVar, kTex, kMedia, kInst, kLeaf>(P, P.prims, W, pix, pxgy, s, A, overflow);
  return true;
}

}  // namespace RT_NS
