// feature_body.h — TEST TOOLING: the host loop over the feature body for ONE precision (included by
// rt_feature_emu.cpp once per precision, after rt_trace.h and rt_features.h of the same RT_F64).

// every tile pixel's samples [0, n_feat) through the instantiation the device's dispatch picks
// (rt_features_kernel.h feature_kernel_of: the variant's class with mats and narrow cleared)
int features(const HostScene& H, const rt_camera_settings* cs0, uint64_t seed, const rt_exec* ex, int n_feat,
             long long* out, std::string& err) {
  using namespace RT_NS;
  rt_camera_settings cs = *cs0;
  cs.samples_per_pixel = n_feat;
  const int variant = rt_host_variant(H);
  LaunchInputs L;
  L.resident_lanes = 4096;
  RT_NS::KernelParams P;
  if (int rc = rt_host_render_params(H, variant, rt_host_records<real>(H), &cs, seed, ex, L, P, err)) return rc;
  const int fw = rt_feat_words(RT_F64);
  const int pixels = P.tile_rows * P.cam.width;
  std::memset(out, 0, sizeof(long long) * (size_t)fw * pixels);
  std::vector<int> stack(P.stack_depth + 1);
  const Trav W{stack.data(), 1, nullptr};
  KernelClass cls = rt_class_of(RT_F64, variant);
  cls.mats = false;
  cls.narrow = false;
  int overflow = 0;
  const bool ran = rt_with_class(cls, [&](auto... k) -> bool {
    constexpr KernelClass c{decltype(k)::value...};
    if constexpr (rt_class_compiled(RT_F64, c) && c.var != RT_VAR_BVH_LOCKSTEP) {
      for (int tp = 0; tp < pixels; ++tp) {
        FeatAcc A{};
        if (!feature_pixel<c.var, c.tex, c.media, c.inst, c.leaf>(P, W, tp, 0, n_feat, A, overflow)) continue;
        for (int w = 0; w < RT_FEAT_WORDS; ++w) out[(size_t)fw * tp + w] = A.w[w];
#if RT_F64
        for (int w = 0; w < RT_FEAT_WORDS - 1; ++w) out[(size_t)fw * tp + RT_FEAT_WORDS + w] = (long long)A.lo[w];
#endif
      }
      return true;
    }
    return false;
  });
  if (!ran) {
    err = "no feature instantiation for this scene's class";
    return RT_E_GENERIC;
  }
  if (overflow) {
    err = "BVH traversal stack overflow";
    return RT_E_STACK;
  }
  return RT_OK;
}
