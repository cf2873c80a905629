// list_body.h — TEST TOOLING: the host loop over the per-pixel path body for ONE precision (included
// by rt_list_emu.cpp once per precision, after rt_trace.h and rt_list.h of the same RT_F64).

// samples [0, counts[tp]) of every tile pixel through the instantiation the device's dispatch picks
// (rt_list_kernel.h list_kernel_of: the variant's class with narrow cleared), resolved with the
// pixel's own count (rt_adaptive.h); out: tile pixels x 3 reals
int render(const HostScene& H, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex, const uint32_t* counts,
           RT_NS::real* out, std::string& err) {
  using namespace RT_NS;
  const int variant = rt_host_variant(H);
  LaunchInputs L;
  L.resident_lanes = 4096;
  RT_NS::KernelParams P;
  if (int rc = rt_host_render_params(H, variant, rt_host_records<real>(H), cs, seed, ex, L, P, err)) return rc;
  const int pixels = P.tile_rows * P.cam.width;
  std::vector<int> stack(P.stack_depth + 1);
  const Trav W{stack.data(), 1, nullptr};
  KernelClass cls = rt_class_of(RT_F64, variant);
  cls.narrow = false;
  int overflow = 0;
  const bool ran = rt_with_class(cls, [&](auto... k) -> bool {
    constexpr KernelClass c{decltype(k)::value...};
    if constexpr (rt_class_compiled(RT_F64, c) && !c.narrow && c.var != RT_VAR_BVH_LOCKSTEP) {
      for (int tp = 0; tp < pixels; ++tp) {
        Acc A;
        acc_clear(A);
        bool bad = false;
        const uint32_t n = counts[tp];
        path_pixel<c.var, c.tex, c.media, c.mats, c.inst, c.leaf>(P, W, tp, 0, (int)n, A, bad, overflow);
        for (int ch = 0; ch < 3; ++ch) {
#if RT_F64
          out[3 * tp + ch] = bad ? NAN : n ? rt_adaptive_resolve64(A.hi[ch], A.lo[ch], n) : 0.0;
#else
          out[3 * tp + ch] = bad ? NAN : n ? rt_adaptive_resolve32(A.hi[ch], n) : 0.f;
#endif
        }
      }
      return true;
    }
    return false;
  });
  if (!ran) {
    err = "no list instantiation for this scene's class";
    return RT_E_GENERIC;
  }
  if (overflow) {
    err = "BVH traversal stack overflow";
    return RT_E_STACK;
  }
  return RT_OK;
}
