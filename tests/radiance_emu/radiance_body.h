// radiance_body.h — TEST TOOLING: the host loops over the radiance-query body for ONE precision
// (included by rt_radiance_emu.cpp once per precision, after rt_trace.h and rt_radiance.h of the same
// RT_F64).

// n_samples samples of every ray through the instantiation the device's dispatch picks
// (rt_radiance_kernel.h radiance_kernel_of: the variant's class with narrow cleared), added to the
// rays' workspace words (kRadWords per ray; zeroed first without RT_RADIANCE_ACCUMULATE) and resolved
// into out, as the device's two kernels do.  The argument block is the library's: rt_host_render_params
// of rt_host_radiance_camera(cs)
int radiance(const HostScene& H, const rt_camera_settings* cs, uint64_t seed, const rt_path_ray* rays, long long n,
             int n_samples, int flags, unsigned long long* work, rt_radiance* out, std::string& err) {
  using namespace RT_NS;
  const int variant = rt_host_variant(H);
  const rt_camera_settings c1 = rt_host_radiance_camera(cs);
  rt_exec ex{};
  ex.n_shards = 1;
  ex.row_block = 4;
  LaunchInputs L;
  L.resident_lanes = 4096;
  RT_NS::KernelParams P;
  if (int rc = rt_host_render_params(H, variant, rt_host_records<real>(H), &c1, seed, &ex, L, P, err)) return rc;
  std::vector<int> stack(P.stack_depth + 1);
  const Trav W{stack.data(), 1, nullptr};
  KernelClass cls = rt_class_of(RT_F64, variant);
  cls.narrow = false;
  int overflow = 0;
  if (!(flags & RT_RADIANCE_ACCUMULATE)) std::memset(work, 0, (size_t)n * kRadWords * sizeof(unsigned long long));
  const bool ran = rt_with_class(cls, [&](auto... k) -> bool {
    constexpr KernelClass c{decltype(k)::value...};
    if constexpr (rt_class_compiled(RT_F64, c) && !c.narrow && c.var != RT_VAR_BVH_LOCKSTEP) {
      for (long long i = 0; i < n; ++i) {
        Acc A;
        acc_clear(A);
        bool bad = false;
        const bool ok = path_record<c.var, c.tex, c.media, c.mats, c.inst, c.leaf>(P, W, rays[i], flags, 0, n_samples, A, bad, overflow);
        unsigned long long* dst = work + (size_t)kRadWords * (size_t)i;
        if (ok) {
          for (int ch = 0; ch < 3; ++ch) dst[ch] += (unsigned long long)A.hi[ch];
#if RT_F64
          for (int ch = 0; ch < 3; ++ch) dst[3 + ch] += A.lo[ch];
#endif
          dst[kRadWords - 1] += rad_count_word((uint32_t)n_samples);
          if (bad) dst[kRadWords - 1] |= 1ull;
        }
        radiance_resolve(dst, ok, out[i]);
      }
      return true;
    }
    return false;
  });
  if (!ran) {
    err = "no radiance instantiation for this scene's class";
    return RT_E_GENERIC;
  }
  if (overflow) {
    err = "BVH traversal stack overflow";
    return RT_E_STACK;
  }
  return RT_OK;
}

// the render's camera ray of (pixel, sample) for every pixel of cs's frame, row-major (one shard)
int camera_rays(const HostScene& H, const rt_camera_settings* cs, uint64_t seed, int sample, rt_path_ray* rays, std::string& err) {
  using namespace RT_NS;
  const int variant = rt_host_variant(H);
  rt_exec ex{};
  ex.n_shards = 1;
  ex.row_block = 4;
  LaunchInputs L;
  L.resident_lanes = 4096;
  RT_NS::KernelParams P;
  if (int rc = rt_host_render_params(H, variant, rt_host_records<real>(H), cs, seed, &ex, L, P, err)) return rc;
  const bool flat = rt_class_of(RT_F64, variant).var == RT_VAR_FLAT;
  for (int gy = 0; gy < P.cam.height; ++gy)
    for (int px = 0; px < P.cam.width; ++px) {
      const int i = gy * P.cam.width + px;
      if (flat)
        camera_ray_record<true>(P, (uint32_t)i, gy, px, sample, rays[i]);
      else
        camera_ray_record<false>(P, (uint32_t)i, gy, px, sample, rays[i]);
    }
  return RT_OK;
}
