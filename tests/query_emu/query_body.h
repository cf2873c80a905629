// query_body.h — TEST TOOLING: the host loop over the query body for ONE precision (included by
// rt_query_emu.cpp once per precision, after rt_trace.h and rt_query.h of the same RT_F64).

// every ray through the instantiation the device's dispatch picks (rt_query_kernel.h
// query_kernel_of_class: the variant's class with tex, media, mats and narrow cleared), its
// arguments made as rt_api_query.hip cast_enqueue makes them (unit_camera, one_shard)
int cast(const HostScene& H, const rt_ray* rays, rt_hit* hits, long long n, int flags, std::string& err) {
  using namespace RT_NS;
  rt_camera_settings cs{};
  cs.look_at[2] = -1.0;
  cs.up[1] = 1.0;
  cs.vfov = 1.0;
  cs.aspect_ratio = 1.0;
  cs.image_width = cs.samples_per_pixel = cs.max_recursion_depth = 1;
  cs.focus_dist = 1.0;
  rt_exec ex{};
  ex.n_shards = 1;
  ex.row_block = 4;
  const int variant = rt_host_variant(H);
  LaunchInputs L;
  L.resident_lanes = 4096;
  RT_NS::KernelParams P;
  if (int rc = rt_host_render_params(H, variant, rt_host_records<real>(H), &cs, 0, &ex, L, P, err)) return rc;
  // (tests: fewer stack rows than the scene's BVH needs, as rt_api_query.hip cast_enqueue reads the knob)
  if (const char* e = rt_knob("RT_AMD_CAST_STACK")) P.stack_depth = std::max(1, std::min(P.stack_depth, atoi(e)));
  std::vector<int> stack(P.stack_depth + 1);
  const Trav W{stack.data(), 1, nullptr};
  KernelClass cls = rt_class_of(RT_F64, variant);
  cls.tex = 0;
  cls.media = 0;
  cls.mats = false;
  cls.narrow = false;
  int overflow = 0;
  const bool ran = rt_with_class(cls, [&](auto... k) -> bool {
    constexpr KernelClass c{decltype(k)::value...};
    if constexpr (rt_class_compiled(RT_F64, c) && c.var != RT_VAR_BVH_LOCKSTEP) {
      for (long long i = 0; i < n; ++i)
        query_ray<c.var, c.inst, c.leaf>(P, P.prims, H.prim_mat.data(), W, rays[i], flags, hits[i], overflow);
      return true;
    }
    return false;
  });
  if (!ran) {
    err = "no query instantiation for this scene's class";
    return RT_E_GENERIC;
  }
  if (overflow) {
    err = "BVH traversal stack overflow";
    return RT_E_STACK;
  }
  return RT_OK;
}
