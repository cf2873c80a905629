// emu_body.h — TEST TOOLING: the host emulator's render loop for ONE precision (included by
// rt_emu.cpp once per precision, after rt_trace.h of the same RT_F64).

struct Shared {
  const RT_NS::KernelParams* P;
  int variant;
  std::atomic<int> next{0};
  std::atomic<int> overflow{0};
  std::vector<std::atomic<long long>>* accum;
  std::vector<std::atomic<unsigned>>* flags;
  std::atomic<long long> cnt[4];
};

// the device kernel's WaveWork without waves: one shared counter, every item committed directly
struct Work {
  Shared* s;
  int grab(bool need, int& slot) {
    slot = -1;
    return need ? s->next.fetch_add(1) : 0;
  }
  int tag(int tp, int slot) const {
    (void)slot;
    return tp;
  }
  template <class AccT>
  void commit(bool c, int tp, const AccT& acc, bool bad) {
    if (!c) return;
    const RT_NS::Acc A = RT_NS::acc_words(acc);
    const size_t w = RT_ACC_WORDS(RT_NS::real);
    for (int k = 0; k < 3; ++k) (*s->accum)[w * (size_t)tp + k] += A.hi[k];
#if RT_F64
    for (int k = 0; k < 3; ++k) (*s->accum)[w * (size_t)tp + 3 + k] += (long long)A.lo[k];
#endif
    if (bad) (*s->flags)[tp] |= 1u;
  }
};

// the lane loop of the variant's kernel class: the device kernels' own dispatch (rt_kernel_class.h
// rt_class_of), so the emulator runs the instantiation the device runs
template <class G>
int run_variant(const RT_NS::KernelParams& P, int variant, G& g, const RT_NS::Trav& W) {
  // the item sums through the device kernels' LDS accumulator (one lane: stride 1)
  unsigned long long words[6] = {0, 0, 0, 0, 0, 0};
  RT_NS::AccLds acc{words, 1};
  KernelClass cls = rt_class_of(RT_F64, variant);
  cls.narrow = false;  // (the workgroup size: nothing the lane loop sees)
  return rt_with_class(cls, [&](auto... k) -> int {
    constexpr KernelClass c{decltype(k)::value...};
    if constexpr (!rt_class_compiled(RT_F64, c))
      return 0;  // (no such kernel: rt_class_of names none of these)
    else if constexpr (c.var == RT_VAR_BVH)
      return RT_NS::lane_loop_bvh<c.tex, c.media, c.mats, c.inst, c.leaf>(P, g, W, P.prims, acc);
    else
      return RT_NS::lane_loop_lockstep<c.var == RT_VAR_FLAT, c.tex, c.media != 0, c.mats>(P, g, W, P.prims, acc);
  });
}

void* worker(void* arg) {
  Shared* s = (Shared*)arg;
  std::vector<int> stack(s->P->stack_depth + 1);
  for (auto& c : rt_emu::counters) c = 0;
  Work g{s};
  const RT_NS::Trav W{stack.data(), 1, nullptr};  // the emulator reads every node from memory
  int ov = run_variant(*s->P, s->variant, g, W);
  if (ov) s->overflow = 1;
  for (int i = 0; i < 4; ++i) s->cnt[i] += rt_emu::counters[i];
  return nullptr;
}

// the kernel arguments of one render of the host scene in this precision: the library's own fill
// (rt_build.cpp rt_host_render_params) over the host's records, as an overlapped render on 4096
// resident lanes with no nodes in LDS; `chunk` > 0 overrides the plan with one item size
int params(const HostScene& H, int variant, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex,
           RT_NS::real* out, int chunk, RT_NS::KernelParams& P, std::string& err) {
  LaunchInputs L;
  L.resident_lanes = 4096;
  if (int rc = rt_host_render_params(H, variant, rt_host_records<RT_NS::real>(H), cs, seed, ex, L, P, err)) return rc;
  P.out = out;
  if (chunk > 0) {
    P.chunk = chunk;
    P.n_chunks = (P.cam.spp + chunk - 1) / chunk;
    P.n_big_chunks = 0;
    P.big_items = 0;
    P.small_start = 0;
    P.div_small = rt_host_fastdiv((uint32_t)P.n_chunks);
    P.n_items = P.n_chunks * P.tile_rows * P.cam.width;
  }
  return RT_OK;
}

// one render of the host scene in this precision; out: tile_rows x width x 3 reals
int render(const HostScene& H, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex, RT_NS::real* out,
           int nthreads, int chunk, long long* counters, std::string& err) {
  using real = RT_NS::real;
  RT_NS::KernelParams P;
  const int variant = rt_host_variant(H);
  if (int rc = params(H, variant, cs, seed, ex, out, chunk, P, err)) return rc;
  const size_t tile_pixels = (size_t)P.tile_rows * P.cam.width;
  const size_t w = RT_ACC_WORDS(real);
  std::vector<std::atomic<long long>> accum(tile_pixels * w);
  std::vector<std::atomic<unsigned>> flags(tile_pixels);
  for (auto& a : accum) a = 0;
  for (auto& f : flags) f = 0;
  Shared s;
  s.P = &P;
  s.variant = variant;
  s.accum = &accum;
  s.flags = &flags;
  for (auto& c : s.cnt) c = 0;
  if (nthreads < 1) nthreads = 1;
  if (nthreads > 64) nthreads = 64;
  pthread_t th[64];
  for (int t = 1; t < nthreads; ++t) pthread_create(&th[t], nullptr, worker, &s);
  worker(&s);
  for (int t = 1; t < nthreads; ++t) pthread_join(th[t], nullptr);
  for (size_t i = 0; i < tile_pixels; ++i)
    for (int c = 0; c < 3; ++c) {
      const long long hi = accum[w * i + c].load();
#if RT_F64
      // as rt_render_kernel.h rt_resolve_kernel
      const double lo = (double)(unsigned long long)accum[w * i + 3 + c].load();
      const double sum = ((double)hi + lo * (1.0 / RT_FIX_SCALE)) * (1.0 / RT_FIX_SCALE);
      out[3 * i + c] = flags[i] ? NAN : sum / (double)P.cam.spp;
#else
      out[3 * i + c] = flags[i] ? NAN : (float)((double)hi * (1.0 / (RT_FIX_SCALE * (double)P.cam.spp)));
#endif
    }
  if (counters) {
    for (int i = 0; i < 3; ++i) counters[i] = s.cnt[i];
    counters[3] = (long long)tile_pixels * P.cam.spp;
  }
  if (s.overflow) {
    err = "BVH traversal stack overflow";
    return RT_E_STACK;
  }
  return RT_OK;
}
