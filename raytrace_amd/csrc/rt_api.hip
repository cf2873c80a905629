// rt_api.hip — scenes and renders behind include/rt.h: scene build (rt_build.cpp, once per
// call however many devices render), upload to HBM (a precision's records on its first render),
// kernel launch (rt_kernel.hip / rt_kernel64.hip), multi-device scenes (one process, many GPUs:
// concurrent uploads, shard renders on per-device streams, a device-side gather by peer copies
// into the first device's framebuffer and ONE device-to-host copy), the 8-bit output epilogue,
// error reporting.  The film, adaptive passes and the denoiser's buffers are rt_api_film.hip's, ray
// queries and ray orders rt_api_query.hip's; rt_api_internal.h holds what the three share.
// A synchronous render (render_sync) runs render_one (one device) or render_many (a thread per
// shard) over the same stages: prepare_part, enqueue_shard, enqueue_readback, fill_stats.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "rt_api_internal.h"
#include "rt_kernel_class.h"

// ---- what the other units call too (declared in rt_api_internal.h)
namespace rt_api {

static thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
int fail_stack() { return fail(RT_E_STACK, "BVH traversal stack overflow"); }

template <class R>
int ensure_precision(const rt_device_scene* s) {
  std::lock_guard<std::mutex> lock(s->mu);
  if (s->have<R>()) return RT_OK;
  auto t0 = Clock::now();
  HIP_TRY(hipSetDevice(s->device));
  DevArrays<R>& A = s->arrays<R>();
  int rc = A.upload(s->host->arrays<R>(), s->nodes, s->perlin_perm);
  if (rc) {
    A.release();
    A = DevArrays<R>();
    return rc;
  }
  A.lds_nodes = 0;
  if ((s->variant & RT_VAR_BASE) != RT_VAR_FLAT) {
    // stage as many top (breadth-first) surface nodes as fit beside the lanes' item sums and
    // stacks in the workgroup's share of the CU's 160 KB LDS at the kernel's occupancy (1 KB
    // granules; 4 x waves-per-SIMD waves per CU, `block` threads per workgroup); env
    // RT_AMD_LDS_NODES caps it (0 disables, for experiments)
    const KernelClass c = rt_class_of(sizeof(R) == 8, s->variant);
    const int waves = std::max(1, rt_class_waves(sizeof(R) == 8, c));
    const int block = rt_class_block(sizeof(R) == 8, c);
    const int per_cu = std::max(1, 4 * waves * 64 / block);
    const int budget = (163840 / per_cu / 1024) * 1024 - 1024;
    const int used = (int)rt_class_lds_bytes(sizeof(R) == 8, c, s->stack_depth, 0);
    A.lds_nodes = std::max(0, std::min(s->host->surface_nodes, (budget - used) / 64));
    if (const char* e = rt_knob("RT_AMD_LDS_NODES")) A.lds_nodes = std::min(A.lds_nodes, std::max(0, atoi(e)));
  }
  A.resident_blocks = rt_render_resident_blocks((const KernelParamsT<R>*)nullptr, s->device, s->stack_depth,
                                                s->variant, A.lds_nodes);
  if (A.resident_blocks <= 0) {
    A.release();
    A = DevArrays<R>();
    return fail(RT_E_HIP, "occupancy query failed");
  }
  s->have<R>() = true;
  s->upload_ms += ms_since(t0);
  return RT_OK;
}
template int ensure_precision<float>(const rt_device_scene*);
template int ensure_precision<double>(const rt_device_scene*);

int ensure_precisions(const rt_device_scene* s, int prec_mask) {
  int rc = RT_OK;
  if ((prec_mask & 1) && (rc = ensure_precision<float>(s))) return rc;
  if ((prec_mask & 2) && (rc = ensure_precision<double>(s))) return rc;
  return RT_OK;
}

// one render of the scene's records of precision R, enqueued on `hip_stream` (render_any's two cases)
template <class R>
static int render_async(const rt_device_scene* s, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex,
                        const RenderCall& c, void* hip_stream) {
  if (int rc = ensure_precision<R>(s)) return rc;
  const DevArrays<R>& A = s->arrays<R>();
  constexpr bool f64 = sizeof(R) == 8;
  LaunchInputs L;
  L.resident_lanes = (long long)A.resident_blocks * rt_class_block(f64, rt_class_of(f64, s->variant));
  L.lds_nodes = A.lds_nodes;
  L.lone = c.lone || (ex && (ex->flags & RT_EXEC_SOLO));  // (the caller says this render runs alone)
  L.sample0 = c.sample0;
  L.out_frame_rows = c.frame_rows;
  L.flat_ring = true;  // (where the scene's class has the ring form: rt_build.cpp rt_host_plan_ring)
  if (const char* e = rt_knob("RT_AMD_POOL_SHIFT")) L.pool_shift = std::max(4, std::min(10, atoi(e)));
  KernelParamsT<R> P;
  std::string err;
  int rc = rt_host_render_params(*s->host, s->variant, A.rec, cs, seed, ex, L, P, err);
  if (rc) return fail(rc, "%s", err.c_str());
  P.status = s->status + kStatusRender;
  P.out = (R*)c.d_out;
  HIP_TRY(hipSetDevice(s->device));
  // stream-ordered workspace: fixed-point sums, NaN flags, queue counter (graph-capturable)
  const Workspace W = workspace_layout((size_t)P.tile_rows * P.cam.width, RT_ACC_WORDS(R));
  hipStream_t st = (hipStream_t)hip_stream;
  char* ws = c.ws && c.ws_cap >= W.bytes ? c.ws : nullptr;
  const bool own = ws == nullptr;
  if (own) HIP_TRY(hipMallocAsync((void**)&ws, W.bytes, st));
  HIP_TRY(hipMemsetAsync(ws, 0, W.bytes, st));
  P.accum = (unsigned long long*)ws;
  P.nanflag = (unsigned int*)(ws + W.off_flag);
  P.counter = (int*)(ws + W.off_ctr);
  rc = RT_OK;
  // The persistent grid can leave RT_GRID_RESERVE workgroup slots free, so that with frames
  // overlapped on two streams this frame's resolve starts as soon as its render ends.  Measured
  // (profiles/r3/iso): with 8 free slots the FP32 resolve still takes 3.1 ms, starved by the next
  // frame's grid; binary64's runs in 23 us either way (its kernel leaves VGPRs free) — so 0.
  int reserve = A.resident_blocks > 16 * RT_GRID_RESERVE ? RT_GRID_RESERVE : 0;
  if (const char* e = rt_knob("RT_AMD_GRID_RESERVE")) reserve = std::max(0, std::min(A.resident_blocks - 1, atoi(e)));
  if (rt_launch_render(P, A.resident_blocks - reserve, s->variant, hip_stream) ||
      (c.resolve && rt_launch_resolve(P, hip_stream)))
    rc = fail(RT_E_HIP, "kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
  if (own) HIP_TRY(hipFreeAsync(ws, st));
  return rc;
}

// the one precision dispatch of a render
int render_any(const rt_device_scene* s, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex, bool f32,
               const RenderCall& c, void* hip_stream) {
  return f32 ? render_async<float>(s, cs, seed, ex, c, hip_stream) : render_async<double>(s, cs, seed, ex, c, hip_stream);
}

int check_flags(const rt_exec* ex) {
  const int known = RT_EXEC_F32 | RT_EXEC_ENCODE8_SRGB | RT_EXEC_ENCODE8_SQRT | RT_EXEC_SOLO;
  if (ex->flags & ~known) return fail(RT_E_INVALID, "unknown rt_exec.flags bits 0x%x", ex->flags & ~known);
  if ((ex->flags & RT_EXEC_ENCODE8_SRGB) && (ex->flags & RT_EXEC_ENCODE8_SQRT))
    return fail(RT_E_INVALID, "rt_exec.flags: RT_EXEC_ENCODE8_SRGB and RT_EXEC_ENCODE8_SQRT are exclusive");
  return RT_OK;
}

int validate_frame(const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex) {
  const int h = rt_host_image_height(cs);
  if (h <= 0 || cs->image_width <= 0) return fail(RT_E_INVALID, "image %dx%d must be non-empty", cs->image_width, h);
  if (rt_host_shard_rows(h, ex) < 0) return fail(RT_E_INVALID, "invalid rt_exec");
  if (int rc = check_flags(ex)) return rc;
  KernelParams P;
  std::string err;
  if (int rc = rt_host_make_params(cs, seed, ex, P, err)) return fail(rc, "%s", err.c_str());
  return RT_OK;
}

int exec_encoding(const rt_exec* ex) {
  if (!ex) return -1;
  if (ex->flags & RT_EXEC_ENCODE8_SRGB) return 0;
  if (ex->flags & RT_EXEC_ENCODE8_SQRT) return 1;
  return -1;
}

int multi_status(const rt_multi_scene* M, int* status) {
  *status = 0;
  for (const rt_device_scene* s : M->scenes) {
    int ps = 0;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(&ps, s->status + kStatusRender, sizeof(int), hipMemcpyDeviceToHost));
    *status |= ps;
  }
  return RT_OK;
}

}  // namespace rt_api

using namespace rt_api;

namespace {

// What a synchronous render clears before it starts: the status words in front of the radiance
// queries' — the renders' own, both casts' (kStatusCastAsync, kStatusCastSync) and the unused word 3
constexpr size_t kRenderStatusClear = kStatusRadianceAsync * sizeof(int);

const double* encode8_table(int encoding) {
  static double thr[2][256];
  static std::once_flag once[2];
  std::call_once(once[encoding], [&] { rt_host_encode8_thresholds(encoding, thr[encoding]); });
  return thr[encoding];
}

void destroy_scene(rt_device_scene* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  (void)hipFree(s->nodes);
  (void)hipFree(s->perlin_perm);
  (void)hipFree(s->status);
  (void)hipFree(s->prim_mat);
  s->f32.release();
  s->f64.release();
  delete s;
}

// the precision-independent part of a device scene: BVH nodes, Perlin permutations, status words,
// the kernel variant and the LDS plan; precisions follow on first render (ensure_precision)
int upload_common(const std::shared_ptr<const HostScene>& Hp, int device, rt_device_scene** out) {
  auto t0 = Clock::now();
  const HostScene& H = *Hp;
  *out = nullptr;
  HIP_TRY(hipSetDevice(device));
  auto* s = new rt_device_scene();
  s->device = device;
  s->host = Hp;
  std::vector<int> status(kStatusWords, 0);
  int rc;
  if ((rc = upload(&s->nodes, H.nodes)) || (rc = upload(&s->perlin_perm, H.perlin_perm)) ||
      (rc = upload(&s->status, status))) {
    destroy_scene(s);
    return rc;
  }
  s->stack_depth = rt_host_stack_depth(H);
  s->variant = rt_host_variant(H);
  s->upload_ms = ms_since(t0);
  *out = s;
  return RT_OK;
}

int check_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(RT_E_HIP, "no HIP device");
  if (device < 0 || device >= ndev) return fail(RT_E_INVALID, "device %d out of range (%d devices)", device, ndev);
  return RT_OK;
}

void multi_destroy(rt_multi_scene* M);

// A multi-device scene from one host build: the distinct devices upload CONCURRENTLY (one host
// thread each; the host build is shared, never repeated per device).  prec_mask: precisions to
// upload now (the rest on first render).
int multi_create(const std::shared_ptr<const HostScene>& H, const int32_t* devices, int n, int prec_mask,
                 rt_multi_scene** out) {
  *out = nullptr;
  if (n < 1 || n > RT_MAX_DEVICES || !devices) return fail(RT_E_INVALID, "invalid device list (%d devices)", n);
  for (int k = 0; k < n; ++k)
    if (int rc = check_device(devices[k])) return rc;
  auto* M = new rt_multi_scene();
  M->devices.assign(devices, devices + n);
  std::vector<int> distinct;
  for (int k = 0; k < n; ++k) {
    int j = (int)(std::find(distinct.begin(), distinct.end(), devices[k]) - distinct.begin());
    if (j == (int)distinct.size()) distinct.push_back(devices[k]);
    M->scene_of.push_back(j);
  }
  M->scenes.assign(distinct.size(), nullptr);
  std::vector<int> rcs(distinct.size(), RT_OK);
  std::vector<std::string> errs(distinct.size());
  auto t0 = Clock::now();
  {
    std::vector<std::thread> th;
    for (size_t j = 0; j < distinct.size(); ++j)
      th.emplace_back([&, j] {
        int rc = upload_common(H, distinct[j], &M->scenes[j]);
        if (!rc) rc = ensure_precisions(M->scenes[j], prec_mask);
        rcs[j] = rc;
        if (rc) errs[j] = rt_last_error();
      });
    for (auto& t : th) t.join();
  }
  M->upload_ms = ms_since(t0);
  for (size_t j = 0; j < distinct.size(); ++j)
    if (rcs[j]) {
      for (rt_device_scene* s : M->scenes) destroy_scene(s);
      delete M;
      return fail(rcs[j], "device %d: %s", distinct[j], errs[j].c_str());
    }
  // per shard: its stream and timing events (its tile and workspace come with the first render)
  M->parts.resize(n);
  for (int k = 0; k < n; ++k) {
    MultiPart& q = M->parts[k];
    q.device = devices[k];
    if (hipSetDevice(q.device) != hipSuccess || hipStreamCreateWithFlags(&q.st, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&q.e0) != hipSuccess || hipEventCreate(&q.e1) != hipSuccess) {
      multi_destroy(M);
      return fail(RT_E_HIP, "stream / events on device %d", devices[k]);
    }
  }
  if (hipSetDevice(devices[0]) != hipSuccess || hipStreamCreateWithFlags(&M->st0, hipStreamNonBlocking) != hipSuccess ||
      hipHostMalloc((void**)&M->h_status, 64, hipHostMallocDefault) != hipSuccess) {
    multi_destroy(M);
    return fail(RT_E_HIP, "stream on device %d", devices[0]);
  }
  // the first device holds the frame: every other device's resolve writes its rows there over
  // xGMI (peer access); a device without peer access renders into its own tile, which is then
  // copied over (HIP stages such copies itself)
  M->peer_ok.assign(distinct.size(), 1);
  for (size_t j = 1; j < distinct.size(); ++j) {
    int can = 0;
    M->peer_ok[j] = 0;
    if (hipDeviceCanAccessPeer(&can, distinct[j], distinct[0]) == hipSuccess && can) {
      (void)hipSetDevice(distinct[j]);
      const hipError_t e = hipDeviceEnablePeerAccess(distinct[0], 0);
      M->peer_ok[j] = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
      (void)hipGetLastError();
    }
  }
  *out = M;
  return RT_OK;
}

void multi_destroy(rt_multi_scene* M) {
  if (!M) return;
  for (MultiPart& q : M->parts) {
    (void)hipSetDevice(q.device);
    if (q.st) (void)hipStreamSynchronize(q.st);
    if (q.e0) (void)hipEventDestroy(q.e0);
    if (q.e1) (void)hipEventDestroy(q.e1);
    if (q.st) (void)hipStreamDestroy(q.st);
    (void)hipFree(q.d_tile);
    (void)hipFree(q.ws);
  }
  if (!M->devices.empty()) {
    (void)hipSetDevice(M->devices[0]);
    if (M->st0) (void)hipStreamDestroy(M->st0);
    if (M->h_status) (void)hipHostFree(M->h_status);
    (void)hipFree(M->d_gather);
    (void)hipFree(M->d_codes);
  }
  for (rt_device_scene* s : M->scenes) destroy_scene(s);
  delete M;
}

// grow a resident device buffer to `need` bytes (on the current device); counts the allocation
int grow(void** p, size_t* cap, size_t need, int* allocs) {
  if (*cap >= need && *p) return RT_OK;
  (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  HIP_TRY(hipMalloc(p, need ? need : 16));
  *cap = need;
  ++*allocs;
  return RT_OK;
}

// ---- a synchronous render of a resident scene: the stages, then the two drivers that run them
// what a render cost, for rt_stats (over shards: the longest times, every allocation)
struct RenderCost {
  double prep_ms = 0;   // the precision's upload, when this render is its first
  float kernel_ms = 0;  // between the part's events e0 and e1
  int allocs = 0;       // grow's
};
// where a shard's resolve writes: its own tile; its rows of the frame on the first device; or its
// tile, which one strided copy then puts into that frame
enum class ShardOut { tile, frame, tile_to_frame };

// shard k's rt_exec: on devices[k], shard k of n for a device list, linear (encoded after the gather)
rt_exec shard_exec(const rt_multi_scene* M, const rt_exec* ex, int k) {
  rt_exec e = *ex;
  e.n_devices = 0, e.devices = nullptr, e.device = M->devices[k];
  e.flags &= ~(RT_EXEC_ENCODE8_SRGB | RT_EXEC_ENCODE8_SQRT);
  if (M->devices.size() > 1) e.n_shards = (int32_t)M->devices.size(), e.shard = k;
  return e;
}

// Stage: shard k's device current, its precision's records resident, its tile (if it renders into
// one) and its workspace large enough for tile_pixels
int prepare_part(rt_multi_scene* M, int k, size_t tile_pixels, bool f32, bool need_tile, RenderCost& cost) {
  MultiPart& q = M->parts[k];
  const rt_device_scene* s = M->scenes[M->scene_of[k]];
  HIP_TRY(hipSetDevice(s->device));
  const auto tp = Clock::now();
  if (int r = ensure_precisions(s, prec_bit(f32))) return r;
  cost.prep_ms = ms_since(tp);
  if (need_tile)
    if (int r = grow(&q.d_tile, &q.tile_cap, tile_pixels * 3 * elem_size_of(f32), &cost.allocs)) return r;
  return grow((void**)&q.ws, &q.ws_cap, workspace_layout(tile_pixels, acc_words_of(f32)).bytes, &cost.allocs);
}

// Stage: shard k's render (ex: shard_exec's) between its events on its stream; a copied shard's way into the frame
int enqueue_shard(rt_multi_scene* M, int k, const rt_camera_settings* cs, uint64_t seed, const rt_exec& ex, ShardOut to) {
  MultiPart& q = M->parts[k];
  const bool f32 = exec_f32(&ex);
  const int h = rt_host_image_height(cs);
  RenderCall c;
  c.d_out = to == ShardOut::frame ? M->d_gather : q.d_tile;
  c.ws = q.ws, c.ws_cap = q.ws_cap;
  c.frame_rows = to == ShardOut::frame ? h : 0;
  c.lone = true;
  HIP_TRY(hipEventRecord(q.e0, q.st));
  if (int r = render_any(M->scenes[M->scene_of[k]], cs, seed, &ex, f32, c, q.st)) return r;
  HIP_TRY(hipEventRecord(q.e1, q.st));
  if (to == ShardOut::tile_to_frame) {
    // shard-local row block b is global block b n + k: one strided copy into the first
    // device's framebuffer (peer-to-peer over xGMI for another device)
    const size_t w = (size_t)ex.row_block * cs->image_width * 3 * elem_size_of(f32);
    HIP_TRY(hipMemcpy2DAsync((char*)M->d_gather + (size_t)k * w, M->devices.size() * w, q.d_tile, w, w,
                             (size_t)rt_host_shard_rows(h, &ex) / ex.row_block, hipMemcpyDeviceToDevice, q.st));
  }
  return RT_OK;
}

// Stage: the n_values linear values at d_img, or their 8-bit codes (the epilogue, into M->d_codes),
// to the host buffer in ONE device-to-host copy on `st`
int enqueue_readback(rt_multi_scene* M, const void* d_img, int64_t n_values, bool f32, int encoding, void* out_host,
                     hipStream_t st) {
  if (encoding < 0) {
    HIP_TRY(hipMemcpyAsync(out_host, d_img, (size_t)n_values * elem_size_of(f32), hipMemcpyDeviceToHost, st));
    return RT_OK;
  }
  if (rt_launch_encode8(d_img, f32 ? 0 : 1, M->d_codes, n_values, encode8_table(encoding), encoding, st))
    return fail(RT_E_HIP, "encode launch failed: %s", hipGetErrorString(hipGetLastError()));
  HIP_TRY(hipMemcpyAsync(out_host, M->d_codes, (size_t)n_values, hipMemcpyDeviceToHost, st));
  return RT_OK;
}

// Stage: the one place that writes a render's rt_stats (ex: the caller's; t0: the call's start)
void fill_stats(rt_stats* stats, const rt_multi_scene* M, const rt_camera_settings* cs, const rt_exec* ex,
                const RenderCost& cost, double build_ms, Clock::time_point t0) {
  const rt_device_scene* s = M->scenes[0];
  const bool f32 = exec_f32(ex);
  std::memset(stats, 0, sizeof *stats);
  stats->upload_ms = build_ms + M->upload_ms + cost.prep_ms;
  stats->kernel_ms = cost.kernel_ms;
  stats->samples = (int64_t)rt_host_shard_rows(rt_host_image_height(cs), ex) * cs->image_width * cs->samples_per_pixel;
  stats->bvh_nodes = s->host->n_nodes;
  stats->max_stack = s->host->max_depth;
  stats->device_allocs = cost.allocs;
  stats->kernel_block = rt_class_block(!f32, rt_class_of(!f32, s->variant));
  stats->total_ms = build_ms + ms_since(t0);
}

// One device (the drop-in's plain rt_render / a one-device scene): everything on the part's
// stream with ONE host synchronisation — status reset, workspace memset, render, resolve, the 8-bit
// epilogue, the image's device-to-host copy and the status word's into pinned memory — instead of a
// thread per shard and a synchronising call for each step (render_many below)
int render_one(rt_multi_scene* M, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex, void* out_host,
               RenderCost& cost) {
  MultiPart& q = M->parts[0];
  const rt_device_scene* s = M->scenes[0];
  const rt_exec e = shard_exec(M, ex, 0);
  const bool f32 = exec_f32(ex);
  const size_t tile_pixels = (size_t)rt_host_shard_rows(rt_host_image_height(cs), ex) * cs->image_width;
  if (int r = prepare_part(M, 0, tile_pixels, f32, true, cost)) return r;
  // everything below is enqueued on q.st; a failure after the first enqueue synchronises the
  // stream before returning, so no copy into out_host is still in flight when the call returns
  auto enqueue = [&]() -> int {
    HIP_TRY(hipMemsetAsync(s->status, 0, kRenderStatusClear, q.st));
    if (int r = enqueue_shard(M, 0, cs, seed, e, ShardOut::tile)) return r;
    // (the image is copied before the status word is read, in the same synchronisation: on
    // RT_E_STACK out_host holds the partial image, include/rt.h)
    if (int r = enqueue_readback(M, q.d_tile, (int64_t)tile_pixels * 3, f32, exec_encoding(ex), out_host, q.st)) return r;
    HIP_TRY(hipMemcpyAsync(M->h_status, s->status + kStatusRender, sizeof(int), hipMemcpyDeviceToHost, q.st));
    return RT_OK;
  };
  if (const int r = enqueue()) {
    (void)hipStreamSynchronize(q.st);
    return r;
  }
  HIP_TRY(hipStreamSynchronize(q.st));
  if (*M->h_status) return fail_stack();
  HIP_TRY(hipEventElapsedTime(&cost.kernel_ms, q.e0, q.e1));
  return RT_OK;
}

// A device list of n > 1 shards (shard k on devices[k]): a host thread per shard prepares, renders
// and synchronises its part; epilogue and read-back of the gathered frame on st0
int render_many(rt_multi_scene* M, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex, void* out_host,
                RenderCost& cost) {
  const int n = (int)M->devices.size();
  const bool f32 = exec_f32(ex);
  const int h = rt_host_image_height(cs);
  // experiments and tests: shards forced onto the tile + strided-copy path a device without peer
  // access takes (RT_AMD_COPY_SHARDS: bit k for shard k, -1 every shard), so one GPU exercises it
  unsigned long long copy_mask = 0;
  if (const char* e = rt_knob("RT_AMD_COPY_SHARDS")) copy_mask = (unsigned long long)strtoll(e, nullptr, 0);
  // a stack overflow of an earlier render must not fail this one: clear each device's status word
  for (size_t j = 0; j < M->scenes.size(); ++j) {
    const rt_device_scene* s = M->scenes[j];
    const MultiPart& q = M->parts[std::find(M->scene_of.begin(), M->scene_of.end(), (int)j) - M->scene_of.begin()];
    if (hipSetDevice(s->device) != hipSuccess || hipMemsetAsync(s->status, 0, kRenderStatusClear, q.st) != hipSuccess ||
        hipStreamSynchronize(q.st) != hipSuccess)
      return fail(RT_E_HIP, "status reset on device %d", s->device);
  }
  std::vector<RenderCost> costs(n);
  std::vector<int> rcs(n, RT_OK);
  std::vector<std::string> errs(n);
  {
    std::vector<std::thread> th;
    for (int k = 0; k < n; ++k)
      th.emplace_back([&, k] {
        const MultiPart& q = M->parts[k];
        const rt_exec e = shard_exec(M, ex, k);
        // the resolve writes the shard's rows straight into the frame on the first device (over
        // xGMI from a peer); without peer access, a tile and a strided copy
        const bool direct = M->peer_ok[M->scene_of[k]] && !((copy_mask >> k) & 1ull);
        auto run = [&]() -> int {
          const size_t tile_pixels = (size_t)rt_host_shard_rows(h, &e) * cs->image_width;
          if (int r = prepare_part(M, k, tile_pixels, f32, !direct, costs[k])) return r;
          if (int r = enqueue_shard(M, k, cs, seed, e, direct ? ShardOut::frame : ShardOut::tile_to_frame)) return r;
          HIP_TRY(hipStreamSynchronize(q.st));
          HIP_TRY(hipEventElapsedTime(&costs[k].kernel_ms, q.e0, q.e1));
          return RT_OK;
        };
        if ((rcs[k] = run())) errs[k] = rt_last_error();
      });
    for (auto& t : th) t.join();
  }
  for (int k = 0; k < n; ++k) {
    if (rcs[k]) return fail(rcs[k], "device %d: %s", M->devices[k], errs[k].c_str());
    cost.prep_ms = std::max(cost.prep_ms, costs[k].prep_ms);
    cost.kernel_ms = std::max(cost.kernel_ms, costs[k].kernel_ms);
    cost.allocs += costs[k].allocs;
  }
  int status = 0;
  if (int r = multi_status(M, &status)) return r;
  if (status) return fail_stack();
  (void)hipSetDevice(M->devices[0]);
  if (int r = enqueue_readback(M, M->d_gather, (int64_t)h * cs->image_width * 3, f32, exec_encoding(ex), out_host, M->st0))
    return r;
  if (hipStreamSynchronize(M->st0) != hipSuccess)
    return fail(RT_E_HIP, "copy back: %s", hipGetErrorString(hipGetLastError()));
  return RT_OK;
}

// Render the image (device list: shard k of n on devices[k]) or, with one device, the rt_exec
// shard; gather on the first device; optional 8-bit epilogue there; ONE copy to the host buffer.
// Every buffer, stream and event is the scene's own (rt_multi_scene), kept across renders.  The
// frame has passed validate_frame; the devices are the scene's, whatever list ex names.
int render_sync(rt_multi_scene* M, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex, void* out_host,
                rt_stats* stats, double build_ms) {
  const auto t0 = Clock::now();
  const int n = (int)M->devices.size();
  if (n > 1 && ex->n_shards != 1) return fail(RT_E_INVALID, "a device list renders the whole image (n_shards must be 1)");
  std::lock_guard<std::mutex> lock(M->mu);
  // the first device's framebuffer: n shard tiles in global row order (n > 1; padded to equal
  // tiles), or the single shard's tile itself, which is its part's; the 8-bit codes of either
  const rt_exec e0 = shard_exec(M, ex, 0);
  const size_t frame_values = (size_t)n * rt_host_shard_rows(rt_host_image_height(cs), &e0) * cs->image_width * 3;
  RenderCost cost;
  if (hipSetDevice(M->devices[0]) != hipSuccess) return fail(RT_E_HIP, "device %d", M->devices[0]);
  if (n > 1)
    if (int rc = grow(&M->d_gather, &M->gather_cap, frame_values * elem_size_of(exec_f32(ex)), &cost.allocs)) return rc;
  if (exec_encoding(ex) >= 0)
    if (int rc = grow((void**)&M->d_codes, &M->codes_cap, std::max<size_t>(16, frame_values), &cost.allocs)) return rc;
  if (int rc = n == 1 ? render_one(M, cs, seed, ex, out_host, cost) : render_many(M, cs, seed, ex, out_host, cost)) return rc;
  if (stats) fill_stats(stats, M, cs, ex, cost, build_ms, t0);
  return RT_OK;
}

int build_host(const rt_scene* sc, std::shared_ptr<const HostScene>& out, double& ms) {
  auto t0 = Clock::now();
  auto H = std::make_shared<HostScene>();
  std::string err;
  int rc = rt_host_build_scene(sc, *H, err);
  if (rc) return fail(rc, "%s", err.c_str());
  out = H;
  ms = ms_since(t0);
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

const char* rt_last_error(void) { return g_err.c_str(); }

int rt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RT_E_HIP, "no HIP device");
  return n;
}

int rt_image_height(const rt_camera_settings* cs) {
  if (!cs) return fail(RT_E_INVALID, "null camera settings");
  int h = rt_host_image_height(cs);
  if (h < 0) return fail(RT_E_INVALID, "image height is not finite");
  return h;
}

int rt_shard_rows(int32_t height, const rt_exec* ex) {
  int r = rt_host_shard_rows(height, ex);
  if (r < 0) return fail(RT_E_INVALID, "invalid rt_exec");
  return r;
}

int rt_shard_row(int32_t t, const rt_exec* ex) {
  if (!ex || ex->n_shards < 1 || ex->row_block < 1) return fail(RT_E_INVALID, "invalid rt_exec");
  return ((t / ex->row_block) * ex->n_shards + ex->shard) * ex->row_block + (t % ex->row_block);
}

int rt_scene_destroy(rt_device_scene* s) {
  destroy_scene(s);
  return RT_OK;
}

int rt_scene_create(const rt_scene* sc, int32_t device, rt_device_scene** out) {
  if (!sc || !out) return fail(RT_E_INVALID, "null argument");
  *out = nullptr;
  std::shared_ptr<const HostScene> H;
  double build_ms = 0;
  if (int rc = build_host(sc, H, build_ms)) return rc;
  if (int rc = check_device(device)) return rc;
  if (int rc = upload_common(H, device, out)) return rc;
  (*out)->build_ms = build_ms;
  return RT_OK;
}

int rt_scene_stats(const rt_device_scene* s, rt_stats* st) {
  if (!s || !st) return fail(RT_E_INVALID, "null argument");
  std::memset(st, 0, sizeof *st);
  st->upload_ms = s->build_ms + s->upload_ms;
  st->bvh_nodes = s->host->n_nodes;
  st->max_stack = s->stack_depth;
  return RT_OK;
}

int rt_render_async(const rt_device_scene* s, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex,
                    void* d_out_rgb, void* hip_stream) {
  if (!s || !d_out_rgb || !ex || !cs) return fail(RT_E_INVALID, "null argument");
  if (ex->n_devices != 0) return fail(RT_E_INVALID, "rt_render_async renders on the scene's device (n_devices = 0)");
  if (int rc = check_flags(ex)) return rc;
  if (exec_encoding(ex) >= 0) return fail(RT_E_INVALID, "rt_render_async writes linear RGB (use rt_encode8_async)");
  RenderCall c;  // (no workspace of the caller's: one from the stream-ordered pool)
  c.d_out = d_out_rgb;
  return render_any(s, cs, seed, ex, exec_f32(ex), c, hip_stream);
}

int rt_multi_scene_create(const rt_scene* sc, const int32_t* devices, int32_t n_devices, rt_multi_scene** out) {
  if (!sc || !out) return fail(RT_E_INVALID, "null argument");
  *out = nullptr;
  std::shared_ptr<const HostScene> H;
  double build_ms = 0;
  if (int rc = build_host(sc, H, build_ms)) return rc;
  if (int rc = multi_create(H, devices, n_devices, 0, out)) return rc;
  (*out)->build_ms = build_ms;
  return RT_OK;
}

int rt_multi_scene_destroy(rt_multi_scene* m) {
  multi_destroy(m);
  return RT_OK;
}

int rt_multi_render(const rt_multi_scene* m, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex,
                    void* out, rt_stats* stats) {
  if (!m || !cs || !ex || !out) return fail(RT_E_INVALID, "null argument");
  if (ex->n_devices != 0) return fail(RT_E_INVALID, "rt_multi_render renders on the scene's devices (n_devices = 0)");
  if (int rc = validate_frame(cs, seed, ex)) return rc;
  // the scene's resident buffers are its internal state (the caller's handle stays const)
  const int rc = render_sync(const_cast<rt_multi_scene*>(m), cs, seed, ex, out, stats, 0.0);
  if (!rc && stats) stats->upload_ms += m->build_ms;  // the scene's one-time cost, as rt_render reports it
  return rc;
}

int rt_render(const rt_camera_settings* cs, const rt_scene* scene, uint64_t seed, const rt_exec* ex, void* out_rgb,
              rt_stats* stats) {
  if (!cs || !scene || !ex || !out_rgb) return fail(RT_E_INVALID, "null argument");
  if (int rc = validate_frame(cs, seed, ex)) return rc;  // before building or touching a device
  if (ex->n_devices < 0 || ex->n_devices > RT_MAX_DEVICES || (ex->n_devices > 0 && !ex->devices))
    return fail(RT_E_INVALID, "invalid device list (%d devices)", ex->n_devices);
  if (ex->n_devices > 0 && ex->n_shards != 1)
    return fail(RT_E_INVALID, "a device list renders the whole image (n_shards must be 1)");
  std::shared_ptr<const HostScene> H;
  double build_ms = 0;
  if (int rc = build_host(scene, H, build_ms)) return rc;  // ONE host build, whatever the device count
  const int32_t one = ex->device;
  const int32_t* devs = ex->n_devices > 0 ? ex->devices : &one;
  const int n = ex->n_devices > 0 ? ex->n_devices : 1;
  rt_multi_scene* M = nullptr;
  if (int rc = multi_create(H, devs, n, prec_bit(exec_f32(ex)), &M)) return rc;  // only this call's precision
  const int rc = render_sync(M, cs, seed, ex, out_rgb, stats, build_ms);  // (the list is M's now: shard_exec drops ex's)
  multi_destroy(M);
  return rc;
}

int rt_encode8_async(const void* d_rgb, int32_t in_f64, uint8_t* d_out, int64_t n_values, int32_t encoding,
                     void* hip_stream) {
  if (!d_rgb || !d_out || n_values < 0) return fail(RT_E_INVALID, "invalid encode arguments");
  if (encoding != 0 && encoding != 1) return fail(RT_E_INVALID, "encoding must be 0 (sRGB) or 1 (sqrt)");
  if (rt_launch_encode8(d_rgb, in_f64 ? 1 : 0, d_out, n_values, encode8_table(encoding), encoding, hip_stream))
    return fail(RT_E_HIP, "encode launch failed: %s", hipGetErrorString(hipGetLastError()));
  return RT_OK;
}

#if defined(RT_PHASE_PROF)
// diagnostic build only: the BVH kernel's phase counters (rt_trace.h RT_PHASE_PROF), read and zeroed
int rt_prof_read(int f64, unsigned long long* out, int n) {
  return f64 ? rt_prof_read_kernel((const KernelParams64*)nullptr, out, n) : rt_prof_read_kernel((const KernelParams*)nullptr, out, n);
}
#endif
#if defined(RT_WAVE_STAMPS)
// diagnostic build only: per-wave (start, queue drained, end, hw id) stamps of the last renders
// (rt_render_kernel.h RT_WAVE_STAMPS), read and zeroed; returns the waves read
int rt_stamps_read(int f64, unsigned long long* out, int n_waves) {
  return f64 ? rt_stamps_read_kernel((const KernelParams64*)nullptr, out, n_waves)
             : rt_stamps_read_kernel((const KernelParams*)nullptr, out, n_waves);
}
#endif

}  // extern "C"
