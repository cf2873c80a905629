// rt_api_query.hip — queries on a resident scene behind include/rt.h: ray casts (rt_scene_cast*;
// kernels in rt_query*.hip), radiance queries (rt_scene_radiance*; rt_radiance*.hip), the render's
// camera rays (rt_scene_camera_rays*) and ray orders (rt_scene_ray_order*, rt_ray_order_*;
// rt_order.hip).  An asynchronous call checks its arguments and enqueues on the caller's stream; a
// synchronous one stages host buffers through ONE device allocation (Staging) on the null stream:
// upload, enqueue, results back, then the status word, so that RT_E_STACK leaves the partial
// results in the caller's buffer.  The scene is rt_api.hip's; rt_api_internal.h holds its struct.
#include <cstdlib>

#include "rt_api_internal.h"

using namespace rt_api;

namespace {

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// The one device allocation of a synchronous call, freed on every exit path.  The call names its
// parts in order (take: right behind the part before; take256: at the next 256-byte boundary),
// then alloc() makes the allocation (on the current device) and at() gives a part's address
struct Staging {
  char* mem = nullptr;
  size_t bytes = 0;
  Staging() = default;
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;
  ~Staging() {
    if (mem) (void)hipFree(mem);
  }
  size_t take(size_t n) {
    const size_t at = bytes;
    bytes += n;
    return at;
  }
  size_t take256(size_t n) {
    bytes = up256(bytes);
    return take(n);
  }
  int alloc() {
    HIP_TRY(hipMalloc((void**)&mem, bytes));
    return RT_OK;
  }
  template <class T>
  T* at(size_t offset) const {
    return (T*)(mem + offset);
  }
};

// a one-shard rt_exec on the scene's device, and a valid 1 x 1 camera: the scene parts of a render's
// argument block are what a query kernel reads, these fill the rest
rt_exec one_shard(const rt_device_scene* s) {
  rt_exec ex{};
  ex.device = s->device;
  ex.n_shards = 1;
  ex.row_block = 4;
  return ex;
}
rt_camera_settings unit_camera() {
  rt_camera_settings cs{};
  cs.look_at[2] = -1.0;
  cs.up[1] = 1.0;
  cs.vfov = 1.0;
  cs.aspect_ratio = 1.0;
  cs.image_width = cs.samples_per_pixel = cs.max_recursion_depth = 1;
  cs.focus_dist = 1.0;
  return cs;
}

// the asynchronous calls' status word `word`, read and cleared (rt_scene_cast_status, rt_scene_radiance_status)
int status_take(const rt_device_scene* s, StatusWord word, int32_t* overflowed) {
  if (!s || !overflowed) return fail(RT_E_INVALID, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  int status = 0;
  HIP_TRY(hipMemcpy(&status, s->status + word, sizeof(int), hipMemcpyDeviceToHost));
  if (status) HIP_TRY(hipMemset(s->status + word, 0, sizeof(int)));
  *overflowed = status ? 1 : 0;
  return RT_OK;
}

// ---- ray orders (include/rt.h rt_scene_ray_order; rt_order.hip)

int order_count_check(int64_t n) {
  if (n >= ((int64_t)1 << 31)) return fail(RT_E_INVALID, "%lld rays: an order holds fewer than 2^31", (long long)n);
  return RT_OK;
}
// the checks of an order call that need no device
int order_check(const rt_device_scene* s, const void* rays, int64_t n, int kind, const void* order) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  if (!rays) return fail(RT_E_INVALID, "null ray buffer");
  if (!order) return fail(RT_E_INVALID, "null order buffer");
  if (n < 0) return fail(RT_E_INVALID, "negative ray count %lld", (long long)n);
  if (int rc = order_count_check(n)) return rc;
  if (kind != RT_ORDER_RAYS && kind != RT_ORDER_PATH_RAYS) return fail(RT_E_INVALID, "unknown record kind %d", kind);
  return RT_OK;
}
// what an ordered asynchronous query checks behind its plain twin's checks
int order_arg_check(bool ordered, const uint32_t* d_order, int64_t n) {
  if (!ordered) return RT_OK;
  if (!d_order) return fail(RT_E_INVALID, "null order buffer");
  return order_count_check(n);
}
int order_stride(int kind) { return kind == RT_ORDER_RAYS ? (int)sizeof(rt_ray) : (int)sizeof(rt_path_ray); }
// a host order is a permutation of [0, n)
int permutation_check(const uint32_t* order, int64_t n) {
  std::vector<bool> seen((size_t)n, false);
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t v = order[i];
    if ((int64_t)v >= n || seen[v]) return fail(RT_E_INVALID, "the order is no permutation of [0, %lld): entry %lld is %u", (long long)n, (long long)i, v);
    seen[v] = true;
  }
  return RT_OK;
}
// The order of a synchronous ordered call into d_order (device, n uint32): the caller's host order
// copied, or (null) computed on the device from d_rays with the scratch d_ws
int order_for_sync(const uint32_t* host_order, const void* d_rays, int64_t n, int kind, uint32_t* d_order, void* d_ws) {
  if (host_order) {
    HIP_TRY(hipMemcpy(d_order, host_order, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    return RT_OK;
  }
  if (rt_launch_ray_order(d_rays, (long long)n, order_stride(kind), d_order, d_ws, nullptr))
    return fail(RT_E_HIP, "order launch failed: %s", hipGetErrorString(hipGetLastError()));
  return RT_OK;
}

// ---- the frame of a synchronous query (cast_sync, radiance_sync), ordered or not

// Behind the call's own checks: an ordered call's count, nothing to do for no rays, a host order's
// permutation check, the scene's device current.  *go: there are rays to trace
int sync_begin(const rt_device_scene* s, int64_t n, bool ordered, const uint32_t* host_order, bool* go) {
  *go = false;
  if (ordered)
    if (int rc = order_count_check(n)) return rc;
  if (n == 0) return RT_OK;
  if (ordered && host_order)
    if (int rc = permutation_check(host_order, n)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  *go = true;
  return RT_OK;
}
// an ordered call's parts behind the plain call's (none if not ordered): the order, then the sort's
// workspace unless the caller gave the order
struct OrderParts { size_t order_at = 0, ws_at = 0; };
OrderParts take_order(Staging& m, int64_t n, bool ordered, const uint32_t* host_order) {
  OrderParts o;
  if (!ordered) return o;
  o.order_at = m.take256((size_t)n * sizeof(uint32_t));
  o.ws_at = m.take256(host_order ? 0 : rt_order_workspace_bytes((long long)n));
  return o;
}
// Behind the results' read-back: the call's status word (`what` failed to come back, if it does)
int sync_end(const rt_device_scene* s, StatusWord word, const char* what) {
  int status = 0;
  if (hipMemcpy(&status, s->status + word, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(RT_E_HIP, "%s read-back failed: %s", what, hipGetErrorString(hipGetLastError()));
  return status ? fail_stack() : RT_OK;
}

// ---- ray queries (include/rt.h rt_scene_cast; rt_query.h)

// n queries of precision R enqueued on st; a stack overflow sets the scene's status word `word`
template <class R>
int cast_enqueue(const rt_device_scene* s, const rt_ray* d_rays, rt_hit* d_hits, int64_t n, int flags, StatusWord word,
                 hipStream_t st, const uint32_t* d_order) {
  if (int rc = ensure_precision<R>(s)) return rc;
  {
    std::lock_guard<std::mutex> lock(s->mu);
    if (!s->prim_mat) {
      HIP_TRY(hipSetDevice(s->device));
      int* d = nullptr;
      if (int rc = upload(&d, s->host->prim_mat)) return rc;
      s->prim_mat = d;
    }
  }
  const rt_camera_settings cs = unit_camera();
  const rt_exec ex = one_shard(s);
  KernelParamsT<R> P;
  if (int rc = lane_params(s, &cs, 0, &ex, P, word)) return rc;
  // (experiments and tests: fewer stack rows than the scene's BVH needs, the defined overflow path)
  if (const char* e = rt_knob("RT_AMD_CAST_STACK")) P.stack_depth = std::max(1, std::min(P.stack_depth, atoi(e)));
  HIP_TRY(hipSetDevice(s->device));
  // (lane i on record d_order[i]: the ordered units' kernels, rt_query_kernel.h RT_QUERY_ORDERED)
  if (d_order ? rt_launch_query_ordered(P, s->variant, d_rays, d_hits, s->prim_mat, (long long)n, flags, d_order, st)
              : rt_launch_query(P, s->variant, d_rays, d_hits, s->prim_mat, (long long)n, flags, st))
    return fail(RT_E_HIP, "query launch failed: %s", hipGetErrorString(hipGetLastError()));
  return RT_OK;
}

// the checks of a cast that need no device
int cast_check(const rt_device_scene* s, const rt_exec* ex, const rt_ray* rays, const rt_hit* hits, int64_t n, int flags) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  if (!ex) return fail(RT_E_INVALID, "null rt_exec");
  if (!rays) return fail(RT_E_INVALID, "null ray buffer");
  if (!hits) return fail(RT_E_INVALID, "null hit buffer");
  if (n < 0) return fail(RT_E_INVALID, "negative ray count %lld", (long long)n);
  if (flags & ~(RT_QUERY_UV | RT_QUERY_ANY_HIT)) return fail(RT_E_INVALID, "unknown query flags 0x%x", flags);
  if (ex->n_devices != 0) return fail(RT_E_INVALID, "a cast runs on the scene's device (n_devices = 0)");
  return check_flags(ex);
}

// rt_scene_cast_async / rt_scene_cast_ordered_async (`ordered`: d_order is the call's argument)
int cast_async(const rt_device_scene* s, const rt_exec* ex, const rt_ray* d_rays, rt_hit* d_hits, int64_t n, int flags,
               bool ordered, const uint32_t* d_order, hipStream_t st) {
  if (int rc = cast_check(s, ex, d_rays, d_hits, n, flags)) return rc;
  if (int rc = order_arg_check(ordered, d_order, n)) return rc;
  if (n == 0) return RT_OK;
  return by_precision(exec_f32(ex), [&](auto r) {
    return cast_enqueue<decltype(r)>(s, d_rays, d_hits, n, flags, kStatusCastAsync, st, d_order);
  });
}

// rt_scene_cast / rt_scene_cast_ordered: ordered with host_order null computes the order on the device
int cast_sync(const rt_device_scene* s, const rt_exec* ex, const rt_ray* host_rays, rt_hit* host_hits, int64_t n, int flags,
              bool ordered, const uint32_t* host_order) {
  if (int rc = cast_check(s, ex, host_rays, host_hits, n, flags)) return rc;
  bool go;
  if (int rc = sync_begin(s, n, ordered, host_order, &go); rc || !go) return rc;
  Staging m;
  const size_t ray_bytes = (size_t)n * sizeof(rt_ray), hit_bytes = (size_t)n * sizeof(rt_hit);
  const size_t rays_at = m.take(ray_bytes), hits_at = m.take(hit_bytes);  // (both multiples of 16 bytes)
  const OrderParts o = take_order(m, n, ordered, host_order);
  if (int rc = m.alloc()) return rc;
  rt_ray* d_rays = m.at<rt_ray>(rays_at);
  rt_hit* d_hits = m.at<rt_hit>(hits_at);
  uint32_t* d_order = ordered ? m.at<uint32_t>(o.order_at) : nullptr;
  if (hipMemcpy(d_rays, host_rays, ray_bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(s->status + kStatusCastSync, 0, sizeof(int)) != hipSuccess)
    return fail(RT_E_HIP, "ray upload failed: %s", hipGetErrorString(hipGetLastError()));
  if (ordered)
    if (int rc = order_for_sync(host_order, d_rays, n, RT_ORDER_RAYS, d_order, m.at<char>(o.ws_at))) return rc;
  if (int rc = by_precision(exec_f32(ex), [&](auto r) {
        return cast_enqueue<decltype(r)>(s, d_rays, d_hits, n, flags, kStatusCastSync, nullptr, d_order);
      }))
    return rc;
  if (hipMemcpy(host_hits, d_hits, hit_bytes, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(RT_E_HIP, "hit read-back failed: %s", hipGetErrorString(hipGetLastError()));
  return sync_end(s, kStatusCastSync, "hit");
}

// ---- radiance queries (include/rt.h rt_scene_radiance; rt_radiance.h)

// the bytes of n rays' workspace words; the kernel's cursor lies behind them (16 bytes)
size_t radiance_words_bytes(int64_t n, bool f32) { return (size_t)n * ((f32 ? 3 : 6) + 1) * sizeof(unsigned long long); }

// n rays of precision R enqueued on st: the workspace zeroed (or only its cursor, accumulate), the
// path kernel, the resolve; a stack overflow sets the scene's status word `word`
template <class R>
int radiance_enqueue(const rt_device_scene* s, const rt_camera_settings* cs, uint64_t seed, const rt_path_ray* d_rays,
                     rt_radiance* d_out, void* d_work, int64_t n, int n_samples, int flags, StatusWord word, hipStream_t st,
                     const uint32_t* d_order) {
  if (int rc = ensure_precision<R>(s)) return rc;
  const rt_camera_settings c1 = rt_host_radiance_camera(cs);
  const rt_exec ex = one_shard(s);
  KernelParamsT<R> P;
  if (int rc = lane_params(s, &c1, seed, &ex, P, word)) return rc;
  // (experiments and tests: fewer stack rows than the scene's BVH needs, the defined overflow path;
  // samples per item — the result does not depend on it)
  if (const char* e = rt_knob("RT_AMD_RADIANCE_STACK")) P.stack_depth = std::max(1, std::min(P.stack_depth, atoi(e)));
  int chunk = 0;
  if (const char* e = rt_knob("RT_AMD_RADIANCE_CHUNK")) chunk = std::max(0, atoi(e));
  const size_t words = radiance_words_bytes(n, sizeof(R) == 4);
  P.counter = (int*)((char*)d_work + words);
  HIP_TRY(hipSetDevice(s->device));
  if (flags & RT_RADIANCE_ACCUMULATE)
    HIP_TRY(hipMemsetAsync(P.counter, 0, 16, st));
  else
    HIP_TRY(hipMemsetAsync(d_work, 0, words + 16, st));
  if (d_order ? rt_launch_radiance_ordered(P, s->variant, d_rays, d_out, (unsigned long long*)d_work, (long long)n, n_samples,
                                           chunk, flags, d_order, st)
              : rt_launch_radiance(P, s->variant, d_rays, d_out, (unsigned long long*)d_work, (long long)n, n_samples, chunk,
                                   flags, st))
    return fail(RT_E_HIP, "radiance launch failed: %s", hipGetErrorString(hipGetLastError()));
  return RT_OK;
}

// the checks of a radiance query that need no device (rt_build.cpp rt_host_radiance_check, then the flags)
int radiance_check(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, const void* rays, const void* out,
                   int64_t n, int n_samples, int flags) {
  std::string err;
  if (int rc = rt_host_radiance_check(s, ex, cs, rays, out, n, n_samples, flags, err)) return fail(rc, "%s", err.c_str());
  return check_flags(ex);
}

// rt_scene_radiance_async / rt_scene_radiance_ordered_async, as cast_async
int radiance_async(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                   const rt_path_ray* d_rays, rt_radiance* d_out, void* d_workspace, int64_t n, int n_samples, int flags,
                   bool ordered, const uint32_t* d_order, hipStream_t st) {
  if (int rc = radiance_check(s, ex, cs, d_rays, d_out, n, n_samples, flags)) return rc;
  if (!d_workspace) return fail(RT_E_INVALID, "null workspace");
  if (int rc = order_arg_check(ordered, d_order, n)) return rc;
  if (n == 0) return RT_OK;
  return by_precision(exec_f32(ex), [&](auto r) {
    return radiance_enqueue<decltype(r)>(s, cs, seed, d_rays, d_out, d_workspace, n, n_samples, flags, kStatusRadianceAsync, st,
                                         d_order);
  });
}

// rt_scene_radiance / rt_scene_radiance_ordered, as cast_sync; a host workspace receives the words,
// and gives them first when the call accumulates
int radiance_sync(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                  const rt_path_ray* host_rays, rt_radiance* host_out, void* host_workspace, int64_t n, int n_samples, int flags,
                  bool ordered, const uint32_t* host_order) {
  if (int rc = radiance_check(s, ex, cs, host_rays, host_out, n, n_samples, flags)) return rc;
  bool go;
  if (int rc = sync_begin(s, n, ordered, host_order, &go); rc || !go) return rc;
  Staging m;
  const size_t ray_bytes = (size_t)n * sizeof(rt_path_ray), out_bytes = (size_t)n * sizeof(rt_radiance);
  const size_t words = radiance_words_bytes(n, exec_f32(ex));
  // (each a multiple of 8 bytes, the first two of 16; the kernel's cursor behind the words)
  const size_t rays_at = m.take(ray_bytes), out_at = m.take(out_bytes), work_at = m.take(words + 16);
  const OrderParts o = take_order(m, n, ordered, host_order);
  if (int rc = m.alloc()) return rc;
  rt_path_ray* d_rays = m.at<rt_path_ray>(rays_at);
  rt_radiance* d_out = m.at<rt_radiance>(out_at);
  char* d_work = m.at<char>(work_at);
  uint32_t* d_order = ordered ? m.at<uint32_t>(o.order_at) : nullptr;
  const bool keep = host_workspace && (flags & RT_RADIANCE_ACCUMULATE);
  if (hipMemcpy(d_rays, host_rays, ray_bytes, hipMemcpyHostToDevice) != hipSuccess ||
      (keep ? hipMemcpy(d_work, host_workspace, words, hipMemcpyHostToDevice) : hipMemset(d_work, 0, words)) != hipSuccess ||
      hipMemset(s->status + kStatusRadianceSync, 0, sizeof(int)) != hipSuccess)
    return fail(RT_E_HIP, "ray upload failed: %s", hipGetErrorString(hipGetLastError()));
  if (ordered)
    if (int rc = order_for_sync(host_order, d_rays, n, RT_ORDER_PATH_RAYS, d_order, m.at<char>(o.ws_at))) return rc;
  if (int rc = by_precision(exec_f32(ex), [&](auto r) {
        return radiance_enqueue<decltype(r)>(s, cs, seed, d_rays, d_out, d_work, n, n_samples, flags, kStatusRadianceSync,
                                             nullptr, d_order);
      }))
    return rc;
  if (hipMemcpy(host_out, d_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
      (host_workspace && hipMemcpy(host_workspace, d_work, words, hipMemcpyDeviceToHost) != hipSuccess))
    return fail(RT_E_HIP, "radiance read-back failed: %s", hipGetErrorString(hipGetLastError()));
  return sync_end(s, kStatusRadianceSync, "radiance");
}

// ---- camera rays (include/rt.h rt_scene_camera_rays)

// the render's camera rays of (cs, seed, sample) in precision R enqueued on st
template <class R>
int camera_rays_enqueue(const rt_device_scene* s, const rt_camera_settings* cs, uint64_t seed, int sample, rt_path_ray* d_rays,
                        hipStream_t st) {
  if (int rc = ensure_precision<R>(s)) return rc;
  const rt_exec ex = one_shard(s);
  KernelParamsT<R> P;
  if (int rc = lane_params(s, cs, seed, &ex, P)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  if (rt_launch_camera_rays(P, s->variant, d_rays, sample, st))
    return fail(RT_E_HIP, "camera-ray launch failed: %s", hipGetErrorString(hipGetLastError()));
  return RT_OK;
}
int camera_rays_any(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed, int sample,
                    rt_path_ray* d_rays, hipStream_t st) {
  return by_precision(exec_f32(ex), [&](auto r) { return camera_rays_enqueue<decltype(r)>(s, cs, seed, sample, d_rays, st); });
}
int camera_rays_check(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, int sample, const void* rays) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  if (!ex) return fail(RT_E_INVALID, "null rt_exec");
  if (!cs) return fail(RT_E_INVALID, "null camera settings");
  if (!rays) return fail(RT_E_INVALID, "null ray buffer");
  if (sample < 0) return fail(RT_E_INVALID, "negative sample index %d", sample);
  if (ex->n_devices != 0) return fail(RT_E_INVALID, "camera rays are made on the scene's device (n_devices = 0)");
  return check_flags(ex);
}

}  // namespace

extern "C" {

int rt_scene_cast_async(const rt_device_scene* s, const rt_exec* ex, const rt_ray* d_rays, rt_hit* d_hits, int64_t n,
                        int32_t flags, void* hip_stream) {
  return cast_async(s, ex, d_rays, d_hits, n, flags, false, nullptr, (hipStream_t)hip_stream);
}

int rt_scene_cast_ordered_async(const rt_device_scene* s, const rt_exec* ex, const rt_ray* d_rays, rt_hit* d_hits, int64_t n,
                                int32_t flags, const uint32_t* d_order, void* hip_stream) {
  return cast_async(s, ex, d_rays, d_hits, n, flags, true, d_order, (hipStream_t)hip_stream);
}

int rt_scene_cast(const rt_device_scene* s, const rt_exec* ex, const rt_ray* host_rays, rt_hit* host_hits, int64_t n,
                  int32_t flags) {
  return cast_sync(s, ex, host_rays, host_hits, n, flags, false, nullptr);
}

int rt_scene_cast_ordered(const rt_device_scene* s, const rt_exec* ex, const rt_ray* host_rays, rt_hit* host_hits, int64_t n,
                          int32_t flags, const uint32_t* host_order) {
  return cast_sync(s, ex, host_rays, host_hits, n, flags, true, host_order);
}

int rt_scene_cast_status(const rt_device_scene* s, int32_t* overflowed) { return status_take(s, kStatusCastAsync, overflowed); }

size_t rt_scene_radiance_workspace_bytes(int64_t n, int32_t exec_flags) {
  return radiance_words_bytes(n < 0 ? 0 : n, (exec_flags & RT_EXEC_F32) != 0) + 16;
}

int rt_scene_radiance_async(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                            const rt_path_ray* d_rays, rt_radiance* d_out, void* d_workspace, int64_t n, int32_t n_samples,
                            int32_t flags, void* hip_stream) {
  return radiance_async(s, ex, cs, seed, d_rays, d_out, d_workspace, n, n_samples, flags, false, nullptr,
                        (hipStream_t)hip_stream);
}

int rt_scene_radiance_ordered_async(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                                    const rt_path_ray* d_rays, rt_radiance* d_out, void* d_workspace, int64_t n,
                                    int32_t n_samples, int32_t flags, const uint32_t* d_order, void* hip_stream) {
  return radiance_async(s, ex, cs, seed, d_rays, d_out, d_workspace, n, n_samples, flags, true, d_order,
                        (hipStream_t)hip_stream);
}

int rt_scene_radiance(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                      const rt_path_ray* host_rays, rt_radiance* host_out, void* host_workspace, int64_t n,
                      int32_t n_samples, int32_t flags) {
  return radiance_sync(s, ex, cs, seed, host_rays, host_out, host_workspace, n, n_samples, flags, false, nullptr);
}

int rt_scene_radiance_ordered(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                              const rt_path_ray* host_rays, rt_radiance* host_out, void* host_workspace, int64_t n,
                              int32_t n_samples, int32_t flags, const uint32_t* host_order) {
  return radiance_sync(s, ex, cs, seed, host_rays, host_out, host_workspace, n, n_samples, flags, true, host_order);
}

int rt_scene_radiance_status(const rt_device_scene* s, int32_t* overflowed) {
  return status_take(s, kStatusRadianceAsync, overflowed);
}

int rt_scene_camera_rays_async(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                               int32_t sample, rt_path_ray* d_rays, void* hip_stream) {
  if (int rc = camera_rays_check(s, ex, cs, sample, d_rays)) return rc;
  return camera_rays_any(s, ex, cs, seed, sample, d_rays, (hipStream_t)hip_stream);
}

int rt_scene_camera_rays(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                         int32_t sample, rt_path_ray* host_rays) {
  if (int rc = camera_rays_check(s, ex, cs, sample, host_rays)) return rc;
  const int h = rt_host_image_height(cs);
  if (h <= 0 || cs->image_width <= 0) return fail(RT_E_INVALID, "bad image size");
  const size_t bytes = (size_t)h * (size_t)cs->image_width * sizeof(rt_path_ray);
  HIP_TRY(hipSetDevice(s->device));
  Staging m;
  const size_t rays_at = m.take(bytes);
  if (int rc = m.alloc()) return rc;
  if (int rc = camera_rays_any(s, ex, cs, seed, sample, m.at<rt_path_ray>(rays_at), nullptr)) return rc;
  if (hipMemcpy(host_rays, m.at<rt_path_ray>(rays_at), bytes, hipMemcpyDeviceToHost) != hipSuccess)
    return fail(RT_E_HIP, "camera-ray read-back failed: %s", hipGetErrorString(hipGetLastError()));
  return RT_OK;
}

size_t rt_ray_order_workspace_bytes(int64_t n) { return rt_order_workspace_bytes((long long)n); }

int rt_scene_ray_order_async(const rt_device_scene* s, const void* d_rays, int64_t n, int32_t kind, uint32_t* d_order,
                             void* d_workspace, void* hip_stream) {
  if (int rc = order_check(s, d_rays, n, kind, d_order)) return rc;
  if (!d_workspace) return fail(RT_E_INVALID, "null workspace");
  if (n == 0) return RT_OK;
  HIP_TRY(hipSetDevice(s->device));
  if (rt_launch_ray_order(d_rays, (long long)n, order_stride(kind), d_order, d_workspace, hip_stream))
    return fail(RT_E_HIP, "order launch failed: %s", hipGetErrorString(hipGetLastError()));
  return RT_OK;
}

int rt_scene_ray_order(const rt_device_scene* s, const void* host_rays, int64_t n, int32_t kind, uint32_t* host_order) {
  if (int rc = order_check(s, host_rays, n, kind, host_order)) return rc;
  if (n == 0) return RT_OK;
  HIP_TRY(hipSetDevice(s->device));
  Staging m;
  const size_t ray_bytes = (size_t)n * order_stride(kind);
  const size_t rays_at = m.take(ray_bytes);
  const OrderParts o = take_order(m, n, true, nullptr);
  if (int rc = m.alloc()) return rc;
  uint32_t* d_order = m.at<uint32_t>(o.order_at);
  if (hipMemcpy(m.at<char>(rays_at), host_rays, ray_bytes, hipMemcpyHostToDevice) != hipSuccess)
    return fail(RT_E_HIP, "ray upload failed: %s", hipGetErrorString(hipGetLastError()));
  if (int rc = order_for_sync(nullptr, m.at<char>(rays_at), n, kind, d_order, m.at<char>(o.ws_at))) return rc;
  if (hipMemcpy(host_order, d_order, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(RT_E_HIP, "order read-back failed: %s", hipGetErrorString(hipGetLastError()));
  return RT_OK;
}

// Test hooks outside rt.h: the sort alone over given keys (only read), and its tile
int rt_order_sort_keys_async(int32_t device, const uint32_t* d_keys, int64_t n, uint32_t* d_order, void* d_workspace,
                             void* hip_stream) {
  if (n < 0 || n >= ((int64_t)1 << 31)) return fail(RT_E_INVALID, "bad key count %lld", (long long)n);
  if (n == 0) return RT_OK;
  if (!d_keys || !d_order || !d_workspace) return fail(RT_E_INVALID, "null argument");
  HIP_TRY(hipSetDevice(device));
  if (rt_launch_order_sort(d_keys, (long long)n, d_order, d_workspace, hip_stream))
    return fail(RT_E_HIP, "sort launch failed: %s", hipGetErrorString(hipGetLastError()));
  return RT_OK;
}
int rt_ray_order_tile(void) { return rt_order_tile(); }

}  // extern "C"
