// rt_api.hip — the C-ABI entry points of include/rt.h: scene build (rt_build.cpp, once per
// call however many devices render), upload to HBM (a precision's records on its first render),
// kernel launch (rt_kernel.hip / rt_kernel64.hip), multi-device scenes (one process, many GPUs:
// concurrent uploads, shard renders on per-device streams, a device-side gather by peer copies
// into the first device's framebuffer and ONE device-to-host copy), the 8-bit output epilogue,
// the progressive film (its state and entry points; kernels in rt_film.hip) and the multi-device
// film (one frame film on the first device, a pass workspace per shard), adaptive film passes (the
// count plane and entry points; kernels in rt_adaptive.hip and rt_list*.hip), error reporting.
// A synchronous render (render_sync) runs render_one (one device) or render_many (a thread per
// shard) over the same stages: prepare_part, enqueue_shard, enqueue_readback, fill_stats.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rt.h"
#include "rt_adaptive.h"
#include "rt_denoise.h"
#include "rt_film.h"
#include "rt_internal.h"
#include "rt_kernel_class.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(RT_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

bool exec_f32(const rt_exec* ex) { return ex && (ex->flags & RT_EXEC_F32) != 0; }
int acc_words_of(bool f32) { return f32 ? RT_ACC_WORDS(float) : RT_ACC_WORDS(double); }
size_t elem_size_of(bool f32) { return f32 ? sizeof(float) : sizeof(double); }
int prec_bit(bool f32) { return f32 ? 1 : 2; }  // ensure_precisions' mask

// the workspace of one render: fixed-point sums at 0, NaN flags at off_flag, queue head words at
// off_ctr (every part 256-byte aligned, zeroed slack behind the sums and the flags: rt_film.hip
// reads both as 16-byte vectors)
struct Workspace { size_t off_flag, off_ctr, bytes; };
Workspace workspace_layout(size_t tile_pixels, int acc_words) {
  const size_t of = (tile_pixels * acc_words * sizeof(long long) + 255) & ~(size_t)255;
  const size_t oc = of + ((tile_pixels * sizeof(unsigned) + 255) & ~(size_t)255);
  return {of, oc, oc + 256 * 8};  // up to 8 queue head words (rt_render_kernel.h RT_QUEUES)
}

template <class T>
int upload(T** dst, const std::vector<T>& src) {
  size_t bytes = src.size() * sizeof(T);
  HIP_TRY(hipMalloc((void**)dst, bytes ? bytes : 16));
  if (bytes) HIP_TRY(hipMemcpy(*dst, src.data(), bytes, hipMemcpyHostToDevice));
  return RT_OK;
}

// the device copies of one precision's records (rt_internal.h HostArraysT)
template <class R>
struct DevArrays {
  SceneRecordsT<R> rec;     // device pointers; nodes and perlin_perm are the scene's (both precisions share them)
  void* owned[12] = {};     // the allocations behind rec, to free
  int n_owned = 0;
  int resident_blocks = 0;  // render-kernel workgroups resident on the device (occupancy query)
  int lds_nodes = 0;        // top surface-BVH nodes this precision's kernel stages in LDS per workgroup
  template <class T>
  int put(const T*& dst, const std::vector<T>& src) {
    T* d = nullptr;
    const int rc = ::upload(&d, src);
    dst = d;
    owned[n_owned++] = d;
    return rc;
  }
  int upload(const HostArraysT<R>& H, const float* nodes, const int* perlin_perm) {
    rec.nodes = nodes, rec.perlin_perm = perlin_perm;
    int rc;
    if ((rc = put(rec.prims, H.prims)) || (rc = put(rec.prim_shade, H.prim_shade)) ||
        (rc = put(rec.prim_uv, H.prim_uv)) || (rc = put(rec.mats, H.mats)) || (rc = put(rec.texs, H.texs)) ||
        (rc = put(rec.motions, H.motions)) || (rc = put(rec.uvframes, H.uvframes)) ||
        (rc = put(rec.flat_recs, H.flat_recs)) || (rc = put(rec.boxes, H.boxes)) || (rc = put(rec.texels, H.texels)) ||
        (rc = put(rec.perlin_grad, H.perlin_grad)) || (rc = put(rec.instances, H.instances)))
      return rc;
    return RT_OK;
  }
  void release() {
    for (int k = 0; k < n_owned; ++k) (void)hipFree(owned[k]);
  }
};

}  // namespace

struct rt_device_scene {
  int device = 0;
  float* nodes = nullptr;
  int* perlin_perm = nullptr;
  int* status = nullptr;     // 8 words: [0] the renders' stack overflow, [1] / [2] the asynchronous / synchronous casts',
                             // [4] / [5] the asynchronous / synchronous radiance queries'
  mutable int* prim_mat = nullptr;  // HostScene::prim_mat, uploaded by the first cast (rt_scene_cast*)
  // a precision's records are uploaded (and its kernel's occupancy queried) on its first render:
  // a caller that renders one precision never pays for the other's copy in HBM or its upload
  std::shared_ptr<const HostScene> host;
  mutable std::mutex mu;
  mutable DevArrays<float> f32;
  mutable DevArrays<double> f64;
  mutable bool have_f32 = false, have_f64 = false;
  int stack_depth = 1;       // LDS stack entries per lane
  int variant = RT_VAR_FLAT;  // render-kernel variant (rt_internal.h RT_VAR_*)
  double build_ms = 0;       // host scene build (shared by every device of a multi-device scene)
  mutable double upload_ms = 0;  // host -> device copies of this device (common + precisions so far)
  template <class R>
  DevArrays<R>& arrays() const;
  template <class R>
  bool& have() const;
};
template <>
DevArrays<float>& rt_device_scene::arrays<float>() const { return f32; }
template <>
DevArrays<double>& rt_device_scene::arrays<double>() const { return f64; }
template <>
bool& rt_device_scene::have<float>() const { return have_f32; }
template <>
bool& rt_device_scene::have<double>() const { return have_f64; }

// The resident per-shard buffers of a multi-device scene: shard k's tile, its render workspace
// (fixed-point sums, NaN flags, queue heads), its stream and timing events on devices[k]
struct MultiPart {
  int device = 0;
  void* d_tile = nullptr;
  size_t tile_cap = 0;
  char* ws = nullptr;
  size_t ws_cap = 0;
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
};
struct rt_multi_scene {
  std::vector<int> devices;                // shard k renders on devices[k]
  std::vector<rt_device_scene*> scenes;    // one per DISTINCT device, in first-use order
  std::vector<int> scene_of;               // devices[k] -> scenes index
  double build_ms = 0, upload_ms = 0;      // one host build; the uploads' wall time (concurrent)
  // kept across renders (grown when a frame needs more): no allocation after the first render
  std::mutex mu;                           // one render at a time: the buffers below are shared
  std::vector<MultiPart> parts;            // per devices[k]
  std::vector<char> peer_ok;               // per distinct device: may write the first device's memory
  void* d_gather = nullptr;                // first device: the n tiles in global row order
  size_t gather_cap = 0;
  uint8_t* d_codes = nullptr;              // first device: the 8-bit epilogue's output
  size_t codes_cap = 0;
  hipStream_t st0 = nullptr;               // first device: epilogue and device-to-host copy
  int* h_status = nullptr;                 // pinned host word: the one-device render's status read-back
};

// A progressive film (include/rt.h rt_film_*, rt_film.h): the device-resident accumulation state of
// one (scene, camera, seed, precision, shard).  One device allocation made at create holds the
// totals, flags and q, the pass workspace a render writes, the resolved tile of rt_film_read and
// the noise figure's partials: rt_film_add allocates nothing.
struct FilmHeader {  // the saved state's header (rt_film_save); totals, flags and q follow
  uint32_t magic, version;
  int32_t f32, width, height, rows, n_shards, shard, row_block, passes;
  uint32_t key0, key1;
  int64_t samples;
  int64_t reserved;
};
static_assert(sizeof(FilmHeader) == 64, "the saved film header is 64 bytes");
constexpr uint32_t kFilmMagic = 0x4d4c4652u;  // "RFLM"
constexpr uint32_t kFilmVersion = 1;          // a uniform film: header, totals, flags, q
constexpr uint32_t kFilmVersionCounts = 2;    // a non-uniform film: those, then the count plane; header samples / passes: the maxima
struct rt_film {
  const rt_device_scene* scene = nullptr;
  rt_camera_settings cs{};
  std::vector<rt_redirect_target> targets;  // cs.redirect_targets points here
  uint64_t seed = 0;
  rt_exec ex{};
  bool f32 = false;
  int width = 0, height = 0, rows = 0, acc_words = 0;
  size_t n_pixels = 0;
  int64_t samples = 0;  // N
  int32_t passes = 0;   // K
  char* mem = nullptr;  // the one allocation; the parts below point into it
  unsigned long long* total = nullptr;
  unsigned int* flags = nullptr;
  double* q = nullptr;
  char* ws = nullptr;  // a pass's workspace, laid out as ws_lay
  Workspace ws_lay{};
  void* tile = nullptr;
  double* partial_sum = nullptr;
  int* partial_cnt = nullptr;
  size_t total_bytes = 0, flag_bytes = 0, q_bytes = 0, state_span = 0;  // (padded; total, flags, q are contiguous)
  hipStream_t last = nullptr;  // the stream of the last enqueue: the synchronous calls run behind it
  std::mutex mu;
  // first-hit features and the denoiser's planes (rt_denoise.h): allocations of their own, made by
  // the first rt_denoise_features / rt_denoise_film and kept; not part of the saved state
  unsigned long long* feat = nullptr;  // rt_feat_words(binary64) int64 per tile pixel
  int feat_samples = 0;                // n_feat of the words in `feat` (0: none yet)
  unsigned long long* feat2 = nullptr; // the remodulation albedo's feature words (rt_denoise_albedo)
  int albedo_samples = 0;              // ... and their sample count (0: none)
  double* dn_mem = nullptr;            // ev[2][4] and guide[8] planes of n_pixels doubles
  bool owned = false;                  // a multi-device film's frame: rt_film_add / load / reset / destroy refuse it
  hipEvent_t e_order = nullptr;        // ... and its event: a new `last` stream waits for the one before (film_follow)
  // adaptive passes (rt_adaptive.h): one allocation of its own, made by the first rt_adaptive_add (or
  // the load of a version-2 state) and kept — the count plane, the selection list and its length
  // word, the select kernels' scratch.  While `nonuniform`, samples / passes above are not read:
  // the counts are the plane's
  char* ad_mem = nullptr;
  uint32_t* counts = nullptr;          // 2 x uint32 per tile pixel: N_p, K_p
  rt_adaptive_rec* ad_list = nullptr;  // the last pass's selection, ascending tile pixels
  int* ad_n = nullptr;                 // ... and its length
  void* ad_scratch = nullptr;
  bool nonuniform = false;
  bool ad_listed = false;              // ad_list / ad_n hold a pass's selection
  int32_t adaptive_passes = 0;
};

// A multi-device film (include/rt.h rt_multi_film_*): ONE accumulation state — `frame`, an ordinary
// one-shard film of the whole image on devices[0] — and per shard k a pass workspace, a stream and
// events on devices[k].  A pass renders shard k's samples on devices[k] and rt_film_merge_rows_kernel
// folds the workspace straight into the frame's rows: launched on devices[k] itself, writing the
// first device's memory (`direct`, as the one-shot resolve does), or, without peer access, on the
// first device from a copy of the workspace's sums and flags (`stage`).
struct FilmPart {
  int device = 0;
  const rt_device_scene* scene = nullptr;
  rt_exec ex{};           // shard k of n on devices[k]
  int tile_rows = 0;
  bool active = false;    // the shard holds rows of the frame (more devices than row blocks: not all do)
  bool direct = true;
  bool own_ws = false;    // (part 0 renders into the frame film's own pass workspace)
  char* ws = nullptr;
  Workspace ws_lay{};
  char* stage = nullptr;          // first device: the copied sums and flags (copy path)
  hipStream_t st = nullptr;       // devices[k]: render, then the merge or the copy
  hipStream_t st_merge = nullptr; // first device: the merge of a copied pass
  hipEvent_t e_copy = nullptr;    // devices[k]: the copy has landed
  hipEvent_t e_merge = nullptr;   // the merge is done (on the device whose stream ran it)
};
struct rt_multi_film {
  const rt_multi_scene* scene = nullptr;
  rt_film* frame = nullptr;
  std::vector<FilmPart> parts;
  hipStream_t st_frame = nullptr;  // first device: waits for every merge; the frame film's `last`
  hipEvent_t e_frame = nullptr;    // first device: what was enqueued on the frame before a pass
  bool single = false;             // one shard merged on its own stream: that stream is st_frame, no events
  int64_t copies = 0;              // shard passes that went through the staging copy so far (rt_multi_film_copies)
  std::mutex mu;
};

namespace {

// the records of precision R on the scene's device (uploaded on first use) and their kernel's
// resident workgroups; thread-safe
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

// RenderCall: what a render is given besides the frame.
// ws / ws_cap: a caller-held workspace (a multi-device scene's resident one), or null: the render
// takes one from the stream-ordered pool (hipMallocAsync / hipFreeAsync).  lone: a synchronous
// call's launch (rt_render, rt_multi_render), whose time includes the end of its queue: the flat
// kernels take 64-id pools there, so no wave holds a second round of items when the queue drains
// (one binary64 Cornell launch 5.385 -> 5.164 ms; with frames overlapped on two streams, as
// rt_render_async callers run them, 128 is as fast and the README scene 2 % faster:
// profiles/r5/pool).  Env RT_AMD_POOL_SHIFT overrides (experiments).
// sample0 / resolve: a film pass (rt_film_add) renders samples [sample0, sample0 + spp) and leaves
// the sums in the workspace (no mean: d_out is unused) for rt_film_merge_kernel.
struct RenderCall {
  void* d_out = nullptr;  // linear RGB of the render's precision, on the scene's device
  char* ws = nullptr;
  size_t ws_cap = 0;
  int frame_rows = 0;     // > 0: d_out is a whole frame of that many rows (KernelParams::out_frame_rows)
  bool lone = false, resolve = true;
  int sample0 = 0;
};

// one render of the scene's records of precision R, enqueued on `hip_stream`
template <class R>
int render_async(const rt_device_scene* s, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex,
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
  P.status = s->status;
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

// rt_exec.flags: known bits only, at most one 8-bit encoding
int check_flags(const rt_exec* ex) {
  const int known = RT_EXEC_F32 | RT_EXEC_ENCODE8_SRGB | RT_EXEC_ENCODE8_SQRT | RT_EXEC_SOLO;
  if (ex->flags & ~known) return fail(RT_E_INVALID, "unknown rt_exec.flags bits 0x%x", ex->flags & ~known);
  if ((ex->flags & RT_EXEC_ENCODE8_SRGB) && (ex->flags & RT_EXEC_ENCODE8_SQRT))
    return fail(RT_E_INVALID, "rt_exec.flags: RT_EXEC_ENCODE8_SRGB and RT_EXEC_ENCODE8_SQRT are exclusive");
  return RT_OK;
}

// A frame's arguments (non-null) checked before a scene is built or a device touched: image, shard,
// flags, camera (a throw-away KernelParams).  For rt_render, rt_multi_render and rt_film_create alone.
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

// rt_exec.flags -> the 8-bit epilogue's encoding (0 sRGB, 1 sqrt) or -1 (linear output)
int exec_encoding(const rt_exec* ex) {
  if (!ex) return -1;
  if (ex->flags & RT_EXEC_ENCODE8_SRGB) return 0;
  if (ex->flags & RT_EXEC_ENCODE8_SQRT) return 1;
  return -1;
}

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

// the precision-independent part of a device scene: BVH nodes, Perlin permutations, status word,
// the kernel variant and the LDS plan; precisions follow on first render (ensure_precision)
int upload_common(const std::shared_ptr<const HostScene>& Hp, int device, rt_device_scene** out) {
  auto t0 = Clock::now();
  const HostScene& H = *Hp;
  *out = nullptr;
  HIP_TRY(hipSetDevice(device));
  auto* s = new rt_device_scene();
  s->device = device;
  s->host = Hp;
  std::vector<int> status(8, 0);
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

int ensure_precisions(const rt_device_scene* s, int prec_mask) {  // bit 0: FP32, bit 1: binary64
  int rc = RT_OK;
  if ((prec_mask & 1) && (rc = ensure_precision<float>(s))) return rc;
  if ((prec_mask & 2) && (rc = ensure_precision<double>(s))) return rc;
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
        if (rc) errs[j] = g_err;
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
    HIP_TRY(hipMemsetAsync(s->status, 0, 4 * sizeof(int), q.st));
    if (int r = enqueue_shard(M, 0, cs, seed, e, ShardOut::tile)) return r;
    // (the image is copied before the status word is read, in the same synchronisation: on
    // RT_E_STACK out_host holds the partial image, include/rt.h)
    if (int r = enqueue_readback(M, q.d_tile, (int64_t)tile_pixels * 3, f32, exec_encoding(ex), out_host, q.st)) return r;
    HIP_TRY(hipMemcpyAsync(M->h_status, s->status, sizeof(int), hipMemcpyDeviceToHost, q.st));
    return RT_OK;
  };
  if (const int r = enqueue()) {
    (void)hipStreamSynchronize(q.st);
    return r;
  }
  HIP_TRY(hipStreamSynchronize(q.st));
  if (*M->h_status) return fail(RT_E_STACK, "BVH traversal stack overflow");
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
    if (hipSetDevice(s->device) != hipSuccess || hipMemsetAsync(s->status, 0, 4 * sizeof(int), q.st) != hipSuccess ||
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
        if ((rcs[k] = run())) errs[k] = g_err;
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
  for (const rt_device_scene* s : M->scenes) {
    int ps = 0;
    (void)hipSetDevice(s->device);
    if (hipMemcpy(&ps, s->status, 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(RT_E_HIP, "status");
    status |= ps;
  }
  if (status) return fail(RT_E_STACK, "BVH traversal stack overflow");
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

// ---- progressive film (rt_film.h)

FilmHeader film_header(const rt_film* f) {
  FilmHeader h{};
  h.magic = kFilmMagic;
  h.version = kFilmVersion;
  h.f32 = f->f32;
  h.width = f->width;
  h.height = f->height;
  h.rows = f->rows;
  h.n_shards = f->ex.n_shards;
  h.shard = f->ex.shard;
  h.row_block = f->ex.row_block;
  h.passes = f->passes;
  h.key0 = (uint32_t)f->seed;  // the Philox key (rt_build.cpp rt_host_make_params)
  h.key1 = (uint32_t)(f->seed >> 32);
  h.samples = f->samples;
  return h;
}
// the saved state: header, totals, flags, q (unpadded); a non-uniform film's: then the count plane
size_t film_sums_bytes(const rt_film* f) { return f->n_pixels * f->acc_words * sizeof(long long); }
size_t film_counts_bytes(const rt_film* f) { return f->n_pixels * 2 * sizeof(uint32_t); }
int64_t film_state_bytes_v1(const rt_film* f) {
  return (int64_t)(sizeof(FilmHeader) + film_sums_bytes(f) + f->n_pixels * (sizeof(unsigned) + sizeof(double)));
}
int64_t film_state_bytes(const rt_film* f) {
  return film_state_bytes_v1(f) + (f->nonuniform ? (int64_t)film_counts_bytes(f) : 0);
}
void film_destroy(rt_film* f) {
  if (!f) return;
  if (f->mem) {
    (void)hipSetDevice(f->scene->device);
    if (f->last) (void)hipStreamSynchronize(f->last);
    (void)hipFree(f->mem);
    (void)hipFree(f->feat);
    (void)hipFree(f->feat2);
    (void)hipFree(f->dn_mem);
    (void)hipFree(f->ad_mem);
  }
  delete f;
}

// ---- adaptive passes (rt_adaptive.h)

// the buffers of the adaptive passes, allocated once (the film's device is current)
int adaptive_alloc(rt_film* f) {
  if (f->ad_mem) return RT_OK;
  auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t cb = pad(film_counts_bytes(f)), lb = pad(f->n_pixels * sizeof(rt_adaptive_rec)), nb = 256;
  HIP_TRY(hipMalloc((void**)&f->ad_mem, cb + lb + nb + pad(rt_adaptive_scratch_bytes((long long)f->n_pixels))));
  char* p = f->ad_mem;
  f->counts = (uint32_t*)p, p += cb;
  f->ad_list = (rt_adaptive_rec*)p, p += lb;
  f->ad_n = (int*)p, p += nb;
  f->ad_scratch = p;
  return RT_OK;
}
// what the count plane says about a non-uniform film, read behind f->last (synchronous; f->mu held)
struct CountStats {
  int64_t total = 0;  // the sum of N_p over the pixels that count
  uint32_t min_n = 0, max_n = 0, max_k = 0;
};
int adaptive_stats(const rt_film* f, CountStats& st, std::vector<uint32_t>* counts_out = nullptr) {
  std::vector<uint32_t> c(2 * f->n_pixels);
  std::vector<unsigned> flags(f->n_pixels);
  HIP_TRY(hipSetDevice(f->scene->device));
  HIP_TRY(hipMemcpyAsync(c.data(), f->counts, film_counts_bytes(f), hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipMemcpyAsync(flags.data(), f->flags, f->n_pixels * sizeof(unsigned), hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipStreamSynchronize(f->last));
  bool any = false;
  for (size_t p = 0; p < f->n_pixels; ++p) {
    st.max_n = std::max(st.max_n, c[2 * p]);
    st.max_k = std::max(st.max_k, c[2 * p + 1]);
    if (flags[p] || !rt_adaptive_inside((long long)p, f->width, f->height, f->ex.n_shards, f->ex.shard, f->ex.row_block))
      continue;
    st.total += c[2 * p];
    st.min_n = any ? std::min(st.min_n, c[2 * p]) : c[2 * p];
    any = true;
  }
  if (counts_out) counts_out->swap(c);
  return RT_OK;
}
// The argument block of a one-lane kernel (rt_lane.h: the list, feature and query kernels) for the
// frame (cs, seed, ex): the render's, with no staged nodes (every node from memory) and a work plan
// nothing reads (the kernels have their own).  A stack overflow sets the scene's status word `word`
template <class R>
int lane_params(const rt_device_scene* s, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex, KernelParamsT<R>& P,
                int word = 0) {
  LaunchInputs L;
  L.resident_lanes = 4096;
  L.lds_nodes = 0;
  std::string err;
  if (int rc = rt_host_render_params(*s->host, s->variant, s->arrays<R>().rec, cs, seed, ex, L, P, err))
    return fail(rc, "%s", err.c_str());
  P.status = s->status + word;
  return RT_OK;
}
// one adaptive pass of precision R on st: select, the zeroed workspace, the list kernel, the merge
template <class R>
int adaptive_pass(rt_film* f, int n_samples, double threshold, long long max_samples, hipStream_t st) {
  const rt_device_scene* s = f->scene;
  if (int rc = ensure_precision<R>(s)) return rc;
  rt_camera_settings cs = f->cs;
  cs.samples_per_pixel = n_samples;
  KernelParamsT<R> P;
  if (int rc = lane_params(s, &cs, f->seed, &f->ex, P)) return rc;
  P.accum = (unsigned long long*)f->ws;
  P.nanflag = (unsigned int*)(f->ws + f->ws_lay.off_flag);
  P.counter = (int*)(f->ws + f->ws_lay.off_ctr);
  int chunk = 0;  // (experiments and tests: samples per item; the state does not depend on it)
  if (const char* e = rt_knob("RT_AMD_LIST_CHUNK")) chunk = std::max(0, atoi(e));
  const long long np = (long long)f->n_pixels;
  if (rt_adaptive_launch_select(f->total, f->flags, f->q, f->counts, np, f->acc_words, n_samples, threshold, max_samples,
                                f->width, f->height, f->ex.n_shards, f->ex.shard, f->ex.row_block, f->ad_scratch, f->ad_list,
                                f->ad_n, st))
    return fail(RT_E_HIP, "select launch failed: %s", hipGetErrorString(hipGetLastError()));
  HIP_TRY(hipMemsetAsync(f->ws, 0, f->ws_lay.bytes, st));
  if (rt_launch_list(P, s->variant, f->ad_list, f->ad_n, n_samples, chunk, st))
    return fail(RT_E_HIP, "list kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
  if (rt_adaptive_launch_merge(f->total, f->flags, f->q, f->counts, P.accum, P.nanflag, f->ad_list, f->ad_n, np, f->acc_words,
                               n_samples, st))
    return fail(RT_E_HIP, "list merge launch failed: %s", hipGetErrorString(hipGetLastError()));
  return RT_OK;
}
// A multi-device film's frame is read like any film, but only the multi film adds to it, loads,
// resets and destroys it (rt_multi_film_*): rt_film_add / load / reset / destroy refuse it
int refuse_owned(const rt_film* f, const char* call) {
  if (f->owned) return fail(RT_E_INVALID, "%s: the film is a multi-device film's frame (use rt_multi_film_*)", call);
  return RT_OK;
}
// Before work on `st`, which then becomes the stream the synchronous calls run behind (`last`).  A
// plain film's calls are ordered by the caller: nothing to do.  A multi-device film's frame is
// filled by merges the caller has no stream for, so there a new stream first waits for the one
// before it (which has waited for the merges)
int film_follow(rt_film* f, hipStream_t st) {
  if (f->e_order && st != f->last) {
    HIP_TRY(hipEventRecord(f->e_order, f->last));
    HIP_TRY(hipStreamWaitEvent(st, f->e_order, 0));
  }
  return RT_OK;
}
// the film's totals as one-shot kernel parameters of N samples: what rt_resolve_kernel reads
template <class R>
int film_resolve(const rt_film* f, void* d_out, hipStream_t st) {
  KernelParamsT<R> P;
  std::memset(&P, 0, sizeof P);
  rt_camera_settings cs = f->cs;
  cs.samples_per_pixel = (int32_t)f->samples;
  std::string err;
  if (int rc = rt_host_make_params(&cs, f->seed, &f->ex, P, err)) return fail(rc, "%s", err.c_str());
  P.accum = f->total;
  P.nanflag = f->flags;
  P.out = (R*)d_out;
  if (rt_launch_resolve(P, st)) return fail(RT_E_HIP, "resolve launch failed: %s", hipGetErrorString(hipGetLastError()));
  return RT_OK;
}
int film_resolve_any(const rt_film* f, void* d_out, hipStream_t st) {
  if (f->samples <= 0) return fail(RT_E_INVALID, "the film holds no samples");
  HIP_TRY(hipSetDevice(f->scene->device));
  if (f->nonuniform) {  // each pixel's mean over its own N_p (rt_adaptive.h)
    if (rt_adaptive_launch_resolve(f->total, f->flags, f->counts, d_out, (long long)f->n_pixels, f->f32, st))
      return fail(RT_E_HIP, "resolve launch failed: %s", hipGetErrorString(hipGetLastError()));
    return RT_OK;
  }
  return f->f32 ? film_resolve<float>(f, d_out, st) : film_resolve<double>(f, d_out, st);
}

// ---- first-hit features and the denoiser (rt_denoise.h, rt_features.h)

// samples [0, n_feat) of every tile pixel into the zeroed feature words `feat`
template <class R>
int film_features(rt_film* f, unsigned long long* feat, int n_feat, hipStream_t st) {
  const rt_device_scene* s = f->scene;
  if (int rc = ensure_precision<R>(s)) return rc;
  rt_camera_settings cs = f->cs;
  cs.samples_per_pixel = n_feat;
  KernelParamsT<R> P;
  if (int rc = lane_params(s, &cs, f->seed, &f->ex, P)) return rc;
  HIP_TRY(hipMemsetAsync(feat, 0, f->n_pixels * rt_feat_words(!f->f32) * sizeof(long long), st));
  if (rt_launch_features(P, s->variant, feat, n_feat, st))
    return fail(RT_E_HIP, "feature launch failed: %s", hipGetErrorString(hipGetLastError()));
  return RT_OK;
}

// ---- ray queries (include/rt.h rt_scene_cast; rt_query.h)

// n queries of precision R enqueued on st; a stack overflow sets the scene's status word `word`
template <class R>
int cast_enqueue(const rt_device_scene* s, const rt_ray* d_rays, rt_hit* d_hits, int64_t n, int flags, int word,
                 hipStream_t st, const uint32_t* d_order = nullptr) {
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
  // the scene parts of a render's argument block are what the kernel reads: a valid 1 x 1 camera fills the rest
  rt_camera_settings cs{};
  cs.look_at[2] = -1.0;
  cs.up[1] = 1.0;
  cs.vfov = 1.0;
  cs.aspect_ratio = 1.0;
  cs.image_width = cs.samples_per_pixel = cs.max_recursion_depth = 1;
  cs.focus_dist = 1.0;
  rt_exec ex{};
  ex.device = s->device;
  ex.n_shards = 1;
  ex.row_block = 4;
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

// ---- radiance queries (include/rt.h rt_scene_radiance; rt_radiance.h)

// the bytes of n rays' workspace words; the kernel's cursor lies behind them (16 bytes)
size_t radiance_words_bytes(int64_t n, bool f32) { return (size_t)n * ((f32 ? 3 : 6) + 1) * sizeof(unsigned long long); }

rt_exec one_shard(const rt_device_scene* s) {
  rt_exec ex{};
  ex.device = s->device;
  ex.n_shards = 1;
  ex.row_block = 4;
  return ex;
}

// n rays of precision R enqueued on st: the workspace zeroed (or only its cursor, accumulate), the
// path kernel, the resolve; a stack overflow sets the scene's status word `word`
template <class R>
int radiance_enqueue(const rt_device_scene* s, const rt_camera_settings* cs, uint64_t seed, const rt_path_ray* d_rays,
                     rt_radiance* d_out, void* d_work, int64_t n, int n_samples, int flags, int word, hipStream_t st,
                     const uint32_t* d_order = nullptr) {
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
int camera_rays_check(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, int sample, const void* rays) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  if (!ex) return fail(RT_E_INVALID, "null rt_exec");
  if (!cs) return fail(RT_E_INVALID, "null camera settings");
  if (!rays) return fail(RT_E_INVALID, "null ray buffer");
  if (sample < 0) return fail(RT_E_INVALID, "negative sample index %d", sample);
  if (ex->n_devices != 0) return fail(RT_E_INVALID, "camera rays are made on the scene's device (n_devices = 0)");
  return check_flags(ex);
}

// ---- ray orders (include/rt.h rt_scene_ray_order; rt_order.hip)

// the checks of an order call that need no device
int order_check(const rt_device_scene* s, const void* rays, int64_t n, int kind, const void* order) {
  if (!s) return fail(RT_E_INVALID, "null scene");
  if (!rays) return fail(RT_E_INVALID, "null ray buffer");
  if (!order) return fail(RT_E_INVALID, "null order buffer");
  if (n < 0) return fail(RT_E_INVALID, "negative ray count %lld", (long long)n);
  if (n >= ((int64_t)1 << 31)) return fail(RT_E_INVALID, "%lld rays: an order holds fewer than 2^31", (long long)n);
  if (kind != RT_ORDER_RAYS && kind != RT_ORDER_PATH_RAYS) return fail(RT_E_INVALID, "unknown record kind %d", kind);
  return RT_OK;
}
int order_count_check(int64_t n) {
  if (n >= ((int64_t)1 << 31)) return fail(RT_E_INVALID, "%lld rays: an order holds fewer than 2^31", (long long)n);
  return RT_OK;
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
size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// rt_scene_cast / rt_scene_cast_ordered: ordered with host_order null computes the order on the device
int cast_sync(const rt_device_scene* s, const rt_exec* ex, const rt_ray* host_rays, rt_hit* host_hits, int64_t n, int flags,
              bool ordered, const uint32_t* host_order) {
  if (int rc = cast_check(s, ex, host_rays, host_hits, n, flags)) return rc;
  if (ordered)
    if (int rc = order_count_check(n)) return rc;
  if (n == 0) return RT_OK;
  if (ordered && host_order)
    if (int rc = permutation_check(host_order, n)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  char* mem = nullptr;
  const size_t ray_bytes = (size_t)n * sizeof(rt_ray), hit_bytes = (size_t)n * sizeof(rt_hit);
  const size_t order_at = up256(ray_bytes + hit_bytes), ws_at = order_at + up256((size_t)n * sizeof(uint32_t));
  const size_t total = !ordered ? ray_bytes + hit_bytes : ws_at + (host_order ? 0 : rt_order_workspace_bytes((long long)n));
  HIP_TRY(hipMalloc((void**)&mem, total));  // (rays and hits both multiples of 16 bytes)
  rt_ray* d_rays = (rt_ray*)mem;
  rt_hit* d_hits = (rt_hit*)(mem + ray_bytes);
  uint32_t* d_order = ordered ? (uint32_t*)(mem + order_at) : nullptr;
  int status = 0;
  int rc = RT_OK;
  if (hipMemcpy(d_rays, host_rays, ray_bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(s->status + 2, 0, sizeof(int)) != hipSuccess)
    rc = fail(RT_E_HIP, "ray upload failed: %s", hipGetErrorString(hipGetLastError()));
  if (!rc && ordered) rc = order_for_sync(host_order, d_rays, n, RT_ORDER_RAYS, d_order, mem + ws_at);
  if (!rc)
    rc = exec_f32(ex) ? cast_enqueue<float>(s, d_rays, d_hits, n, flags, 2, nullptr, d_order)
                      : cast_enqueue<double>(s, d_rays, d_hits, n, flags, 2, nullptr, d_order);
  if (!rc && (hipMemcpy(host_hits, d_hits, hit_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
              hipMemcpy(&status, s->status + 2, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess))
    rc = fail(RT_E_HIP, "hit read-back failed: %s", hipGetErrorString(hipGetLastError()));
  (void)hipFree(mem);
  if (!rc && status) return fail(RT_E_STACK, "BVH traversal stack overflow");
  return rc;
}

// rt_scene_radiance / rt_scene_radiance_ordered, as cast_sync
int radiance_sync(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                  const rt_path_ray* host_rays, rt_radiance* host_out, void* host_workspace, int64_t n, int n_samples, int flags,
                  bool ordered, const uint32_t* host_order) {
  if (int rc = radiance_check(s, ex, cs, host_rays, host_out, n, n_samples, flags)) return rc;
  if (ordered)
    if (int rc = order_count_check(n)) return rc;
  if (n == 0) return RT_OK;
  if (ordered && host_order)
    if (int rc = permutation_check(host_order, n)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  char* mem = nullptr;
  const size_t ray_bytes = (size_t)n * sizeof(rt_path_ray), out_bytes = (size_t)n * sizeof(rt_radiance);
  const size_t words = radiance_words_bytes(n, exec_f32(ex));
  const size_t plain = ray_bytes + out_bytes + words + 16;  // (each a multiple of 8 bytes, the first two of 16)
  const size_t order_at = up256(plain), ws_at = order_at + up256((size_t)n * sizeof(uint32_t));
  const size_t total = !ordered ? plain : ws_at + (host_order ? 0 : rt_order_workspace_bytes((long long)n));
  HIP_TRY(hipMalloc((void**)&mem, total));
  rt_path_ray* d_rays = (rt_path_ray*)mem;
  rt_radiance* d_out = (rt_radiance*)(mem + ray_bytes);
  char* d_work = mem + ray_bytes + out_bytes;
  uint32_t* d_order = ordered ? (uint32_t*)(mem + order_at) : nullptr;
  const bool keep = host_workspace && (flags & RT_RADIANCE_ACCUMULATE);
  int status = 0;
  int rc = RT_OK;
  if (hipMemcpy(d_rays, host_rays, ray_bytes, hipMemcpyHostToDevice) != hipSuccess ||
      (keep ? hipMemcpy(d_work, host_workspace, words, hipMemcpyHostToDevice) : hipMemset(d_work, 0, words)) != hipSuccess ||
      hipMemset(s->status + 5, 0, sizeof(int)) != hipSuccess)
    rc = fail(RT_E_HIP, "ray upload failed: %s", hipGetErrorString(hipGetLastError()));
  if (!rc && ordered) rc = order_for_sync(host_order, d_rays, n, RT_ORDER_PATH_RAYS, d_order, mem + ws_at);
  if (!rc)
    rc = exec_f32(ex) ? radiance_enqueue<float>(s, cs, seed, d_rays, d_out, d_work, n, n_samples, flags, 5, nullptr, d_order)
                      : radiance_enqueue<double>(s, cs, seed, d_rays, d_out, d_work, n, n_samples, flags, 5, nullptr, d_order);
  if (!rc && (hipMemcpy(host_out, d_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
              (host_workspace && hipMemcpy(host_workspace, d_work, words, hipMemcpyDeviceToHost) != hipSuccess) ||
              hipMemcpy(&status, s->status + 5, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess))
    rc = fail(RT_E_HIP, "radiance read-back failed: %s", hipGetErrorString(hipGetLastError()));
  (void)hipFree(mem);
  if (!rc && status) return fail(RT_E_STACK, "BVH traversal stack overflow");
  return rc;
}

// the checks of rt_denoise_film / _read that need no device; p: the parameters in effect
int denoise_check(const rt_film* f, const rt_denoise_params* p) {
  if (!rt_dn_params_ok(p))
    return fail(RT_E_INVALID, "denoise parameters: levels 1..8 (%d), k 0..16 (%d), sigma and eps positive", p->levels, p->k);
  if (f->ex.n_shards > 1)
    return fail(RT_E_UNSUPPORTED, "a film of %d shards holds interleaved rows: the filter needs a pixel's neighbours",
                f->ex.n_shards);
  if (f->nonuniform)
    return fail(RT_E_UNSUPPORTED,
                "the film is non-uniform (adaptive passes): the filter's variance uses one sample and pass count for every "
                "pixel; denoise a uniform film, or rt_film_reset this one");
  if (f->passes < 2) return fail(RT_E_INVALID, "the denoiser's variance needs two passes (the film has %d)", f->passes);
  if (f->feat_samples <= 0) return fail(RT_E_INVALID, "the film's features have not been computed (rt_denoise_features)");
  return RT_OK;
}

// prepare, one launch per level over the two ev buffers, finish
int film_denoise(rt_film* f, const rt_denoise_params* p, void* d_out, hipStream_t st) {
  HIP_TRY(hipSetDevice(f->scene->device));
  const size_t n = f->n_pixels;
  if (!f->dn_mem)
    HIP_TRY(hipMalloc((void**)&f->dn_mem, (2 * RT_DN_EV_PLANES + RT_DN_GUIDE_PLANES) * n * sizeof(double)));
  double* ev[2] = {f->dn_mem, f->dn_mem + RT_DN_EV_PLANES * n};
  double* guide = f->dn_mem + 2 * RT_DN_EV_PLANES * n;
  int rc = rt_denoise_launch_prepare(f->total, f->q, (const long long*)f->feat, ev[0], guide, (long long)n, f->acc_words,
                                     f->samples, f->passes, f->feat_samples,
                                     f->albedo_samples > 0 ? (const long long*)f->feat2 : nullptr, f->albedo_samples, st);
  int cur = 0;
  for (int i = 0; i < p->levels && !rc; ++i, cur ^= 1)
    rc = rt_denoise_launch_level(ev[cur], ev[cur ^ 1], guide, f->flags, p, f->width, f->height, 1 << i, st);
  if (!rc) rc = rt_denoise_launch_finish(ev[cur], guide, f->flags, d_out, f->f32, (long long)n, st);
  if (rc) return fail(RT_E_HIP, "denoise launch failed: %s", hipGetErrorString(hipGetLastError()));
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

// ---- progressive film

int rt_film_create(const rt_device_scene* s, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex,
                   rt_film** out) {
  if (!s || !cs || !ex || !out) return fail(RT_E_INVALID, "null argument");
  *out = nullptr;
  if (ex->n_devices != 0) return fail(RT_E_INVALID, "a film lives on the scene's device (n_devices = 0)");
  if (cs->n_redirect_targets < 0 || cs->n_redirect_targets > RT_MAX_TARGETS || (cs->n_redirect_targets && !cs->redirect_targets))
    return fail(cs->n_redirect_targets > RT_MAX_TARGETS ? RT_E_UNSUPPORTED : RT_E_INVALID, "invalid redirect targets (%d)",
                cs->n_redirect_targets);
  // (the camera's samples_per_pixel is checked too; it is not read afterwards)
  if (int rc = validate_frame(cs, seed, ex)) return rc;
  if (exec_encoding(ex) >= 0) return fail(RT_E_INVALID, "a film resolves to linear RGB (use rt_encode8_async)");
  const int h = rt_host_image_height(cs);
  std::unique_ptr<rt_film, void (*)(rt_film*)> f(new rt_film(), film_destroy);
  f->scene = s;
  f->cs = *cs;
  f->targets.assign(cs->redirect_targets, cs->redirect_targets + cs->n_redirect_targets);
  f->cs.redirect_targets = f->targets.empty() ? nullptr : f->targets.data();
  f->seed = seed;
  f->ex = *ex;
  f->ex.flags |= RT_EXEC_SOLO;  // a pass is followed by its merge on the same stream: it runs alone
  f->ex.devices = nullptr;
  f->f32 = exec_f32(ex);
  f->width = cs->image_width;
  f->height = h;
  f->rows = rt_host_shard_rows(h, ex);
  f->acc_words = acc_words_of(f->f32);
  f->n_pixels = (size_t)f->rows * f->width;
  if (int rc = ensure_precisions(s, prec_bit(f->f32))) return rc;
  auto pad = [](size_t b) { return (b + 16 + 255) & ~(size_t)255; };  // >= 16 bytes of slack, 256-byte parts
  f->total_bytes = pad(film_sums_bytes(f.get()));
  f->flag_bytes = pad(f->n_pixels * sizeof(unsigned));
  f->q_bytes = pad(f->n_pixels * sizeof(double));
  f->state_span = f->total_bytes + f->flag_bytes + f->q_bytes;
  f->ws_lay = workspace_layout(f->n_pixels, f->acc_words);
  const size_t tile_bytes = pad(f->n_pixels * 3 * elem_size_of(f->f32));
  const size_t blocks = (size_t)rt_film_blocks((long long)f->n_pixels);
  const size_t part_bytes = pad(blocks * sizeof(double)) + pad(blocks * sizeof(int));
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipMalloc((void**)&f->mem, f->state_span + f->ws_lay.bytes + tile_bytes + part_bytes));
  char* p = f->mem;
  f->total = (unsigned long long*)p, p += f->total_bytes;
  f->flags = (unsigned int*)p, p += f->flag_bytes;
  f->q = (double*)p, p += f->q_bytes;
  f->ws = p, p += f->ws_lay.bytes;
  f->tile = p, p += tile_bytes;
  f->partial_sum = (double*)p, p += pad(blocks * sizeof(double));
  f->partial_cnt = (int*)p;
  HIP_TRY(hipMemset(f->mem, 0, f->state_span));
  *out = f.release();
  return RT_OK;
}

int rt_film_destroy(rt_film* f) {
  if (f)
    if (int rc = refuse_owned(f, "rt_film_destroy")) return rc;
  film_destroy(f);
  return RT_OK;
}

namespace {
int film_reset(rt_film* f) {
  std::lock_guard<std::mutex> lock(f->mu);
  HIP_TRY(hipSetDevice(f->scene->device));
  HIP_TRY(hipMemsetAsync(f->mem, 0, f->state_span, f->last));
  HIP_TRY(hipStreamSynchronize(f->last));
  f->samples = 0;
  f->passes = 0;
  f->nonuniform = false;  // the count plane is dropped (its allocation is kept for the next adaptive pass)
  f->ad_listed = false;
  f->adaptive_passes = 0;
  return RT_OK;
}
}  // namespace

int rt_film_reset(rt_film* f) {
  if (!f) return fail(RT_E_INVALID, "null argument");
  if (int rc = refuse_owned(f, "rt_film_reset")) return rc;
  return film_reset(f);
}

int rt_film_add(rt_film* f, int32_t n_samples, void* hip_stream) {
  if (!f) return fail(RT_E_INVALID, "null argument");
  if (int rc = refuse_owned(f, "rt_film_add")) return rc;
  if (n_samples <= 0) return fail(RT_E_INVALID, "a pass adds at least one sample (%d)", n_samples);
  std::lock_guard<std::mutex> lock(f->mu);
  if (f->nonuniform)
    return fail(RT_E_INVALID,
                "rt_film_add: the film is non-uniform (adaptive passes); rt_adaptive_add with a negative threshold adds "
                "%d samples to every pixel",
                n_samples);
  if (f->samples + n_samples > RT_FILM_MAX_SAMPLES)
    return fail(RT_E_INVALID, "a film holds at most 2^24 samples per pixel (%lld + %d)", (long long)f->samples, n_samples);
  rt_camera_settings cs = f->cs;
  cs.samples_per_pixel = n_samples;
  RenderCall c;  // samples [N, N + n) summed into the film's workspace, no mean
  c.ws = f->ws, c.ws_cap = f->ws_lay.bytes;
  c.lone = true;
  c.sample0 = (int)f->samples;
  c.resolve = false;
  if (int rc = render_any(f->scene, &cs, f->seed, &f->ex, f->f32, c, hip_stream)) return rc;
  f->last = (hipStream_t)hip_stream;
  if (rt_film_launch_merge(f->total, f->flags, f->q, (const unsigned long long*)f->ws,
                           (const unsigned int*)(f->ws + f->ws_lay.off_flag), (long long)f->n_pixels, f->acc_words, n_samples,
                           hip_stream))
    return fail(RT_E_HIP, "merge launch failed: %s", hipGetErrorString(hipGetLastError()));
  f->samples += n_samples;
  f->passes += 1;
  return RT_OK;
}

int rt_film_resolve(const rt_film* f, void* d_out_rgb, void* hip_stream) {
  if (!f || !d_out_rgb) return fail(RT_E_INVALID, "null argument");
  if (!f->owned) return film_resolve_any(f, d_out_rgb, (hipStream_t)hip_stream);  // (ordered by the caller)
  // A multi-device film's frame: the caller has no stream to order this read against the merges
  // with.  The stream first waits for the frame's last stream (which has waited for the merges) and
  // becomes the last itself, so the next pass's merges wait for this read (multi_film_pass)
  rt_film* g = const_cast<rt_film*>(f);
  std::lock_guard<std::mutex> lock(g->mu);
  HIP_TRY(hipSetDevice(g->scene->device));
  if (int rc = film_follow(g, (hipStream_t)hip_stream)) return rc;
  if (int rc = film_resolve_any(g, d_out_rgb, (hipStream_t)hip_stream)) return rc;
  g->last = (hipStream_t)hip_stream;
  return RT_OK;
}

int rt_film_read(const rt_film* f, void* host_out_rgb) {
  if (!f || !host_out_rgb) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(const_cast<rt_film*>(f)->mu);  // (the tile is the film's scratch)
  if (int rc = film_resolve_any(f, f->tile, f->last)) return rc;
  const size_t bytes = f->n_pixels * 3 * elem_size_of(f->f32);
  int status = 0;
  HIP_TRY(hipMemcpyAsync(host_out_rgb, f->tile, bytes, hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipMemcpyAsync(&status, f->scene->status, sizeof(int), hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipStreamSynchronize(f->last));
  if (status) return fail(RT_E_STACK, "BVH traversal stack overflow");
  return RT_OK;
}

int rt_film_noise(const rt_film* f, float* d_map_or_null, double* noise) {
  if (!f || !noise) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(const_cast<rt_film*>(f)->mu);  // (the partials are the film's scratch)
  if (f->passes < 2) return fail(RT_E_INVALID, "a noise estimate needs two passes (the film has %d)", f->passes);
  HIP_TRY(hipSetDevice(f->scene->device));
  if (f->nonuniform ? rt_adaptive_launch_noise(f->total, f->flags, f->q, f->counts, d_map_or_null, f->partial_sum,
                                               f->partial_cnt, (long long)f->n_pixels, f->acc_words, f->width, f->height,
                                               f->ex.n_shards, f->ex.shard, f->ex.row_block, f->last)
                    : rt_film_launch_noise(f->total, f->flags, f->q, d_map_or_null, f->partial_sum, f->partial_cnt,
                                           (long long)f->n_pixels, f->acc_words, f->samples, f->passes, f->width, f->height,
                                           f->ex.n_shards, f->ex.shard, f->ex.row_block, f->last))
    return fail(RT_E_HIP, "noise launch failed: %s", hipGetErrorString(hipGetLastError()));
  const size_t blocks = (size_t)rt_film_blocks((long long)f->n_pixels);
  std::vector<double> ps(blocks);
  std::vector<int> pc(blocks);
  HIP_TRY(hipMemcpyAsync(ps.data(), f->partial_sum, blocks * sizeof(double), hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipMemcpyAsync(pc.data(), f->partial_cnt, blocks * sizeof(int), hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipStreamSynchronize(f->last));
  double sum = 0.0;  // the workgroups' partials in index order: the same figure on every run
  long long cnt = 0;
  for (size_t b = 0; b < blocks; ++b) sum += ps[b], cnt += pc[b];
  *noise = cnt > 0 ? std::sqrt(sum / (double)cnt) : std::nan("");
  return RT_OK;
}

int rt_film_get_info(const rt_film* f, rt_film_info* info) {
  if (!f || !info) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(const_cast<rt_film*>(f)->mu);
  std::vector<unsigned> flags(f->n_pixels);
  HIP_TRY(hipSetDevice(f->scene->device));
  HIP_TRY(hipMemcpyAsync(flags.data(), f->flags, f->n_pixels * sizeof(unsigned), hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipStreamSynchronize(f->last));
  info->samples = f->samples;
  info->passes = f->passes;
  if (f->nonuniform) {  // the largest N_p and K_p
    CountStats cst;
    if (int rc = adaptive_stats(f, cst)) return rc;
    info->samples = cst.max_n;
    info->passes = (int32_t)cst.max_k;
  }
  info->width = f->width;
  info->rows = f->rows;
  info->nan_pixels = (int32_t)std::count_if(flags.begin(), flags.end(), [](unsigned v) { return v != 0u; });
  info->f32 = f->f32;
  return RT_OK;
}

int rt_film_state_bytes(const rt_film* f, int64_t* bytes) {
  if (!f || !bytes) return fail(RT_E_INVALID, "null argument");
  *bytes = film_state_bytes(f);
  return RT_OK;
}

int rt_film_save(const rt_film* f, void* host_buf, int64_t cap) {
  if (!f || !host_buf) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(const_cast<rt_film*>(f)->mu);
  if (cap < film_state_bytes(f))
    return fail(RT_E_INVALID, "the film's state takes %lld bytes (buffer: %lld)", (long long)film_state_bytes(f), (long long)cap);
  FilmHeader h = film_header(f);
  char* p = (char*)host_buf;
  if (f->nonuniform) {  // layout version 2: the count plane behind the version-1 bytes, the maxima in the header
    CountStats cst;
    std::vector<uint32_t> counts;
    if (int rc = adaptive_stats(f, cst, &counts)) return rc;
    h.version = kFilmVersionCounts;
    h.samples = cst.max_n;
    h.passes = (int32_t)cst.max_k;
    std::memcpy(p + film_state_bytes_v1(f), counts.data(), film_counts_bytes(f));
  }
  std::memcpy(p, &h, sizeof h), p += sizeof h;
  HIP_TRY(hipSetDevice(f->scene->device));
  HIP_TRY(hipMemcpyAsync(p, f->total, film_sums_bytes(f), hipMemcpyDeviceToHost, f->last));
  p += film_sums_bytes(f);
  HIP_TRY(hipMemcpyAsync(p, f->flags, f->n_pixels * sizeof(unsigned), hipMemcpyDeviceToHost, f->last));
  p += f->n_pixels * sizeof(unsigned);
  HIP_TRY(hipMemcpyAsync(p, f->q, f->n_pixels * sizeof(double), hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipStreamSynchronize(f->last));
  return RT_OK;
}

namespace {
// counts_ok: a version-2 state (a non-uniform film's) is accepted and makes the film non-uniform
int film_load(rt_film* f, const void* host_buf, int64_t bytes, bool counts_ok) {
  std::lock_guard<std::mutex> lock(f->mu);
  if (bytes < (int64_t)sizeof(FilmHeader)) return fail(RT_E_INVALID, "not a saved film (%lld bytes)", (long long)bytes);
  FilmHeader h;
  std::memcpy(&h, host_buf, sizeof h);
  if (h.magic != kFilmMagic || (h.version != kFilmVersion && h.version != kFilmVersionCounts))
    return fail(RT_E_INVALID, "not a saved film of layout version %u or %u", kFilmVersion, kFilmVersionCounts);
  const bool v2 = h.version == kFilmVersionCounts;
  if (v2 && !counts_ok)
    return fail(RT_E_INVALID,
                "the saved film is non-uniform (layout version 2, adaptive passes): a multi-device film has no adaptive "
                "passes; load it into a one-device rt_film");
  const FilmHeader w = film_header(f);
  if (h.f32 != w.f32 || h.width != w.width || h.height != w.height || h.rows != w.rows || h.n_shards != w.n_shards ||
      h.shard != w.shard || h.row_block != w.row_block || h.key0 != w.key0 || h.key1 != w.key1)
    return fail(RT_E_INVALID,
                "the saved film (%s, %dx%d, shard %d of %d by %d rows, key %08x%08x) does not match this film (%s, "
                "%dx%d, shard %d of %d by %d rows, key %08x%08x)",
                h.f32 ? "f32" : "f64", h.width, h.height, h.shard, h.n_shards, h.row_block, h.key1, h.key0,
                w.f32 ? "f32" : "f64", w.width, w.height, w.shard, w.n_shards, w.row_block, w.key1, w.key0);
  const int64_t want = film_state_bytes_v1(f) + (v2 ? (int64_t)film_counts_bytes(f) : 0);
  if (bytes != want || h.samples < 0 || h.samples > RT_FILM_MAX_SAMPLES || h.passes < 0 || h.passes > h.samples)
    return fail(RT_E_INVALID, "the saved film is damaged (%lld bytes, %lld samples, %d passes)", (long long)bytes,
                (long long)h.samples, h.passes);
  const char* p = (const char*)host_buf + sizeof h;
  HIP_TRY(hipSetDevice(f->scene->device));
  if (v2) {  // the count plane: every pixel within the header's maxima, a padding row empty
    std::vector<uint32_t> c(2 * f->n_pixels);
    std::memcpy(c.data(), (const char*)host_buf + film_state_bytes_v1(f), film_counts_bytes(f));
    for (size_t i = 0; i < f->n_pixels; ++i) {
      const bool in = rt_adaptive_inside((long long)i, f->width, f->height, f->ex.n_shards, f->ex.shard, f->ex.row_block);
      const uint32_t N = c[2 * i], K = c[2 * i + 1];
      if (in ? (K < 2 || K > N || (int64_t)N > h.samples || (int64_t)K > h.passes) : (N != 0 || K != 0))
        return fail(RT_E_INVALID, "the saved film's count plane is damaged (tile pixel %zu: %u samples, %u passes)", i, N, K);
    }
    if (int rc = adaptive_alloc(f)) return rc;
    HIP_TRY(hipMemcpyAsync(f->counts, c.data(), film_counts_bytes(f), hipMemcpyHostToDevice, f->last));
    HIP_TRY(hipStreamSynchronize(f->last));  // (c is this call's)
  }
  f->nonuniform = v2;
  f->ad_listed = false;
  f->adaptive_passes = 0;
  HIP_TRY(hipMemcpyAsync(f->total, p, film_sums_bytes(f), hipMemcpyHostToDevice, f->last));
  p += film_sums_bytes(f);
  HIP_TRY(hipMemcpyAsync(f->flags, p, f->n_pixels * sizeof(unsigned), hipMemcpyHostToDevice, f->last));
  p += f->n_pixels * sizeof(unsigned);
  HIP_TRY(hipMemcpyAsync(f->q, p, f->n_pixels * sizeof(double), hipMemcpyHostToDevice, f->last));
  HIP_TRY(hipStreamSynchronize(f->last));
  f->samples = h.samples;
  f->passes = h.passes;
  return RT_OK;
}
}  // namespace

int rt_film_load(rt_film* f, const void* host_buf, int64_t bytes) {
  if (!f || !host_buf) return fail(RT_E_INVALID, "null argument");
  if (int rc = refuse_owned(f, "rt_film_load")) return rc;
  return film_load(f, host_buf, bytes, true);
}

// ---- adaptive film passes

int rt_adaptive_add(rt_film* f, int32_t n_samples, double threshold, int32_t max_samples, void* hip_stream) {
  if (!f) return fail(RT_E_INVALID, "null argument");
  if (n_samples <= 0) return fail(RT_E_INVALID, "a pass adds at least one sample (%d)", n_samples);
  if (threshold != threshold) return fail(RT_E_INVALID, "the threshold is NaN");
  if (max_samples < 0 || max_samples > RT_FILM_MAX_SAMPLES)
    return fail(RT_E_INVALID, "max_samples: 0 (2^24, the film's limit) to 2^24 (%d)", max_samples);
  if (int rc = refuse_owned(f, "rt_adaptive_add")) return rc;
  std::lock_guard<std::mutex> lock(f->mu);
  if (f->passes < 2)
    return fail(RT_E_INVALID, "an adaptive pass selects by the noise estimate, which needs two passes (the film has %d)",
                f->passes);
  // (the list kernel's item ids stay below 2^31: rt_list_kernel.h)
  if ((long long)f->n_pixels * n_samples > 0x7fffffffLL - (1 << 20))
    return fail(RT_E_INVALID, "an adaptive pass of %d samples over %zu pixels is too large (pixels x samples < 2^31)",
                n_samples, f->n_pixels);
  const long long cap = max_samples ? max_samples : RT_FILM_MAX_SAMPLES;
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(hipSetDevice(f->scene->device));
  if (int rc = adaptive_alloc(f)) return rc;  // (the first call only)
  if (!f->nonuniform) {
    if (rt_adaptive_launch_init(f->counts, (long long)f->n_pixels, (uint32_t)f->samples, (uint32_t)f->passes, f->width,
                                f->height, f->ex.n_shards, f->ex.shard, f->ex.row_block, st))
      return fail(RT_E_HIP, "count plane launch failed: %s", hipGetErrorString(hipGetLastError()));
    f->nonuniform = true;
  }
  f->last = st;
  f->ad_listed = false;
  if (int rc = f->f32 ? adaptive_pass<float>(f, n_samples, threshold, cap, st)
                      : adaptive_pass<double>(f, n_samples, threshold, cap, st))
    return rc;
  f->ad_listed = true;
  f->adaptive_passes += 1;
  return RT_OK;
}

int rt_adaptive_get_info(const rt_film* f, rt_adaptive_info* info) {
  if (!f || !info) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(const_cast<rt_film*>(f)->mu);
  std::memset(info, 0, sizeof *info);
  info->nonuniform = f->nonuniform;
  info->adaptive_passes = f->adaptive_passes;
  HIP_TRY(hipSetDevice(f->scene->device));
  if (f->nonuniform) {
    CountStats cst;
    if (int rc = adaptive_stats(f, cst)) return rc;
    info->total_samples = cst.total;
    info->min_samples = (int32_t)cst.min_n;
    info->max_samples = (int32_t)cst.max_n;
  } else {  // every pixel that counts holds the film's N
    std::vector<unsigned> flags(f->n_pixels);
    HIP_TRY(hipMemcpyAsync(flags.data(), f->flags, f->n_pixels * sizeof(unsigned), hipMemcpyDeviceToHost, f->last));
    HIP_TRY(hipStreamSynchronize(f->last));
    int64_t counting = 0;
    for (size_t p = 0; p < f->n_pixels; ++p)
      counting += !flags[p] &&
                  rt_adaptive_inside((long long)p, f->width, f->height, f->ex.n_shards, f->ex.shard, f->ex.row_block);
    info->total_samples = counting * f->samples;
    info->min_samples = info->max_samples = (int32_t)f->samples;
  }
  if (f->ad_listed) {
    int n = 0;
    HIP_TRY(hipMemcpyAsync(&n, f->ad_n, sizeof n, hipMemcpyDeviceToHost, f->last));
    HIP_TRY(hipStreamSynchronize(f->last));
    info->selected = n;
  }
  return RT_OK;
}

int rt_adaptive_counts_read(const rt_film* f, uint32_t* host) {
  if (!f || !host) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(const_cast<rt_film*>(f)->mu);
  HIP_TRY(hipSetDevice(f->scene->device));
  if (f->nonuniform) {
    HIP_TRY(hipMemcpyAsync(host, f->counts, film_counts_bytes(f), hipMemcpyDeviceToHost, f->last));
    HIP_TRY(hipStreamSynchronize(f->last));
    return RT_OK;
  }
  // a uniform film: (N, K) inside the frame, (0, 0) on a shard's padding rows — what the plane would start as
  for (size_t p = 0; p < f->n_pixels; ++p) {
    const bool in = rt_adaptive_inside((long long)p, f->width, f->height, f->ex.n_shards, f->ex.shard, f->ex.row_block);
    host[2 * p] = in ? (uint32_t)f->samples : 0u;
    host[2 * p + 1] = in ? (uint32_t)f->passes : 0u;
  }
  return RT_OK;
}

int rt_adaptive_selection_read(const rt_film* f, int32_t* host_tile_pixels, int64_t cap, int64_t* n) {
  if (!f || !n || cap < 0 || (cap > 0 && !host_tile_pixels)) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(const_cast<rt_film*>(f)->mu);
  *n = 0;
  if (!f->ad_listed) return RT_OK;  // no adaptive pass since create / reset / load
  HIP_TRY(hipSetDevice(f->scene->device));
  int count = 0;
  HIP_TRY(hipMemcpyAsync(&count, f->ad_n, sizeof count, hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipStreamSynchronize(f->last));
  if (count < 0 || (size_t)count > f->n_pixels) return fail(RT_E_GENERIC, "the selection's length word is damaged (%d)", count);
  *n = count;
  const size_t take = (size_t)std::min<int64_t>(cap, count);
  if (!take) return RT_OK;
  std::vector<rt_adaptive_rec> recs(take);
  HIP_TRY(hipMemcpyAsync(recs.data(), f->ad_list, take * sizeof(rt_adaptive_rec), hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipStreamSynchronize(f->last));
  for (size_t i = 0; i < take; ++i) host_tile_pixels[i] = recs[i].tp;
  return RT_OK;
}

// ---- multi-device film

namespace {

void multi_film_destroy(rt_multi_film* F) {
  if (!F) return;
  const int dev0 = F->scene->devices[0];
  for (FilmPart& p : F->parts)
    if (p.st && hipSetDevice(p.device) == hipSuccess) (void)hipStreamSynchronize(p.st);
  (void)hipSetDevice(dev0);
  for (FilmPart& p : F->parts)
    if (p.st_merge) (void)hipStreamSynchronize(p.st_merge);
  if (F->st_frame) (void)hipStreamSynchronize(F->st_frame);
  if (F->frame && F->frame->e_order) (void)hipEventDestroy(F->frame->e_order);
  film_destroy(F->frame);  // (waits for its last stream, which may be st_frame: before that goes)
  for (FilmPart& p : F->parts) {
    (void)hipSetDevice(p.device);
    if (p.direct && p.e_merge) (void)hipEventDestroy(p.e_merge);
    if (p.e_copy) (void)hipEventDestroy(p.e_copy);
    if (p.st) (void)hipStreamDestroy(p.st);
    if (p.own_ws) (void)hipFree(p.ws);
    (void)hipSetDevice(dev0);
    if (!p.direct && p.e_merge) (void)hipEventDestroy(p.e_merge);
    if (p.st_merge) (void)hipStreamDestroy(p.st_merge);
    (void)hipFree(p.stage);
  }
  if (F->e_frame) (void)hipEventDestroy(F->e_frame);
  if (F->st_frame && !F->single) (void)hipStreamDestroy(F->st_frame);
  delete F;
}

// everything enqueued on every part, on the first device's merge streams and on the frame is done
int multi_film_wait(rt_multi_film* F) {
  for (FilmPart& p : F->parts) {
    HIP_TRY(hipSetDevice(p.device));
    HIP_TRY(hipStreamSynchronize(p.st));
  }
  HIP_TRY(hipSetDevice(F->scene->devices[0]));
  for (FilmPart& p : F->parts)
    if (p.st_merge) HIP_TRY(hipStreamSynchronize(p.st_merge));
  HIP_TRY(hipStreamSynchronize(F->st_frame));
  std::lock_guard<std::mutex> lock(F->frame->mu);
  if (F->frame->last != F->st_frame) HIP_TRY(hipStreamSynchronize(F->frame->last));
  return RT_OK;
}

// One pass: shard k's samples [N, N + n) on devices[k] and their merge into the frame's rows, every
// shard enqueued without waiting for another.  Ordered by events alone: a merge follows its render
// (stream order; on the copy path the first device's merge stream waits for the copy) and what
// was enqueued on the frame before this pass (e_frame); the frame's stream waits for every merge;
// the part's next pass (its workspace memset first) waits for its merge.
int multi_film_pass(rt_multi_film* F, int n_samples) {
  rt_film* fr = F->frame;
  const int dev0 = F->scene->devices[0];
  rt_camera_settings cs = fr->cs;
  cs.samples_per_pixel = n_samples;
  // (st_frame itself carries only waits and the work of synchronous calls, which has finished:
  // there is something to wait for only after a call that put a stream of the caller's in its place)
  const bool after_frame = fr->last != F->st_frame;
  if (after_frame) {
    HIP_TRY(hipSetDevice(dev0));
    HIP_TRY(hipEventRecord(F->e_frame, fr->last));
  }
  for (FilmPart& p : F->parts) {
    if (!p.active) continue;
    HIP_TRY(hipSetDevice(p.device));
    if (!p.direct) HIP_TRY(hipStreamWaitEvent(p.st, p.e_merge, 0));  // (a direct merge ran on p.st itself)
    RenderCall c;  // as rt_film_add's: the sums stay in the workspace
    c.ws = p.ws, c.ws_cap = p.ws_lay.bytes;
    c.lone = true;
    c.sample0 = (int)fr->samples;
    c.resolve = false;
    if (int rc = render_any(p.scene, &cs, fr->seed, &p.ex, fr->f32, c, p.st)) return rc;
    const char* src = p.ws;
    hipStream_t ms = p.st;
    if (!p.direct) {
      HIP_TRY(hipMemcpyPeerAsync(p.stage, dev0, p.ws, p.device, p.ws_lay.off_ctr, p.st));  // sums and flags
      HIP_TRY(hipEventRecord(p.e_copy, p.st));
      ++F->copies;
      HIP_TRY(hipSetDevice(dev0));
      HIP_TRY(hipStreamWaitEvent(p.st_merge, p.e_copy, 0));
      src = p.stage, ms = p.st_merge;
    }
    if (after_frame) HIP_TRY(hipStreamWaitEvent(ms, F->e_frame, 0));
    if (rt_film_launch_merge_rows(fr->total, fr->flags, fr->q, (const unsigned long long*)src,
                                  (const unsigned int*)(src + p.ws_lay.off_flag), fr->width, fr->height, p.tile_rows,
                                  p.ex.n_shards, p.ex.shard, p.ex.row_block, fr->acc_words, n_samples, ms))
      return fail(RT_E_HIP, "merge launch failed: %s", hipGetErrorString(hipGetLastError()));
    if (!F->single) HIP_TRY(hipEventRecord(p.e_merge, ms));
  }
  if (!F->single) {
    HIP_TRY(hipSetDevice(dev0));
    for (FilmPart& p : F->parts)
      if (p.active) HIP_TRY(hipStreamWaitEvent(F->st_frame, p.e_merge, 0));
  }
  fr->last = F->st_frame;
  return RT_OK;
}

}  // namespace

int rt_multi_film_create(const rt_multi_scene* m, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex,
                         rt_multi_film** out) {
  if (!m || !cs || !ex || !out) return fail(RT_E_INVALID, "null argument");
  *out = nullptr;
  if (ex->n_devices != 0) return fail(RT_E_INVALID, "a multi-device film renders on the scene's devices (n_devices = 0)");
  if (ex->n_shards != 1) return fail(RT_E_INVALID, "a multi-device film holds the whole image (n_shards must be 1)");
  const int n = (int)m->devices.size(), dev0 = m->devices[0];
  std::unique_ptr<rt_multi_film, void (*)(rt_multi_film*)> F(new rt_multi_film(), multi_film_destroy);
  F->scene = m;
  // the frame: an ordinary one-shard film of the whole image on the first device (its checks are
  // this call's: camera, flags, no 8-bit encoding)
  rt_exec e1 = *ex;
  e1.device = dev0;
  if (int rc = rt_film_create(m->scenes[0], cs, seed, &e1, &F->frame)) return rc;
  rt_film* fr = F->frame;
  fr->owned = true;
  HIP_TRY(hipSetDevice(dev0));
  HIP_TRY(hipDeviceSynchronize());  // (the frame's zeroing: the streams below do not wait for the null stream)
  HIP_TRY(hipStreamCreateWithFlags(&F->st_frame, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&F->e_frame, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&fr->e_order, hipEventDisableTiming));
  fr->last = F->st_frame;
  // RT_AMD_COPY_SHARDS (experiments and tests, as rt_multi_render's): bit k puts shard k on the path
  // a device without peer access takes, so one GPU exercises it
  unsigned long long copy_mask = 0;
  if (const char* e = rt_knob("RT_AMD_COPY_SHARDS")) copy_mask = (unsigned long long)strtoll(e, nullptr, 0);
  F->parts.resize(n);
  for (int k = 0; k < n; ++k) {
    FilmPart& p = F->parts[k];
    p.device = m->devices[k];
    p.scene = m->scenes[m->scene_of[k]];
    p.ex = fr->ex;  // (planned to run alone, like a film's pass)
    p.ex.device = p.device;
    if (n > 1) p.ex.n_shards = n, p.ex.shard = k;
    p.tile_rows = rt_host_shard_rows(fr->height, &p.ex);
    p.active = rt_film_block_span(0, fr->width, fr->height, p.ex.n_shards, p.ex.shard, p.ex.row_block).n_pixels > 0;
    p.direct = m->peer_ok[m->scene_of[k]] && !((copy_mask >> k) & 1ull);
    p.ws_lay = workspace_layout((size_t)p.tile_rows * fr->width, fr->acc_words);
    if (int rc = ensure_precisions(p.scene, prec_bit(fr->f32))) return rc;
    HIP_TRY(hipSetDevice(p.device));
    HIP_TRY(hipStreamCreateWithFlags(&p.st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&p.e_copy, hipEventDisableTiming));
    if (k == 0 && p.ws_lay.bytes <= fr->ws_lay.bytes) {
      p.ws = fr->ws;  // the frame film never adds a pass of its own: its workspace is shard 0's
    } else {
      HIP_TRY(hipMalloc((void**)&p.ws, p.ws_lay.bytes));
      p.own_ws = true;
    }
    if (!p.direct) {
      HIP_TRY(hipSetDevice(dev0));
      HIP_TRY(hipMalloc((void**)&p.stage, p.ws_lay.off_ctr));
      HIP_TRY(hipStreamCreateWithFlags(&p.st_merge, hipStreamNonBlocking));
    }
    HIP_TRY(hipEventCreateWithFlags(&p.e_merge, hipEventDisableTiming));  // on the device that merges
  }
  if (n == 1 && F->parts[0].direct) {
    // a list of one device: render and merge follow one another on one stream, as a plain film's
    // pass does; that stream is the frame's, and a pass records and waits for no event
    HIP_TRY(hipSetDevice(dev0));
    HIP_TRY(hipStreamDestroy(F->st_frame));
    F->st_frame = fr->last = F->parts[0].st;
    F->single = true;
  }
  *out = F.release();
  return RT_OK;
}

int rt_multi_film_destroy(rt_multi_film* f) {
  multi_film_destroy(f);
  return RT_OK;
}

int rt_multi_film_reset(rt_multi_film* f) {
  if (!f) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(f->mu);
  if (int rc = multi_film_wait(f)) return rc;
  return film_reset(f->frame);
}

int rt_multi_film_add(rt_multi_film* f, int32_t n_samples) {
  if (!f) return fail(RT_E_INVALID, "null argument");
  if (n_samples <= 0) return fail(RT_E_INVALID, "a pass adds at least one sample (%d)", n_samples);
  std::lock_guard<std::mutex> lock(f->mu);
  rt_film* fr = f->frame;
  std::lock_guard<std::mutex> frame_lock(fr->mu);
  if (fr->samples + n_samples > RT_FILM_MAX_SAMPLES)
    return fail(RT_E_INVALID, "a film holds at most 2^24 samples per pixel (%lld + %d)", (long long)fr->samples, n_samples);
  if (int rc = multi_film_pass(f, n_samples)) return rc;
  fr->samples += n_samples;
  fr->passes += 1;
  return RT_OK;
}

int rt_multi_film_load(rt_multi_film* f, const void* host_buf, int64_t bytes) {
  if (!f || !host_buf) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(f->mu);
  if (int rc = multi_film_wait(f)) return rc;
  return film_load(f->frame, host_buf, bytes, false);
}

int rt_multi_film_frame(rt_multi_film* f, rt_film** frame) {
  if (!f || !frame) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(f->mu);
  *frame = f->frame;
  if (int rc = multi_film_wait(f)) return rc;
  int status = 0;
  for (const rt_device_scene* s : f->scene->scenes) {
    int ps = 0;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(&ps, s->status, sizeof(int), hipMemcpyDeviceToHost));
    status |= ps;
  }
  if (status) return fail(RT_E_STACK, "BVH traversal stack overflow");
  return RT_OK;
}

int rt_multi_film_copies(const rt_multi_film* f, int64_t* n) {
  if (!f || !n) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(const_cast<rt_multi_film*>(f)->mu);
  *n = f->copies;
  return RT_OK;
}

// ---- first-hit features and the denoiser

int rt_denoise_default_params(rt_denoise_params* p) {
  if (!p) return fail(RT_E_INVALID, "null argument");
  rt_dn_defaults(p);
  return RT_OK;
}

int rt_denoise_features(rt_film* f, int32_t n_feat, void* hip_stream) {
  if (!f) return fail(RT_E_INVALID, "null argument");
  if (n_feat < 1 || n_feat > 4096) return fail(RT_E_INVALID, "1 to 4096 feature samples per pixel (%d)", n_feat);
  std::lock_guard<std::mutex> lock(f->mu);
  HIP_TRY(hipSetDevice(f->scene->device));
  if (!f->feat) HIP_TRY(hipMalloc((void**)&f->feat, f->n_pixels * rt_feat_words(!f->f32) * sizeof(long long)));
  f->feat_samples = 0;
  hipStream_t st = (hipStream_t)hip_stream;
  if (int rc = film_follow(f, st)) return rc;
  if (int rc = f->f32 ? film_features<float>(f, f->feat, n_feat, st) : film_features<double>(f, f->feat, n_feat, st)) return rc;
  f->feat_samples = n_feat;
  f->last = st;
  return RT_OK;
}

int rt_denoise_albedo(rt_film* f, int32_t n_albedo, void* hip_stream) {
  if (!f) return fail(RT_E_INVALID, "null argument");
  if (n_albedo < 0 || n_albedo > 4096) return fail(RT_E_INVALID, "0 to 4096 albedo samples per pixel (%d)", n_albedo);
  std::lock_guard<std::mutex> lock(f->mu);
  if (n_albedo == 0) {  // back to multiplying by the features' own albedo
    f->albedo_samples = 0;
    return RT_OK;
  }
  HIP_TRY(hipSetDevice(f->scene->device));
  if (!f->feat2) HIP_TRY(hipMalloc((void**)&f->feat2, f->n_pixels * rt_feat_words(!f->f32) * sizeof(long long)));
  f->albedo_samples = 0;
  hipStream_t st = (hipStream_t)hip_stream;
  if (int rc = film_follow(f, st)) return rc;
  if (int rc = f->f32 ? film_features<float>(f, f->feat2, n_albedo, st) : film_features<double>(f, f->feat2, n_albedo, st))
    return rc;
  f->albedo_samples = n_albedo;
  f->last = st;
  return RT_OK;
}

namespace {
// a feature buffer's words to the host, behind the film's last stream
int features_read(const rt_film* f, const unsigned long long* words, int samples, const char* what, int64_t* host_words,
                  int32_t* n_out) {
  if (!f || !host_words || !n_out) return fail(RT_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(const_cast<rt_film*>(f)->mu);
  if (samples <= 0) return fail(RT_E_INVALID, "the film's features have not been computed (%s)", what);
  int status = 0;
  HIP_TRY(hipSetDevice(f->scene->device));
  HIP_TRY(hipMemcpyAsync(host_words, words, f->n_pixels * rt_feat_words(!f->f32) * sizeof(long long), hipMemcpyDeviceToHost,
                         f->last));
  HIP_TRY(hipMemcpyAsync(&status, f->scene->status, sizeof(int), hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipStreamSynchronize(f->last));
  *n_out = samples;
  if (status) return fail(RT_E_STACK, "BVH traversal stack overflow");
  return RT_OK;
}
}  // namespace

int rt_denoise_features_read(const rt_film* f, int64_t* host_words, int32_t* n_feat) {
  if (!f) return fail(RT_E_INVALID, "null argument");
  return features_read(f, f->feat, f->feat_samples, "rt_denoise_features", host_words, n_feat);
}

int rt_denoise_albedo_read(const rt_film* f, int64_t* host_words, int32_t* n_albedo) {
  if (!f) return fail(RT_E_INVALID, "null argument");
  return features_read(f, f->feat2, f->albedo_samples, "rt_denoise_albedo", host_words, n_albedo);
}

int rt_denoise_film(rt_film* f, const rt_denoise_params* p, void* d_out_rgb, void* hip_stream) {
  if (!f || !d_out_rgb) return fail(RT_E_INVALID, "null argument");
  rt_denoise_params dp;
  rt_dn_defaults(&dp);
  if (p) dp = *p;
  std::lock_guard<std::mutex> lock(f->mu);
  if (int rc = denoise_check(f, &dp)) return rc;
  HIP_TRY(hipSetDevice(f->scene->device));
  if (int rc = film_follow(f, (hipStream_t)hip_stream)) return rc;
  if (int rc = film_denoise(f, &dp, d_out_rgb, (hipStream_t)hip_stream)) return rc;
  f->last = (hipStream_t)hip_stream;
  return RT_OK;
}

int rt_denoise_film_read(rt_film* f, const rt_denoise_params* p, void* host_out_rgb) {
  if (!f || !host_out_rgb) return fail(RT_E_INVALID, "null argument");
  rt_denoise_params dp;
  rt_dn_defaults(&dp);
  if (p) dp = *p;
  std::lock_guard<std::mutex> lock(f->mu);  // (the tile is the film's scratch)
  if (int rc = denoise_check(f, &dp)) return rc;
  if (int rc = film_denoise(f, &dp, f->tile, f->last)) return rc;
  HIP_TRY(hipMemcpyAsync(host_out_rgb, f->tile, f->n_pixels * 3 * elem_size_of(f->f32), hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipStreamSynchronize(f->last));
  return RT_OK;
}

int rt_scene_cast_async(const rt_device_scene* s, const rt_exec* ex, const rt_ray* d_rays, rt_hit* d_hits, int64_t n,
                        int32_t flags, void* hip_stream) {
  if (int rc = cast_check(s, ex, d_rays, d_hits, n, flags)) return rc;
  if (n == 0) return RT_OK;
  return exec_f32(ex) ? cast_enqueue<float>(s, d_rays, d_hits, n, flags, 1, (hipStream_t)hip_stream)
                      : cast_enqueue<double>(s, d_rays, d_hits, n, flags, 1, (hipStream_t)hip_stream);
}

int rt_scene_cast(const rt_device_scene* s, const rt_exec* ex, const rt_ray* host_rays, rt_hit* host_hits, int64_t n,
                  int32_t flags) {
  return cast_sync(s, ex, host_rays, host_hits, n, flags, false, nullptr);
}

int rt_scene_cast_status(const rt_device_scene* s, int32_t* overflowed) {
  if (!s || !overflowed) return fail(RT_E_INVALID, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  int status = 0;
  HIP_TRY(hipMemcpy(&status, s->status + 1, sizeof(int), hipMemcpyDeviceToHost));
  if (status) HIP_TRY(hipMemset(s->status + 1, 0, sizeof(int)));
  *overflowed = status ? 1 : 0;
  return RT_OK;
}

size_t rt_scene_radiance_workspace_bytes(int64_t n, int32_t exec_flags) {
  return radiance_words_bytes(n < 0 ? 0 : n, (exec_flags & RT_EXEC_F32) != 0) + 16;
}

int rt_scene_radiance_async(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                            const rt_path_ray* d_rays, rt_radiance* d_out, void* d_workspace, int64_t n, int32_t n_samples,
                            int32_t flags, void* hip_stream) {
  if (int rc = radiance_check(s, ex, cs, d_rays, d_out, n, n_samples, flags)) return rc;
  if (!d_workspace) return fail(RT_E_INVALID, "null workspace");
  if (n == 0) return RT_OK;
  return exec_f32(ex)
             ? radiance_enqueue<float>(s, cs, seed, d_rays, d_out, d_workspace, n, n_samples, flags, 4, (hipStream_t)hip_stream)
             : radiance_enqueue<double>(s, cs, seed, d_rays, d_out, d_workspace, n, n_samples, flags, 4, (hipStream_t)hip_stream);
}

int rt_scene_radiance(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                      const rt_path_ray* host_rays, rt_radiance* host_out, void* host_workspace, int64_t n,
                      int32_t n_samples, int32_t flags) {
  return radiance_sync(s, ex, cs, seed, host_rays, host_out, host_workspace, n, n_samples, flags, false, nullptr);
}

int rt_scene_radiance_status(const rt_device_scene* s, int32_t* overflowed) {
  if (!s || !overflowed) return fail(RT_E_INVALID, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  int status = 0;
  HIP_TRY(hipMemcpy(&status, s->status + 4, sizeof(int), hipMemcpyDeviceToHost));
  if (status) HIP_TRY(hipMemset(s->status + 4, 0, sizeof(int)));
  *overflowed = status ? 1 : 0;
  return RT_OK;
}

int rt_scene_camera_rays_async(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                               int32_t sample, rt_path_ray* d_rays, void* hip_stream) {
  if (int rc = camera_rays_check(s, ex, cs, sample, d_rays)) return rc;
  return exec_f32(ex) ? camera_rays_enqueue<float>(s, cs, seed, sample, d_rays, (hipStream_t)hip_stream)
                      : camera_rays_enqueue<double>(s, cs, seed, sample, d_rays, (hipStream_t)hip_stream);
}

int rt_scene_camera_rays(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                         int32_t sample, rt_path_ray* host_rays) {
  if (int rc = camera_rays_check(s, ex, cs, sample, host_rays)) return rc;
  const int h = rt_host_image_height(cs);
  if (h <= 0 || cs->image_width <= 0) return fail(RT_E_INVALID, "bad image size");
  const size_t bytes = (size_t)h * (size_t)cs->image_width * sizeof(rt_path_ray);
  HIP_TRY(hipSetDevice(s->device));
  rt_path_ray* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, bytes));
  int rc = exec_f32(ex) ? camera_rays_enqueue<float>(s, cs, seed, sample, d, nullptr)
                        : camera_rays_enqueue<double>(s, cs, seed, sample, d, nullptr);
  if (!rc && hipMemcpy(host_rays, d, bytes, hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(RT_E_HIP, "camera-ray read-back failed: %s", hipGetErrorString(hipGetLastError()));
  (void)hipFree(d);
  return rc;
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
  const size_t ray_bytes = up256((size_t)n * order_stride(kind)), order_bytes = up256((size_t)n * sizeof(uint32_t));
  char* mem = nullptr;
  HIP_TRY(hipMalloc((void**)&mem, ray_bytes + order_bytes + rt_order_workspace_bytes((long long)n)));
  uint32_t* d_order = (uint32_t*)(mem + ray_bytes);
  int rc = RT_OK;
  if (hipMemcpy(mem, host_rays, (size_t)n * order_stride(kind), hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(RT_E_HIP, "ray upload failed: %s", hipGetErrorString(hipGetLastError()));
  if (!rc) rc = order_for_sync(nullptr, mem, n, kind, d_order, mem + ray_bytes + order_bytes);
  if (!rc && hipMemcpy(host_order, d_order, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(RT_E_HIP, "order read-back failed: %s", hipGetErrorString(hipGetLastError()));
  (void)hipFree(mem);
  return rc;
}

int rt_scene_cast_ordered_async(const rt_device_scene* s, const rt_exec* ex, const rt_ray* d_rays, rt_hit* d_hits, int64_t n,
                                int32_t flags, const uint32_t* d_order, void* hip_stream) {
  if (int rc = cast_check(s, ex, d_rays, d_hits, n, flags)) return rc;
  if (!d_order) return fail(RT_E_INVALID, "null order buffer");
  if (int rc = order_count_check(n)) return rc;
  if (n == 0) return RT_OK;
  return exec_f32(ex) ? cast_enqueue<float>(s, d_rays, d_hits, n, flags, 1, (hipStream_t)hip_stream, d_order)
                      : cast_enqueue<double>(s, d_rays, d_hits, n, flags, 1, (hipStream_t)hip_stream, d_order);
}

int rt_scene_cast_ordered(const rt_device_scene* s, const rt_exec* ex, const rt_ray* host_rays, rt_hit* host_hits, int64_t n,
                          int32_t flags, const uint32_t* host_order) {
  return cast_sync(s, ex, host_rays, host_hits, n, flags, true, host_order);
}

int rt_scene_radiance_ordered_async(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                                    const rt_path_ray* d_rays, rt_radiance* d_out, void* d_workspace, int64_t n,
                                    int32_t n_samples, int32_t flags, const uint32_t* d_order, void* hip_stream) {
  if (int rc = radiance_check(s, ex, cs, d_rays, d_out, n, n_samples, flags)) return rc;
  if (!d_workspace) return fail(RT_E_INVALID, "null workspace");
  if (!d_order) return fail(RT_E_INVALID, "null order buffer");
  if (int rc = order_count_check(n)) return rc;
  if (n == 0) return RT_OK;
  return exec_f32(ex) ? radiance_enqueue<float>(s, cs, seed, d_rays, d_out, d_workspace, n, n_samples, flags, 4,
                                                (hipStream_t)hip_stream, d_order)
                      : radiance_enqueue<double>(s, cs, seed, d_rays, d_out, d_workspace, n, n_samples, flags, 4,
                                                 (hipStream_t)hip_stream, d_order);
}

int rt_scene_radiance_ordered(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                              const rt_path_ray* host_rays, rt_radiance* host_out, void* host_workspace, int64_t n,
                              int32_t n_samples, int32_t flags, const uint32_t* host_order) {
  return radiance_sync(s, ex, cs, seed, host_rays, host_out, host_workspace, n, n_samples, flags, true, host_order);
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
