// rt_api_internal.h — what the units behind include/rt.h share: rt_api.hip (scenes and renders),
// rt_api_film.hip (the film and what lives on it) and rt_api_query.hip (ray queries and orders).
// Error reporting, the handles' struct definitions, the small inline helpers and the declarations
// of the functions one unit calls in another.  Everything but the handles (whose names include/rt.h
// declares) is in namespace rt_api, hidden from the library's exports.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rt.h"
#include "rt_adaptive.h"
#include "rt_internal.h"

namespace rt_api __attribute__((visibility("hidden"))) {

// ---- error reporting: one thread-local message for the whole library (rt_api.hip), read through
// rt_last_error (a shard's thread copies its own out that way)
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail_stack();  // RT_E_STACK, "BVH traversal stack overflow"

#define HIP_TRY(expr)                                                                                \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) return ::rt_api::fail(RT_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

inline bool exec_f32(const rt_exec* ex) { return ex && (ex->flags & RT_EXEC_F32) != 0; }
inline int acc_words_of(bool f32) { return f32 ? RT_ACC_WORDS(float) : RT_ACC_WORDS(double); }
inline size_t elem_size_of(bool f32) { return f32 ? sizeof(float) : sizeof(double); }
inline int prec_bit(bool f32) { return f32 ? 1 : 2; }  // ensure_precisions' mask
// f(R()) with R the precision: a float / double pair of calls written with one argument list
template <class F>
int by_precision(bool f32, F&& f) {
  return f32 ? f(float()) : f(double());
}

// the workspace of one render: fixed-point sums at 0, NaN flags at off_flag, queue head words at
// off_ctr (every part 256-byte aligned, zeroed slack behind the sums and the flags: rt_film.hip
// reads both as 16-byte vectors)
struct Workspace { size_t off_flag, off_ctr, bytes; };
inline Workspace workspace_layout(size_t tile_pixels, int acc_words) {
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
    const int rc = rt_api::upload(&d, src);
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

// rt_device_scene::status: the words a kernel's stack overflow sets, one per kind of call, so that
// a query running beside a render (or a synchronous query beside an asynchronous one) reads its own
enum StatusWord {
  kStatusRender = 0,         // renders, film passes, feature passes, camera rays
  kStatusCastAsync = 1,      // rt_scene_cast_async / _ordered_async (rt_scene_cast_status)
  kStatusCastSync = 2,       // rt_scene_cast / _ordered
  kStatusRadianceAsync = 4,  // rt_scene_radiance_async / _ordered_async (rt_scene_radiance_status)
  kStatusRadianceSync = 5,   // rt_scene_radiance / _ordered
  kStatusWords = 8
};

}  // namespace rt_api

struct rt_device_scene {
  int device = 0;
  float* nodes = nullptr;
  int* perlin_perm = nullptr;
  int* status = nullptr;     // rt_api::kStatusWords words, addressed by rt_api::StatusWord
  mutable int* prim_mat = nullptr;  // HostScene::prim_mat, uploaded by the first cast (rt_scene_cast*)
  // a precision's records are uploaded (and its kernel's occupancy queried) on its first render:
  // a caller that renders one precision never pays for the other's copy in HBM or its upload
  std::shared_ptr<const HostScene> host;
  mutable std::mutex mu;
  mutable rt_api::DevArrays<float> f32;
  mutable rt_api::DevArrays<double> f64;
  mutable bool have_f32 = false, have_f64 = false;
  int stack_depth = 1;       // LDS stack entries per lane
  int variant = RT_VAR_FLAT;  // render-kernel variant (rt_internal.h RT_VAR_*)
  double build_ms = 0;       // host scene build (shared by every device of a multi-device scene)
  mutable double upload_ms = 0;  // host -> device copies of this device (common + precisions so far)
  template <class R>
  rt_api::DevArrays<R>& arrays() const;
  template <class R>
  bool& have() const;
};
template <>
inline rt_api::DevArrays<float>& rt_device_scene::arrays<float>() const { return f32; }
template <>
inline rt_api::DevArrays<double>& rt_device_scene::arrays<double>() const { return f64; }
template <>
inline bool& rt_device_scene::have<float>() const { return have_f32; }
template <>
inline bool& rt_device_scene::have<double>() const { return have_f64; }

namespace rt_api __attribute__((visibility("hidden"))) {

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

}  // namespace rt_api

struct rt_multi_scene {
  std::vector<int> devices;                // shard k renders on devices[k]
  std::vector<rt_device_scene*> scenes;    // one per DISTINCT device, in first-use order
  std::vector<int> scene_of;               // devices[k] -> scenes index
  double build_ms = 0, upload_ms = 0;      // one host build; the uploads' wall time (concurrent)
  // kept across renders (grown when a frame needs more): no allocation after the first render
  std::mutex mu;                           // one render at a time: the buffers below are shared
  std::vector<rt_api::MultiPart> parts;    // per devices[k]
  std::vector<char> peer_ok;               // per distinct device: may write the first device's memory
  void* d_gather = nullptr;                // first device: the n tiles in global row order
  size_t gather_cap = 0;
  uint8_t* d_codes = nullptr;              // first device: the 8-bit epilogue's output
  size_t codes_cap = 0;
  hipStream_t st0 = nullptr;               // first device: epilogue and device-to-host copy
  int* h_status = nullptr;                 // pinned host word: the one-device render's status read-back
};

namespace rt_api __attribute__((visibility("hidden"))) {

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

}  // namespace rt_api

// A progressive film (include/rt.h rt_film_*, rt_film.h): the device-resident accumulation state of
// one (scene, camera, seed, precision, shard).  One device allocation made at create holds the
// totals, flags and q, the pass workspace a render writes, the resolved tile of rt_film_read and
// the noise figure's partials: rt_film_add allocates nothing.
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
  rt_api::Workspace ws_lay{};
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

namespace rt_api __attribute__((visibility("hidden"))) {

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

}  // namespace rt_api

struct rt_multi_film {
  const rt_multi_scene* scene = nullptr;
  rt_film* frame = nullptr;
  std::vector<rt_api::FilmPart> parts;
  hipStream_t st_frame = nullptr;  // first device: waits for every merge; the frame film's `last`
  hipEvent_t e_frame = nullptr;    // first device: what was enqueued on the frame before a pass
  bool single = false;             // one shard merged on its own stream: that stream is st_frame, no events
  int64_t copies = 0;              // shard passes that went through the staging copy so far (rt_multi_film_copies)
  std::mutex mu;
};

namespace rt_api __attribute__((visibility("hidden"))) {

// ---- rt_api.hip

// the records of precision R (float, double) on the scene's device (uploaded on first use) and
// their kernel's resident workgroups; thread-safe
template <class R>
int ensure_precision(const rt_device_scene* s);
extern template int ensure_precision<float>(const rt_device_scene*);
extern template int ensure_precision<double>(const rt_device_scene*);
int ensure_precisions(const rt_device_scene* s, int prec_mask);  // bit 0: FP32, bit 1: binary64

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
// one render of the scene's records of precision f32 / binary64, enqueued on `hip_stream`
int render_any(const rt_device_scene* s, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex, bool f32,
               const RenderCall& c, void* hip_stream);

// rt_exec.flags: known bits only, at most one 8-bit encoding
int check_flags(const rt_exec* ex);
// A frame's arguments (non-null) checked before a scene is built or a device touched: image, shard,
// flags, camera (a throw-away KernelParams).  For rt_render, rt_multi_render and rt_film_create alone.
int validate_frame(const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex);
// rt_exec.flags -> the 8-bit epilogue's encoding (0 sRGB, 1 sqrt) or -1 (linear output)
int exec_encoding(const rt_exec* ex);
// the render status words of a multi-device scene's devices, ORed (synchronous; changes the current device)
int multi_status(const rt_multi_scene* M, int* status);

// The argument block of a one-lane kernel (rt_lane.h: the list, feature and query kernels) for the
// frame (cs, seed, ex): the render's, with no staged nodes (every node from memory) and a work plan
// nothing reads (the kernels have their own).  A stack overflow sets the scene's status word `word`
template <class R>
int lane_params(const rt_device_scene* s, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex, KernelParamsT<R>& P,
                StatusWord word = kStatusRender) {
  LaunchInputs L;
  L.resident_lanes = 4096;
  L.lds_nodes = 0;
  std::string err;
  if (int rc = rt_host_render_params(*s->host, s->variant, s->arrays<R>().rec, cs, seed, ex, L, P, err))
    return fail(rc, "%s", err.c_str());
  P.status = s->status + word;
  return RT_OK;
}

}  // namespace rt_api
