// rt_api_film.hip — the film and what lives on it, behind include/rt.h: the progressive film
// (rt_film_*: its state and entry points; kernels in rt_film.hip), adaptive passes (rt_adaptive_*:
// the count plane and entry points; kernels in rt_adaptive.hip and rt_list*.hip), the multi-device
// film (rt_multi_film_*: one frame film on the first device, a pass workspace per shard) and the
// denoiser's buffers (rt_denoise_*; kernels in rt_denoise.hip, rt_features*.hip).  A pass is a
// render of rt_api.hip (render_any); rt_api_internal.h holds the structs.
#include <cmath>
#include <cstdlib>

#include "rt_api_internal.h"
#include "rt_denoise.h"
#include "rt_film.h"

using namespace rt_api;

namespace {

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
// the film's NaN flags to the host, read behind f->last (synchronous; the film's device is current)
int film_flags_read(const rt_film* f, std::vector<unsigned>& flags) {
  flags.resize(f->n_pixels);
  HIP_TRY(hipMemcpyAsync(flags.data(), f->flags, f->n_pixels * sizeof(unsigned), hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipStreamSynchronize(f->last));
  return RT_OK;
}
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
  std::vector<unsigned> flags;
  HIP_TRY(hipSetDevice(f->scene->device));
  HIP_TRY(hipMemcpyAsync(c.data(), f->counts, film_counts_bytes(f), hipMemcpyDeviceToHost, f->last));
  if (int rc = film_flags_read(f, flags)) return rc;
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

// ---- multi-device film

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
  HIP_TRY(hipMemcpyAsync(&status, f->scene->status + kStatusRender, sizeof(int), hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipStreamSynchronize(f->last));
  *n_out = samples;
  if (status) return fail_stack();
  return RT_OK;
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
  HIP_TRY(hipMemcpyAsync(&status, f->scene->status + kStatusRender, sizeof(int), hipMemcpyDeviceToHost, f->last));
  HIP_TRY(hipStreamSynchronize(f->last));
  if (status) return fail_stack();
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
  std::vector<unsigned> flags;
  HIP_TRY(hipSetDevice(f->scene->device));
  if (int rc = film_flags_read(f, flags)) return rc;
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
  if (int rc = by_precision(f->f32, [&](auto r) { return adaptive_pass<decltype(r)>(f, n_samples, threshold, cap, st); }))
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
    std::vector<unsigned> flags;
    if (int rc = film_flags_read(f, flags)) return rc;
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
  if (int rc = multi_status(f->scene, &status)) return rc;
  if (status) return fail_stack();
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
  if (int rc = by_precision(f->f32, [&](auto r) { return film_features<decltype(r)>(f, f->feat, n_feat, st); })) return rc;
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
  if (int rc = by_precision(f->f32, [&](auto r) { return film_features<decltype(r)>(f, f->feat2, n_albedo, st); })) return rc;
  f->albedo_samples = n_albedo;
  f->last = st;
  return RT_OK;
}

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

}  // extern "C"
