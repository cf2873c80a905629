/*
 * rt.h — C ABI of the MI355X path-tracing kernel library (librt_amd.so).
 *
 * Drop-in boundary for the reference's hot path
 *     raytrace :: ToRandom m => CameraSettings -> Geometry m Material -> StdGen -> A.Matrix D Color
 *     (UnaryPlus/raytrace src/Graphics/Ray.hs:121-238)
 * The reference has no FFI of its own (pure Haskell, no `foreign import`); the entry points
 * below are what its Haskell side binds with `foreign import ccall safe` (INTEGRATION.md shows
 * the binding).  Plain C types only: no HIP or torch types cross this boundary; device
 * pointers and streams are passed as `void*` / `float*` owned by the caller.
 *
 * Scene contract.  The reference's Geometry / Material / Texture / background are closures
 * (Geometry.hs:42, Material.hs:17, Texture.hs:15, Ray.hs:57).  The caller reifies them through
 * a deep embedding of the same smart constructors and passes the FLATTENED scene:
 *   - every leaf surface (sphere / parallelogram / triangle) with rigid `transform`s baked in,
 *     its material (outermost `<$` wins), its `moving` motion and its depth-first `order`
 *     (the reference's closest-hit tie-break: earlier leaf wins on equal t, Geometry.hs:340-361);
 *   - every `constantMedium` lifted to the top level with its boundary leaves in their own set.
 * The library builds its own bounding-volume hierarchy over that list; the closest hit (and
 * therefore the image) does not depend on the tree the caller wrote.
 *
 * Precision.  By default the kernel computes in IEEE binary64, as the reference does (every
 * `Vec3` is `V3 Double`, Core.hs:29-31), and writes double output.  rt_exec.flags RT_EXEC_F32
 * selects the FP32 fast path (float output): the same algorithm, scheduling and random stream.
 *
 * Output.  Linear RGB, row-major [row][column][rgb] — row 0 is the TOP of the image — each
 * pixel the MEAN over `samples_per_pixel` samples (Ray.hs:226-232); double (default) or float
 * (RT_EXEC_F32) per channel.  Randomness is a counter-based Philox4x32-10 stream keyed by
 * `seed` and indexed by (pixel, sample, segment, event), so results are deterministic for a
 * given (scene, camera, seed, precision) and independent of the shard layout, of the device
 * list and of the GPU count.
 */
#ifndef RT_AMD_H
#define RT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 6

/* status codes */
#define RT_OK 0
#define RT_E_GENERIC (-1)
#define RT_E_INVALID (-2)      /* malformed scene/camera (reference: `error` / NaN)              */
#define RT_E_UNSUPPORTED (-3)  /* closure the device cannot evaluate; caller falls back to CPU   */
#define RT_E_HIP (-4)          /* HIP runtime failure (no device, launch failure, OOM)            */
#define RT_E_STACK (-5)        /* BVH traversal stack overflow (scene too deep)                   */

/* primitive kinds (Geometry.hs:58-176) */
#define RT_PRIM_SPHERE 0
#define RT_PRIM_PARALLELOGRAM 1
#define RT_PRIM_TRIANGLE 2

/* material kinds (Material.hs:41-129) */
#define RT_MAT_LIGHT_SOURCE 0
#define RT_MAT_PITCH_BLACK 1
#define RT_MAT_LAMBERTIAN 2
#define RT_MAT_LOMMEL_SEELIGER 3
#define RT_MAT_MIRROR 4
#define RT_MAT_METAL 5        /* param = fuzz */
#define RT_MAT_DIELECTRIC 6   /* param = index of refraction */
#define RT_MAT_TRANSPARENT 7
#define RT_MAT_ISOTROPIC 8
#define RT_MAT_ANISOTROPIC 9  /* param = Henyey-Greenstein g */

/* texture kinds (Texture.hs:18-78) */
#define RT_TEX_CONSTANT 0     /* c0 */
#define RT_TEX_CHECKER 1      /* nu, nv, c0, c1 */
#define RT_TEX_IMAGE 2        /* nu = width, nv = height, image = first texel in rt_scene.texels
                                 (row-major, row 0 = top of the image, 3 floats per texel) */
#define RT_TEX_NOISE 3        /* nu = layers; params[0] = frequency, params[1..3] = shift; c0, c1
                                 (fractal Perlin noise, needs rt_scene.perlin) */
#define RT_TEX_MARBLE 4       /* params[0..2] = stripe direction, params[3] = frequency,
                                 params[4..6] = shift (turbulence, needs rt_scene.perlin) */

/* background kinds (cs_background restricted to reifiable closures) */
#define RT_BG_CONST 0         /* c0 */
#define RT_BG_LERP_Y 1        /* (1 - a) c0 + a c1, a = 0.5 (dir.y + 1)  (`sky`, `grayFade`) */

/* rt_prim.set of the object-space leaves of instanced object b (rt_instance.blas == b) */
#define RT_SET_BLAS(b) (-1 - (b))

/* One leaf surface.  Ray.hs/Geometry.hs semantics; coordinates in world space, or in the
 * object space of an instanced object (set RT_SET_BLAS(b)). */
typedef struct rt_prim {
  int32_t kind;      /* RT_PRIM_* */
  int32_t material;  /* index into rt_scene.materials (ignored for medium boundaries; -1 allowed
                        for an instanced object's leaves when every instance of it has one)   */
  int32_t set;       /* 0 = visible surface; k >= 1 = boundary of rt_scene.media[k-1];
                        RT_SET_BLAS(b) = a leaf of instanced object b (object space)          */
  int32_t motion;    /* -1 or index into rt_scene.motions (`moving`, Geometry.hs:449-456)      */
  int32_t gid;       /* geometric identity: the same source leaf under the same transform has
                        the same gid in every set (used to skip self-intersection)          */
  int32_t order;     /* depth-first position of the leaf in the caller's tree (tie-break);
                        for an instanced object's leaf: its position inside the object        */
  int32_t uvframe;   /* -1 or index into rt_scene.uvframes: rotation R^T for sphereUV         */
  int32_t pad;
  double p[9];       /* sphere: center[3], radius, -; plane: q[3], u[3], v[3]                 */
  double uv[6];      /* plane shapes: uv0, uv1, uv2 (parallelogram: (0,0),(1,0),(0,1))         */
} rt_prim;

typedef struct rt_medium {   /* constantMedium (Geometry.hs:298-330) */
  double density;
  int32_t material;
  int32_t order;
} rt_medium;

typedef struct rt_material {
  int32_t kind;      /* RT_MAT_* */
  int32_t texture;   /* index into rt_scene.textures */
  double param;
} rt_material;

typedef struct rt_texture {
  int32_t kind;      /* RT_TEX_* */
  int32_t nu, nv;    /* checker dimensions | image width, height | noise layers */
  int32_t image;     /* image: index of its first texel in rt_scene.texels, else -1 */
  double c0[3], c1[3];
  double params[8];  /* noise / marble parameters (see RT_TEX_*) */
} rt_texture;

/* The Perlin tables of Noise.hs:21-92: the three fixed permutations (permX/Y/Z) and the 256
   gradients (`replicateM 256 randomUnitVector` evaluated with mkStdGen 666). */
typedef struct rt_perlin {
  int32_t perm[3][256];
  double grad[256][3];
} rt_perlin;

typedef struct rt_motion {
  double v0[3], v1[3];   /* world-space shift (1 - time) v0 + time v1 */
} rt_motion;

typedef struct rt_uvframe {
  double r[9];           /* row-major 3x3: object-space normal = r * world-space normal */
} rt_uvframe;

/* Two-level instancing of `transform` (Geometry.hs:382-391): one placement of an instanced
 * object (the leaves with set RT_SET_BLAS(blas), traced in object space under its own BVH).
 * The world ray enters the object through the inverse of the rigid transform m; t is unchanged
 * (rigid), hit points / normals go back through m.  The instance's leaves take depth-first
 * orders order .. order + (leaves of the object) - 1 in the tie-break. */
typedef struct rt_instance {
  int32_t blas;      /* instanced object */
  int32_t material;  /* material of every surface of this placement (the outermost `<$`), or -1:
                        the leaves' own materials */
  int32_t order;     /* depth-first order of the object's first leaf in the caller's tree */
  int32_t pad;
  double m[12];      /* object -> world, row-major 3 x 4, rigid (R^T R = I) */
} rt_instance;

typedef struct rt_scene {
  int32_t n_prims;      const rt_prim* prims;
  int32_t n_media;      const rt_medium* media;
  int32_t n_materials;  const rt_material* materials;
  int32_t n_textures;   const rt_texture* textures;
  int32_t n_motions;    const rt_motion* motions;
  int32_t n_uvframes;   const rt_uvframe* uvframes;
  int32_t n_texels;     const float* texels;      /* image textures' linear RGB, 3 floats each */
  const rt_perlin* perlin;                        /* required by noise / marble textures   */
  int32_t n_instances;  const rt_instance* instances;  /* two-level instancing (may be 0)  */
} rt_scene;

typedef struct rt_redirect_target {   /* cs_redirectTargets element (p, q, u, v) */
  double prob;
  double q[3], u[3], v[3];
} rt_redirect_target;

/* CameraSettings (Ray.hs:40-68) with the background reified. */
typedef struct rt_camera_settings {
  double center[3];
  double look_at[3];
  double up[3];
  double vfov;              /* radians */
  double aspect_ratio;
  int32_t image_width;
  int32_t samples_per_pixel;
  int32_t max_recursion_depth;
  int32_t background_kind;  /* RT_BG_* */
  double background_c0[3];
  double background_c1[3];
  double defocus_angle;     /* radians */
  double focus_dist;
  int32_t n_redirect_targets;
  int32_t pad;
  const rt_redirect_target* redirect_targets;
} rt_camera_settings;

/* rt_exec.flags (any other bit, or both RT_EXEC_ENCODE8_* bits, is RT_E_INVALID) */
#define RT_EXEC_F32 1          /* FP32 kernel, float output (default: binary64, double output) */
/* 8-bit output (rt_render / rt_multi_render only): out_rgb receives uint8 codes, one per channel,
   exactly what writeImage (sRGB) / writeImageSqrt (sqrt) store (Ray.hs:248-260):
   min(255, floor(256 * transfer(clamp01 x))) of the linear mean, NaN -> 0 — the fused epilogue
   of rt_encode8_async, run on the gathering device after the gather.  Bit-identical to encoding
   the linear render on the host. */
#define RT_EXEC_ENCODE8_SRGB 2
#define RT_EXEC_ENCODE8_SQRT 4
/* rt_render_async only: this render does not overlap another on the device (one stream, or the
   caller waits for it), so its work is planned for a short end, as rt_render's: 16-sample big
   items instead of up to 64 (rt_build.cpp rt_host_plan_work).  Images are identical either way. */
#define RT_EXEC_SOLO 8

#define RT_MAX_DEVICES 64

/* Which rows this call renders, on which devices, in which precision.
 *
 * Rows are dealt to shards in blocks of `row_block` round-robin: shard r owns global rows y
 * with (y / row_block) % n_shards == r.  With n_shards > 1 every shard has the same padded row
 * count (rt_shard_rows); padding rows are written as zeros.  With n_shards == 1 the tile is
 * exactly the image (height rows).  This is the one-process-per-GPU form (each rank renders
 * its shard on `device`).
 *
 * Device list (rt_render only; one process, many GPUs).  With n_devices >= 1 and n_shards == 1
 * the call renders the WHOLE image over devices[0 .. n_devices-1]: device k renders shard k of
 * n_devices (same row interleave), all devices concurrently on their own streams.  The scene is
 * built on the host ONCE and uploaded to the distinct devices concurrently; each device copies its
 * tile into devices[0]'s framebuffer (peer-to-peer over xGMI, the rows un-permuted by the copy's
 * stride), and one device-to-host copy fills out_rgb.  A device may appear more than once (two
 * shards on one GPU).  The image is bit-identical to the single-device render.  n_devices == 0:
 * `device` alone.  rt_multi_scene_create keeps such a scene resident across renders. */
typedef struct rt_exec {
  int32_t device;       /* HIP device ordinal (n_devices == 0) */
  int32_t n_shards;     /* >= 1 */
  int32_t shard;        /* 0 .. n_shards-1 */
  int32_t row_block;    /* >= 1 */
  int32_t flags;        /* RT_EXEC_* */
  int32_t n_devices;    /* 0, or 1 .. RT_MAX_DEVICES entries of `devices` (rt_render only) */
  const int32_t* devices;
} rt_exec;

typedef struct rt_stats {
  double upload_ms;     /* scene build + host->device copy (all devices) */
  double kernel_ms;     /* device time of the render (the slowest device of a device list) */
  double total_ms;      /* wall time of the call */
  int64_t samples;      /* pixels x spp rendered by this call */
  int32_t bvh_nodes;    /* nodes of all sets */
  int32_t max_stack;    /* deepest traversal stack the build can require */
  int32_t device_allocs; /* device allocations (hipMalloc) this call made: a resident multi-device
                            scene allocates its buffers on its first render (or a larger frame)
                            only, so later rt_multi_render calls report 0 (ABI v5) */
  int32_t kernel_block; /* workgroup size of the render kernel the call launched (ABI v6; the
                           1024-lane BVH classes run a 512-lane twin for a BVH whose traversal
                           stacks do not fit one 1024-lane workgroup's LDS); 0 from rt_scene_stats */
} rt_stats;

typedef struct rt_device_scene rt_device_scene;   /* opaque, device-resident scene */
typedef struct rt_multi_scene rt_multi_scene;     /* opaque, resident on a list of devices */

int rt_abi_version(void);
const char* rt_last_error(void);   /* thread-local message of the last failing call */
/* number of visible HIP devices (>= 1), or RT_E_HIP when there is none — what a caller puts in a
 * device list to render on every GPU of the node (rt_exec.devices) */
int rt_device_count(void);

/* image height for a width and aspect ratio: round (w / aspect), banker's rounding (Ray.hs:123) */
int rt_image_height(const rt_camera_settings* cs);
/* padded rows per shard for an image of `height` rows under `ex` */
int rt_shard_rows(int32_t height, const rt_exec* ex);
/* global row of shard-local row t (may be >= height for padding rows) */
int rt_shard_row(int32_t t, const rt_exec* ex);

/* One-shot host-buffer call — the Haskell binding's entry point (replaces Ray.hs:121-238).
 * out_rgb: caller-owned host buffer of rt_shard_rows(h, ex) * image_width * 3 doubles (floats
 * with RT_EXEC_F32, uint8 codes with RT_EXEC_ENCODE8_*); the whole image when n_shards == 1.  Returns RT_OK or a negative RT_E_*
 * code.  On RT_E_STACK a one-device call has written the partial image to out_rgb (a device list
 * leaves it untouched); the caller renders such a scene on the CPU path.  No copy into out_rgb is
 * in flight once the call has returned, whatever the code. */
int rt_render(const rt_camera_settings* cs, const rt_scene* scene, uint64_t seed, const rt_exec* ex,
              void* out_rgb, rt_stats* stats);

/* Device-resident path (used when inputs already live in HBM, e.g. bench.py / torch callers).
 * The scene is built on the host at create; a precision's records are uploaded on its first
 * render (rt_stats.upload_ms of rt_scene_stats covers what has been uploaded so far).  That first
 * render of a precision is therefore NOT asynchronous: it makes synchronous device allocations and
 * copies (and queries the kernel's occupancy) before it enqueues; a caller that captures the
 * stream into a HIP graph, or needs the first call to return at once, renders that precision
 * once beforehand. */
int rt_scene_create(const rt_scene* scene, int32_t device, rt_device_scene** out);
int rt_scene_destroy(rt_device_scene* s);
int rt_scene_stats(const rt_device_scene* s, rt_stats* stats);
/* Enqueue one render on `hip_stream` (a hipStream_t, or NULL for the default stream) of the
 * scene's device.  d_out_rgb: device buffer of rt_shard_rows(h, ex) * image_width * 3 doubles
 * (floats with RT_EXEC_F32).  ex->n_devices must be 0.  Asynchronous; the scene must outlive
 * the work.  Renders are planned for frames that overlap on two or more streams (the next frame
 * fills the end of this one); RT_EXEC_SOLO plans a render that runs alone. */
int rt_render_async(const rt_device_scene* s, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex,
                    void* d_out_rgb, void* hip_stream);

/* Multi-device resident scene (one process, many GPUs; what a caller that renders the same scene
 * more than once keeps between rt_render-like calls): one host build, concurrent uploads to the
 * distinct devices of the list, and per device its tile, render workspace, stream and events plus
 * the first device's gather and 8-bit buffers, all kept across renders (allocated on the first
 * render, or again for a larger frame: rt_stats.device_allocs).  Renders of one scene are
 * serialised (a mutex); the status word (traversal-stack overflow) is cleared before each.  rt_multi_render renders as rt_render does with this device list
 * (ex->n_devices must be 0; ex->n_shards 1, row_block and flags as in rt_render) into the
 * caller's host buffer out_rgb (h * width * 3 doubles, floats with RT_EXEC_F32, bytes with
 * RT_EXEC_ENCODE8_*).  A list of one device also renders an rt_exec shard (n_shards > 1). */
int rt_multi_scene_create(const rt_scene* scene, const int32_t* devices, int32_t n_devices, rt_multi_scene** out);
int rt_multi_scene_destroy(rt_multi_scene* m);
int rt_multi_render(const rt_multi_scene* m, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex,
                    void* out_rgb, rt_stats* stats);

/* Fused output epilogue of writeImage / writeImageSqrt (Ray.hs:248-260): linear RGB (float, or
 * double with in_f64 = 1) -> 8-bit codes min(255, floor(256 * transfer(clamp01 x))), transfer =
 * sRGB (encoding 0) or sqrt (encoding 1), evaluated in binary64; NaN -> 0.  Bit-exact against
 * the host encoder.  Device pointers, asynchronous on hip_stream. */
int rt_encode8_async(const void* d_rgb, int32_t in_f64, uint8_t* d_out, int64_t n_values, int32_t encoding,
                     void* hip_stream);

/* Progressive film: the device-resident accumulation state of one (scene, camera, seed, precision,
 * shard).  Samples are added in passes, and the film can be resolved to an image, asked for a noise
 * estimate, saved and loaded at any time.  The sample index is a word of the Philox counter and the
 * per-pixel sums are integers, so passes of a, b, c, ... samples give the image of ONE render of
 * a + b + c + ... samples, bit for bit (rt_render / rt_render_async with that samples_per_pixel).
 *
 * rt_film_create: `s` is the film's scene and must outlive it; ex as for rt_render_async (n_devices
 *   0, no RT_EXEC_ENCODE8_* bit; a shard is allowed: the film then holds that shard's tile).
 *   cs->samples_per_pixel is validated and then not read: the film's count is what has been added.
 *   Every device buffer is allocated here (the first film of a precision also uploads the scene's
 *   records of that precision): rt_film_add allocates nothing.  A pass runs alone on its stream
 *   (its merge follows it), so passes are planned as RT_EXEC_SOLO renders whatever ex->flags says.
 * rt_film_add: enqueue samples [N, N + n_samples) of every pixel and their merge on hip_stream;
 *   n_samples <= 0 or a total beyond 2^24 samples is RT_E_INVALID.  Asynchronous.  A film's calls
 *   are ordered by the caller: one stream, or events between streams.
 * rt_film_resolve: enqueue the mean of the samples so far into d_out_rgb (a device buffer as
 *   rt_render_async's: rt_shard_rows(h, ex) * width * 3 doubles, floats with RT_EXEC_F32).
 * The synchronous calls (read, noise, get_info, save, load, reset) run behind the stream of the
 *   last rt_film_add and wait for it.  rt_film_read: the resolved tile in a host buffer; RT_E_STACK
 *   (image written) when the scene's traversal-stack word is set.
 * rt_film_noise: the relative standard error of each pixel's mean R + G + B, estimated from the
 *   passes (batch means; any pass sizes; needs two passes, else RT_E_INVALID), against
 *   max(mean, 3 / 256); *noise = sqrt(mean of its square) over the pixels that count (not NaN-
 *   flagged, not a shard's padding row; those are NaN in the map), identical from run to run.
 *   d_map_or_null: a device buffer of one float per tile pixel, or NULL.
 * rt_film_save / rt_film_load: the state (rt_film_state_bytes: a 64-byte header — magic, layout
 *   version, precision, width, height, tile rows, shard triple, Philox key, samples, passes — then
 *   the sums, the NaN flags and the estimator's word per pixel) to / from a host buffer.  Load
 *   rejects a state whose header does not match the film it is loaded into (RT_E_INVALID).  The
 *   header does NOT identify the scene or the camera's position: loading a state into a film of
 *   the scene and camera it was saved from is the caller's responsibility. */
typedef struct rt_film rt_film;
typedef struct rt_film_info {
  int64_t samples;       /* per pixel, all passes */
  int32_t passes;
  int32_t width, rows;   /* the tile: rt_shard_rows(h, ex) rows */
  int32_t nan_pixels;    /* pixels with a non-finite sample so far (NaN in the image) */
  int32_t f32;           /* 1: RT_EXEC_F32 */
} rt_film_info;
int rt_film_create(const rt_device_scene* s, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex,
                   rt_film** out);
int rt_film_destroy(rt_film* f);
int rt_film_reset(rt_film* f);   /* back to 0 samples */
int rt_film_add(rt_film* f, int32_t n_samples, void* hip_stream);
int rt_film_resolve(const rt_film* f, void* d_out_rgb, void* hip_stream);
int rt_film_read(const rt_film* f, void* host_out_rgb);
int rt_film_noise(const rt_film* f, float* d_map_or_null, double* noise);
int rt_film_get_info(const rt_film* f, rt_film_info* info);
int rt_film_state_bytes(const rt_film* f, int64_t* bytes);
int rt_film_save(const rt_film* f, void* host_buf, int64_t cap);
int rt_film_load(rt_film* f, const void* host_buf, int64_t bytes);

/* Adaptive film passes: add samples only where the film's own noise estimate asks for them.
 *
 * A film becomes NON-UNIFORM at its first rt_adaptive_add: it gains a count plane, two uint32 per
 * tile pixel — the pixel's samples N_p and passes K_p —, allocated by that call (with the selection
 * list and scratch; no later call allocates) and started at the film's (N, K) inside the frame and
 * (0, 0) on a shard's padding rows.  A film that never makes the call allocates nothing more and
 * behaves and saves bit for bit as before.
 *
 * rt_adaptive_add: enqueue one adaptive pass on hip_stream (asynchronous, no host synchronisation).
 *   A pixel COUNTS if it lies inside the frame and is not NaN-flagged; a counting pixel is SELECTED
 *   iff its relative error — what rt_film_noise maps, in binary64 before the cast to float, from the
 *   pixel's own (N_p, K_p) — is > threshold (a negative threshold selects every counting pixel) and
 *   N_p + n_samples <= max_samples (0: 2^24, the film's limit).  Every selected pixel receives
 *   samples [N_p, N_p + n_samples) of its own stream — the key, events and arithmetic of a render, so
 *   the pixel's sums, flag and colour are bit for bit those of a uniform film at N_p + n_samples —,
 *   its estimator word one more batch, and (N_p, K_p) += (n_samples, 1).  Unselected pixels are not
 *   touched.  The selection is taken in ascending tile-pixel order.  Needs two passes in the film;
 *   RT_E_INVALID otherwise and for a null film, n_samples <= 0, a NaN threshold, max_samples outside
 *   [0, 2^24] or a multi-device film's frame, each before any device call.
 *   The threshold reads an estimate made from the pixel's own earlier samples, so the adaptive mean
 *   carries the usual small adaptive-sampling bias; nothing here corrects it.
 * On a non-uniform film: rt_film_resolve / rt_film_read divide each pixel by its own N_p (the
 *   one-shot resolve's operation sequence); rt_film_noise uses each pixel's (N_p, K_p);
 *   rt_film_get_info reports the largest N_p and K_p; rt_film_save writes layout version 2 — the
 *   version-1 bytes, then the count plane, the header's samples / passes the maxima
 *   (rt_film_state_bytes counts it) — and rt_film_load accepts versions 1 and 2, a version-2 state
 *   making the film non-uniform.  rt_film_add is RT_E_INVALID (a uniform continuation is
 *   rt_adaptive_add with a negative threshold), rt_denoise_film / rt_denoise_film_read are
 *   RT_E_UNSUPPORTED (the filter's variance uses one N, K), rt_multi_film_load of a version-2 state
 *   is RT_E_INVALID.  rt_film_reset drops the plane: the film is uniform again.
 * The calls below are synchronous behind the film's last stream.
 * rt_adaptive_get_info: the counts' summary.  rt_adaptive_counts_read: the plane, tile pixels x 2
 *   uint32 (N_p, K_p); on a uniform film (N, K) inside the frame and (0, 0) on padding rows.
 * rt_adaptive_selection_read: the last adaptive pass's selection, ascending tile pixels: *n its
 *   length, the first min(cap, *n) entries written (host_tile_pixels may be NULL with cap 0);
 *   *n = 0 when no adaptive pass has run since create, reset or load. */
typedef struct rt_adaptive_info {
  int64_t total_samples;   /* the sum of N_p over the pixels that count */
  int32_t min_samples;     /* the smallest and ...                       */
  int32_t max_samples;     /* ... largest N_p of a pixel that counts     */
  int32_t selected;        /* pixels the last adaptive pass selected     */
  int32_t adaptive_passes; /* since create, reset or load                */
  int32_t nonuniform;      /* 1: the film holds a count plane            */
  int32_t reserved;
} rt_adaptive_info;
int rt_adaptive_add(rt_film* f, int32_t n_samples, double threshold, int32_t max_samples, void* hip_stream);
int rt_adaptive_get_info(const rt_film* f, rt_adaptive_info* info);
int rt_adaptive_counts_read(const rt_film* f, uint32_t* host);
int rt_adaptive_selection_read(const rt_film* f, int32_t* host_tile_pixels, int64_t cap, int64_t* n);

/* Multi-device film: progressive passes over a multi-device scene's device list, ONE frame.
 *
 * The film holds one accumulation state, on the scene's first device: an ordinary one-shard film of
 * the whole image (the "frame").  A pass of n samples renders shard k's samples [N, N + n) on
 * devices[k] (the rt_exec row interleave, every device on its own stream, none waiting for another)
 * and a merge kernel folds each shard's pass sums straight into the frame's rows — run by devices[k]
 * writing the first device's memory (peer access, as the one-shot resolve), or, without peer access,
 * by the first device on a copy of the shard's sums and flags.  The sums are integers keyed by global
 * pixel and sample index, so after the merges the frame is, bit for bit, the state an rt_film on one
 * device holds after the same passes: sums, NaN flags and the estimator's word.  A saved state does
 * not depend on the device count.
 *
 * rt_multi_film_create: the devices are the scene's (`m` must outlive the film; a list of one device
 *   and a list that repeats a device are valid; a shard that holds only padding rows — more devices
 *   than row blocks — contributes nothing).  ex gives the precision and row_block: n_devices 0,
 *   n_shards 1 (else RT_E_INVALID), no RT_EXEC_ENCODE8_* bit; cs as for rt_film_create.  Every buffer,
 *   stream and event is allocated here: rt_multi_film_add allocates nothing.
 * rt_multi_film_add: enqueue one pass on every device; limits as rt_film_add's.  Asynchronous: no
 *   host thread and no host synchronisation, the work is ordered by events, behind whatever was
 *   enqueued through the frame handle before (rt_film_resolve, rt_denoise_* on a stream of the
 *   caller's: the pass's merges wait for that stream).  If it fails after the first enqueue (a HIP
 *   error), shards enqueued before the failure are merged all the same and the sample count is not
 *   advanced: the frame holds a partial pass, and only rt_multi_film_reset or rt_multi_film_load
 *   gives a defined state again.
 * rt_multi_film_reset, rt_multi_film_load: as rt_film_reset / rt_film_load, after waiting for the
 *   passes in flight.  Load accepts exactly the state a one-shard rt_film of this frame saves (the
 *   same header checks, against n_shards = 1).
 * rt_multi_film_frame: waits for everything enqueued on every device and hands out the frame, which
 *   the multi film owns (valid until rt_multi_film_destroy).  RT_E_STACK (frame handed out all the
 *   same) when the traversal-stack word of any of the scene's devices is set.  On the handle every
 *   reading call works as on any one-shard film — rt_film_read, resolve, noise, get_info,
 *   state_bytes, save and every rt_denoise_* call (the feature and albedo passes are first-hit
 *   passes, cheap next to a render pass: they run on the first device alone) — and follows the
 *   passes added so far, without another rt_multi_film_frame: the asynchronous ones
 *   (rt_film_resolve, rt_denoise_features / albedo / film) make their stream wait for the merges
 *   first.  Only rt_multi_film_frame reports the other devices' RT_E_STACK.  rt_film_add,
 *   rt_film_load, rt_film_reset and rt_film_destroy on it return RT_E_INVALID.
 * rt_multi_film_copies: the number of shard passes so far whose sums went to the first device by
 *   the staging copy (0 where every device has peer access to the first). */
typedef struct rt_multi_film rt_multi_film;
int rt_multi_film_create(const rt_multi_scene* m, const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex,
                         rt_multi_film** out);
int rt_multi_film_destroy(rt_multi_film* f);
int rt_multi_film_reset(rt_multi_film* f);
int rt_multi_film_add(rt_multi_film* f, int32_t n_samples);
int rt_multi_film_load(rt_multi_film* f, const void* host_buf, int64_t bytes);
int rt_multi_film_frame(rt_multi_film* f, rt_film** frame);
int rt_multi_film_copies(const rt_multi_film* f, int64_t* n);

/* First-hit feature buffers and a variance-guided denoiser for a film's preview.
 *
 * rt_denoise_features: for samples [0, n_feat) of every tile pixel (1 <= n_feat <= 4096), trace the
 *   primary ray the render uses for that sample (same Philox key and events) to its first event,
 *   found as the render's first segment finds it (surfaces, then the segment's medium events), and
 *   add 8 int64 words per pixel: albedo RGB (the hit material's texture; 1 for dielectric, 0 for
 *   pitchBlack; the phase material's texture in a medium; the background on a miss), the unit
 *   normal facing the ray (0 in a medium and on a miss) and the hit distance — each in units of
 *   2^-32, as the render's sums — and the number of samples that hit; a binary64 film adds 8 more
 *   words, the next 32 bits of each of those sums (the last unused), as its colour sums have.
 *   Integer sums: identical from run to run.  The buffers are allocated on the first call (a film that never asks
 *   allocates nothing) and are a function of scene, camera and seed: rt_film_add / reset / load do
 *   not touch them, and they are not part of rt_film_save's state.  Asynchronous on hip_stream.
 * rt_denoise_features_read: the words (tile pixels x 8 int64; x 16 for a binary64 film) and their
 *   n_feat to the host, behind
 *   the film's last stream; RT_E_INVALID before rt_denoise_features.
 * rt_denoise_albedo: the same pass over samples [0, n_albedo) into a second buffer of the same
 *   layout (allocated on its first call), of which the filter reads the albedo alone: it divides the
 *   colour by the albedo of rt_denoise_features' samples — the film's own first samples, whose
 *   coverage noise at an emitter's or a texture's edge the two then share and the quotient loses —
 *   and multiplies the filtered quotient by this better estimate of the same albedo.  Optional:
 *   without it the filter multiplies by what it divided by.  64 samples cost eight feature passes
 *   of 8, once per film: like the features, the buffer does not change as samples are added.
 *   n_albedo = 0 drops it again.
 * rt_denoise_albedo_read: rt_denoise_albedo's words, as rt_denoise_features_read.
 * rt_denoise_film: enqueue the filtered image into d_out_rgb (as rt_film_resolve's).  The mean
 *   colour (the sums' high words) is divided by the albedo, filtered by `levels` passes of a 5 x 5
 *   a-trous kernel at steps 1, 2, 4, ... whose taps are weighted by normal, depth, albedo and — scaled
 *   by the film's variance estimate — luminance similarity, and multiplied by the albedo again
 *   (DESIGN.md "Denoiser": the exact operation sequence, binary64 whatever the film's precision;
 *   raytrace_amd.denoise.denoise_reference restates it in numpy bit for bit).  NaN-flagged pixels
 *   stay NaN and are not read by their neighbours.  RT_E_INVALID unless the film holds two passes and
 *   its features have been computed, for levels outside 1..8, k outside 0..16 or a sigma / eps that
 *   is not positive; RT_E_UNSUPPORTED for a film of n_shards > 1 (its rows are interleaved with
 *   other shards', and the filter needs a pixel's neighbours; a device list is denoised through
 *   rt_multi_film_frame's frame, which is one whole image).  The working buffers are allocated on
 *   the first call and kept.  p == NULL: rt_denoise_default_params.
 * rt_denoise_film_read: the same into a host buffer, synchronous (as rt_film_read). */
typedef struct rt_denoise_params {
  int32_t levels;          /* 1..8 filter passes; pass i steps 2^i pixels (default 5) */
  int32_t k;               /* normal weight: cosine to the power 2^k (default 5) */
  double sigma_z;          /* relative depth difference at which the depth weight is 1/2 (0.1) */
  double sigma_l;          /* luminance difference in standard deviations at which its weight is 1/2 (4) */
  double sigma_a;          /* relative albedo difference at which the albedo weight is 1/2 (0.1) */
  double eps_n;            /* |mean normal|^2 below this: a featureless pixel (1e-6) */
  double eps_z;            /* floor of the depth scale (1e-6) */
  double eps_l;            /* added to the luminance weight's variance term (1e-10) */
} rt_denoise_params;
int rt_denoise_default_params(rt_denoise_params* p);
int rt_denoise_features(rt_film* f, int32_t n_feat, void* hip_stream);
int rt_denoise_albedo(rt_film* f, int32_t n_albedo, void* hip_stream);
int rt_denoise_features_read(const rt_film* f, int64_t* host_words, int32_t* n_feat);
int rt_denoise_albedo_read(const rt_film* f, int64_t* host_words, int32_t* n_albedo);
int rt_denoise_film(rt_film* f, const rt_denoise_params* p, void* d_out_rgb, void* hip_stream);
int rt_denoise_film_read(rt_film* f, const rt_denoise_params* p, void* host_out_rgb);

/* Batched ray queries on a resident scene: closest hit and any hit.
 *
 * The reference's other public type is `Geometry`: a hit function time -> Ray -> (tmin, tmax) ->
 * Maybe (HitRecord, a) (Geometry.hs:42, Core.hs:155-160).  rt_scene_cast evaluates it for n rays
 * against the scene's SURFACE set, exactly as segment 0 of a render queries it (the flat sets, or the
 * surface prefix and the BVH traversal of the scene's kernel class).  `constantMedium` volumes are
 * not hit: their events are random draws keyed by pixel and sample, which a query does not have.
 *
 * rt_ray: the ray origin + t dir / |dir|.  The direction may have any non-zero length and is
 *   normalised in binary64 before anything else, so t is a DISTANCE; the reference's sphere test
 *   assumes a unit direction (Geometry.hs:63-68), so for unit directions t is its hr_t.  The interval
 *   (tmin, tmax) is open at both ends, 0 <= tmin < tmax, tmax may be +infinity (with RT_EXEC_F32 both
 *   ends are rounded to float first).  time in [0, 1] places `moving` geometry; the kernel keeps it as
 *   the render does, in 24 bits: floor(time 2^24) / 2^24, and a time of 1 is 1 - 2^-24.
 * rt_hit: hit = 1 with every field set, 0 for a miss, -1 for a malformed ray (a non-finite field,
 *   a zero direction, tmin < 0, tmax <= tmin, time outside [0, 1]): nothing else in the record is
 *   defined then.  normal is the unit normal facing the ray, as the materials see it (hr_normal), and
 *   front is hr_frontSide; for an instanced leaf the point is the world-space one and the normal is
 *   rotated to world space.  leaf is the leaf's depth-first order in the caller's tree (rt_prim.order;
 *   an instanced object's leaf: rt_instance.order + its order inside the object; a flat scene
 *   reports the leaf's rank among the surface leaves in that order) — on equal t the smaller one
 *   wins, as in the reference (Geometry.hs:340-361).  instance is the rt_scene.instances index of the
 *   placement or -1; material the rt_scene.materials index, the placement's material where it has one.
 * flags: RT_QUERY_UV computes uv (sphereUV or the plane shape's uv lerp), without it uv is 0.
 *   RT_QUERY_ANY_HIT asks only WHETHER the interval holds a hit: hit is exactly the closest-hit
 *   query's, t is the distance of some accepted hit inside the interval, every other field is
 *   unspecified; the BVH classes leave their traversal at the first accepted hit.
 * One lane per ray, 64 consecutive rays per wave, in the caller's order: that order is the kernel's
 *   coherence.  rt_scene_cast_ordered (below) traces the same rays in a coherence order instead;
 *   nothing is compacted.
 *
 * rt_scene_cast_async: d_rays / d_hits are device buffers of n records on the scene's device;
 *   enqueues on hip_stream.  ex gives the precision (RT_EXEC_F32) and must name no device list; the
 *   first cast of a precision uploads that precision's records (as a first render does) and is not
 *   asynchronous.  n == 0 is a no-op.  A traversal-stack overflow sets a word of the scene that stays
 *   set until rt_scene_cast_status reads it.
 * rt_scene_cast: the same from and to host buffers, synchronous; RT_E_STACK (hits written) if a
 *   traversal stack overflowed.
 * rt_scene_cast_status: *overflowed = 1 if an rt_scene_cast_async since the last call overflowed a
 *   traversal stack (such rays' records are not reliable), and clears the word; call it after
 *   synchronising the casts' stream.
 * Null arguments and n < 0 are RT_E_INVALID before any device call. */
#define RT_QUERY_UV 1
#define RT_QUERY_ANY_HIT 2
typedef struct rt_ray {
  double origin[3];
  double dir[3];
  double tmin, tmax;
  double time;
  double reserved;   /* not read: the record is 80 bytes, five 16-byte vectors */
} rt_ray;
typedef struct rt_hit {
  double t;
  double point[3];
  double normal[3];
  double uv[2];
  int32_t hit;       /* 1 hit, 0 miss, -1 malformed ray */
  int32_t front;     /* hr_frontSide */
  int32_t leaf;
  int32_t instance;  /* or -1 */
  int32_t material;
  int32_t reserved;
} rt_hit;
int rt_scene_cast_async(const rt_device_scene* s, const rt_exec* ex, const rt_ray* d_rays, rt_hit* d_hits, int64_t n,
                        int32_t flags, void* hip_stream);
int rt_scene_cast(const rt_device_scene* s, const rt_exec* ex, const rt_ray* host_rays, rt_hit* host_hits, int64_t n,
                  int32_t flags);
int rt_scene_cast_status(const rt_device_scene* s, int32_t* overflowed);

/* Batched radiance queries on a resident scene: the path tracer on the caller's rays.
 *
 * rayColor (Ray.hs:174-224) is private to `raytrace` in the reference; rt_scene_radiance evaluates it
 * for n rays of the caller: an orthographic or panoramic camera, irradiance probes, a lightmap.
 * Unlike rt_scene_cast it draws random numbers, includes the `constantMedium` events and shades.
 *
 * rt_path_ray: ray i receives samples sample0 + [0, n_samples); each is ONE evaluation of
 *   rayColor max_recursion_depth time ray.  Sample k uses the Philox words (stream, sample0 + k,
 *   segment, event) under the key of `seed`, exactly as sample sample0 + k of a render's pixel whose
 *   global id is `stream` does after its camera ray (the camera's own draws sit under events of their
 *   own), so the ray a render makes for (pixel, sample) — rt_scene_camera_rays writes those — returns
 *   that render's sample, word for word.  The direction may have any non-zero length and is
 *   normalised as an rt_ray's; with RT_RADIANCE_UNIT_DIR it is unit already and its bits are used as
 *   they stand (with RT_EXEC_F32: rounded to float).  time as rt_ray.time (24 bits).
 * cs: only max_recursion_depth, the background and the redirect targets are read; the camera
 *   geometry, image_width and samples_per_pixel are not.  max_recursion_depth <= 0: every sample is 0.
 * rt_radiance: rgb is the mean over ALL samples the workspace holds for the ray, resolved as a film
 *   pixel holding that many samples is (rt_film_resolve).  status 1: ok; -1: a malformed ray (a
 *   non-finite field, a zero direction, time outside [0, 1]): nothing was added for it and rgb is 0;
 *   2: some sample was NaN or out of the sums' range: rgb is NaN, as a film's flagged pixel.
 * The workspace belongs to the caller: rt_scene_radiance_workspace_bytes(n, ex->flags) bytes, 16-byte
 *   aligned, on the scene's device.  Per ray it holds W + 1 64-bit words, W = 6 (3 with RT_EXEC_F32):
 *   the W fixed-point sum words in the film state's order (the high words of R, G, B in units of
 *   2^-32; binary64: then their low words, units of 2^-64), then one word whose low 32 bits are the
 *   NaN flag and whose high 32 bits are the ray's sample count.  Behind the n rays' words lie 16 bytes
 *   of the kernel's own (its work cursor).  Without RT_RADIANCE_ACCUMULATE the call zeroes the
 *   workspace on the stream first; with it the call adds onto what the workspace holds (of the same
 *   n and precision), and rgb is the mean over the accumulated count.  Sums are integers: the result
 *   does not depend on the schedule, and k calls of one sample accumulate to one call of k.
 * A wave takes 64 consecutive (ray, sample chunk) items in the caller's ray order and waits for its
 *   longest path: that order is the kernel's coherence.  rt_scene_radiance_ordered (below) takes the
 *   rays in a coherence order instead; nothing is compacted and no single lane is refilled.
 *
 * rt_scene_radiance_async: d_rays / d_out / d_workspace are device buffers on the scene's device;
 *   enqueues on hip_stream.  ex gives the precision and must name no device list; the first call of
 *   a precision uploads that precision's records and is not asynchronous, after that nothing is
 *   allocated.  n == 0 is a no-op.  A traversal-stack overflow sets a word of the scene that stays
 *   set until rt_scene_radiance_status reads it (as rt_scene_cast_status).
 * rt_scene_radiance: the same from and to host buffers, synchronous; host_workspace may be NULL (the
 *   call allocates and frees its own: RT_RADIANCE_ACCUMULATE then adds onto zeros) or a host copy of
 *   the rays' words (n x (W + 1) words, without the tail), read before the call with
 *   RT_RADIANCE_ACCUMULATE and written after it.  RT_E_STACK (results written) on overflow.
 * rt_scene_camera_rays_async: for every pixel of cs's frame (rt_image_height(cs) x image_width,
 *   row-major, one shard) the ray the render makes for sample `sample` of that pixel: origin, unit
 *   direction (FP32 values widened exactly), time = the time word's 24 bits, stream = the global
 *   pixel id, sample0 = sample.  Traced with RT_RADIANCE_UNIT_DIR and the same seed and precision
 *   they return the render's samples; through rt_scene_cast they give G-buffers aligned with them.
 * rt_scene_camera_rays: the same into a host buffer, synchronous.
 * Null arguments, n < 0, n_samples <= 0 or above 2^24, unknown flags, a device list in ex and
 *   n x n_samples at or above 2^31 - 2^18 (the item ids of one launch) are RT_E_INVALID before any device call. */
#define RT_RADIANCE_UNIT_DIR 1
#define RT_RADIANCE_ACCUMULATE 2
typedef struct rt_path_ray {      /* 64 bytes, four 16-byte vectors */
  double origin[3];
  double dir[3];
  double time;                    /* [0, 1] */
  uint32_t stream;                /* Philox counter word 0: where a render puts the global pixel id */
  uint32_t sample0;               /* first sample index of this ray in this call */
} rt_path_ray;
typedef struct rt_radiance {      /* 32 bytes */
  double rgb[3];
  int32_t status;                 /* 1 ok, -1 malformed ray, 2 flagged */
  uint32_t samples;               /* samples the workspace holds for this ray after the call */
} rt_radiance;
size_t rt_scene_radiance_workspace_bytes(int64_t n, int32_t exec_flags);
int rt_scene_radiance_async(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                            const rt_path_ray* d_rays, rt_radiance* d_out, void* d_workspace, int64_t n, int32_t n_samples,
                            int32_t flags, void* hip_stream);
int rt_scene_radiance(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                      const rt_path_ray* host_rays, rt_radiance* host_out, void* host_workspace, int64_t n,
                      int32_t n_samples, int32_t flags);
int rt_scene_radiance_status(const rt_device_scene* s, int32_t* overflowed);
int rt_scene_camera_rays_async(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                               int32_t sample, rt_path_ray* d_rays, void* hip_stream);
int rt_scene_camera_rays(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                         int32_t sample, rt_path_ray* host_rays);

/* Ray orders: sort a batch by a coherence key once, trace it in that order as often as needed.
 *
 * The queries above give lane i record i.  An ORDER is a permutation of [0, n) as uint32: in the
 * ordered calls lane i takes record order[i] and writes result order[i], so every buffer keeps the
 * caller's indexing and the results are those of the unordered call, bit for bit (a radiance query's
 * workspace words too: RT_RADIANCE_ACCUMULATE mixes ordered and unordered calls freely).  Only the
 * grouping of rays into waves changes.
 *
 * rt_scene_ray_order_async computes the order of a batch on the device: a 30-bit key per ray — the
 *   origin's cell in a 64^3 grid over the box of the batch's own origins (Morton order), then the
 *   direction's cell in a 64 x 64 octahedral map (Morton order); DESIGN section 4g has the formula —
 *   and a stable radix sort of (key, index).  The key reads only origin and dir, which rt_ray
 *   (RT_ORDER_RAYS) and rt_path_ray (RT_ORDER_PATH_RAYS) share; a record with a non-finite value there
 *   or a zero direction sorts last.  Equal keys keep their index order, so the order is a pure
 *   function of the records.  It depends on no scene: s only names the device.  d_rays, d_order (n
 *   uint32) and d_workspace (rt_ray_order_workspace_bytes(n) bytes, 16-byte aligned) are device
 *   buffers; everything is enqueued on hip_stream, nothing is allocated or read back.  An order stays
 *   valid while origins and directions do: tmin / tmax / time / sample0 may change between uses.
 * rt_scene_ray_order: the same from and to host buffers, synchronous.
 * rt_scene_cast_ordered_async / rt_scene_radiance_ordered_async: rt_scene_cast_async /
 *   rt_scene_radiance_async with d_order, n uint32 on the device.  The order is trusted, except that
 *   an entry >= n is skipped (nothing is read or written for it); an index that is missing from the
 *   order leaves its result as it was, a repeated one is computed twice (a radiance query then adds
 *   its samples twice).
 * rt_scene_cast_ordered / rt_scene_radiance_ordered: the synchronous forms.  host_order NULL: the
 *   call computes the order on the device and uses it, without a host round trip; otherwise it must
 *   be a permutation of [0, n) (RT_E_INVALID if not).
 * Status words, RT_E_STACK and the argument checks are the unordered calls'; in addition null
 *   pointers, n < 0, n >= 2^31 and an unknown kind are RT_E_INVALID before any device call; n == 0 is
 *   a no-op. */
#define RT_ORDER_RAYS 0        /* records are rt_ray */
#define RT_ORDER_PATH_RAYS 1   /* records are rt_path_ray */
size_t rt_ray_order_workspace_bytes(int64_t n);
int rt_scene_ray_order_async(const rt_device_scene* s, const void* d_rays, int64_t n, int32_t kind, uint32_t* d_order,
                             void* d_workspace, void* hip_stream);
int rt_scene_ray_order(const rt_device_scene* s, const void* host_rays, int64_t n, int32_t kind, uint32_t* host_order);
int rt_scene_cast_ordered_async(const rt_device_scene* s, const rt_exec* ex, const rt_ray* d_rays, rt_hit* d_hits, int64_t n,
                                int32_t flags, const uint32_t* d_order, void* hip_stream);
int rt_scene_cast_ordered(const rt_device_scene* s, const rt_exec* ex, const rt_ray* host_rays, rt_hit* host_hits, int64_t n,
                          int32_t flags, const uint32_t* host_order);
int rt_scene_radiance_ordered_async(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                                    const rt_path_ray* d_rays, rt_radiance* d_out, void* d_workspace, int64_t n,
                                    int32_t n_samples, int32_t flags, const uint32_t* d_order, void* hip_stream);
int rt_scene_radiance_ordered(const rt_device_scene* s, const rt_exec* ex, const rt_camera_settings* cs, uint64_t seed,
                              const rt_path_ray* host_rays, rt_radiance* host_out, void* host_workspace, int64_t n,
                              int32_t n_samples, int32_t flags, const uint32_t* host_order);

#ifdef __cplusplus
}
#endif

#endif /* RT_AMD_H */
