// rt_emu.cpp — TEST TOOLING: the device logic of raytrace_amd/csrc/rt_trace.h compiled for
// the host, so the kernel's algorithm can be checked against the FP64 oracle without a GPU
// and kernel faults can be reproduced on the CPU.  Never linked into librt_amd.so.
#define RT_HOST_EMU 1
#include <pthread.h>

#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt.h"
#include "../../raytrace_amd/csrc/rt_internal.h"
#include "../../raytrace_amd/csrc/rt_kernel_class.h"
#include "../target_defer/kp_members.h"
// The device's FP32 reciprocal (v_rcp_f32) is within 1 ulp of 1/x, not correctly rounded:
// rt_emu_set_rcp_ulps(k) makes the emulator's reciprocal the IEEE result moved k ulps (k < 0:
// toward -inf), so the node test's conservativeness check covers both roundings the device can
// produce (tests/test_node_test.py).
namespace rt_emu {
int rcp_ulps = 0;
}
static inline float rt_emu_rcpf(float x) {
  float r = 1.0f / x;
  for (int k = rt_emu::rcp_ulps; k > 0; --k) r = std::nextafter(r, HUGE_VALF);
  for (int k = rt_emu::rcp_ulps; k < 0; ++k) r = std::nextafter(r, -HUGE_VALF);
  return r;
}
#define RT_RCPF(x) rt_emu_rcpf(x)
// The element-wise probes of tests/device_probe/probe_body.h on host arrays (rt_emu_probe_<name>_f32
// / _f64): the same entry points tests/device_probe/rt_probe.hip gives the device, as plain loops.
#define RT_PROBE_CAT2(a, b) a##b
#define RT_PROBE_CAT(a, b) RT_PROBE_CAT2(a, b)
#define RT_PROBE_DEFINE(name, params, args)                                                      \
  extern "C" int RT_PROBE_CAT(rt_emu_probe_##name, RT_PROBE_SFX)(int n, RT_PROBE_UNPACK params) { \
    for (int i = 0; i < n; ++i) pb_##name(i, RT_PROBE_UNPACK args);                              \
    return 0;                                                                                    \
  }
#define RT_F64 0
#include "../../raytrace_amd/csrc/rt_trace.h"
namespace emu32 {
#include "emu_body.h"
}  // namespace emu32
#define RT_PROBE_SFX _f32
namespace probe32 {
#include "../device_probe/probe_body.h"
}  // namespace probe32
#undef RT_PROBE_SFX
#undef RT_F64
#define RT_F64 1
#include "../../raytrace_amd/csrc/rt_trace.h"
namespace emu64 {
#include "emu_body.h"
}  // namespace emu64
#define RT_PROBE_SFX _f64
namespace probe64 {
#include "../device_probe/probe_body.h"
}  // namespace probe64
#undef RT_PROBE_SFX

namespace rt_emu {
thread_local long long counters[4];
}

extern "C" {
// the KernelParams bytes of a shade probe call (probe_body.h pb_shade_params), for both backends
long long rt_emu_probe_shade_params_f32(void* out, long long cap, const void* mats, int med_mat, uint32_t k0,
                                        uint32_t k1, int n_targets, const void* targets, const double* cfg) {
  return probe32::pb_shade_params(out, cap, mats, med_mat, k0, k1, n_targets, targets, cfg);
}
long long rt_emu_probe_shade_params_f64(void* out, long long cap, const void* mats, int med_mat, uint32_t k0,
                                        uint32_t k1, int n_targets, const void* targets, const double* cfg) {
  return probe64::pb_shade_params(out, cap, mats, med_mat, k0, k1, n_targets, targets, cfg);
}
}

namespace {
thread_local std::string g_err;
}  // namespace

extern "C" {
const char* rt_emu_last_error(void) { return g_err.c_str(); }

// counters (optional, 4 values): BVH nodes visited, primitives tested, segments, samples.
// f64 = 1: the binary64 kernel (out: doubles), else the FP32 kernel (out: floats)
int rt_emu_render(const rt_camera_settings* cs, const rt_scene* sc, uint64_t seed, const rt_exec* ex, void* out,
                  int nthreads, int chunk, long long* counters, int f64) {
  HostScene H;
  int rc = rt_host_build_scene(sc, H, g_err);
  if (rc) return rc;
  if (f64) return emu64::render(H, cs, seed, ex, (double*)out, nthreads, chunk, counters, g_err);
  return emu32::render(H, cs, seed, ex, (float*)out, nthreads, chunk, counters, g_err);
}
}

extern "C" {
void rt_emu_set_rcp_ulps(int k) { rt_emu::rcp_ulps = k; }

// the sin / cos table of rt_math64::sincos_turns as the compiler reads it: 2 * 128 doubles
int rt_emu_probe_sincos_table(double* out) {
  for (int k = 0; k < 2 * RT_SINCOS_TABLE_N; ++k) out[k] = rt_math64::rt_sincos_tab[k];
  return RT_SINCOS_TABLE_N;
}

// The binary64 kernel's FP32 BVH node test (rtk64::prep_ray + node_slabs_f32) for n rays, each
// against one box given as both children of a node: box = (xmin, xmax, ymin, ymax, zmin, zmax)
// floats, o / d / (tmin, tmax) doubles; accept[i] = 1 when the kernel would enter the box.
void rt_emu_node_test_f64(int n, const double* o, const double* d, const float* box, const double* tr, int* accept) {
  for (int i = 0; i < n; ++i) {
    rtk64::RayCtx R{};
    R.o = rtk64::f3{o[3 * i], o[3 * i + 1], o[3 * i + 2]};
    R.d = rtk64::f3{d[3 * i], d[3 * i + 1], d[3 * i + 2]};
    rtk64::prep_ray(R);
    const float* b = box + 6 * i;
    const rtk64::v4f n0{b[0], b[1], b[2], b[3]}, n1{b[0], b[1], b[2], b[3]}, n2{b[4], b[5], b[4], b[5]};
    float ln, lf, rn, rf;
    rtk64::node_slabs_f32(R, n0, n1, n2, (float)tr[2 * i], (float)tr[2 * i + 1], ln, lf, rn, rf);
    accept[i] = (ln <= lf ? 1 : 0) | (rn <= rf ? 2 : 0);
  }
}

// scene summary of the host build (test tooling): n_nodes, surface_nodes, max_depth, n_prims, flat
int rt_emu_scene_info(const rt_scene* sc, int* info) {
  HostScene H;
  int rc = rt_host_build_scene(sc, H, g_err);
  if (rc) return rc;
  info[0] = H.n_nodes;
  info[1] = H.surface_nodes;
  info[2] = H.max_depth;
  info[3] = H.n_prims;
  info[4] = H.flat ? 1 : 0;
  info[5] = H.n_boxes;
  // BVH scenes: primitives tested before the surface BVH (prefix records + box-group faces)
  int pre = 0;
  if (!H.flat) {
    const DevFlatSet& F = H.flat_sets[0];
    pre = F.end - F.first;
    for (int b = F.box_first; b < F.box_end; ++b)
      for (int f = 0; f < 6; ++f) pre += ((H.f32.boxes[b].ord_code >> (5 * f)) & 31) != RT_BOX_NO_FACE;
  }
  info[6] = pre;
  info[7] = H.leaf_kind;
  return RT_OK;
}
}

// Which kernel class a scene gets (test tooling, tests/class_scenes.py): the product's own
// rt_host_variant and rt_class_of, passed through.
extern "C" {
// the variant code the host gives this scene (rt_host_variant(H)) in *variant
int rt_emu_scene_variant(const rt_scene* sc, int* variant) {
  HostScene H;
  int rc = rt_host_build_scene(sc, H, g_err);
  if (rc) return rc;
  *variant = rt_host_variant(H);
  return RT_OK;
}
// the variant code of a scene's properties one by one (the scalar rt_host_variant)
int rt_emu_variant_of(int flat, int n_media, int noise, int mats, int tex, int inst, int leaf_kind, int media_late,
                      int stack_depth) {
  return rt_host_variant(flat != 0, n_media, noise != 0, mats != 0, tex != 0, inst != 0, leaf_kind, media_late != 0,
                         stack_depth);
}
// rt_class_of(f64, variant) as out[0..6] = var, tex, media, mats, inst, leaf, narrow; out[7] = rt_class_block,
// out[8] = rt_class_compiled of that class
void rt_emu_class_of(int f64, int variant, int* out) {
  const KernelClass c = rt_class_of(f64 != 0, variant);
  const int f[9] = {c.var, c.tex, c.media, c.mats, c.inst, c.leaf, c.narrow, rt_class_block(f64 != 0, c),
                    rt_class_compiled(f64 != 0, c)};
  for (int k = 0; k < 9; ++k) out[k] = f[k];
}
}

// The kernel arguments of a render (test tooling, tests/test_render_params.py): every member of
// KernelParams (../target_defer/kp_members.h) by name with its values as doubles (exact for every
// int, uint32, float and double), records field by field (no padding), pointers as null (0) or not (1).
namespace {
struct ParamsDump {
  const char** names;
  int* counts;
  double* values;
  int cap_members, cap_values, m = 0, v = 0;
  template <class T>
  void add(const T& x) {  // T: an arithmetic type or a pointer
    if (v < cap_values) {
      if constexpr (std::is_pointer_v<T>) values[v] = x != nullptr;
      else values[v] = (double)x;
    }
    ++v;
  }
  template <class T, size_t N>
  void add(const T (&a)[N]) {
    for (const T& x : a) add(x);
  }
  void add(const FastDiv& d) { add(d.m), add(d.s), add(d.d), add(d.pad); }
  void add(const DevFlatSet& d) {
    add(d.first), add(d.end_quad), add(d.end_tri), add(d.end_sphere), add(d.end), add(d.box_first), add(d.box_end),
        add(d.pad);
  }
  template <class R>
  void add(const DevMediumT<R>& d) {
    add(d.neg_inv_density), add(d.material), add(d.root), add(d.alias_surface);
  }
  template <class R>
  void add(const DevTargetT<R>& d) {
    add(d.q), add(d.u), add(d.v), add(d.n), add(d.wa), add(d.wb), add(d.cr), add(d.prob), add(d.thresh), add(d.prob_icr);
  }
  template <class R>
  void add(const DevCameraT<R>& d) {
    add(d.center), add(d.top_left), add(d.pixel_u), add(d.pixel_v), add(d.disk_u), add(d.disk_v), add(d.bg0), add(d.bg1);
    add(d.width), add(d.height), add(d.spp), add(d.max_depth), add(d.bg_kind), add(d.pad);
  }
  template <class T>
  void member(const char* name, const T& x) {
    const int v0 = v;
    add(x);
    if (m < cap_members) names[m] = name, counts[m] = v - v0;
    ++m;
  }
  template <class R>
  void all(const KernelParamsT<R>& P) {
#define RT_EMU_KP_ONE(x) member(#x, P.x);
    RT_TD_KP_MEMBERS(RT_EMU_KP_ONE)
#undef RT_EMU_KP_ONE
  }
};
}  // namespace

extern "C" {
// the arguments emu32 / emu64 render() gives the lane loop for this scene, settings and rt_exec;
// names / counts: one entry per member (at most cap_members are written), values: the members'
// values back to back (at most cap_values); n_out[0] = members, n_out[1] = values
int rt_emu_render_params(const rt_camera_settings* cs, const rt_scene* sc, uint64_t seed, const rt_exec* ex, int f64,
                         int chunk, const char** names, int* counts, int cap_members, double* values, int cap_values,
                         int* n_out) {
  HostScene H;
  int rc = rt_host_build_scene(sc, H, g_err);
  if (rc) return rc;
  ParamsDump D{names, counts, values, cap_members, cap_values};
  const int variant = rt_host_variant(H);
  if (f64) {
    double out = 0;
    rtk64::KernelParams P;
    if ((rc = emu64::params(H, variant, cs, seed, ex, &out, chunk, P, g_err))) return rc;
    D.all(P);
  } else {
    float out = 0;
    rtk::KernelParams P;
    if ((rc = emu32::params(H, variant, cs, seed, ex, &out, chunk, P, g_err))) return rc;
    D.all(P);
  }
  n_out[0] = D.m;
  n_out[1] = D.v;
  return RT_OK;
}
}

// Digest of the host build (test tooling): one (length, 64-bit FNV-1a) pair per item of HostScene,
// every Dev* record hashed field by field (struct padding is unspecified).
namespace {
struct Fnv {
  uint64_t h = 0xcbf29ce484222325ull;
  template <class T>
  void add(const T& v) {  // T: int, float or double
    unsigned char b[sizeof(T)];
    std::memcpy(b, &v, sizeof(T));
    for (unsigned char c : b) h = (h ^ c) * 0x100000001b3ull;
  }
  template <class T, size_t N>
  void add(const T (&a)[N]) {
    for (const T& v : a) add(v);
  }
  template <class R>
  void add(const DevMaterialT<R>& d) {
    add(d.kind), add(d.tex), add(d.param), add(d.tex_const), add(d.c0), add(d.pad);
  }
  template <class R>
  void add(const DevTextureT<R>& d) {
    add(d.kind), add(d.nu), add(d.nv), add(d.off), add(d.c0), add(d.c1), add(d.prm), add(d.pad);
  }
  template <class R>
  void add(const DevMediumT<R>& d) {
    add(d.neg_inv_density), add(d.material), add(d.root), add(d.alias_surface);
  }
  void add(const DevFlatSet& d) {
    add(d.first), add(d.end_quad), add(d.end_tri), add(d.end_sphere), add(d.end), add(d.box_first), add(d.box_end),
        add(d.pad);
  }
  template <class R>
  void add(const DevBoxT<R>& d) {
    add(d.sc), add(d.ord_base), add(d.a0), add(d.ord_code), add(d.a1), add(d.gid_base), add(d.a2), add(d.gid_code),
        add(d.prim_base), add(d.prim_code), add(d.pad);
  }
  template <class R>
  void add(const DevInstanceT<R>& d) {
    add(d.m), add(d.root), add(d.material), add(d.order), add(d.pad);
  }
};
struct Digest {
  uint64_t* out;
  int n = 0;
  template <class T>
  void item(const T* p, size_t len) {
    Fnv f;
    for (size_t i = 0; i < len; ++i) f.add(p[i]);
    out[2 * n] = len;
    out[2 * n + 1] = f.h;
    ++n;
  }
  template <class T>
  void item(const std::vector<T>& v) { item(v.data(), v.size()); }
};
template <class R>
void digest_arrays(const HostArraysT<R>& A, int n_media, Digest& D) {
  D.item(A.prims), D.item(A.prim_uv), D.item(A.flat_recs), D.item(A.motions), D.item(A.uvframes), D.item(A.texels);
  D.item(A.perlin_grad), D.item(A.prim_shade), D.item(A.mats), D.item(A.texs), D.item(A.boxes), D.item(A.instances);
  D.item(A.media, (size_t)n_media);
}
}  // namespace

extern "C" {
// RT_EMU_DIGEST_ITEMS = 31 items, two words each (length in elements, hash), in this order
// (tests/kernel_emu/emu.py DIGEST_ITEMS names them):
//   nodes, perlin_perm, prim_mat, flat_sets (all 1 + RT_MAX_MEDIA),
//   scalars (as ints, in declaration order: surface_root, n_media, n_nodes, n_prims, max_depth, n_boxes,
//     surface_nodes, flat, noise, uv_tex, leaf_exit_pct, leaf_exit_pct64, trav_exit_pct, trav_exit_pct64,
//     full_mats, n_instances, leaf_kind),
//   then for f32 and for f64: prims, prim_uv, flat_recs, motions, uvframes, texels, perlin_grad, prim_shade,
//     mats, texs, boxes, instances, media[0, n_media).
// Returns the build's error (message: rt_emu_last_error) or RT_OK; n: words `out` holds (>= 62).
int rt_emu_scene_digest(const rt_scene* sc, uint64_t* out, int n) {
  if (!out || n < 2 * 31) return RT_E_INVALID;
  HostScene H;
  int rc = rt_host_build_scene(sc, H, g_err);
  if (rc) return rc;
  Digest D{out};
  D.item(H.nodes), D.item(H.perlin_perm), D.item(H.prim_mat);
  D.item(H.flat_sets, (size_t)(1 + RT_MAX_MEDIA));
  const int scalars[] = {H.surface_root, H.n_media,         H.n_nodes,         H.n_prims,       H.max_depth,
                         H.n_boxes,      H.surface_nodes,   H.flat,            H.noise,         H.uv_tex,
                         H.leaf_exit_pct, H.leaf_exit_pct64, H.trav_exit_pct,  H.trav_exit_pct64, H.full_mats,
                         H.n_instances,  H.leaf_kind};
  D.item(scalars, sizeof scalars / sizeof scalars[0]);
  digest_arrays(H.f32, H.n_media, D);
  digest_arrays(H.f64, H.n_media, D);
  return D.n == 31 ? RT_OK : RT_E_GENERIC;
}
}

// Read-only export of the host build's arrays by name (test tooling: the element-wise probes of
// tests/device_probe are fed the records the product's own builder makes).  The names are those of
// the digest above; a record array comes as the records' bytes, padding included.
namespace {
struct ArrayOut {
  const char* want;
  void* out;
  long long cap;
  long long* info;  // bytes, bytes per element
  bool found = false;
  template <class T>
  void item(const char* name, const T* p, size_t len) {
    if (std::strcmp(name, want) != 0) return;
    found = true;
    info[0] = (long long)(len * sizeof(T));
    info[1] = (long long)sizeof(T);
    if (out && info[0] <= cap && len) std::memcpy(out, p, len * sizeof(T));
  }
  template <class T>
  void item(const char* name, const std::vector<T>& v) { item(name, v.data(), v.size()); }
};
template <class R>
void export_arrays(const HostArraysT<R>& A, ArrayOut& O) {
  O.item("prims", A.prims), O.item("prim_uv", A.prim_uv), O.item("flat_recs", A.flat_recs);
  O.item("uvframes", A.uvframes), O.item("texels", A.texels), O.item("perlin_grad", A.perlin_grad);
  O.item("prim_shade", A.prim_shade), O.item("mats", A.mats), O.item("texs", A.texs), O.item("boxes", A.boxes);
}
}  // namespace

extern "C" {
// info[0] = the array's bytes, info[1] = bytes per element; the bytes are copied when out is not
// null and cap >= info[0].  An unknown name is RT_E_INVALID.
int rt_emu_scene_arrays(const rt_scene* sc, int f64, const char* name, void* out, long long cap, long long* info) {
  if (!name || !info) return RT_E_INVALID;
  HostScene H;
  int rc = rt_host_build_scene(sc, H, g_err);
  if (rc) return rc;
  ArrayOut O{name, out, cap, info};
  O.item("perlin_perm", H.perlin_perm);
  O.item("flat_sets", H.flat_sets, (size_t)(1 + RT_MAX_MEDIA));
  if (f64) export_arrays(H.f64, O);
  else export_arrays(H.f32, O);
  if (!O.found) {
    g_err = std::string("rt_emu_scene_arrays: no array named ") + name;
    return RT_E_INVALID;
  }
  return RT_OK;
}
}
