// rt_build.cpp — host-side scene image and launch parameters (no HIP calls).
//
//  * validates the flattened scene of include/rt.h,
//  * precomputes the plane-shape frame of Geometry.hs:117-131 (unit normal n, and the
//    vectors wa = v x nS, wb = nS x u so that a = nS.((p-q) x v) = (p-q).wa and
//    b = nS.(u x (p-q)) = (p-q).wb) in binary64 and rounds it once to FP32,
//  * builds one BVH per primitive set (surfaces, then each medium's boundary),
//  * evaluates the camera set-up of Ray.hs:122-155 in binary64, in the reference's order.
//
// rt_host_build_scene is a driver over stages, each a free function of its inputs:
//   1 read_knobs         the RT_AMD_* experiment knobs, once per call (nothing else reads the environment)
//   2 validate_tables, validate_geometry   every check that needs only the caller's tables, and the scene flags
//   3 gather_sets        each primitive's and placement's bounds, per set and per instanced object
//   4 medium_aliases     media whose boundary is the surface set
//   5 split_prefix       the large surface primitives tested before the BVH, and the set without them
//   6 build_hierarchies  one BVH per set and per object: nodes, record order, roots, depths
//   7 layout_records     flat sets grouped by class, box groups and their codes, slots
//   8 fill_geometry, fill_shading   the device records of both precisions
//   9 traversal_policy   the leaf kind and the exit percentages of the scene
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <utility>

#include "../../include/rt.h"
#include "rt_bvh.h"
#include "rt_encode8_table.h"
#include "rt_internal.h"
#include "rt_kernel_class.h"
#include "rt_order.h"

const char* rt_knob(const char* name) {
  const char* on = std::getenv("RT_AMD_EXPERIMENTS");
  if (!on || !*on || std::atoi(on) == 0) return nullptr;
  return std::getenv(name);
}

namespace {

struct d3 {
  double x, y, z;
};
inline d3 D3(const double* p) { return {p[0], p[1], p[2]}; }
inline d3 operator+(d3 a, d3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline d3 operator-(d3 a, d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline d3 operator-(d3 a) { return {-a.x, -a.y, -a.z}; }
inline d3 smul(double s, d3 a) { return {s * a.x, s * a.y, s * a.z}; }
inline d3 divs(d3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
inline double dot(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline d3 cross(d3 a, d3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline d3 normalize_hs(d3 v) {  // linear's normalize
  double l = dot(v, v);
  if (std::fabs(l) <= 1e-12 || std::fabs(1 - l) <= 1e-12) return v;
  return divs(v, std::sqrt(l));
}
template <class R>
inline void put3(R* dst, d3 v) {
  dst[0] = (R)v.x;
  dst[1] = (R)v.y;
  dst[2] = (R)v.z;
}
inline bool finite_n(const double* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}
// an int stored in an R array: its 32-bit pattern in the low word (rt_trace.h RT_R2I)
template <class R>
inline R ibits(int v);
template <>
inline float ibits<float>(int v) {
  float f;
  std::memcpy(&f, &v, 4);
  return f;
}
template <>
inline double ibits<double>(int v) {
  const uint64_t u = (uint32_t)v;
  double d;
  std::memcpy(&d, &u, 8);
  return d;
}

int fail(std::string& err, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int fail(std::string& err, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  err = buf;
  return code;
}


// Box groups (rt_internal.h DevBox): parallelograms that are full faces of one rectangular box.
struct BoxFound {
  d3 c, a[3];       // corner, axis_k / L_k
  int face[6];      // caller primitive index of face f = 2 axis + side, -1 if absent
};

// Among `rects` (caller indices of static parallelograms of one set) find boxes with >= 3 faces;
// every primitive is used at most once.  Binary64, relative tolerance 1e-9 of the box size.
std::vector<BoxFound> find_boxes(const rt_scene* sc, const std::vector<int>& rects) {
  std::vector<BoxFound> out;
  const int n = (int)rects.size();
  std::vector<char> used(n, 0);
  auto corners = [&](int i, d3* c4) {
    const double* p = sc->prims[rects[i]].p;
    d3 q = D3(p), u = D3(p + 3), v = D3(p + 6);
    c4[0] = q;
    c4[1] = q + u;
    c4[2] = q + v;
    c4[3] = q + u + v;
  };
  auto is_rect = [&](int i) {
    const double* p = sc->prims[rects[i]].p;
    d3 u = D3(p + 3), v = D3(p + 6);
    double lu = std::sqrt(dot(u, u)), lv = std::sqrt(dot(v, v));
    return lu > 0 && lv > 0 && std::fabs(dot(u, v)) <= 1e-12 * lu * lv;
  };
  for (int i = 0; i < n; ++i) {
    if (used[i] || !is_rect(i)) continue;
    const double* pi = sc->prims[rects[i]].p;
    d3 ui = D3(pi + 3), vi = D3(pi + 6);
    d3 e0 = divs(ui, std::sqrt(dot(ui, ui))), e1 = divs(vi, std::sqrt(dot(vi, vi))), e2 = cross(e0, e1);
    e2 = divs(e2, std::sqrt(dot(e2, e2)));
    d3 ci[4];
    corners(i, ci);
    for (int j = 0; j < n; ++j) {
      if (j == i || used[j] || !is_rect(j)) continue;
      d3 cj[4];
      corners(j, cj);
      const double h = dot(e2, cj[0] - ci[0]);
      const double size = std::sqrt(std::max(dot(ui, ui), dot(vi, vi)));
      const double tol = 1e-9 * std::max(size, std::fabs(h));
      if (!(std::fabs(h) > tol)) continue;
      bool match = true;  // j = i translated by h e2, corner for corner (as sets)
      for (int a = 0; a < 4 && match; ++a) {
        d3 t = cj[a] - smul(h, e2);
        bool any = false;
        for (int b = 0; b < 4; ++b) {
          d3 d = t - ci[b];
          any = any || std::sqrt(dot(d, d)) <= tol;
        }
        match = any;
      }
      if (!match) continue;
      // the box spanned by i and j, in the frame (e0, e1, e2)
      const d3 E[3] = {e0, e1, e2};
      double lo[3], hi[3];
      for (int k = 0; k < 3; ++k) {
        lo[k] = INFINITY;
        hi[k] = -INFINITY;
        for (int a = 0; a < 4; ++a) {
          for (const d3& p : {ci[a], cj[a]}) {
            double x = dot(E[k], p - ci[0]);
            lo[k] = std::min(lo[k], x);
            hi[k] = std::max(hi[k], x);
          }
        }
      }
      BoxFound B;
      B.c = ci[0] + smul(lo[0], e0) + smul(lo[1], e1) + smul(lo[2], e2);
      for (int k = 0; k < 3; ++k) B.a[k] = divs(E[k], hi[k] - lo[k]);
      for (int f = 0; f < 6; ++f) B.face[f] = -1;
      std::vector<int> members;
      for (int m = 0; m < n; ++m) {
        if (used[m] || !is_rect(m)) continue;
        d3 cm[4];
        corners(m, cm);
        double sc4[4][3];
        for (int a = 0; a < 4; ++a)
          for (int k = 0; k < 3; ++k) sc4[a][k] = dot(B.a[k], cm[a] - B.c);
        const double et = 1e-9;
        auto near01 = [&](double x, int& bit) {
          if (std::fabs(x) <= et) return bit = 0, true;
          if (std::fabs(x - 1) <= et) return bit = 1, true;
          return false;
        };
        int face = -1;
        for (int ax = 0; ax < 3 && face < 0; ++ax) {
          int side0 = -1, mask = 0;
          bool ok = true;
          for (int a = 0; a < 4 && ok; ++a) {
            int bits[3];
            for (int k = 0; k < 3 && ok; ++k) ok = near01(sc4[a][k], bits[k]);
            if (!ok) break;
            if (side0 < 0) side0 = bits[ax];
            ok = bits[ax] == side0;
            const int b1 = bits[(ax + 1) % 3], b2 = bits[(ax + 2) % 3];
            mask |= 1 << (b1 * 2 + b2);
          }
          if (ok && mask == 15) face = 2 * ax + side0;  // the four corners of that face
        }
        if (face >= 0 && B.face[face] < 0) {
          B.face[face] = rects[m];
          members.push_back(m);
        }
      }
      if (members.size() >= 3) {
        for (int m : members) used[m] = 1;
        out.push_back(B);
        break;
      }
    }
  }
  return out;
}

struct BoxCodes {
  int ord_base, ord_code, gid_base, gid_code, prim_base, prim_code;
};

// ---- stage 1: the experiment knobs of the build (rt_internal.h rt_knob: null without
// RT_AMD_EXPERIMENTS), read once per call; no other stage touches the environment
struct BuildKnobs {
  bool no_alias = false, no_prefix = false, no_box = false;
  std::optional<double> prefix_area, prefix_shrink;
  std::optional<int> leaf_max, leaf_exit_pct, trav_pct;  // clamped to their ranges
};

BuildKnobs read_knobs() {
  BuildKnobs K;
  auto on = [](const char* name) {
    const char* e = rt_knob(name);
    return e && atoi(e);
  };
  K.no_alias = on("RT_AMD_NO_ALIAS");    // experiments: always traverse boundaries
  K.no_prefix = on("RT_AMD_NO_PREFIX");  // experiments: everything in the BVH
  K.no_box = on("RT_AMD_NO_BOX");        // experiments: every face its own test
  if (const char* e = rt_knob("RT_AMD_PREFIX_AREA")) K.prefix_area = atof(e);
  if (const char* e = rt_knob("RT_AMD_PREFIX_SHRINK")) K.prefix_shrink = atof(e);
  if (const char* e = rt_knob("RT_AMD_LEAF_MAX")) K.leaf_max = std::max(1, std::min(RT_FLAT_MAX, atoi(e)));
  if (const char* e = rt_knob("RT_AMD_LEAF_EXIT_PCT")) K.leaf_exit_pct = std::max(1, std::min(100, atoi(e)));
  if (const char* e = rt_knob("RT_AMD_TRAV_PCT")) K.trav_pct = std::max(0, std::min(100, atoi(e)));
  return K;
}

// ---- stage 2: validation of the caller's tables (reads only `sc`; the first failing check, in
// this order, is the error a scene reports)
struct SceneFlags {
  bool noise = false;      // some texture is a noise / marble texture
  bool full_mats = false;  // some material is not lightSource / pitchBlack / lambertian
  bool uv_tex = false;     // some material reads a non-constant texture
};

// two-level instancing: instanced objects (prims with set RT_SET_BLAS(b)) and their placements
int n_objects(const rt_scene* sc) {
  int n_blas = 0;
  for (int i = 0; i < sc->n_prims; ++i)
    if (sc->prims[i].set < 0) n_blas = std::max(n_blas, -sc->prims[i].set);
  return n_blas;
}

int validate_tables(const rt_scene* sc, SceneFlags& flags, std::string& err) {
  if (!sc) return fail(err, RT_E_INVALID, "null scene");
  if (sc->n_prims < 0 || sc->n_media < 0 || sc->n_materials < 0 || sc->n_textures < 0 || sc->n_motions < 0 ||
      sc->n_uvframes < 0)
    return fail(err, RT_E_INVALID, "negative count");
  if (sc->n_media > RT_MAX_MEDIA)
    return fail(err, RT_E_UNSUPPORTED, "%d media (at most %d)", sc->n_media, RT_MAX_MEDIA);
  if ((sc->n_prims && !sc->prims) || (sc->n_media && !sc->media) || (sc->n_materials && !sc->materials) ||
      (sc->n_textures && !sc->textures) || (sc->n_motions && !sc->motions) || (sc->n_uvframes && !sc->uvframes))
    return fail(err, RT_E_INVALID, "null array with nonzero count");
  if (sc->n_texels < 0 || (sc->n_texels && !sc->texels)) return fail(err, RT_E_INVALID, "bad texel array");
  for (int i = 0; i < sc->n_textures; ++i) {
    const rt_texture& t = sc->textures[i];
    if (t.kind < RT_TEX_CONSTANT || t.kind > RT_TEX_MARBLE)
      return fail(err, RT_E_UNSUPPORTED, "texture %d: kind %d is not evaluated on the device", i, t.kind);
    if (!finite_n(t.c0, 3) || !finite_n(t.c1, 3)) return fail(err, RT_E_INVALID, "texture %d: non-finite colour", i);
    if (!finite_n(t.params, 8)) return fail(err, RT_E_INVALID, "texture %d: non-finite parameters", i);
    if (t.kind == RT_TEX_IMAGE &&
        (t.nu <= 0 || t.nv <= 0 || t.image < 0 || (long long)t.image + (long long)t.nu * t.nv > sc->n_texels))
      return fail(err, RT_E_INVALID, "texture %d: image %dx%d at texel %d exceeds the %d texels", i, t.nu, t.nv,
                  t.image, sc->n_texels);
    if (t.kind == RT_TEX_NOISE && t.nu < 0) return fail(err, RT_E_INVALID, "texture %d: negative noise layers", i);
    if (t.kind == RT_TEX_NOISE || t.kind == RT_TEX_MARBLE) flags.noise = true;
  }
  if (flags.noise) {
    if (!sc->perlin) return fail(err, RT_E_INVALID, "noise / marble textures need rt_scene.perlin");
    for (int a = 0; a < 3; ++a)
      for (int k = 0; k < 256; ++k)
        if (sc->perlin->perm[a][k] < 0 || sc->perlin->perm[a][k] > 255)
          return fail(err, RT_E_INVALID, "perlin permutation entry out of [0, 255]");
    for (int k = 0; k < 256; ++k)
      if (!finite_n(sc->perlin->grad[k], 3)) return fail(err, RT_E_INVALID, "non-finite perlin gradient");
  }
  for (int i = 0; i < sc->n_materials; ++i) {
    const rt_material& m = sc->materials[i];
    if (m.kind != RT_MAT_LIGHT_SOURCE && m.kind != RT_MAT_PITCH_BLACK && m.kind != RT_MAT_LAMBERTIAN)
      flags.full_mats = true;
    if (m.texture >= 0 && m.texture < sc->n_textures && sc->textures[m.texture].kind != RT_TEX_CONSTANT)
      flags.uv_tex = true;
    if (m.kind < 0 || m.kind > RT_MAT_ANISOTROPIC)
      return fail(err, RT_E_UNSUPPORTED, "material %d: kind %d", i, m.kind);
    if (m.texture < 0 || m.texture >= sc->n_textures)
      return fail(err, RT_E_INVALID, "material %d: bad texture index", i);
  }
  for (int k = 0; k < sc->n_media; ++k) {
    const rt_medium& m = sc->media[k];
    if (!(m.density > 0) || !std::isfinite(m.density))
      return fail(err, RT_E_INVALID, "medium %d: density must be > 0", k);
    if (m.material < 0 || m.material >= sc->n_materials) return fail(err, RT_E_INVALID, "medium %d: bad material", k);
  }
  return RT_OK;
}

// the placements, then the primitives (each with its motion)
int validate_geometry(const rt_scene* sc, std::string& err) {
  const int n_sets = 1 + sc->n_media;
  if (sc->n_instances < 0 || (sc->n_instances && !sc->instances)) return fail(err, RT_E_INVALID, "bad instance array");
  const int n_blas = n_objects(sc);
  for (int k = 0; k < sc->n_instances; ++k) {
    const rt_instance& I = sc->instances[k];
    if (I.blas < 0 || I.blas >= n_blas) return fail(err, RT_E_INVALID, "instance %d: object %d has no leaves", k, I.blas);
    if (I.material < -1 || I.material >= sc->n_materials) return fail(err, RT_E_INVALID, "instance %d: bad material", k);
    if (!finite_n(I.m, 12)) return fail(err, RT_E_INVALID, "instance %d: non-finite transform", k);
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        const double d = I.m[a] * I.m[b] + I.m[4 + a] * I.m[4 + b] + I.m[8 + a] * I.m[8 + b];
        if (std::fabs(d - (a == b ? 1.0 : 0.0)) > 1e-9)
          return fail(err, RT_E_UNSUPPORTED, "instance %d: transform is not rigid (Geometry.hs:379-381)", k);
      }
  }
  for (int i = 0; i < sc->n_prims; ++i) {
    const rt_prim& p = sc->prims[i];
    if (p.kind < RT_PRIM_SPHERE || p.kind > RT_PRIM_TRIANGLE) return fail(err, RT_E_INVALID, "prim %d: bad kind", i);
    if (p.set >= n_sets) return fail(err, RT_E_INVALID, "prim %d: bad set %d", i, p.set);
    if (p.set == 0 && (p.material < 0 || p.material >= sc->n_materials))
      return fail(err, RT_E_INVALID, "prim %d: surface without a valid material", i);
    if (p.set < 0 && (p.material < -1 || p.material >= sc->n_materials))
      return fail(err, RT_E_INVALID, "prim %d: bad material", i);
    if (p.motion >= sc->n_motions || p.uvframe >= sc->n_uvframes)
      return fail(err, RT_E_INVALID, "prim %d: bad motion/uvframe index", i);
    if (!finite_n(p.p, p.kind == RT_PRIM_SPHERE ? 4 : 9))
      return fail(err, RT_E_INVALID, "prim %d: non-finite geometry", i);
    if (p.motion >= 0) {
      const rt_motion& m = sc->motions[p.motion];
      if (!finite_n(m.v0, 3) || !finite_n(m.v1, 3)) return fail(err, RT_E_INVALID, "motion %d non-finite", p.motion);
    }
  }
  return RT_OK;
}

// ---- stage 3: the primitive sets with their bounds
double box_area(const double* lo, const double* hi) {
  double d[3];
  for (int a = 0; a < 3; ++a) d[a] = std::max(0.0, hi[a] - lo[a]);
  return 2.0 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]);
}
struct Bounds {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  void grow(const double* l, const double* h) {  // a box
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(lo[a], l[a]);
      hi[a] = std::max(hi[a], h[a]);
    }
  }
  void grow(const double* p) { grow(p, p); }  // a point
  double area() const { return box_area(lo, hi); }
  BuildPrim item(int index, int inst) const {  // the BVH builder's record of a primitive or placement
    BuildPrim bp;
    bp.index = index;
    bp.inst = inst;
    std::copy(lo, lo + 3, bp.lo);
    std::copy(hi, hi + 3, bp.hi);
    return bp;
  }
};
Bounds bounds_of(const std::vector<BuildPrim>& prims) {
  Bounds b;
  for (const BuildPrim& p : prims) b.grow(p.lo, p.hi);
  return b;
}

// a primitive's box, swept over its motion (std::fmin / fmax here, std::min / max in Bounds: they
// differ on NaN and degenerate primitives reach this code)
Bounds prim_bounds(const rt_scene* sc, const rt_prim& p) {
  Bounds bp;
  if (p.kind == RT_PRIM_SPHERE) {
    double r = std::fabs(p.p[3]);
    for (int a = 0; a < 3; ++a) {
      bp.lo[a] = p.p[a] - r;
      bp.hi[a] = p.p[a] + r;
    }
  } else {
    for (int a = 0; a < 3; ++a) {
      double q = p.p[a], u = p.p[3 + a], v = p.p[6 + a];
      double c[4] = {q, q + u, q + v, q + u + v};
      int nc = p.kind == RT_PRIM_PARALLELOGRAM ? 4 : 3;
      bp.lo[a] = bp.hi[a] = c[0];
      for (int k = 1; k < nc; ++k) {
        bp.lo[a] = std::fmin(bp.lo[a], c[k]);
        bp.hi[a] = std::fmax(bp.hi[a], c[k]);
      }
    }
  }
  if (p.motion >= 0) {
    const rt_motion& m = sc->motions[p.motion];
    for (int a = 0; a < 3; ++a) {
      double lo = bp.lo[a], hi = bp.hi[a];
      bp.lo[a] = std::fmin(lo + m.v0[a], lo + m.v1[a]);
      bp.hi[a] = std::fmax(hi + m.v0[a], hi + m.v1[a]);
    }
  }
  return bp;
}

struct PrimSets {
  std::vector<std::vector<BuildPrim>> sets;       // [0] surfaces and placements, [k + 1] medium k's boundary
  std::vector<std::vector<BuildPrim>> blas_sets;  // per instanced object, in object space
};

int gather_sets(const rt_scene* sc, PrimSets& P, std::string& err) {
  const int n_blas = n_objects(sc);
  P.sets.assign(1 + sc->n_media, {});
  P.blas_sets.assign(n_blas, {});
  std::vector<char> blas_all_mats(n_blas, 1);
  for (int i = 0; i < sc->n_prims; ++i) {
    const rt_prim& p = sc->prims[i];
    if (p.set < 0 && p.material < 0) blas_all_mats[-1 - p.set] = 0;
    (p.set < 0 ? P.blas_sets[-1 - p.set] : P.sets[p.set]).push_back(prim_bounds(sc, p).item(i, -1));
  }
  for (int k = 0; k < sc->n_media; ++k)
    if (P.sets[k + 1].empty()) return fail(err, RT_E_INVALID, "medium %d has an empty boundary", k);
  // every placement is one item of the surface set, boxed by its object's box under the transform
  for (int k = 0; k < sc->n_instances; ++k) {
    const rt_instance& I = sc->instances[k];
    if (P.blas_sets[I.blas].empty()) return fail(err, RT_E_INVALID, "instance %d: object %d has no leaves", k, I.blas);
    if (I.material < 0 && !blas_all_mats[I.blas])
      return fail(err, RT_E_INVALID, "instance %d: a leaf of object %d has no material", k, I.blas);
    const Bounds obj = bounds_of(P.blas_sets[I.blas]);
    Bounds placed;
    for (int c = 0; c < 8; ++c) {
      const double x[3] = {(c & 1) ? obj.hi[0] : obj.lo[0], (c & 2) ? obj.hi[1] : obj.lo[1], (c & 4) ? obj.hi[2] : obj.lo[2]};
      double w[3];
      for (int a = 0; a < 3; ++a) w[a] = I.m[4 * a] * x[0] + I.m[4 * a + 1] * x[1] + I.m[4 * a + 2] * x[2] + I.m[4 * a + 3];
      placed.grow(w);
    }
    P.sets[0].push_back(placed.item(-1, k));
  }
  return RT_OK;
}

// ---- stage 4: media whose boundary is, leaf for leaf in depth-first order, the surface set (DevMedium)
std::vector<int> medium_aliases(const rt_scene* sc, const BuildKnobs& knobs) {
  std::vector<int> alias(sc->n_media, 0);
  // experiments: always traverse boundaries; the surface set also holds placements
  if (knobs.no_alias || sc->n_instances > 0) return alias;
  std::vector<std::vector<int>> by_set(1 + sc->n_media);
  for (int i = 0; i < sc->n_prims; ++i)
    if (sc->prims[i].set >= 0) by_set[sc->prims[i].set].push_back(i);  // instanced objects' leaves: not a set
  for (auto& v : by_set)
    std::stable_sort(v.begin(), v.end(), [&](int x, int y) { return sc->prims[x].order < sc->prims[y].order; });
  auto same = [&](const rt_prim& a, const rt_prim& b) {
    if (a.kind != b.kind || a.motion != b.motion || a.gid != b.gid || a.uvframe != b.uvframe) return false;
    for (int j = 0; j < 9; ++j)
      if (a.p[j] != b.p[j]) return false;
    return true;
  };
  for (int k = 0; k < sc->n_media; ++k) {
    const auto& a = by_set[0];
    const auto& b = by_set[k + 1];
    bool eq = !a.empty() && a.size() == b.size();
    for (size_t j = 0; eq && j < a.size(); ++j) eq = same(sc->prims[a[j]], sc->prims[b[j]]);
    alias[k] = eq ? 1 : 0;
  }
  return alias;
}

// the class of a primitive's test (rt_internal.h DevFlatSet): 0 parallelogram, 1 triangle, 2 sphere;
// in a flat set the moving primitives of any kind are class 3
int prim_class(const rt_prim& p, bool motion_is_a_class) {
  if (motion_is_a_class && p.motion >= 0) return 3;
  return p.kind == RT_PRIM_PARALLELOGRAM ? 0 : p.kind == RT_PRIM_TRIANGLE ? 1 : 2;
}

// ---- stage 5: the surface prefix
// Large-primitive prefix of the surface set (BVH scenes).  Primitives whose box is a large
// fraction of the whole set's (the Cornell walls around a mesh, demo1's ground sphere) overlap
// almost every ray and sit at the top of any BVH; taken out of it, they are tested first by
// the whole wave with wave-uniform records (scalar loads, like the flat kernel), and their
// closest hit then bounds the traversal of the remaining BVH (rt_trace.h prefix_hits).  The
// 64-bit closest-hit key carries each leaf's global depth-first order, so the result is the
// same closest hit, tie for tie.  Only static primitives; grouped by class like a flat set.
struct SurfacePrefix {
  std::vector<int> prims;  // caller indices, class-grouped
  int cnt[4] = {0, 0, 0, 0};  // per class (no moving primitives)
  std::vector<BuildPrim> rest;  // the surface set without them
};

// marks the members of `set` (the whole surface set) that the prefix takes
std::vector<char> select_prefix(const rt_scene* sc, const BuildKnobs& knobs, const std::vector<BuildPrim>& set) {
  auto is_static = [&](const BuildPrim& b) { return b.inst < 0 && sc->prims[b.index].motion < 0; };
  const double root_area = bounds_of(set).area();
  const double frac = knobs.prefix_area.value_or(RT_PREFIX_AREA);
  std::vector<std::pair<double, int>> big;  // (area, position in the set)
  for (size_t j = 0; j < set.size(); ++j) {
    const double a = box_area(set[j].lo, set[j].hi);
    if (is_static(set[j]) && a >= frac * root_area) big.push_back({-a, (int)j});
  }
  std::stable_sort(big.begin(), big.end());
  if (big.size() > RT_PREFIX_MAX) big.resize(RT_PREFIX_MAX);
  std::vector<char> taken(set.size(), 0);
  for (auto& b : big) taken[b.second] = 1;
  // then outliers: a primitive that alone holds a face of the remaining set's box out by a
  // lot (the Cornell light above the bunny: without it the BVH root shrinks to the bunny)
  const double shrink = knobs.prefix_shrink.value_or(RT_PREFIX_SHRINK);
  auto bounds_without = [&](int skip) {
    Bounds r;
    for (size_t j = 0; j < set.size(); ++j)
      if (!taken[j] && (int)j != skip) r.grow(set[j].lo, set[j].hi);
    return r;
  };
  for (int added = (int)big.size(); added < RT_PREFIX_MAX && shrink < 1.0; ++added) {
    const Bounds all = bounds_without(-1);
    const double a0 = all.area();
    int best_j = -1;
    double best_a = a0;
    for (size_t j = 0; j < set.size(); ++j) {  // candidates: the primitives on the box's faces
      const BuildPrim& b = set[j];
      bool extreme = false;
      for (int a = 0; a < 3; ++a) extreme = extreme || b.lo[a] == all.lo[a] || b.hi[a] == all.hi[a];
      if (taken[j] || !extreme || !is_static(b)) continue;
      const double a = bounds_without((int)j).area();
      if (a < best_a) {
        best_a = a;
        best_j = (int)j;
      }
    }
    if (best_j < 0 || !(best_a <= (1.0 - shrink) * a0)) break;
    taken[best_j] = 1;
  }
  return taken;
}

SurfacePrefix split_prefix(const rt_scene* sc, const BuildKnobs& knobs, std::vector<BuildPrim> surface) {
  SurfacePrefix out;
  if ((int)surface.size() <= RT_FLAT_MAX + RT_PREFIX_MAX || knobs.no_prefix) {
    out.rest = std::move(surface);
    return out;
  }
  const std::vector<char> taken = select_prefix(sc, knobs, surface);
  for (size_t j = 0; j < surface.size(); ++j) {
    if (taken[j])
      out.prims.push_back(surface[j].index);
    else
      out.rest.push_back(surface[j]);
  }
  auto cls = [&](int i) { return prim_class(sc->prims[i], false); };
  std::stable_sort(out.prims.begin(), out.prims.end(), [&](int x, int y) { return cls(x) < cls(y); });
  for (int i : out.prims) out.cnt[cls(i)]++;
  return out;
}

// ---- stage 6: one BVH per set; primitives stored in leaf order, set after set (the prefix first)
struct Hierarchies {
  std::vector<float> nodes;    // HostScene::nodes
  std::vector<int> order;      // caller index of every record: the prefix, each set's leaves, each object's
  std::vector<int> roots;      // per set
  std::vector<int> set_begin;  // per set, and the end of the last: its range of `order`
  std::vector<int> blas_root;  // per instanced object
  int surface_nodes = 0, max_depth = 0;
};

// the BVH of `prims` after the nodes and records so far
BvhOut append_bvh(const std::vector<BuildPrim>& prims, int leaf_max, Hierarchies& H) {
  BvhOut bo;
  rt_build_bvh(prims, (int)(H.nodes.size() / 16), (int)H.order.size(), bo, leaf_max);
  H.nodes.insert(H.nodes.end(), bo.nodes.begin(), bo.nodes.end());
  H.order.insert(H.order.end(), bo.order.begin(), bo.order.end());
  return bo;
}

Hierarchies build_hierarchies(const rt_scene* sc, const BuildKnobs& knobs, const PrimSets& P,
                              const std::vector<int>& prefix) {
  const int n_sets = (int)P.sets.size(), n_blas = (int)P.blas_sets.size();
  Hierarchies H;
  H.order = prefix;
  H.roots.assign(n_sets, 0);
  H.set_begin.assign(n_sets + 1, 0);
  H.set_begin[0] = (int)prefix.size();
  int surface_depth = 0;
  for (int s = 0; s < n_sets; ++s) {
    // leaves of at most 2 triangles / quads (bunny-Cornell 112 -> 107 ms, pawn+fog -1.2 % against
    // 8 under the leaf-exit policy); sphere sets keep 8 (demo1 +0.6 % at 2)
    bool spheres = true;
    for (const BuildPrim& b : P.sets[s]) spheres = spheres && b.inst < 0 && sc->prims[b.index].kind == RT_PRIM_SPHERE;
    const BvhOut a = append_bvh(P.sets[s], knobs.leaf_max.value_or(spheres ? RT_LEAF_MAX : 2), H);
    H.roots[s] = a.root;
    H.max_depth = std::max(H.max_depth, a.max_depth);
    H.set_begin[s + 1] = (int)H.order.size();
    if (s == 0) {
      H.surface_nodes = (int)(H.nodes.size() / 16);
      surface_depth = a.max_depth;
    }
  }
  // instanced objects: one object-space BVH each (leaves of at most 2 primitives, as meshes),
  // after the sets; the stack holds the world levels, the exit marker and the object's levels
  H.blas_root.assign(n_blas, RT_EMPTY_ROOT);
  int blas_depth = 0;
  for (int b = 0; b < n_blas && sc->n_instances > 0; ++b) {
    const BvhOut a = append_bvh(P.blas_sets[b], 2, H);
    H.blas_root[b] = a.root;
    blas_depth = std::max(blas_depth, a.max_depth);
  }
  if (sc->n_instances > 0) H.max_depth = std::max(H.max_depth, surface_depth + 1 + blas_depth + 1);
  return H;
}

// ---- stage 7: layout of the tested records
struct Layout {
  std::vector<int> order;  // Hierarchies::order with flat sets class-grouped and box faces after their set's tests
  DevFlatSet flat_sets[1 + RT_MAX_MEDIA] = {};
  std::vector<BoxFound> boxes;
  std::vector<BoxCodes> box_codes;
  std::vector<int> slot_of;  // flat scenes: per record, its slot (else 0)
};

// the ranges of a class-grouped set at `first`: cnt[0] parallelograms, cnt[1] triangles, cnt[2]
// spheres, cnt[3] moving primitives; no box groups
DevFlatSet class_ranges(int first, const int* cnt) {
  DevFlatSet F{};
  F.first = first;
  F.end_quad = F.first + cnt[0];
  F.end_tri = F.end_quad + cnt[1];
  F.end_sphere = F.end_tri + cnt[2];
  F.end = F.end_sphere + cnt[3];
  return F;
}

// group each flat set's single leaf by class (rt_internal.h DevFlatSet); stable within a class
void group_by_class(const rt_scene* sc, const std::vector<int>& set_begin, Layout& L) {
  auto cls = [&](int i) { return prim_class(sc->prims[i], true); };
  for (size_t s = 0; s + 1 < set_begin.size(); ++s) {
    int* b = L.order.data() + set_begin[s];
    int* e = L.order.data() + set_begin[s + 1];
    std::stable_sort(b, e, [&](int x, int y) { return cls(x) < cls(y); });
    int cnt[4] = {0, 0, 0, 0};
    for (int* it = b; it != e; ++it) cnt[cls(*it)]++;
    L.flat_sets[s] = class_ranges(set_begin[s], cnt);
  }
}

// box groups among a flat set's static parallelograms (or the surface prefix's), F's range of
// L.order up to set_end: their faces move to the end of the range, after the tested classes (DevBox)
void move_box_faces(const rt_scene* sc, int set_end, DevFlatSet& F, Layout& L) {
  std::vector<int> quads(L.order.begin() + F.first, L.order.begin() + F.end_quad);
  std::vector<BoxFound> found;
  for (const BoxFound& B : find_boxes(sc, quads)) {
    // the faces' key orders and gids must fit the 5-bit offset codes (slot spans are at
    // most the order spans)
    int olo = INT32_MAX, ohi = INT32_MIN, glo = INT32_MAX, ghi = INT32_MIN;
    for (int f = 0; f < 6; ++f) {
      if (B.face[f] < 0) continue;
      const rt_prim& p = sc->prims[B.face[f]];
      olo = std::min(olo, p.order);
      ohi = std::max(ohi, p.order);
      glo = std::min(glo, p.gid);
      ghi = std::max(ghi, p.gid);
    }
    if ((long long)ohi - olo < RT_BOX_NO_FACE && (long long)ghi - glo < RT_BOX_NO_FACE) found.push_back(B);
  }
  F.box_first = F.box_end = (int)L.boxes.size();
  if (found.empty()) return;
  std::vector<char> in_box(sc->n_prims, 0);
  std::vector<int> rest, faces;
  for (const BoxFound& B : found) {
    for (int f = 0; f < 6; ++f)
      if (B.face[f] >= 0) {
        in_box[B.face[f]] = 1;
        faces.push_back(B.face[f]);
      }
    L.boxes.push_back(B);
  }
  for (int j = F.first; j < set_end; ++j)
    if (!in_box[L.order[j]]) rest.push_back(L.order[j]);
  const int removed = set_end - F.first - (int)rest.size();
  std::copy(rest.begin(), rest.end(), L.order.begin() + F.first);
  std::copy(faces.begin(), faces.end(), L.order.begin() + F.first + rest.size());
  F.end_quad -= removed;
  F.end_tri -= removed;
  F.end_sphere -= removed;
  F.end -= removed;
  F.box_end = (int)L.boxes.size();
}

// flat scenes: slot of each primitive (rank of its order within the set) and slot -> index
std::vector<int> slots(const rt_scene* sc, const std::vector<int>& order, const std::vector<int>& set_begin) {
  std::vector<int> slot_of(order.size(), 0);
  for (size_t s = 0; s + 1 < set_begin.size(); ++s) {
    std::vector<int> pos;
    for (int j = set_begin[s]; j < set_begin[s + 1]; ++j) pos.push_back(j);
    std::stable_sort(pos.begin(), pos.end(),
                     [&](int x, int y) { return sc->prims[order[x]].order < sc->prims[order[y]].order; });
    for (size_t r = 0; r < pos.size(); ++r) slot_of[pos[r]] = set_begin[s] + (int)r;
  }
  return slot_of;
}

// box groups: the faces' key orders, gids and primitive indices as base + 5-bit codes
int encode_boxes(const rt_scene* sc, bool flat, Layout& L, std::string& err) {
  std::vector<int> pos_of(sc->n_prims, -1);
  for (size_t j = 0; j < L.order.size(); ++j) pos_of[L.order[j]] = (int)j;
  for (size_t b = 0; b < L.boxes.size(); ++b) {
    const BoxFound& B = L.boxes[b];
    BoxCodes d{};
    int ord[6], gid[6], prm[6];
    int ob = INT32_MAX, gb = INT32_MAX, pb = INT32_MAX;
    for (int f = 0; f < 6; ++f) {
      if (B.face[f] < 0) continue;
      const int j = pos_of[B.face[f]];
      ord[f] = flat ? L.slot_of[j] : sc->prims[B.face[f]].order;
      gid[f] = sc->prims[B.face[f]].gid;
      prm[f] = flat ? L.slot_of[j] : j;
      ob = std::min(ob, ord[f]);
      gb = std::min(gb, gid[f]);
      pb = std::min(pb, prm[f]);
    }
    d.ord_base = ob;
    d.gid_base = gb;
    d.prim_base = pb;
    bool fits = true;
    for (int f = 0; f < 6; ++f) {
      int oo = RT_BOX_NO_FACE, go = RT_BOX_NO_FACE, po = RT_BOX_NO_FACE;
      if (B.face[f] >= 0) {
        oo = ord[f] - ob;
        go = gid[f] - gb;
        po = prm[f] - pb;
        fits = fits && oo < RT_BOX_NO_FACE && go < RT_BOX_NO_FACE && po < RT_BOX_NO_FACE;
      }
      d.ord_code |= oo << (5 * f);
      d.gid_code |= go << (5 * f);
      d.prim_code |= po << (5 * f);
    }
    if (!fits) return fail(err, RT_E_GENERIC, "box group %d: face offsets exceed the 5-bit codes", (int)b);
    L.box_codes.push_back(d);
  }
  return RT_OK;
}

int layout_records(const rt_scene* sc, const BuildKnobs& knobs, bool flat, const SurfacePrefix& pre,
                   const std::vector<int>& set_begin, std::vector<int> order, Layout& L, std::string& err) {
  L.order = std::move(order);
  if (!pre.prims.empty()) L.flat_sets[0] = class_ranges(0, pre.cnt);  // BVH scenes: the surface prefix
  if (flat) group_by_class(sc, set_begin, L);
  if (flat && !knobs.no_box) {
    for (size_t s = 0; s + 1 < set_begin.size(); ++s) move_box_faces(sc, set_begin[s + 1], L.flat_sets[s], L);
  } else if (!pre.prims.empty() && !knobs.no_box) {
    move_box_faces(sc, (int)pre.prims.size(), L.flat_sets[0], L);
  }
  L.slot_of = flat ? slots(sc, L.order, set_begin) : std::vector<int>(L.order.size(), 0);
  return encode_boxes(sc, flat, L, err);
}

// ---- stage 8: the device records
// test order -> slot order (flat scenes: prim index = slot): row j of w values goes to row slot_of[j]
template <class T>
std::vector<T> to_slot_order(const std::vector<T>& rows, int w, const std::vector<int>& slot_of) {
  std::vector<T> out(rows.size());
  for (size_t j = 0; j < slot_of.size(); ++j)
    std::copy(rows.begin() + w * j, rows.begin() + w * (j + 1), out.begin() + w * (size_t)slot_of[j]);
  return out;
}

// material index per record (-1: medium boundary)
std::vector<int> prim_materials(const rt_scene* sc, const Layout& L, bool flat) {
  std::vector<int> mat(L.order.size(), -1);
  for (size_t j = 0; j < mat.size(); ++j) {
    const rt_prim& p = sc->prims[L.order[j]];
    mat[j] = p.set <= 0 ? p.material : -1;
  }
  return flat ? to_slot_order(mat, 1, L.slot_of) : mat;
}

// The geometry records of one precision (rt_internal.h layout): the box groups and the primitives in
// L.order (slot order for flat scenes, with class-grouped test copies).  The plane-shape frame of
// Geometry.hs:117-131 (unit normal n, wa = v x nS, wb = nS x u, so that a = nS.((p-q) x v) =
// (p-q).wa and b = nS.(u x (p-q)) = (p-q).wb) is computed in binary64 and rounded once to R.
template <class R>
void fill_geometry(const rt_scene* sc, const Layout& L, bool flat, HostArraysT<R>& A) {
  const int n = (int)L.order.size();
  A.boxes.clear();
  for (size_t b = 0; b < L.boxes.size(); ++b) {
    const BoxFound& B = L.boxes[b];
    const BoxCodes& C = L.box_codes[b];
    DevBoxT<R> d;
    std::memset(&d, 0, sizeof d);
    // the slab offsets a_k . c in binary64, rounded once (the kernel's s_k = a_k . o - sc[k], three
    // FMAs per axis instead of the ray origin relative to the corner and a dot product)
    for (int k = 0; k < 3; ++k) d.sc[k] = (R)dot(B.a[k], B.c);
    put3(d.a0, B.a[0]);
    put3(d.a1, B.a[1]);
    put3(d.a2, B.a[2]);
    d.ord_base = C.ord_base;
    d.ord_code = C.ord_code;
    d.gid_base = C.gid_base;
    d.gid_code = C.gid_code;
    d.prim_base = C.prim_base;
    d.prim_code = C.prim_code;
    A.boxes.push_back(d);
  }
  A.prims.assign((size_t)n * 16, (R)0);
  A.prim_uv.assign((size_t)n * 6, (R)0);
  for (int j = 0; j < n; ++j) {
    const rt_prim& p = sc->prims[L.order[j]];
    R* f = A.prims.data() + 16 * (size_t)j;
    int kf = (p.kind == RT_PRIM_SPHERE ? 0 : p.kind == RT_PRIM_PARALLELOGRAM ? 1 : 2) |
             (p.motion >= 0 ? RT_FLAG_MOTION : 0);
    if (p.kind == RT_PRIM_SPHERE) {
      f[0] = (R)p.p[0];
      f[1] = (R)p.p[1];
      f[2] = (R)p.p[2];
      f[4] = (R)p.p[3];
      f[5] = (R)(p.p[3] * p.p[3]);
      f[6] = ibits<R>(p.uvframe);
    } else {
      d3 q = D3(p.p), u = D3(p.p + 3), v = D3(p.p + 6);
      d3 cp = cross(u, v);
      double ncp = std::sqrt(dot(cp, cp));
      d3 nrm = divs(cp, ncp), nS = divs(nrm, ncp);
      put3(f, nrm);
      put3(f + 4, q);
      put3(f + 8, cross(v, nS));
      put3(f + 12, cross(nS, u));
      if (!(ncp > 0)) f[0] = f[1] = f[2] = (R)0;  // the reference's normal is NaN: never hit
      for (int k = 0; k < 6; ++k) A.prim_uv[6 * (size_t)j + k] = (R)p.uv[k];
    }
    f[3] = ibits<R>(kf);
    f[7] = ibits<R>(p.gid);
    f[11] = ibits<R>(flat ? L.slot_of[j] : p.order);
    f[15] = ibits<R>(p.motion);
  }
  A.flat_recs.clear();
  if (flat) {  // the shading arrays in slot order, the test records as they are
    A.flat_recs = std::move(A.prims);
    A.prims = to_slot_order(A.flat_recs, 16, L.slot_of);
    A.prim_uv = to_slot_order(A.prim_uv, 6, L.slot_of);
  }
}

// The shading tables of one precision: the materials (and one copy per record), the textures,
// texels, Perlin gradients, motions, sphereUV frames and placements.
template <class R>
void fill_shading(const rt_scene* sc, const std::vector<int>& prim_mat, const std::vector<int>& blas_root,
                  HostArraysT<R>& A) {
  A.mats.assign(sc->n_materials, DevMaterialT<R>{});
  for (int i = 0; i < sc->n_materials; ++i) {
    DevMaterialT<R>& d = A.mats[i];
    d.kind = sc->materials[i].kind;
    d.tex = sc->materials[i].texture;
    d.param = (R)sc->materials[i].param;
    const rt_texture& t = sc->textures[d.tex];
    d.tex_const = t.kind == RT_TEX_CONSTANT ? 1 : 0;
    for (int a = 0; a < 3; ++a) d.c0[a] = (R)t.c0[a];
  }
  A.prim_shade.assign(prim_mat.size(), DevMaterialT<R>{});
  for (size_t j = 0; j < prim_mat.size(); ++j)
    if (prim_mat[j] >= 0) A.prim_shade[j] = A.mats[prim_mat[j]];
  A.texs.assign(sc->n_textures, DevTextureT<R>{});
  for (int i = 0; i < sc->n_textures; ++i) {
    const rt_texture& t = sc->textures[i];
    DevTextureT<R>& d = A.texs[i];
    d.kind = t.kind;
    d.nu = t.nu;
    d.nv = t.nv;
    d.off = t.kind == RT_TEX_IMAGE ? t.image : 0;
    for (int a = 0; a < 3; ++a) {
      d.c0[a] = (R)t.c0[a];
      d.c1[a] = (R)t.c1[a];
    }
    for (int a = 0; a < 8; ++a) d.prm[a] = (R)t.params[a];
  }
  A.texels.assign((size_t)sc->n_texels * 4, (R)0);
  for (int i = 0; i < sc->n_texels; ++i)
    for (int a = 0; a < 3; ++a) A.texels[4 * (size_t)i + a] = (R)sc->texels[3 * (size_t)i + a];
  A.perlin_grad.assign(256 * 4, (R)0);
  if (sc->perlin)
    for (int k = 0; k < 256; ++k)
      for (int a = 0; a < 3; ++a) A.perlin_grad[4 * k + a] = (R)sc->perlin->grad[k][a];
  A.motions.assign((size_t)sc->n_motions * 8, (R)0);
  for (int i = 0; i < sc->n_motions; ++i)
    for (int a = 0; a < 3; ++a) {
      A.motions[8 * (size_t)i + a] = (R)sc->motions[i].v0[a];
      A.motions[8 * (size_t)i + 4 + a] = (R)sc->motions[i].v1[a];
    }
  A.uvframes.assign((size_t)sc->n_uvframes * 12, (R)0);
  for (int i = 0; i < sc->n_uvframes; ++i)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) A.uvframes[12 * (size_t)i + 4 * r + c] = (R)sc->uvframes[i].r[3 * r + c];
  A.instances.assign(sc->n_instances, DevInstanceT<R>{});
  for (int k = 0; k < sc->n_instances; ++k) {
    const rt_instance& I = sc->instances[k];
    DevInstanceT<R>& d = A.instances[k];
    for (int a = 0; a < 12; ++a) d.m[a] = (R)I.m[a];
    d.root = blas_root[I.blas];
    d.material = I.material;
    d.order = I.order;
    d.pad = 0;
  }
}

// ---- stage 9: the traversal policy of the scene
struct TraversalPolicy {
  int leaf_kind, leaf_exit_pct, leaf_exit_pct64, trav_exit_pct, trav_exit_pct64;
};

// BVH traversal policy (KernelParams::leaf_exit_pct), measured per scene class on MI355X:
// testing leaves once a fifth to a third of the lanes hold one beats waiting for all of them
// on triangle meshes (bunny-Cornell 138 -> 113 ms at 20-30 %, 124 at 10); with media in the queries 50-60 %
// (pawn+fog 415 -> 385 ms; 30 % is no gain there); sphere-only leaves are cheapest tested all
// together (demo1: 100 % best, 60 % +1 %)
TraversalPolicy traversal_policy(const rt_scene* sc, const std::vector<int>& order, int n_prefix,
                                 const std::vector<int>& roots, const std::vector<int>& set_begin,
                                 const BuildKnobs& knobs) {
  TraversalPolicy T;
  const int n = (int)order.size();
  bool spheres_only = true, static_tris = true, static_spheres = true;
  for (int j = n_prefix; j < n; ++j) {
    const rt_prim& p = sc->prims[order[j]];
    spheres_only = spheres_only && p.kind == RT_PRIM_SPHERE;
  }
  // one-class leaves: the classes of the leaves the traversal reaches through BVH nodes (the
  // surface set, and the media sets with a BVH); a medium set that is a single leaf (a fog
  // sphere) is tested by the generic test (rt_trace.h test_leaf_generic)
  for (size_t s = 0; s < roots.size(); ++s) {
    if (s > 0 && roots[s] < 0) continue;
    for (int j = set_begin[s]; j < set_begin[s + 1]; ++j) {
      const rt_prim& p = sc->prims[order[j]];
      static_tris = static_tris && p.kind == RT_PRIM_TRIANGLE && p.motion < 0;
      static_spheres = static_spheres && p.kind == RT_PRIM_SPHERE && p.motion < 0;
    }
  }
  // the leaf tests of the BVH kernel specialised to one primitive class (rt_trace.h trav_round
  // kLeaf): bunny-Cornell 144.0 -> 139.7 ms binary64, demo1 63.9 -> 61.6 (profiles/r3/agg)
  T.leaf_kind = n == n_prefix ? 0 : static_tris ? 1 : static_spheres ? 2 : 0;
  // With media: round 5's media kernels (shading-phase events, binary64 in one 1024-lane
  // workgroup per CU with the whole pawn BVH staged, FP32 at 6 waves) re-swept with the lane-loop
  // exit below (profiles/r5/policy): FP32 leaves at 40 % and lane-loop exit 50 %, pawn+fog
  // 275.5 -> 260.5 ms; binary64 55 % and 40 %, 428.3 -> 398.9 ms (round 4: 55 / 70 and 75).
  // Sphere-only leaves: binary64 100 %; FP32 70 % since round 5 (demo1 37.73 -> 37.44 ms; binary64
  // at 70 %: +0.6 %).
  T.leaf_exit_pct = spheres_only ? 70 : sc->n_media > 0 ? 40 : 25;
  T.leaf_exit_pct64 = spheres_only ? 100 : sc->n_media > 0 ? 55 : T.leaf_exit_pct;
  if (knobs.leaf_exit_pct) T.leaf_exit_pct = T.leaf_exit_pct64 = *knobs.leaf_exit_pct;
  // and the decoupled lane loop's exit (KernelParams::trav_exit_pct): demo1 49.2 -> 48.5 ms at 25 %
  // (round 3), the bunny flat between 50 and 75, FP32 pawn+fog best at 50 since round 5's re-sweep
  // (profiles/r5/policy; binary64 media scenes at 40 %, below)
  T.trav_exit_pct = spheres_only ? 25 : 50;
  T.trav_exit_pct64 = !spheres_only && sc->n_media > 0 ? 40 : T.trav_exit_pct;
  if (knobs.trav_pct) T.trav_exit_pct = T.trav_exit_pct64 = *knobs.trav_pct;
  return T;
}

}  // namespace

int rt_host_image_height(const rt_camera_settings* cs) {
  double h = (double)cs->image_width / cs->aspect_ratio;
  if (!std::isfinite(h) || h > 1e9) return -1;
  return (int)std::nearbyint(h);  // round-half-even under the default rounding mode (Ray.hs:123)
}

int rt_host_shard_rows(int height, const rt_exec* ex) {
  if (!ex || ex->n_shards < 1 || ex->row_block < 1 || ex->shard < 0 || ex->shard >= ex->n_shards || height < 0)
    return RT_E_INVALID;
  if (ex->n_shards == 1) return height;  // the whole image, unpadded
  int blocks = (height + ex->row_block - 1) / ex->row_block;
  int per = (blocks + ex->n_shards - 1) / ex->n_shards;
  return per * ex->row_block;
}

int rt_host_build_scene(const rt_scene* sc, HostScene& S, std::string& err) {
  const BuildKnobs knobs = read_knobs();
  SceneFlags flags;
  if (int rc = validate_tables(sc, flags, err)) return rc;
  if (int rc = validate_geometry(sc, err)) return rc;
  S.noise = flags.noise;
  S.full_mats = flags.full_mats;
  S.uv_tex = flags.uv_tex;

  PrimSets P;
  if (int rc = gather_sets(sc, P, err)) return rc;
  const std::vector<int> alias = medium_aliases(sc, knobs);
  SurfacePrefix pre = split_prefix(sc, knobs, std::move(P.sets[0]));
  P.sets[0] = std::move(pre.rest);

  Hierarchies H = build_hierarchies(sc, knobs, P, pre.prims);
  if (H.nodes.size() / 16 >= (size_t)RT_MAX_NODES)
    return fail(err, RT_E_UNSUPPORTED, "%zu BVH nodes exceed the kernels' 32-bit node offsets (%d)", H.nodes.size() / 16,
                RT_MAX_NODES);
  if (H.max_depth > RT_STACK_DEPTH)
    return fail(err, RT_E_STACK, "BVH depth %d exceeds the traversal stack (%d)", H.max_depth, RT_STACK_DEPTH);
  S.nodes = std::move(H.nodes);
  S.n_nodes = (int)(S.nodes.size() / 16);
  S.surface_nodes = H.surface_nodes;
  S.max_depth = H.max_depth;
  S.surface_root = H.roots[0];
  S.n_prims = (int)H.order.size();
  S.flat = S.nodes.empty() && S.n_prims <= RT_LDS_PRIMS_MAX && pre.prims.empty() && sc->n_instances == 0;

  Layout L;
  if (int rc = layout_records(sc, knobs, S.flat, pre, H.set_begin, std::move(H.order), L, err)) return rc;
  std::copy(L.flat_sets, L.flat_sets + 1 + RT_MAX_MEDIA, S.flat_sets);
  S.n_boxes = (int)L.boxes.size();

  S.prim_mat = prim_materials(sc, L, S.flat);
  fill_geometry(sc, L, S.flat, S.f32);
  fill_geometry(sc, L, S.flat, S.f64);
  fill_shading(sc, S.prim_mat, H.blas_root, S.f32);
  fill_shading(sc, S.prim_mat, H.blas_root, S.f64);
  S.n_instances = sc->n_instances;
  S.perlin_perm.assign(3 * 256, 0);
  if (sc->perlin)
    for (int a = 0; a < 3; ++a)
      for (int k = 0; k < 256; ++k) S.perlin_perm[256 * a + k] = sc->perlin->perm[a][k];
  S.n_media = sc->n_media;
  for (int k = 0; k < sc->n_media; ++k) {
    S.f32.media[k] = DevMedium{(float)(-(1.0 / sc->media[k].density)), sc->media[k].material, H.roots[k + 1], alias[k]};
    S.f64.media[k] = DevMediumT<double>{-(1.0 / sc->media[k].density), sc->media[k].material, H.roots[k + 1], alias[k]};
  }

  const TraversalPolicy T = traversal_policy(sc, L.order, (int)pre.prims.size(), H.roots, H.set_begin, knobs);
  S.leaf_kind = T.leaf_kind;
  S.leaf_exit_pct = T.leaf_exit_pct;
  S.leaf_exit_pct64 = T.leaf_exit_pct64;
  S.trav_exit_pct = T.trav_exit_pct;
  S.trav_exit_pct64 = T.trav_exit_pct64;
  return RT_OK;
}

int rt_host_variant(bool flat, int n_media, bool noise, bool mats, bool tex, bool inst, int leaf_kind, bool media_late,
                    int stack_depth) {
  int v = flat ? RT_VAR_FLAT : RT_VAR_BVH;
  // the BVH kernels' 1024-lane classes (rt_kernel_class.h rt_class_block_wide) hold RT_WIDE_STACK_ROWS
  // stack rows per lane; a deeper BVH takes the 512-lane twin of its class
  const int narrow = !flat && stack_depth + 1 > RT_WIDE_STACK_ROWS ? RT_VAR_NARROW : 0;
  // media events in the shading phase; env RT_AMD_MEDIA_LATE=0 keeps them in the traversal loop's
  // query chain (A/B, tests: the images are bit-identical)
  if (const char* e = rt_knob("RT_AMD_MEDIA_LATE")) media_late = media_late && atoi(e) != 0;
  const int late = n_media > 0 && media_late ? RT_VAR_MEDIA_LATE : 0;
  if (inst) return RT_VAR_BVH | RT_VAR_INST | (noise ? RT_VAR_NOISE : 0) | (n_media > 0 ? RT_VAR_MEDIA : 0) |
                   (mats ? RT_VAR_MATS : 0) | (tex ? RT_VAR_TEX : 0) | late | narrow;  // two-level traversal: the decoupled BVH loop
  if (const char* e = rt_knob("RT_AMD_VARIANT")) {
    const int f = atoi(e);
    // (the lockstep kernels exist only in experiment builds, RT_LOCKSTEP_KERNELS)
    const bool ok = f == RT_VAR_BVH || (RT_LOCKSTEP_KERNELS && f == RT_VAR_BVH_LOCKSTEP) || (flat && f == RT_VAR_FLAT);
    if (ok) v = f;  // flat scenes run on any variant
  }
  // one-class BVH leaves: the decoupled kernel (leaf_kind covers the leaves below BVH nodes of the
  // surface and media sets; the kernel dispatch keeps the generic test where no one-class
  // instantiation exists; env RT_AMD_LEAF_KIND=0 keeps the generic test)
  int leaf = 0;
  if (v == RT_VAR_BVH) leaf = leaf_kind == 1 ? RT_VAR_LEAF_TRI : leaf_kind == 2 ? RT_VAR_LEAF_SPHERE : 0;
  if (const char* e = rt_knob("RT_AMD_LEAF_KIND"))
    if (atoi(e) == 0) leaf = 0;
  return v | (noise ? RT_VAR_NOISE : 0) | (n_media > 0 ? RT_VAR_MEDIA : 0) | (mats ? RT_VAR_MATS : 0) |
         (tex ? RT_VAR_TEX : 0) | leaf | (v == RT_VAR_BVH ? late : 0) | narrow;
}
int rt_host_variant(const HostScene& H) {
  return rt_host_variant(H.flat, H.n_media, H.noise, H.full_mats, H.uv_tex, H.n_instances > 0, H.leaf_kind,
                         rt_host_media_late(H), rt_host_stack_depth(H));
}

template <class R>
int rt_host_make_params(const rt_camera_settings* cs, uint64_t seed, const rt_exec* ex, KernelParamsT<R>& P,
                        std::string& err) {
  if (!cs || !ex) return fail(err, RT_E_INVALID, "null argument");
  if (cs->image_width <= 0) return fail(err, RT_E_INVALID, "image width must be positive");
  if (cs->samples_per_pixel <= 0) return fail(err, RT_E_INVALID, "samples per pixel must be positive");
  if (!(cs->aspect_ratio > 0)) return fail(err, RT_E_INVALID, "aspect ratio must be positive");
  int h = rt_host_image_height(cs);
  if (h <= 0) return fail(err, RT_E_INVALID, "image height %d must be positive", h);
  // the kernels carry a pixel's column and row in 16 bits each (rt_trace.h ItemCtx)
  if (cs->image_width > 65535 || h > 65535)
    return fail(err, RT_E_UNSUPPORTED, "image %dx%d exceeds 65535 x 65535", cs->image_width, h);
  if (cs->background_kind != RT_BG_CONST && cs->background_kind != RT_BG_LERP_Y)
    return fail(err, RT_E_UNSUPPORTED, "background kind %d", cs->background_kind);
  if (cs->n_redirect_targets < 0 || cs->n_redirect_targets > RT_MAX_TARGETS)
    return fail(err, RT_E_UNSUPPORTED, "%d redirect targets (at most %d)", cs->n_redirect_targets, RT_MAX_TARGETS);
  if (cs->n_redirect_targets && !cs->redirect_targets) return fail(err, RT_E_INVALID, "null redirect targets");
  if (!finite_n(cs->center, 3) || !finite_n(cs->look_at, 3) || !finite_n(cs->up, 3) || !std::isfinite(cs->vfov) ||
      !std::isfinite(cs->focus_dist) || !std::isfinite(cs->defocus_angle))
    return fail(err, RT_E_INVALID, "non-finite camera settings");
  int rows = rt_host_shard_rows(h, ex);
  if (rows < 0) return fail(err, RT_E_INVALID, "invalid rt_exec");
  // pixel and work-item ids are 32-bit ints: one render's tile holds at most 0x7fffff00 pixels
  if ((long long)rows * cs->image_width > 0x7fffff00LL)
    return fail(err, RT_E_UNSUPPORTED, "a tile of %d x %d pixels exceeds 2^31 (split it over shards)", cs->image_width,
                rows);
  // Ray.hs:122-136, 153-155 in binary64, rounded once to R
  d3 center = D3(cs->center), look = D3(cs->look_at), up = D3(cs->up);
  double vh = cs->focus_dist * std::tan(cs->vfov / 2) * 2;
  double vw = vh * (double)cs->image_width / (double)h;
  d3 w = normalize_hs(center - look);
  d3 u = normalize_hs(cross(up, w));
  d3 v = cross(w, u);
  d3 across = smul(vw, u);
  d3 down = -smul(vh, v);
  d3 top_left = ((center - smul(cs->focus_dist, w)) - divs(across, 2)) - divs(down, 2);
  double dr = cs->focus_dist * std::tan(cs->defocus_angle / 2);
  std::memset(&P.cam, 0, sizeof P.cam);
  put3(P.cam.center, center);
  put3(P.cam.top_left, top_left);
  put3(P.cam.pixel_u, divs(across, (double)cs->image_width));
  put3(P.cam.pixel_v, divs(down, (double)h));
  put3(P.cam.disk_u, smul(dr, u));
  put3(P.cam.disk_v, smul(dr, v));
  put3(P.cam.bg0, D3(cs->background_c0));
  put3(P.cam.bg1, D3(cs->background_c1));
  P.cam.width = cs->image_width;
  P.cam.height = h;
  P.cam.spp = cs->samples_per_pixel;
  P.cam.max_depth = cs->max_recursion_depth;
  P.cam.bg_kind = cs->background_kind;
  // (the rounded fields, as camera_ray would compare them)
  P.cam_defocus = 0;
  for (int k = 0; k < 3; ++k) P.cam_defocus |= P.cam.disk_u[k] != (R)0 || P.cam.disk_v[k] != (R)0;
  P.target_defer = 0;  // rt_host_match_target, which needs the scene, may set them
  P.target_rec = -1;
  // redirect targets (Ray.hs:138-151)
  double cum = 0, psum = 0;
  P.n_targets = cs->n_redirect_targets;
  std::memset(P.targets, 0, sizeof P.targets);
  for (int k = 0; k < cs->n_redirect_targets; ++k) {
    const rt_redirect_target& t = cs->redirect_targets[k];
    DevTargetT<R>& T = P.targets[k];
    d3 q = D3(t.q), uu = D3(t.u), vv = D3(t.v);
    d3 cp = cross(uu, vv);
    double ncp = std::sqrt(dot(cp, cp));
    if (!(ncp > 0) || !std::isfinite(t.prob)) return fail(err, RT_E_INVALID, "redirect target %d is degenerate", k);
    d3 nrm = divs(cp, ncp), nS = divs(nrm, ncp);
    put3(T.q, q);
    put3(T.u, uu);
    put3(T.v, vv);
    put3(T.n, nrm);
    put3(T.wa, cross(vv, nS));
    put3(T.wb, cross(nS, uu));
    put3(T.cr, cp);
    cum = (k == 0) ? t.prob : cum + t.prob;
    psum = (k == 0) ? t.prob : psum + t.prob;
    T.prob = (R)t.prob;
    T.thresh = (R)cum;
    T.prob_icr = (R)(t.prob / ncp);
  }
  P.rem_prob = (R)(1.0 - psum);
  P.key0 = (uint32_t)seed;
  P.key1 = (uint32_t)(seed >> 32);
  P.n_shards = ex->n_shards;
  P.shard = ex->shard;
  P.row_block = ex->row_block;
  P.tile_rows = rows;
  return RT_OK;
}

// The redirect target as a record of the flat surface set.  A target and a parallelogram built from
// the same q, u, v get the same n, q, wa, wb (the same binary64 expressions, rounded once to R:
// fill_geometry, rt_host_make_params; both normals are unit, so no scale is needed), and then the
// next segment's test of that record computes what the scatter's target test would: the same
// plane, origin and direction.  Matched only where the old and the new order are the same
// estimator: one target (the pdf's one term), no media (every segment starts at a scatter), a
// diffuse flat class (the one scatter site that defers), a record tested by the quad loop (static,
// outside the box groups) whose material ends the path, so no ray ever starts on it.  The match
// reads the scene's host arrays.
template <class R>
int rt_host_match_target(const HostScene& H, int variant, KernelParamsT<R>& P) {
  P.target_defer = 0;
  P.target_rec = -1;
  if (!H.flat || (variant & RT_VAR_BASE) != RT_VAR_FLAT || (variant & (RT_VAR_MATS | RT_VAR_MEDIA))) return 0;
  if (const char* e = rt_knob("RT_AMD_TARGET_DEFER"))
    if (atoi(e) == 0) return 0;
  // a pinned kernel variant (experiments) compares the flat kernel with the BVH kernels on one
  // scene bit for bit; only the flat classes can defer, so under it none does
  if (rt_knob("RT_AMD_VARIANT")) return 0;
  const HostArraysT<R>& A = H.arrays<R>();  // (the host's copy: P's record pointers may be a device's)
  if (P.n_targets != 1 || H.n_media != 0 || A.flat_recs.empty() || A.prim_shade.empty()) return 0;
  const DevFlatSet& S = H.flat_sets[0];
  const DevTargetT<R>& T = P.targets[0];
  for (int k = S.first; k < S.end_quad; ++k) {
    const R* f = A.flat_recs.data() + 16 * (size_t)k;
    if (std::memcmp(f, T.n, 3 * sizeof(R)) || std::memcmp(f + 4, T.q, 3 * sizeof(R)) ||
        std::memcmp(f + 8, T.wa, 3 * sizeof(R)) || std::memcmp(f + 12, T.wb, 3 * sizeof(R)))
      continue;
    int kf, slot;
    std::memcpy(&kf, f + 3, 4);
    std::memcpy(&slot, f + 11, 4);
    if (kf != 1 || slot < 0 || slot >= (int)A.prim_shade.size()) continue;  // (a static parallelogram)
    if (A.prim_shade[slot].kind >= 2) continue;  // rays leave this surface: lightSource / pitchBlack only
    P.target_defer = 1;
    P.target_rec = k;
    return 1;
  }
  return 0;
}

// Screen rectangles for the camera segments (KernelParams::cull_box / cull_quad; rt_trace.h
// closest_flat_primary).  A pinhole camera's rays leave cam.center towards top_left + a pixel_u +
// b pixel_v with (a, b) in the pixel's footprint [px, px + 1) x [gy, gy + 1).  A point X strictly in
// front of the camera, X - center = c (top_left - center + a pixel_u + b pixel_v) with c > 0, is
// met only by the ray through (a, b); a convex record whose corners are all in front projects into
// the convex hull of its corners' (a, b).  The rectangle is their bounding rectangle in whole
// pixels, padded by one pixel on every side (the projection's and the tests' rounding, edge
// pixels).  Everything in binary64 from the records and camera fields the kernel reads.
namespace {
constexpr uint32_t kCullAllLo = 0u, kCullAllHi = 0xffffffffu;
// rows m[0..2] times x = b (Cramer); false: singular
bool solve3(const d3* m, d3 b, d3& x) {
  const double det = dot(m[0], cross(m[1], m[2]));
  if (!(std::fabs(det) > 0) || !std::isfinite(det)) return false;
  const d3 c0 = cross(m[1], m[2]), c1 = cross(m[2], m[0]), c2 = cross(m[0], m[1]);
  x = divs(smul(b.x, c0) + smul(b.y, c1) + smul(b.z, c2), det);
  return std::isfinite(x.x) && std::isfinite(x.y) && std::isfinite(x.z);
}
template <class R>
void cull_rect(const KernelParamsT<R>& P, const d3* corners, int n, uint32_t* out) {
  out[0] = kCullAllLo, out[1] = kCullAllHi;
  const d3 center = {(double)P.cam.center[0], (double)P.cam.center[1], (double)P.cam.center[2]};
  const d3 pu = {(double)P.cam.pixel_u[0], (double)P.cam.pixel_u[1], (double)P.cam.pixel_u[2]};
  const d3 pv = {(double)P.cam.pixel_v[0], (double)P.cam.pixel_v[1], (double)P.cam.pixel_v[2]};
  const d3 w0 = d3{(double)P.cam.top_left[0], (double)P.cam.top_left[1], (double)P.cam.top_left[2]} - center;
  // X - center = a' pu + b' pv + c' w0: the matrix with those columns, as rows of its transpose
  const d3 rows[3] = {{pu.x, pv.x, w0.x}, {pu.y, pv.y, w0.y}, {pu.z, pv.z, w0.z}};
  double a0 = INFINITY, a1 = -INFINITY, b0 = INFINITY, b1 = -INFINITY;
  for (int i = 0; i < n; ++i) {
    d3 s;
    if (!solve3(rows, corners[i] - center, s)) return;
    if (!(s.z > 1e-9)) return;  // not strictly in front of the camera
    const double a = s.x / s.z, b = s.y / s.z;
    if (!std::isfinite(a) || !std::isfinite(b)) return;
    a0 = std::min(a0, a), a1 = std::max(a1, a), b0 = std::min(b0, b), b1 = std::max(b1, b);
  }
  const double x0 = std::floor(a0) - 1, x1 = std::floor(a1) + 1, y0 = std::floor(b0) - 1, y1 = std::floor(b1) + 1;
  if (x1 < 0 || y1 < 0 || x0 > 65535 || y0 > 65535) {  // off the frame: no pixel (lo > hi)
    out[0] = 1u, out[1] = 0u;
    return;
  }
  const uint32_t px0 = (uint32_t)std::max(0.0, x0), px1 = (uint32_t)std::min(65535.0, x1);
  const uint32_t gy0 = (uint32_t)std::max(0.0, y0), gy1 = (uint32_t)std::min(65535.0, y1);
  out[0] = gy0 << 16 | px0;
  out[1] = gy1 << 16 | px1;
}
}  // namespace
template <class R>
void rt_host_cull_rects(const HostScene& H, KernelParamsT<R>& P) {
  for (int j = 0; j < RT_CULL_BOXES; ++j) P.cull_box[j][0] = kCullAllLo, P.cull_box[j][1] = kCullAllHi;
  for (int j = 0; j < RT_CULL_QUADS; ++j) P.cull_quad[j][0] = kCullAllLo, P.cull_quad[j][1] = kCullAllHi;
  if (!H.flat || P.cam_defocus) return;
  if (const char* e = rt_knob("RT_AMD_PRIMARY_CULL"))
    if (atoi(e) == 0) return;
  const HostArraysT<R>& A = H.arrays<R>();
  const DevFlatSet& S = H.flat_sets[0];
  for (int b = S.box_first; b < S.box_end && b - S.box_first < RT_CULL_BOXES && b < (int)A.boxes.size(); ++b) {
    // the box {p : 0 <= a_k . p - sc_k <= 1}: corner s in {0, 1}^3 solves a_k . p = s_k + sc_k
    const DevBoxT<R>& B = A.boxes[b];
    const d3 rows[3] = {{(double)B.a0[0], (double)B.a0[1], (double)B.a0[2]},
                        {(double)B.a1[0], (double)B.a1[1], (double)B.a1[2]},
                        {(double)B.a2[0], (double)B.a2[1], (double)B.a2[2]}};
    d3 c[8];
    bool ok = true;
    for (int i = 0; i < 8 && ok; ++i)
      ok = solve3(rows, d3{(double)B.sc[0] + (i & 1), (double)B.sc[1] + (i >> 1 & 1), (double)B.sc[2] + (i >> 2 & 1)}, c[i]);
    if (ok) cull_rect(P, c, 8, P.cull_box[b - S.box_first]);
  }
  for (int k = S.first; k < S.end_quad && k - S.first < RT_CULL_QUADS && 16 * (size_t)(k + 1) <= A.flat_recs.size(); ++k) {
    // a static parallelogram record: n, q, wa, wb with wa . u = 1, wb . u = 0, n . u = 0 and
    // wa . v = 0, wb . v = 1, n . v = 0 (rt_host_make_params' target has the same fields)
    const R* f = A.flat_recs.data() + 16 * (size_t)k;
    const d3 rows[3] = {{(double)f[8], (double)f[9], (double)f[10]},
                        {(double)f[12], (double)f[13], (double)f[14]},
                        {(double)f[0], (double)f[1], (double)f[2]}};
    const d3 q = {(double)f[4], (double)f[5], (double)f[6]};
    d3 u, v;
    if (!solve3(rows, d3{1, 0, 0}, u) || !solve3(rows, d3{0, 1, 0}, v)) continue;
    const d3 c[4] = {q, q + u, q + v, q + u + v};
    cull_rect(P, c, 4, P.cull_quad[k - S.first]);
  }
}

template <class R>
SceneRecordsT<R> rt_host_records(const HostScene& H) {
  const HostArraysT<R>& A = H.arrays<R>();
  SceneRecordsT<R> r;
  r.nodes = H.nodes.data(), r.perlin_perm = H.perlin_perm.data();
  r.prims = A.prims.data(), r.prim_uv = A.prim_uv.data(), r.motions = A.motions.data();
  r.uvframes = A.uvframes.data(), r.texels = A.texels.data(), r.perlin_grad = A.perlin_grad.data();
  r.flat_recs = A.flat_recs.data(), r.prim_shade = A.prim_shade.data(), r.mats = A.mats.data();
  r.texs = A.texs.data(), r.boxes = A.boxes.data(), r.instances = A.instances.data();
  return r;
}

template <class R>
int rt_host_render_params(const HostScene& H, int variant, const SceneRecordsT<R>& r, const rt_camera_settings* cs,
                          uint64_t seed, const rt_exec* ex, const LaunchInputs& L, KernelParamsT<R>& P,
                          std::string& err) {
  constexpr bool f64 = sizeof(R) == 8;
  const bool flat = (variant & RT_VAR_BASE) == RT_VAR_FLAT;
  std::memset(&P, 0, sizeof P);
  if (int rc = rt_host_make_params(cs, seed, ex, P, err)) return rc;
  P.nodes = r.nodes, P.perlin_perm = r.perlin_perm;
  P.prims = r.prims, P.prim_uv = r.prim_uv, P.motions = r.motions, P.uvframes = r.uvframes, P.texels = r.texels;
  P.perlin_grad = r.perlin_grad, P.flat_recs = r.flat_recs, P.prim_shade = r.prim_shade, P.mats = r.mats;
  P.texs = r.texs, P.boxes = r.boxes, P.instances = r.instances;
  P.surface_root = H.surface_root;
  P.leaf_exit_pct = f64 ? H.leaf_exit_pct64 : H.leaf_exit_pct;
  // flat_sets[0] is a prefix only beside a BVH.  A scene without nodes that is not flat (an instance
  // alone, over RT_LDS_PRIMS_MAX leaves in single-leaf sets) has none: its flat_sets[0] is empty
  P.surface_prefix = !flat && H.n_nodes > 0 ? 1 : 0;
  P.n_media = H.n_media;
  for (int k = 0; k < H.n_media; ++k) P.media[k] = H.arrays<R>().media[k];
  for (int k = 0; k <= RT_MAX_MEDIA; ++k) P.flat_sets[k] = H.flat_sets[k];
  P.stack_depth = rt_host_stack_depth(H);
  P.lds_nodes = L.lds_nodes;
  P.n_prims = H.n_prims;
  // (a synchronous call's flat kernel: 64-id pools, rt_api.hip render_async)
  P.pool_shift = L.pool_shift ? L.pool_shift : L.lone && flat ? 6 : 0;
  rt_host_plan_work(P, L.resident_lanes, flat, L.lone);
  if (L.flat_ring) rt_host_plan_ring(P, variant, L.lone, L.pool_shift, L.resident_lanes);  // (the ring form's plan in place of that one)
  P.trav_exit_pct = f64 ? H.trav_exit_pct64 : H.trav_exit_pct;
  P.out_frame_rows = L.out_frame_rows;
  P.sample0 = L.sample0;
  rt_host_match_target(H, variant, P);
  rt_host_cull_rects(H, P);
  return RT_OK;
}
#define RT_INSTANTIATE(R)                                                                                           \
  template void rt_host_cull_rects<R>(const HostScene&, KernelParamsT<R>&);                                         \
  template int rt_host_match_target<R>(const HostScene&, int, KernelParamsT<R>&);                                   \
  template SceneRecordsT<R> rt_host_records<R>(const HostScene&);                                                   \
  template int rt_host_render_params<R>(const HostScene&, int, const SceneRecordsT<R>&, const rt_camera_settings*, \
                                        uint64_t, const rt_exec*, const LaunchInputs&, KernelParamsT<R>&, std::string&);
RT_INSTANTIATE(float)
RT_INSTANTIATE(double)
#undef RT_INSTANTIATE

bool rt_host_media_late(const HostScene& H) {
  if (H.n_media == 0) return false;
  for (int m = 0; m < H.n_media; ++m) {  // (the roots and aliases are the same in both precisions)
    const DevMediumT<double>& M = H.f64.media[m];
    if (!M.alias_surface && !(M.root < 0 && M.root != RT_EMPTY_ROOT)) return false;
  }
  return true;
}

FastDiv rt_host_fastdiv(uint32_t d) {
  FastDiv f{0u, 0, d, 0};
  if (d <= 1) return f;
  int l = 0;
  while ((1ull << l) < d) ++l;  // ceil(log2 d)
  f.m = (uint32_t)((((1ull << 32) * ((1ull << l) - d)) / d) + 1);
  f.s = l - 1;
  return f;
}

template <class R>
void rt_host_plan_work(KernelParamsT<R>& P, long long resident_lanes, bool two_sizes, bool lone) {
  P.div_width = rt_host_fastdiv((uint32_t)P.cam.width);
  P.div_block = rt_host_fastdiv((uint32_t)P.row_block);
  const bool pool_given = P.pool_shift >= 4;  // (the caller may set 4-10: 16- to 1024-id pools)
  if (!pool_given) P.pool_shift = __builtin_ctz(RT_POOL);
  P.trav_exit_pct = 50;  // the caller sets the scene's policy (HostScene::trav_exit_pct) afterwards
  // Items = (tile pixel, chunk of consecutive samples), claimed in pixel order.  Small chunks
  // keep the 64 lanes of a wave on neighbouring pixels (coherent rays) and make the queue tail
  // short; below ~2 samples the per-item commit (3 atomics) dominates.  Measured on MI355X,
  // Cornell 600x600x200 (tools/sweep_chunk.sh, an early kernel): 1 -> 14.3 ms, 2 -> 8.70, 4 -> 8.79, 8 -> 8.97,
  // 34 -> 10.3, 200 -> 16.5.  The image does not depend on this choice (fixed-point sums).
  const long long tile_pixels = (long long)P.tile_rows * P.cam.width;
  const int spp = P.cam.spp;
  // 16-sample items cut the commit atomics 4x where every lane still runs many items (bunny-
  // Cornell / pawn+fog at 1 GPU: -2.4 % / -1 %); with fewer than ~64 items per resident lane (an
  // 8-GPU rank's share, the Cornell box) the longer last items cost more than that (bunny at 8
  // shards: 20.7 -> 22.0 ms), so those keep 4.
  // The flat kernel's small (tail) items hold 3 samples since round 4 (one-wave workgroups, 5 / 8
  // waves per SIMD): Cornell 5.045 -> 4.992 ms binary64 at 1 GPU, one rank's share of 8 0.715 ->
  // 0.706, README's share of 8 0.161 -> 0.134, README at 1 GPU 0.620 -> 0.628 (+1.3 %);
  // profiles/r4/chunk_sweep.  The BVH kernels keep 4.
  const int small = two_sizes ? 3 : 4;
  int chunk = spp < small ? spp : small;
  if (resident_lanes > 0 && (long long)P.tile_rows * P.cam.width * spp / 16 >= 64 * resident_lanes) chunk = 16;
  if (const char* env = rt_knob("RT_AMD_CHUNK")) {  // tuning knob for experiments
    int c = std::atoi(env);
    if (c > 0) chunk = c;
  }
  // Big items for the bulk of the samples, small ones for the tail: the last T samples of every
  // pixel go in `chunk`-sample items, T such that the tail alone still gives every resident lane
  // `tail_items` items, and the first spp - T in as few items of at most `big` samples as cover
  // them exactly.  Two policies since the tail sample stealing (round 6, profiles/r6/sweeps/big):
  // * renders whose frames overlap (rt_render_async: the bench line) take up to 64-sample big items
  //   and 8 tail items per lane — fewer item openings and commits, and the next frame fills the
  //   longer end: Cornell binary64 4.858 -> 4.761 ms, FP32 2.950 -> 2.800, README binary64 0.407
  //   -> 0.392, the 8-GPU share unchanged (its tail covers every sample);
  // * a synchronous call's one launch ends on its last big items, so it keeps 16-sample items and
  //   16 / 32 tail items (one Cornell call 5.25 ms against 5.49 with 48-sample items).
  int big = lone ? RT_BIG_CHUNK_MAX : RT_BIG_CHUNK_MAX_ASYNC, n_big = 0;
  if (const char* env = rt_knob("RT_AMD_BIG_CHUNK")) big = std::max(1, std::atoi(env));
  int tail_items = !lone ? RT_TAIL_ITEMS_ASYNC : sizeof(R) == 8 ? RT_TAIL_ITEMS_F64 : RT_TAIL_ITEMS_F32;
  if (const char* env = rt_knob("RT_AMD_TAIL_ITEMS")) tail_items = std::atoi(env);
  if (two_sizes && chunk < big && tail_items > 0 && resident_lanes > 0 && tile_pixels > 0) {
    long long t = ((long long)tail_items * chunk * resident_lanes + tile_pixels - 1) / tile_pixels;
    if (const char* env = rt_knob("RT_AMD_TAIL_SAMPLES")) t = std::max(0, std::atoi(env));  // tests
    const long long tail = ((t + chunk - 1) / chunk) * chunk;  // tail samples, a multiple of chunk
    if (tail < spp) {
      const long long bulk = spp - tail;
      auto split = [&](int cap) {
        n_big = (int)((bulk + cap - 1) / cap);
        big = (int)((bulk + n_big - 1) / n_big);  // <= cap; n_big items cover the bulk
        big = std::min(big, spp / n_big);          // the small items cover [n_big big, spp)
      };
      split(big);
      // the waves' first pools are static (rt_render_kernel.h WaveWork): a lane's share of its
      // first pool's big items must stay below the mean work per lane, or the lanes of the first
      // waves end the frame alone (README with 26-sample items from 6 tail items: 0.39 -> 0.51 ms)
      const double per_lane = (double)spp * (double)tile_pixels / (double)resident_lanes;
      for (int pass = 0; pass < 2 && !lone; ++pass) {  // (the pool follows the item size: below)
        const int pool_items = (pool_given ? 1 << P.pool_shift : big >= 32 ? 64 : RT_POOL) / 64;
        const int cap = (int)(0.9 * per_lane / pool_items);
        if (cap >= 1 && big > cap) split(cap);
      }
      if (big <= chunk) n_big = 0;
    }
  }
  const int n_chunks = (spp - n_big * big + chunk - 1) / chunk;
  long long items = (long long)(n_big + n_chunks) * tile_pixels;
  if (items > 0x7fffff00LL) {  // keep item ids in int: one item size, grow the chunk
    n_big = 0;
    chunk = (int)((long long)spp * tile_pixels / 0x7fffff00LL) + 1;
    items = (long long)((spp + chunk - 1) / chunk) * tile_pixels;
  }
  P.chunk = chunk;
  P.n_chunks = (spp - n_big * big + chunk - 1) / chunk;
  P.big_chunk = big;
  P.n_big_chunks = n_big;
  P.big_items = (int)((long long)n_big * tile_pixels);
  P.small_start = n_big * big;
  // long big items (>= 32 samples): 64-id pools, one item per lane, so the waves' last pools are
  // even (Cornell binary64 4.760 -> 4.730 ms, FP32 2.803 -> 2.782); shorter ones keep RT_POOL ids
  // per refill (README's 17-sample items: 0.392 -> 0.402 with 64)
  if (!pool_given && !lone && n_big > 0 && big >= 32) P.pool_shift = 6;
  P.div_big = rt_host_fastdiv((uint32_t)std::max(1, n_big));
  P.div_small = rt_host_fastdiv((uint32_t)std::max(1, P.n_chunks));
  P.n_items = (int)items;
  // commit aggregation: a phase qualifies when a pool of RT_POOL consecutive ids spans at most a
  // slot's pixels (rt_render_kernel.h WaveWork); env RT_AMD_AGG=0 turns it off (A/B, same LDS)
  // (the slot width depends on the class's base and media only: rt_kernel_class.h rt_class_agg_pix)
  const KernelClass c{two_sizes ? RT_VAR_FLAT : RT_VAR_BVH, 0, P.n_media > 0 ? 1 : 0, false, false, 0, false};
  const int slot_pix = rt_class_agg_pix(sizeof(R) == 8, c);
  const int pool = 1 << P.pool_shift;
  auto spans = [&](int n) { return n > 0 && (pool - 1 + n - 1) / n + 1 <= slot_pix; };
  bool agg = tile_pixels < (1ll << 24);  // the item's aggregation code shares its tile-pixel word
  if (const char* env = rt_knob("RT_AMD_AGG")) agg = agg && std::atoi(env) != 0;
  P.agg_big = agg && spans(n_big);
  P.agg_small = agg && spans(P.n_chunks);
}

// The ring form of the flat lane loop (rt_trace.h lane_loop_flat_ring): the wave owns a stream of
// samples, so an item is ONE sample, id = tile pixel x spp + (sample - sample0), pixel-major and
// sample-minor — open_item's small-item decode with chunk 1 and no big items.  Every (pixel, sample)
// pair is still one item, rendered once; the Philox counters depend on the pair alone and the sums
// are integers, so the image is the legacy plan's bit for bit.  A pool of consecutive ids is a
// contiguous range of the stream.  A wave waits for the queue's returning atomic with all its lanes
// (the ring is empty when it refills), so pools are large: 1024 ids where frames overlap, 512 for a
// synchronous call, whose launch ends on the pools the waves still hold (Cornell binary64, overlapped:
// 4.341 / 4.229 / 4.174 / 4.158 ms with 128 / 256 / 512 / 1024 ids; synchronous: 4.340 / 4.229 /
// 4.174 with 128 / 256 / 512; profiles/flat_ring) — halved while the resident waves would get fewer
// than 8 pools each (a small image still spreads over the device) or the pool's pixel span
// ceil((pool - 1) / spp) + 1 exceeds a slot (RT_RING_AGG_PIX), down to 64.  After rt_host_plan_work
// (the divisors).  The class: flat, constant textures, the diffuse materials, no media.
template <class R>
bool rt_host_plan_ring(KernelParamsT<R>& P, int variant, bool lone, int pool_shift, long long resident_lanes) {
  P.flat_ring = 0;
  if (!rt_class_has_ring(rt_class_of(sizeof(R) == 8, variant))) return false;
  if (const char* e = rt_knob("RT_AMD_FLAT_RING"))
    if (std::atoi(e) == 0) return false;
  const long long tile_pixels = (long long)P.tile_rows * P.cam.width;
  const int spp = P.cam.spp;
  if (spp <= 0 || tile_pixels <= 0 || tile_pixels * spp > 0x7fffff00LL) return false;
  const bool pool_given = pool_shift >= 4;  // (LaunchInputs::pool_shift)
  int shift = pool_given ? pool_shift : lone ? 9 : 10;
  auto spans = [&](int s) { return ((1 << s) - 1 + spp - 1) / spp + 1 <= RT_RING_AGG_PIX; };
  const long long waves = resident_lanes / 64;
  auto spreads = [&](int s) { return waves <= 0 || (8ll << s) * waves <= tile_pixels * spp; };
  while (!pool_given && shift > 6 && !(spans(shift) && spreads(shift))) --shift;
  P.pool_shift = shift;
  P.chunk = 1;
  P.n_chunks = spp;
  P.big_chunk = 1;
  P.n_big_chunks = 0;
  P.big_items = 0;
  P.small_start = 0;
  P.div_big = rt_host_fastdiv(1u);
  P.div_small = rt_host_fastdiv((uint32_t)spp);
  P.n_items = (int)(tile_pixels * spp);
  bool agg = tile_pixels < (1ll << 24);  // the item's aggregation code shares its tile-pixel word
  if (const char* env = rt_knob("RT_AMD_AGG")) agg = agg && std::atoi(env) != 0;
  P.agg_big = 0;
  P.agg_small = agg && spans(shift);
  P.flat_ring = 1;
  return true;
}
template bool rt_host_plan_ring<float>(KernelParamsT<float>&, int, bool, int, long long);
template bool rt_host_plan_ring<double>(KernelParamsT<double>&, int, bool, int, long long);

template int rt_host_make_params<float>(const rt_camera_settings*, uint64_t, const rt_exec*, KernelParamsT<float>&,
                                        std::string&);
template int rt_host_make_params<double>(const rt_camera_settings*, uint64_t, const rt_exec*, KernelParamsT<double>&,
                                         std::string&);
template void rt_host_plan_work<float>(KernelParamsT<float>&, long long, bool, bool);
template void rt_host_plan_work<double>(KernelParamsT<double>&, long long, bool, bool);

// The 8-bit code thresholds of writeImage / writeImageSqrt's quantisation (rt_encode8_table.h,
// generated with the transfer evaluated exactly; raytrace_amd.ray.encode8 reads the same table).
void rt_host_encode8_thresholds(int encoding, double* thr) {
  const double* t = encoding == 1 ? kEnc8Sqrt : kEnc8Srgb;
  for (int k = 0; k < 256; ++k) thr[k] = t[k];
}

// ---- radiance queries (include/rt.h rt_scene_radiance): what needs no device

// the frame a radiance query's argument block is made for: a valid 1 x 1 camera (as a cast's) with
// the caller's depth, background and redirect targets — nothing else of cs is read
rt_camera_settings rt_host_radiance_camera(const rt_camera_settings* cs) {
  rt_camera_settings c{};
  c.look_at[2] = -1.0;
  c.up[1] = 1.0;
  c.vfov = 1.0;
  c.aspect_ratio = 1.0;
  c.image_width = c.samples_per_pixel = 1;
  c.focus_dist = 1.0;
  c.max_recursion_depth = cs->max_recursion_depth;
  c.background_kind = cs->background_kind;
  std::memcpy(c.background_c0, cs->background_c0, sizeof c.background_c0);
  std::memcpy(c.background_c1, cs->background_c1, sizeof c.background_c1);
  c.n_redirect_targets = cs->n_redirect_targets;
  c.redirect_targets = cs->redirect_targets;
  return c;
}

int rt_host_radiance_check(const void* scene, const rt_exec* ex, const rt_camera_settings* cs, const void* rays, const void* out,
                           int64_t n, int n_samples, int flags, std::string& err) {
  if (!scene) return fail(err, RT_E_INVALID, "null scene");
  if (!ex) return fail(err, RT_E_INVALID, "null rt_exec");
  if (!cs) return fail(err, RT_E_INVALID, "null camera settings");
  if (!rays) return fail(err, RT_E_INVALID, "null ray buffer");
  if (!out) return fail(err, RT_E_INVALID, "null result buffer");
  if (n < 0) return fail(err, RT_E_INVALID, "negative ray count %lld", (long long)n);
  if (n_samples <= 0 || n_samples > RT_RADIANCE_MAX_SAMPLES)
    return fail(err, RT_E_INVALID, "n_samples %d outside 1..%d", n_samples, RT_RADIANCE_MAX_SAMPLES);
  if (flags & ~(RT_RADIANCE_UNIT_DIR | RT_RADIANCE_ACCUMULATE)) return fail(err, RT_E_INVALID, "unknown radiance flags 0x%x", flags);
  if (ex->n_devices != 0) return fail(err, RT_E_INVALID, "a radiance query runs on the scene's device (n_devices = 0)");
  if (n > (int64_t)RT_RADIANCE_MAX_IDS / n_samples)
    return fail(err, RT_E_INVALID, "%lld rays x %d samples exceed the %d item ids of one call", (long long)n, n_samples,
                RT_RADIANCE_MAX_IDS);
  return RT_OK;
}

// ---- ray orders (include/rt.h rt_scene_ray_order): the host twin of rt_order.hip from the same
// header — the keys (keys_out, may be null) and their stable order (order_out, may be null) of n
// records of `kind`.  A test hook, exported but not declared in rt.h.
extern "C" int rt_host_ray_order(const void* rays, int64_t n, int32_t kind, uint32_t* keys_out, uint32_t* order_out) {
  if (n < 0 || n >= ((int64_t)1 << 31) || (!rays && n > 0)) return RT_E_INVALID;
  if (kind != RT_ORDER_RAYS && kind != RT_ORDER_PATH_RAYS) return RT_E_INVALID;
  rt_order_host(rays, n, kind == RT_ORDER_RAYS ? sizeof(rt_ray) : sizeof(rt_path_ray), keys_out, order_out);
  return RT_OK;
}
