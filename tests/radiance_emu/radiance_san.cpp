// radiance_san.cpp — TEST TOOLING: a stand-alone program (its own main) that drives the host build
// of the radiance-query body (rt_radiance_emu.cpp) and the host-side argument checks
// (rt_build.cpp rt_host_radiance_check) over closed-form cases and malformed rays; the Makefile's
// `san` target builds it with -fsanitize=address,undefined.  Exit status 0: every case came out as
// expected (and no sanitizer report ended the run).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/rt.h"
#include "../../raytrace_amd/csrc/rt_internal.h"

extern "C" {
const char* rt_radiance_emu_last_error(void);
int rt_radiance_emu(const rt_camera_settings* cs, const rt_scene* sc, uint64_t seed, const rt_path_ray* rays, int64_t n,
                    int32_t n_samples, int32_t flags, unsigned long long* work, rt_radiance* out, int f64);
int rt_radiance_emu_camera_rays(const rt_camera_settings* cs, const rt_scene* sc, uint64_t seed, int32_t sample,
                                rt_path_ray* rays, int f64);
}

static int g_failed = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
      ++g_failed;                                                     \
    }                                                                 \
  } while (0)

static rt_path_ray ray(double ox, double oy, double oz, double dx, double dy, double dz, double time = 0.0, uint32_t stream = 0) {
  rt_path_ray r{};
  r.origin[0] = ox, r.origin[1] = oy, r.origin[2] = oz;
  r.dir[0] = dx, r.dir[1] = dy, r.dir[2] = dz;
  r.time = time;
  r.stream = stream;
  return r;
}

int main() {
  // a lambertian sphere of albedo 0.5 at the origin and an emitter (0.5, 2, 0.25) facing -z at z = 5
  rt_texture tex[2] = {};
  tex[0].kind = RT_TEX_CONSTANT, tex[0].image = -1;
  tex[0].c0[0] = tex[0].c0[1] = tex[0].c0[2] = 0.5;
  tex[1].kind = RT_TEX_CONSTANT, tex[1].image = -1;
  tex[1].c0[0] = 0.5, tex[1].c0[1] = 2.0, tex[1].c0[2] = 0.25;
  rt_material mat[2] = {};
  mat[0].kind = RT_MAT_LAMBERTIAN, mat[0].texture = 0;
  mat[1].kind = RT_MAT_LIGHT_SOURCE, mat[1].texture = 1;
  rt_prim prim[2] = {};
  prim[0].kind = RT_PRIM_SPHERE, prim[0].material = 0, prim[0].motion = -1, prim[0].uvframe = -1, prim[0].gid = 0, prim[0].order = 0;
  prim[0].p[3] = 1.0;
  prim[1].kind = RT_PRIM_PARALLELOGRAM, prim[1].material = 1, prim[1].motion = -1, prim[1].uvframe = -1, prim[1].gid = 1;
  prim[1].order = 1;
  const double quad[9] = {-1, -1, 5, 2, 0, 0, 0, 2, 0};
  std::memcpy(prim[1].p, quad, sizeof quad);
  prim[1].uv[2] = 1.0, prim[1].uv[5] = 1.0;
  rt_scene sc{};
  sc.n_prims = 2, sc.prims = prim;
  sc.n_materials = 2, sc.materials = mat;
  sc.n_textures = 2, sc.textures = tex;
  rt_camera_settings cs{};
  cs.look_at[2] = -1.0, cs.up[1] = 1.0, cs.vfov = 1.0, cs.aspect_ratio = 1.0;
  cs.image_width = 4, cs.samples_per_pixel = 1, cs.max_recursion_depth = 8, cs.focus_dist = 1.0;
  cs.background_kind = RT_BG_CONST;
  cs.background_c0[0] = 0.25, cs.background_c0[1] = 0.5, cs.background_c0[2] = 1.0;

  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  std::vector<rt_path_ray> rays = {
      ray(0, 0, 3, 0, 0, 2),        // 0: into the emitter
      ray(0, 5, 0, 0, 3, 0),        // 1: a miss
      ray(0, 0, -4, 0, 0, 1),       // 2: onto the sphere
      ray(nan, 0, 0, 0, 0, 1),      // 3..8: malformed
      ray(0, 0, 0, inf, 0, 1),
      ray(0, 0, 0, 0, 0, 0),
      ray(0, 0, 0, 0, 0, 1, -0.1),
      ray(0, 0, 0, 0, 0, 1, 1.5),
      ray(0, 0, 0, 0, 0, 1, nan),
      ray(0, 5, 0, 0, 3, 0, 1.0),   // 9: a miss again, time 1
  };
  const int64_t n = (int64_t)rays.size();
  for (int f64 = 0; f64 < 2; ++f64) {
    const int words = f64 ? 7 : 4;
    std::vector<unsigned long long> work((size_t)n * words, 0xA5A5A5A5A5A5A5A5ull);
    std::vector<rt_radiance> out((size_t)n);
    for (int depth : {8, 1, 0}) {
      cs.max_recursion_depth = depth;
      const int samples = 5;
      int rc = rt_radiance_emu(&cs, &sc, 7, rays.data(), n, samples, 0, work.data(), out.data(), f64);
      EXPECT(rc == RT_OK);
      if (rc != RT_OK) std::fprintf(stderr, "%s\n", rt_radiance_emu_last_error());
      for (int i : {0, 1, 2, 9}) EXPECT(out[i].status == 1 && out[i].samples == (uint32_t)samples);
      if (depth > 0) {
        EXPECT(out[0].rgb[0] == 0.5 && out[0].rgb[1] == 2.0 && out[0].rgb[2] == 0.25);
        EXPECT(out[1].rgb[0] == 0.25 && out[1].rgb[1] == 0.5 && out[1].rgb[2] == 1.0);
        EXPECT(std::memcmp(out[9].rgb, out[1].rgb, sizeof out[1].rgb) == 0);
      } else {
        for (int i : {0, 1, 2, 9}) EXPECT(out[i].rgb[0] == 0.0 && out[i].rgb[1] == 0.0 && out[i].rgb[2] == 0.0);
      }
      if (depth == 1) EXPECT(out[2].rgb[0] == 0.0 && out[2].rgb[1] == 0.0 && out[2].rgb[2] == 0.0);
      if (depth == 8) EXPECT(out[2].rgb[2] > 0.0 && out[2].rgb[2] < 1.0);
      for (int i = 3; i <= 8; ++i) {
        EXPECT(out[i].status == -1 && out[i].samples == 0u);
        EXPECT(out[i].rgb[0] == 0.0 && out[i].rgb[1] == 0.0 && out[i].rgb[2] == 0.0);
        for (int w = 0; w < words; ++w) EXPECT(work[(size_t)i * words + w] == 0ull);
      }
    }
    // accumulate: the counts add up and a malformed ray's words stay as they are
    cs.max_recursion_depth = 8;
    EXPECT(rt_radiance_emu(&cs, &sc, 7, rays.data(), n, 5, 0, work.data(), out.data(), f64) == RT_OK);
    for (int w = 0; w < words; ++w) work[(size_t)3 * words + w] = 0x1111ull;
    EXPECT(rt_radiance_emu(&cs, &sc, 7, rays.data(), n, 3, RT_RADIANCE_ACCUMULATE, work.data(), out.data(), f64) == RT_OK);
    EXPECT(out[0].samples == 8u && out[0].rgb[1] == 2.0 && out[1].rgb[2] == 1.0);
    for (int w = 0; w < words; ++w) EXPECT(work[(size_t)3 * words + w] == 0x1111ull);
    // camera rays of a 4 x 4 frame: unit directions, streams in row order
    std::vector<rt_path_ray> cam(16);
    EXPECT(rt_radiance_emu_camera_rays(&cs, &sc, 7, 2, cam.data(), f64) == RT_OK);
    for (int i = 0; i < 16; ++i) {
      const double l = std::sqrt(cam[i].dir[0] * cam[i].dir[0] + cam[i].dir[1] * cam[i].dir[1] + cam[i].dir[2] * cam[i].dir[2]);
      EXPECT(cam[i].stream == (uint32_t)i && cam[i].sample0 == 2u && std::fabs(l - 1.0) < 1e-6 && cam[i].time >= 0.0 &&
             cam[i].time < 1.0);
    }
  }
  // the argument checks
  rt_exec ex{};
  ex.n_shards = 1, ex.row_block = 4;
  std::string err;
  rt_radiance o1;
  const void *S = &sc, *R = rays.data(), *O = &o1;
  EXPECT(rt_host_radiance_check(S, &ex, &cs, R, O, 1, 1, 0, err) == RT_OK);
  EXPECT(rt_host_radiance_check(nullptr, &ex, &cs, R, O, 1, 1, 0, err) == RT_E_INVALID);
  EXPECT(rt_host_radiance_check(S, nullptr, &cs, R, O, 1, 1, 0, err) == RT_E_INVALID);
  EXPECT(rt_host_radiance_check(S, &ex, nullptr, R, O, 1, 1, 0, err) == RT_E_INVALID);
  EXPECT(rt_host_radiance_check(S, &ex, &cs, nullptr, O, 1, 1, 0, err) == RT_E_INVALID);
  EXPECT(rt_host_radiance_check(S, &ex, &cs, R, nullptr, 1, 1, 0, err) == RT_E_INVALID);
  EXPECT(rt_host_radiance_check(S, &ex, &cs, R, O, -1, 1, 0, err) == RT_E_INVALID);
  EXPECT(rt_host_radiance_check(S, &ex, &cs, R, O, 1, 0, 0, err) == RT_E_INVALID);
  EXPECT(rt_host_radiance_check(S, &ex, &cs, R, O, 1, (1 << 24) + 1, 0, err) == RT_E_INVALID);
  EXPECT(rt_host_radiance_check(S, &ex, &cs, R, O, 1, 1, 4, err) == RT_E_INVALID);
  EXPECT(rt_host_radiance_check(S, &ex, &cs, R, O, (int64_t)RT_RADIANCE_MAX_IDS, 1, 0, err) == RT_OK);
  EXPECT(rt_host_radiance_check(S, &ex, &cs, R, O, (int64_t)RT_RADIANCE_MAX_IDS + 1, 1, 0, err) == RT_E_INVALID);
  EXPECT(rt_host_radiance_check(S, &ex, &cs, R, O, (int64_t)1 << 40, 1 << 24, 0, err) == RT_E_INVALID);
  EXPECT(rt_host_radiance_check(S, &ex, &cs, R, O, 0, 1, 0, err) == RT_OK);
  const int32_t dev0 = 0;
  ex.n_devices = 1, ex.devices = &dev0;
  EXPECT(rt_host_radiance_check(S, &ex, &cs, R, O, 1, 1, 0, err) == RT_E_INVALID);
  std::printf("radiance_san: %d failed\n", g_failed);
  return g_failed ? 1 : 0;
}
