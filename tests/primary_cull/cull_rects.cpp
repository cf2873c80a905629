// cull_rects.cpp — TEST TOOLING: the screen rectangles of the ring loop's camera segments
// (raytrace_amd/csrc/rt_build.cpp rt_host_cull_rects) against a brute-force sweep of camera rays
// through the flat loops' own hit tests (rt_trace.h under RT_HOST_EMU), on the host.  A stand-alone
// program: tests/test_primary_cull_host.py builds it once (g++ -ffp-contract=off, with rt_build.cpp
// and rt_bvh.cpp) and runs it per scene and camera.  Checks: cull_body.h.  Never linked into
// librt_amd.so.
//   cull_rects <scene file> <width> <aspect> <cx cy cz> <lx ly lz> <vfov> <defocus angle> <focus dist>
// The scene file: int32 n_prims, n_materials, n_textures, then the rt_prim, rt_material and
// rt_texture records of include/rt.h (no media, motions, frames, texels or instances).
#define RT_HOST_EMU 1
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt.h"
#include "../../raytrace_amd/csrc/rt_internal.h"

#define RT_F64 0
#include "../../raytrace_amd/csrc/rt_trace.h"
namespace cull32 {
#include "cull_body.h"
}  // namespace cull32
#undef RT_F64
#undef PC_PREC
#define RT_F64 1
#include "../../raytrace_amd/csrc/rt_trace.h"
namespace cull64 {
#include "cull_body.h"
}  // namespace cull64

namespace rt_emu {
thread_local long long counters[4];
}

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, int n) {
  v.resize((size_t)n);
  return n == 0 || std::fread(v.data(), sizeof(T), (size_t)n, f) == (size_t)n;
}

int main(int argc, char** argv) {
  if (argc != 13) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  int32_t n[3];
  if (!f || std::fread(n, 4, 3, f) != 3) return 2;
  std::vector<rt_prim> prims;
  std::vector<rt_material> mats;
  std::vector<rt_texture> texs;
  if (!read_n(f, prims, n[0]) || !read_n(f, mats, n[1]) || !read_n(f, texs, n[2])) return 2;
  std::fclose(f);
  rt_scene sc{};
  sc.n_prims = n[0], sc.prims = prims.data();
  sc.n_materials = n[1], sc.materials = mats.data();
  sc.n_textures = n[2], sc.textures = texs.data();
  HostScene H;
  std::string err;
  if (rt_host_build_scene(&sc, H, err) != RT_OK) {
    std::printf("FAIL build: %s\n", err.c_str());
    return 1;
  }
  rt_camera_settings cs{};
  cs.image_width = std::atoi(argv[2]);
  cs.aspect_ratio = std::atof(argv[3]);
  for (int k = 0; k < 3; ++k) cs.center[k] = std::atof(argv[4 + k]), cs.look_at[k] = std::atof(argv[7 + k]);
  cs.up[1] = 1.0;
  cs.vfov = std::atof(argv[10]);
  cs.defocus_angle = std::atof(argv[11]);
  cs.focus_dist = std::atof(argv[12]);
  cs.samples_per_pixel = 1;
  cs.max_recursion_depth = 4;
  cs.background_kind = RT_BG_CONST;
  const int bad = cull32::run(H, cs) + cull64::run(H, cs);
  return bad ? 1 : 0;
}
