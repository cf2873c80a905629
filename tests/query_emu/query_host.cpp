// query_host.cpp — TEST TOOLING: a stand-alone host program over rt_query_emu.cpp, for sanitizer runs
// (tests/test_query_host.py): a small scene built here — a parallelogram floor, a triangle, static
// and moving spheres, enough small spheres for a BVH — the rays read from a file of rt_ray records,
// the hits written as rt_hit records.
//   query_host <rays.bin> <hits.bin> <f64: 0 | 1> <flags> <n_small_spheres>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/rt.h"

extern "C" int rt_query_emu(const rt_scene* sc, const rt_ray* rays, rt_hit* hits, long long n, int flags, int f64, int* variant);
extern "C" const char* rt_query_emu_last_error(void);

static rt_prim prim(int kind, int order, int motion, std::initializer_list<double> p) {
  rt_prim r{};
  r.kind = kind;
  r.material = 0;
  r.set = 0;
  r.motion = motion;
  r.gid = order;
  r.order = order;
  r.uvframe = -1;
  int k = 0;
  for (double v : p) r.p[k++] = v;
  r.uv[2] = 1.0;
  r.uv[5] = 1.0;
  return r;
}

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int f64 = atoi(argv[3]), flags = atoi(argv[4]), n_small = atoi(argv[5]);
  std::vector<rt_prim> prims;
  prims.push_back(prim(RT_PRIM_PARALLELOGRAM, 0, -1, {-8, 0, -8, 16, 0, 0, 0, 0, 16}));
  prims.push_back(prim(RT_PRIM_TRIANGLE, 1, -1, {-1, 0.5, 0, 2, 0, 0, 0, 2, 0.5}));
  prims.push_back(prim(RT_PRIM_SPHERE, 2, -1, {2, 1, 2, 1}));
  prims.push_back(prim(RT_PRIM_SPHERE, 3, 0, {-2, 1, 2, 0.75}));
  for (int k = 0; k < n_small; ++k)
    prims.push_back(prim(RT_PRIM_SPHERE, 4 + k, -1, {-6.0 + 1.5 * (k % 9), 0.25, -6.0 + 1.5 * (k / 9), 0.25}));
  rt_material mat{RT_MAT_LAMBERTIAN, 0, 0.0};
  rt_texture tex{};
  tex.kind = RT_TEX_CONSTANT;
  tex.image = -1;
  tex.c0[0] = tex.c0[1] = tex.c0[2] = 0.5;
  rt_motion mo{{0, 0, 0}, {0, 1, 0}};
  rt_scene sc{};
  sc.n_prims = (int)prims.size();
  sc.prims = prims.data();
  sc.n_materials = 1;
  sc.materials = &mat;
  sc.n_textures = 1;
  sc.textures = &tex;
  sc.n_motions = 1;
  sc.motions = &mo;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  const long long n = bytes / (long)sizeof(rt_ray);
  std::vector<rt_ray> rays(n);
  std::vector<rt_hit> hits(n);
  if (n && fread(rays.data(), sizeof(rt_ray), n, f) != (size_t)n) return 3;
  fclose(f);
  int variant = 0;
  const int rc = rt_query_emu(&sc, rays.data(), hits.data(), n, flags, f64, &variant);
  if (rc) {
    fprintf(stderr, "rt_query_emu %d: %s\n", rc, rt_query_emu_last_error());
    return 1;
  }
  f = fopen(argv[2], "wb");
  if (!f) return 3;
  if (n) fwrite(hits.data(), sizeof(rt_hit), n, f);
  fclose(f);
  printf("%lld rays, variant %d\n", n, variant);
  return 0;
}
