// order_san.cpp — TEST TOOLING: a stand-alone program over the host twin of the ray order
// (rt_build.cpp rt_host_ray_order, from rt_order.h), built by tests/test_ray_order_host.py with
// AddressSanitizer and UBSan together with rt_build.cpp / rt_bvh.cpp.
//   order_san <in> <out>
// in:  int64 n, int64 kind, then n records of the kind (rt_ray: 80 bytes, rt_path_ray: 64 bytes)
// out: n uint32 keys, n uint32 order
// The keys and the order go through exactly-sized heap buffers, so a write or read past n is caught.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/rt.h"

extern "C" int rt_host_ray_order(const void* rays, int64_t n, int32_t kind, uint32_t* keys_out, uint32_t* order_out);

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t head[2];
  if (std::fread(head, sizeof head, 1, f) != 1) return 2;
  const int64_t n = head[0];
  const int32_t kind = (int32_t)head[1];
  const size_t stride = kind == RT_ORDER_RAYS ? sizeof(rt_ray) : sizeof(rt_path_ray);
  char* rays = (char*)std::malloc(n > 0 ? (size_t)n * stride : 1);
  if (n > 0 && std::fread(rays, stride, (size_t)n, f) != (size_t)n) return 2;
  std::fclose(f);
  uint32_t* keys = (uint32_t*)std::malloc(n > 0 ? (size_t)n * sizeof(uint32_t) : 1);
  uint32_t* order = (uint32_t*)std::malloc(n > 0 ? (size_t)n * sizeof(uint32_t) : 1);
  if (rt_host_ray_order(rays, n, kind, keys, order) != RT_OK) return 3;
  // the refusals, and the outputs being optional
  if (rt_host_ray_order(rays, -1, kind, keys, order) != RT_E_INVALID) return 4;
  if (rt_host_ray_order(rays, n, 2, keys, order) != RT_E_INVALID) return 4;
  if (rt_host_ray_order(rays, n, kind, nullptr, nullptr) != RT_OK) return 4;
  FILE* g = std::fopen(argv[2], "wb");
  if (!g) return 2;
  if (n > 0) {
    std::fwrite(keys, sizeof(uint32_t), (size_t)n, g);
    std::fwrite(order, sizeof(uint32_t), (size_t)n, g);
  }
  std::fclose(g);
  std::free(rays), std::free(keys), std::free(order);
  std::printf("ok %lld\n", (long long)n);
  return 0;
}
