// rt_order.h — the coherence key of a ray batch (include/rt.h rt_scene_ray_order), one
// text for the device (rt_order.hip) and the host (rt_build.cpp rt_host_ray_order, tests/ray_order).
// Binary64 whatever the trace precision; only + - * /, abs, copysign, compares and floor, and no
// expression of the form a * b + c, so nothing here can be contracted: a numpy twin reproduces every
// key bit for bit (tests/test_ray_order_host.py).
//
// A record is the 48 bytes origin[3], dir[3] that rt_ray and rt_path_ray both start with.
//   valid   the six values finite, dir != 0; an invalid ray's key is RT_ORDER_KEY_LAST
//   box     lo_a / hi_a = min / max of origin_a over the valid rays of the batch
//   scale   s_a = RT_ORDER_CELLS / (hi_a - lo_a) if hi_a > lo_a, else 0
//   cell(x) RT_ORDER_CELLS - 1 if x >= RT_ORDER_CELLS - 1; floor(x) if x >= 0; else 0 (a NaN: 0)
//   origin  c_a = cell((origin_a - lo_a) * s_a)
//   dir     L = (|dx| + |dy|) + |dz|, px = dx / L, py = dy / L; if dz < 0:
//           (px, py) <- (copysign(1 - |py|, px), copysign(1 - |px|, py)), both from the old values;
//           u = cell((px + 1) * (RT_ORDER_CELLS / 2)), v = cell((py + 1) * (RT_ORDER_CELLS / 2))
//   key     morton3(c_x, c_y, c_z) << 12 | morton2(u, v), x (u) in the lowest bit of each interleave:
//           RT_ORDER_KEY_BITS = 30 bits, origin-major
// THE BIT SPLIT LIVES HERE: 6 bits per origin axis, 6 + 6 for the direction's octahedral map.
#ifndef RT_ORDER_H
#define RT_ORDER_H
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_ORDER_FN __host__ __device__ inline
#else
#define RT_ORDER_FN inline
#endif

#define RT_ORDER_AXIS_BITS 6
#define RT_ORDER_CELLS 64  // 1 << RT_ORDER_AXIS_BITS
#define RT_ORDER_KEY_BITS 30
#define RT_ORDER_KEY_LAST 0xFFFFFFFFu

RT_ORDER_FN bool rt_order_valid(const double* r) {
  const double inf = __builtin_huge_val();
  const bool finite = __builtin_fabs(r[0]) < inf && __builtin_fabs(r[1]) < inf && __builtin_fabs(r[2]) < inf &&
                      __builtin_fabs(r[3]) < inf && __builtin_fabs(r[4]) < inf && __builtin_fabs(r[5]) < inf;  // (a NaN fails)
  return finite && (r[3] != 0.0 || r[4] != 0.0 || r[5] != 0.0);
}

RT_ORDER_FN double rt_order_scale(double lo, double hi) { return hi > lo ? (double)RT_ORDER_CELLS / (hi - lo) : 0.0; }

RT_ORDER_FN uint32_t rt_order_cell(double x) {
  if (x >= (double)(RT_ORDER_CELLS - 1)) return RT_ORDER_CELLS - 1;
  if (x >= 0.0) return (uint32_t)(int)__builtin_floor(x);
  return 0;
}

// bit k of x to bit 3 k (6 bits) / to bit 2 k (6 bits)
RT_ORDER_FN uint32_t rt_order_spread3(uint32_t x) {
  x = (x | x << 8) & 0x0300F;
  x = (x | x << 4) & 0x030C3;
  x = (x | x << 2) & 0x09249;
  return x;
}
RT_ORDER_FN uint32_t rt_order_spread2(uint32_t x) {
  x = (x | x << 4) & 0x30F;
  x = (x | x << 2) & 0x333;
  x = (x | x << 1) & 0x555;
  return x;
}

// the key of one record; lo, s: the batch's box minimum and scale per axis
RT_ORDER_FN uint32_t rt_order_key(const double* r, const double* lo, const double* s) {
  if (!rt_order_valid(r)) return RT_ORDER_KEY_LAST;
  const uint32_t cx = rt_order_cell((r[0] - lo[0]) * s[0]);
  const uint32_t cy = rt_order_cell((r[1] - lo[1]) * s[1]);
  const uint32_t cz = rt_order_cell((r[2] - lo[2]) * s[2]);
  const double L = (__builtin_fabs(r[3]) + __builtin_fabs(r[4])) + __builtin_fabs(r[5]);
  double px = r[3] / L, py = r[4] / L;
  if (r[5] < 0.0) {
    const double qx = __builtin_copysign(1.0 - __builtin_fabs(py), px);
    const double qy = __builtin_copysign(1.0 - __builtin_fabs(px), py);
    px = qx, py = qy;
  }
  const uint32_t u = rt_order_cell((px + 1.0) * (double)(RT_ORDER_CELLS / 2));
  const uint32_t v = rt_order_cell((py + 1.0) * (double)(RT_ORDER_CELLS / 2));
  const uint32_t org = rt_order_spread3(cx) | rt_order_spread3(cy) << 1 | rt_order_spread3(cz) << 2;
  return org << (2 * RT_ORDER_AXIS_BITS) | rt_order_spread2(u) | rt_order_spread2(v) << 1;
}

// The host twin: keys_out[i] (may be null) and the stable order of the keys, order_out[j] = the
// index of the j-th record in key order, ties in index order (may be null).  stride: a record's bytes.
#include <algorithm>
#include <cstring>
#include <vector>
inline void rt_order_host(const void* rays, int64_t n, size_t stride, uint32_t* keys_out, uint32_t* order_out) {
  const char* base = (const char*)rays;
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, s[3], r[6];
  bool any = false;
  for (int64_t i = 0; i < n; ++i) {
    std::memcpy(r, base + (size_t)i * stride, sizeof r);
    if (!rt_order_valid(r)) continue;
    for (int a = 0; a < 3; ++a) {
      if (!any || r[a] < lo[a]) lo[a] = r[a];
      if (!any || r[a] > hi[a]) hi[a] = r[a];
    }
    any = true;
  }
  for (int a = 0; a < 3; ++a) s[a] = rt_order_scale(lo[a], hi[a]);
  std::vector<uint32_t> keys((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    std::memcpy(r, base + (size_t)i * stride, sizeof r);
    keys[(size_t)i] = rt_order_key(r, lo, s);
  }
  if (keys_out && n > 0) std::memcpy(keys_out, keys.data(), (size_t)n * sizeof(uint32_t));
  if (order_out) {
    for (int64_t i = 0; i < n; ++i) order_out[i] = (uint32_t)i;
    std::stable_sort(order_out, order_out + n, [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  }
}

#endif  // RT_ORDER_H
