// rt_radiance_kernel.h — the radiance-query kernels (include/rt.h rt_scene_radiance,
// rt_scene_camera_rays) and their launchers for ONE precision: included by rt_radiance.hip (RT_F64
// 0) and rt_radiance64_nl.hip (RT_F64 1), each its own translation unit.  The per-lane logic is
// rt_radiance.h over rt_lane.h and rt_trace.h's functions; the render, list, feature and query
// kernels' translation units do not see this file and the spill gate does not count these kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernel_class.h"
#include "rt_trace.h"
#include "rt_radiance.h"

// RT_RADIANCE_ORDERED 1 (rt_radiance_ord.hip, rt_radiance64_ord_nl.hip): the ordered form of the path
// kernel and its launcher under names of their own — an item's ray is order[id / n_chunks]
// (include/rt.h rt_scene_radiance_ordered); the workspace and the result stay indexed by the ray, so
// the resolve and the camera-ray kernels are the unordered units' alone, whose text is unchanged by it.
#ifndef RT_RADIANCE_ORDERED
#define RT_RADIANCE_ORDERED 0
#endif
#if RT_RADIANCE_ORDERED
#define RT_RADIANCE_KERNEL rt_radiance_ordered_kernel
#define RT_RADIANCE_ORDER_PARAM , const uint32_t* __restrict__ order, uint32_t n_rays
#define RT_RADIANCE_ORDER_TYPE , const uint32_t*, uint32_t
#define RT_RADIANCE_LAUNCH rt_launch_radiance_ordered
#else
#define RT_RADIANCE_LAUNCH rt_launch_radiance
#define RT_RADIANCE_KERNEL rt_radiance_kernel
#define RT_RADIANCE_ORDER_PARAM
#define RT_RADIANCE_ORDER_TYPE
#endif

namespace RT_NS {

// the records move as 16-byte vectors: a wave's 64 rays are 4 KB contiguous, its results 2 KB
struct alignas(16) r16 {
  double x, y;
};
static_assert(sizeof(rt_path_ray) == 4 * sizeof(r16) && sizeof(rt_radiance) == 2 * sizeof(r16), "rt.h record sizes");
static_assert((long long)RT_RADIANCE_MAX_IDS + (kLaneResident / kLaneBlock + 1) * kLaneBlock <= 0x7fffffffLL,
              "rt_internal.h RT_RADIANCE_MAX_IDS: the cursor stays below 2^31");
__device__ __forceinline__ double r_ints(uint32_t lo, uint32_t hi) {
  return __builtin_bit_cast(double, (unsigned long long)lo | ((unsigned long long)hi << 32));
}
__device__ __forceinline__ rt_path_ray load_path_ray(const rt_path_ray* __restrict__ rays, long long i) {
  const r16* rp = reinterpret_cast<const r16*>(rays + i);
  const r16 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3];
  const unsigned long long w = __builtin_bit_cast(unsigned long long, r3.y);
  return rt_path_ray{{r0.x, r0.y, r1.x}, {r1.y, r2.x, r2.y}, r3.x, (uint32_t)w, (uint32_t)(w >> 32)};
}

// Items are (ray, sample chunk): item id = ray x n_chunks + k covers samples sample0 + [k chunk,
// min(n_samples, (k + 1) chunk)) of rays[ray], so consecutive ids are the chunks of one ray and then
// the next ray of the caller's order (a wave's lanes on neighbouring rays).  n is a host value, so
// the grid, the chunk and n_chunks are sized by the launcher; the grid fills the device (or is
// smaller, if the items are) and its waves claim 64 consecutive ids at a time from the cursor —
// P.counter[0], in the workspace's tail, zeroed by the call — until the ids are exhausted.  A lane
// sums its chunk in an Acc and adds the nonzero words and the count to the ray's workspace words
// with 64-bit integer atomics, the flag with atomicOr: the sums do not depend on the chunking or the
// schedule.  Nothing is compacted (the ordered form takes the rays in a given order) and no single lane is refilled: the wave waits for its
// longest lane, as rt_list_kernel's.  Block and stack: rt_lane.h.  The kernel's first argument is
// its KernelParams (rt_trace.h RT_KARGS).
template <int kVar, int kTex, int kMedia, bool kMats, bool kInst, int kLeaf>
__global__ __launch_bounds__(kLaneBlock) void RT_RADIANCE_KERNEL(KernelParams P, const rt_path_ray* __restrict__ rays,
                                                                 unsigned long long* __restrict__ work, long long n_items,
                                                                 int n_samples, int chunk, int n_chunks,
                                                                 int flags RT_RADIANCE_ORDER_PARAM) {
  extern __shared__ int smem[];
  const Trav W{smem + threadIdx.x, kLaneBlock, nullptr};
  int overflow = 0;
  for (;;) {
    int base = 0;
    if (threadIdx.x == 0) base = atomicAdd(P.counter, kLaneBlock);
    base = __builtin_amdgcn_readfirstlane(base);
    // wave-uniform exit (the launcher bounds the ids below 2^31); the claim above is reached by the
    // whole wave, the lanes' work below rejoins before the next one
    if (base < 0 || base >= n_items) break;
    const long long id = (long long)base + threadIdx.x;
#if RT_RADIANCE_ORDERED
    // an entry that is no ray's index is skipped: nothing is read or written for it
    const long long slot = id < n_items ? id / n_chunks : 0;
    const uint32_t ray_of = id < n_items ? order[slot] : n_rays;  // (the launcher bounds the rays below 2^31)
    if (ray_of < n_rays) {
      const long long ray = (long long)ray_of;
      const int k = (int)(id - slot * n_chunks);
#else
    if (id < n_items) {  // (the last claim may leave lanes idle; the next claim ends the wave)
      const long long ray = id / n_chunks;
      const int k = (int)(id - ray * n_chunks);
#endif
      const rt_path_ray q = load_path_ray(rays, ray);
      const int k0 = k * chunk, k1 = min(n_samples, (k + 1) * chunk);
      Acc A;
      acc_clear(A);
      bool bad = false;
      if (path_record<kVar, kTex, kMedia, kMats, kInst, kLeaf>(P, W, q, flags, k0, k1, A, bad, overflow)) {
        unsigned long long* dst = work + (size_t)kRadWords * (size_t)ray;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (A.hi[c]) atomicAdd(dst + c, (unsigned long long)A.hi[c]);
#if RT_F64
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (A.lo[c]) atomicAdd(dst + 3 + c, A.lo[c]);
#endif
        atomicAdd(dst + kRadWords - 1, rad_count_word((uint32_t)(k1 - k0)));
        if (bad) atomicOr(reinterpret_cast<unsigned int*>(dst + kRadWords - 1), 1u);  // (little-endian: the low half)
      }
    }
  }
  if (overflow) atomicOr(P.status, 1);
}

#if !RT_RADIANCE_ORDERED
// one thread per ray: the workspace's words to the caller's record (rt_radiance.h radiance_resolve)
__global__ __launch_bounds__(256) void rt_radiance_resolve_kernel(const rt_path_ray* __restrict__ rays,
                                                                  const unsigned long long* __restrict__ work,
                                                                  rt_radiance* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const rt_path_ray q = load_path_ray(rays, i);
  unsigned long long w[kRadWords];
#pragma unroll
  for (int c = 0; c < kRadWords; ++c) w[c] = work[(size_t)kRadWords * (size_t)i + c];
  rt_radiance o;
  radiance_resolve(w, path_ray_ok(q), o);
  r16* op = reinterpret_cast<r16*>(out + i);
  op[0] = r16{o.rgb[0], o.rgb[1]};
  op[1] = r16{o.rgb[2], r_ints((uint32_t)o.status, o.samples)};
}

// one thread per pixel of the frame, row-major (rt_radiance.h camera_ray_record)
template <bool kFlat>
__global__ __launch_bounds__(256) void rt_camera_rays_kernel(KernelParams P, rt_path_ray* __restrict__ rays, int sample) {
  const int n = P.cam.width * P.cam.height;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int gy = i / P.cam.width, px = i - gy * P.cam.width;
  rt_path_ray q;
  camera_ray_record<kFlat>(P, (uint32_t)i, gy, px, sample, q);
  r16* rp = reinterpret_cast<r16*>(rays + i);
  rp[0] = r16{q.origin[0], q.origin[1]};
  rp[1] = r16{q.origin[2], q.dir[0]};
  rp[2] = r16{q.dir[1], q.dir[2]};
  rp[3] = r16{q.time, r_ints(q.stream, q.sample0)};
}

#endif  // !RT_RADIANCE_ORDERED

typedef void (*radiance_fn)(KernelParams, const rt_path_ray*, unsigned long long*, long long, int, int, int,
                            int RT_RADIANCE_ORDER_TYPE);
// the instantiation of a variant's class: the render's (var, tex, media, mats, inst, leaf) with the
// workgroup size's field cleared, as rt_list_kernel.h list_kernel_of; the lockstep BVH base has none
static radiance_fn radiance_kernel_of(int variant) {
  KernelClass cls = rt_class_of(RT_F64, variant);
  cls.narrow = false;
  return rt_with_class(cls, [](auto... k) -> radiance_fn {
    constexpr KernelClass c{decltype(k)::value...};
    if constexpr (rt_class_compiled(RT_F64, c) && !c.narrow && c.var != RT_VAR_BVH_LOCKSTEP)
      return RT_RADIANCE_KERNEL<c.var, c.tex, c.media, c.mats, c.inst, c.leaf>;
    return nullptr;
  });
}

}  // namespace RT_NS

int RT_RADIANCE_LAUNCH(const KernelParamsT<RT_NS::real>& p, int variant, const rt_path_ray* rays, rt_radiance* out,
                       unsigned long long* work, long long n, int n_samples, int chunk_arg, int flags,
#if RT_RADIANCE_ORDERED
                       const uint32_t* order,
#endif
                       void* stream) {
  using namespace RT_NS;
  if (n <= 0 || n_samples <= 0) return 0;
  if (n * n_samples > (long long)RT_RADIANCE_MAX_IDS) return -1;
  const radiance_fn fn = radiance_kernel_of(variant);
  if (!fn) return -1;
  // chunk_arg > 0 fixes the chunk (experiments and tests); otherwise about 16 items per resident
  // lane: short chunks even out the lanes' path lengths (rt_list_kernel.h's rule, on the host)
  const int resident = kLaneResident;
  const long long fill_lanes = 16LL * resident;
  int chunk = chunk_arg;
  if (chunk <= 0) {
    const int want = (int)std::max<long long>(1, std::min<long long>(n_samples, fill_lanes / n));
    chunk = (n_samples + want - 1) / want;
  }
  chunk = std::min(chunk, n_samples);
  const int n_chunks = (n_samples + chunk - 1) / chunk;
  const long long n_items = n * n_chunks;
  const long long blocks = std::min<long long>((n_items + kLaneBlock - 1) / kLaneBlock, resident / kLaneBlock);
  const size_t lds = lane_stack_bytes(variant, p.stack_depth);
  hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(kLaneBlock), lds, (hipStream_t)stream, p, rays, work, n_items, n_samples,
                     chunk, n_chunks, flags
#if RT_RADIANCE_ORDERED
                     , order, (uint32_t)n
#endif
  );
  if (hipGetLastError() != hipSuccess) return -1;
#if RT_RADIANCE_ORDERED
  return rt_launch_radiance_resolve(p, rays, work, out, n, stream);
}
#else
  hipLaunchKernelGGL(rt_radiance_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rays,
                     (const unsigned long long*)work, out, n);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the resolve alone, for the ordered unit's launcher (p names the precision)
int rt_launch_radiance_resolve(const KernelParamsT<RT_NS::real>& p, const rt_path_ray* rays, const unsigned long long* work,
                               rt_radiance* out, long long n, void* stream) {
  using namespace RT_NS;
  (void)p;
  hipLaunchKernelGGL(rt_radiance_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rays, work,
                     out, n);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rt_launch_camera_rays(const KernelParamsT<RT_NS::real>& p, int variant, rt_path_ray* rays, int sample, void* stream) {
  using namespace RT_NS;
  const long long n = (long long)p.cam.width * p.cam.height;
  if (n <= 0) return 0;
  const unsigned blocks = (unsigned)((n + 255) / 256);
  if (rt_class_of(RT_F64, variant).var == RT_VAR_FLAT)
    hipLaunchKernelGGL(rt_camera_rays_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, rays, sample);
  else
    hipLaunchKernelGGL(rt_camera_rays_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, rays, sample);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#endif  // !RT_RADIANCE_ORDERED
