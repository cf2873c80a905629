// rt_query_kernel.h — the ray-query kernel (include/rt.h rt_scene_cast) and its launcher for ONE
// precision: included by rt_query.hip (RT_F64 0: every class), rt_query64.hip (RT_F64 1: the flat
// class and the launcher) and rt_query64_bvh.hip (RT_F64 1: the BVH classes), each its own
// translation unit.  The per-lane logic is rt_query.h over rt_lane.h and rt_trace.h's closest-hit code; the render
// and feature kernels' translation units do not see this file.
//   RT_QUERY_PART 0: every class and the launcher; 1: the flat class and the launcher; 2: the BVH classes
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernel_class.h"
#include "rt_trace.h"
#include "rt_query.h"

#ifndef RT_QUERY_PART
#define RT_QUERY_PART 0
#endif
// RT_QUERY_ORDERED 1 (rt_query*_ord.hip): the ordered form of the same text under names of its own —
// lane id traces rays[order[id]] into hits[order[id]] (include/rt.h rt_scene_cast_ordered).  The
// unordered units' text is unchanged by it.
#ifndef RT_QUERY_ORDERED
#define RT_QUERY_ORDERED 0
#endif
#if RT_QUERY_ORDERED
#define RT_QUERY_KERNEL rt_query_ordered_kernel
#define RT_QUERY_LAUNCH rt_launch_query_ordered
#define RT_QUERY_BVH_KERNEL rt_query64_bvh_ordered_kernel
#define RT_QUERY_ORDER_PARAM , const uint32_t* __restrict__ order
#define RT_QUERY_ORDER_TYPE , const uint32_t*
#define RT_QUERY_ORDER_ARG , order
#else
#define RT_QUERY_KERNEL rt_query_kernel
#define RT_QUERY_LAUNCH rt_launch_query
#define RT_QUERY_BVH_KERNEL rt_query64_bvh_kernel
#define RT_QUERY_ORDER_PARAM
#define RT_QUERY_ORDER_TYPE
#define RT_QUERY_ORDER_ARG
#endif

namespace RT_NS {

// the records move as 16-byte vectors: a wave's 64 rays are 5 KB contiguous, its hits 6 KB
struct alignas(16) q16 {
  double x, y;
};
static_assert(sizeof(rt_ray) == 5 * sizeof(q16) && sizeof(rt_hit) == 6 * sizeof(q16), "rt.h record sizes");
__device__ __forceinline__ double q_ints(int lo, int hi) {
  return __builtin_bit_cast(double, (unsigned long long)(unsigned)lo | ((unsigned long long)(unsigned)hi << 32));
}

// One lane per ray, in the caller's order: lane id traces rays[id] into hits[id] — the caller's
// coherence is the kernel's — or, in the ordered form, rays[order[id]] into hits[order[id]]
// (rt_order.hip makes such orders).  Nothing is compacted.  Block and stack: rt_lane.h.  The
// kernel's first argument is its KernelParams, as the render kernels' (rt_trace.h RT_KARGS).
template <int kVar, bool kInst, int kLeaf>
__global__ __launch_bounds__(kLaneBlock) void RT_QUERY_KERNEL(KernelParams P, const rt_ray* __restrict__ rays,
                                                               rt_hit* __restrict__ hits, const int* __restrict__ prim_mat,
                                                               long long n, int flags RT_QUERY_ORDER_PARAM) {
  extern __shared__ int smem[];
#if RT_QUERY_ORDERED
  // an entry that is no record's index is skipped: nothing is read or written for it
  const long long slot = (long long)blockIdx.x * kLaneBlock + threadIdx.x;
  if (slot >= n) return;
  const long long id = (long long)order[slot];
  if (id >= n) return;
#else
  const long long id = (long long)blockIdx.x * kLaneBlock + threadIdx.x;
  if (id >= n) return;
#endif
  const q16* rp = reinterpret_cast<const q16*>(rays + id);
  const q16 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3], r4 = rp[4];
  const rt_ray q{{r0.x, r0.y, r1.x}, {r1.y, r2.x, r2.y}, r3.x, r3.y, r4.x, 0.0};
  const Trav W{smem + threadIdx.x, kLaneBlock, nullptr};
  rt_hit H;
  int overflow = 0;
  query_ray<kVar, kInst, kLeaf>(P, P.prims, prim_mat, W, q, flags, H, overflow);
  q16* hp = reinterpret_cast<q16*>(hits + id);
  hp[0] = q16{H.t, H.point[0]};
  hp[1] = q16{H.point[1], H.point[2]};
  hp[2] = q16{H.normal[0], H.normal[1]};
  hp[3] = q16{H.normal[2], H.uv[0]};
  hp[4] = q16{H.uv[1], q_ints(H.hit, H.front)};
  hp[5] = q16{q_ints(H.leaf, H.instance), q_ints(H.material, 0)};
  if (overflow) atomicOr(P.status, 1);
}

typedef void (*query_fn)(KernelParams, const rt_ray*, rt_hit*, const int*, long long, int RT_QUERY_ORDER_TYPE);
// the instantiation of a class: rt_kernel_class.h's dispatch, with every field a surface hit does
// not see (texture level, media mode, material set, workgroup size) at its first value — only
// var x inst x leaf is instantiated
template <bool kFlatPart>
static query_fn query_kernel_of_class(KernelClass cls) {
  cls.tex = 0;
  cls.media = 0;
  cls.mats = false;
  cls.narrow = false;
  return rt_with_class(cls, [](auto... k) -> query_fn {
    constexpr KernelClass c{decltype(k)::value...};
    if constexpr (rt_class_compiled(RT_F64, c) && c.tex == 0 && c.media == 0 && !c.mats && !c.narrow &&
                  c.var != RT_VAR_BVH_LOCKSTEP && (c.var == RT_VAR_FLAT) == kFlatPart)
      return RT_QUERY_KERNEL<c.var, c.inst, c.leaf>;
    return nullptr;
  });
}

}  // namespace RT_NS

#if RT_QUERY_PART == 2
void* RT_QUERY_BVH_KERNEL(KernelClass cls) { return (void*)RT_NS::query_kernel_of_class<false>(cls); }
#else
#if RT_QUERY_PART == 1
void* RT_QUERY_BVH_KERNEL(KernelClass cls);  // rt_query64_bvh.hip (rt_query64_bvh_ord.hip)
#endif

int RT_QUERY_LAUNCH(const KernelParamsT<RT_NS::real>& p, int variant, const rt_ray* rays, rt_hit* hits,
                    const int* prim_mat, long long n, int flags RT_QUERY_ORDER_PARAM, void* stream) {
  using namespace RT_NS;
  if (n <= 0) return 0;
  const KernelClass c = rt_class_of(RT_F64, variant);
  query_fn fn = nullptr;
  if (c.var == RT_VAR_FLAT) fn = query_kernel_of_class<true>(c);
#if RT_QUERY_PART == 1
  else fn = (query_fn)RT_QUERY_BVH_KERNEL(c);
#else
  else fn = query_kernel_of_class<false>(c);
#endif
  if (!fn) return -1;
  const long long blocks = (n + kLaneBlock - 1) / kLaneBlock;
  if (blocks > 0x7fffffffLL) return -1;
  const size_t lds = lane_stack_bytes(variant, p.stack_depth);
  hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(kLaneBlock), lds, (hipStream_t)stream, p, rays, hits, prim_mat, n,
                     flags RT_QUERY_ORDER_ARG);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#endif
