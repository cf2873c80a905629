// rt_features_kernel.h — the first-hit feature kernel and its launcher for ONE precision: included
// by rt_features.hip (RT_F64 0) and rt_features64_nl.hip (RT_F64 1), each its own translation unit.
// The per-lane logic is rt_features.h over rt_lane.h and rt_trace.h's closest-hit code; the render kernels'
// translation units do not see this file.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_denoise.h"
#include "rt_kernel_class.h"
#include "rt_trace.h"
#include "rt_features.h"

namespace RT_NS {

// One lane per (tile pixel, sample chunk): lane id = tile pixel x n_chunks + chunk, chunk k covers
// samples [k chunk, min(n_feat, (k + 1) chunk)).  The lane sums its samples' 8 words in registers
// and adds the nonzero ones to the pixel's words (rt_feat_words per pixel) with 64-bit integer atomics (commutative: the buffer
// is the same for any chunking and schedule).  Block and stack: rt_lane.h.  The kernel's first
// argument is its KernelParams, as the render kernels'.
template <int kVar, int kTex, int kMedia, bool kInst, int kLeaf>
__global__ __launch_bounds__(kLaneBlock) void rt_feature_kernel(KernelParams P, unsigned long long* __restrict__ feat,
                                                                long long n_lanes, int n_feat, int chunk, int n_chunks) {
  extern __shared__ int smem[];
  const long long id = (long long)blockIdx.x * kLaneBlock + threadIdx.x;
  if (id >= n_lanes) return;
  const int tp = (int)(id / n_chunks), k = (int)(id - (long long)tp * n_chunks);
  const int s0 = k * chunk, s1 = min(n_feat, s0 + chunk);
  const Trav W{smem + threadIdx.x, kLaneBlock, nullptr};
  FeatAcc A{};
  int overflow = 0;
  if (!feature_pixel<kVar, kTex, kMedia, kInst, kLeaf>(P, W, tp, s0, s1, A, overflow)) return;
  unsigned long long* dst = feat + (size_t)rt_feat_words(RT_F64) * (size_t)tp;
#pragma unroll
  for (int w = 0; w < RT_FEAT_WORDS; ++w)
    if (A.w[w]) atomicAdd(dst + w, (unsigned long long)A.w[w]);
#if RT_F64
#pragma unroll
  for (int w = 0; w < RT_FEAT_WORDS - 1; ++w)
    if (A.lo[w]) atomicAdd(dst + RT_FEAT_WORDS + w, A.lo[w]);
#endif
  if (overflow) atomicOr(P.status, 1);
}

typedef void (*feature_fn)(KernelParams, unsigned long long*, long long, int, int, int);
// the instantiation of a variant's class: rt_kernel_class.h's table and dispatch, with the fields
// a first hit does not see (material set, workgroup size) at their first value
static feature_fn feature_kernel_of(int variant) {
  KernelClass cls = rt_class_of(RT_F64, variant);
  cls.mats = false;
  cls.narrow = false;
  return rt_with_class(cls, [](auto... k) -> feature_fn {
    constexpr KernelClass c{decltype(k)::value...};
    if constexpr (rt_class_compiled(RT_F64, c) && !c.mats && !c.narrow && c.var != RT_VAR_BVH_LOCKSTEP)
      return rt_feature_kernel<c.var, c.tex, c.media, c.inst, c.leaf>;
    return nullptr;
  });
}

}  // namespace RT_NS

int rt_launch_features(const KernelParamsT<RT_NS::real>& p, int variant, unsigned long long* feat, int n_feat,
                       void* stream) {
  using namespace RT_NS;
  const long long pixels = (long long)p.tile_rows * p.cam.width;
  if (pixels <= 0 || n_feat <= 0) return 0;
  const feature_fn fn = feature_kernel_of(variant);
  if (!fn) return -1;
  // enough lanes to fill the device where the tile alone does not
  int n_chunks = (int)std::min<long long>(n_feat, std::max<long long>(1, (kLaneResident + pixels - 1) / pixels));
  const int chunk = (n_feat + n_chunks - 1) / n_chunks;
  n_chunks = (n_feat + chunk - 1) / chunk;
  const long long n_lanes = pixels * n_chunks;
  const long long blocks = (n_lanes + kLaneBlock - 1) / kLaneBlock;
  if (blocks > 0x7fffffffLL) return -1;
  const size_t lds = lane_stack_bytes(variant, p.stack_depth);
  hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(kLaneBlock), lds, (hipStream_t)stream, p, feat, n_lanes, n_feat, chunk,
                     n_chunks);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
