// rt_list_kernel.h — the pixel-list kernel and its launcher for ONE precision: included by
// rt_list.hip (RT_F64 0) and rt_list64_nl.hip (RT_F64 1), each its own translation unit.  The per-lane
// logic is rt_list.h over rt_lane.h and rt_trace.h's functions; the render kernels' translation units do not see
// this file and the spill gate does not count this kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_adaptive.h"
#include "rt_kernel_class.h"
#include "rt_trace.h"
#include "rt_list.h"

namespace RT_NS {

// An adaptive pass's samples (rt_adaptive.h): list entry e = {tile pixel, N_p} of the *n_list entries
// the select kernel wrote receives samples [N_p, N_p + n_samples) in chunks: item id = e x n_chunks +
// k covers samples N_p + [k chunk, min(n_samples, (k + 1) chunk)), so consecutive ids are the chunks
// of one pixel and then the next pixel of the ascending list (a wave's lanes on neighbouring pixels).
// The list length is a device word: the grid is sized by the host to fill the device (or by the
// tile, if smaller) and its waves claim 64 consecutive ids at a time from the cursor — P.counter[0],
// zeroed with the pass workspace — until the ids are exhausted; a wave that finds none exits at
// once.  chunk_arg > 0 fixes the chunk (experiments and tests); otherwise it is chosen here from the
// list length so that there are about `fill_lanes` items (the launcher's 16 per resident lane: one-
// sample chunks up to a selection of 131 072 pixels at 16 samples, chunks of 4 at 360 000 — the
// fastest of the chunks measured at both, profiles/adaptive).  A lane sums its chunk in an Acc and
// adds the nonzero words to the pass workspace (P.accum, P.nanflag) at its tile pixel with 64-bit
// integer atomics: the sums do not depend on the chunking or the schedule.  Block and stack: rt_lane.h.
// The kernel's first argument is its KernelParams (rt_trace.h RT_KARGS).
template <int kVar, int kTex, int kMedia, bool kMats, bool kInst, int kLeaf>
__global__ __launch_bounds__(kLaneBlock) void rt_list_kernel(KernelParams P, const rt_adaptive_rec* __restrict__ list,
                                                             const int* __restrict__ n_list, int n_samples, int chunk_arg,
                                                             int fill_lanes) {
  extern __shared__ int smem[];
  const int count = __builtin_amdgcn_readfirstlane(*n_list);
  if (count <= 0) return;
  int chunk = chunk_arg;
  if (chunk <= 0) {
    const int want = max(1, min(n_samples, fill_lanes / count));
    chunk = (n_samples + want - 1) / want;
  }
  chunk = min(chunk, n_samples);
  const int n_chunks = (n_samples + chunk - 1) / chunk;
  const long long n_items = (long long)count * n_chunks;
  const Trav W{smem + threadIdx.x, kLaneBlock, nullptr};
  int overflow = 0;
  for (;;) {
    int base = 0;
    if (threadIdx.x == 0) base = atomicAdd(P.counter, kLaneBlock);
    base = __builtin_amdgcn_readfirstlane(base);
    // wave-uniform exit (a cursor past 2^31 never happens: the launcher bounds the ids); the claim
    // above is reached by the whole wave, the lanes' work below rejoins before the next one
    if (base < 0 || base >= n_items) break;
    const long long id = (long long)base + threadIdx.x;
    if (id < n_items) {  // (the last claim may leave lanes idle; the next claim ends the wave)
      const int e = (int)(id / n_chunks), k = (int)(id - (long long)e * n_chunks);
      const rt_adaptive_rec rec = list[e];
      const int s0 = (int)rec.n + k * chunk, s1 = (int)rec.n + min(n_samples, (k + 1) * chunk);
      Acc A;
      acc_clear(A);
      bool bad = false;
      if (path_pixel<kVar, kTex, kMedia, kMats, kInst, kLeaf>(P, W, rec.tp, s0, s1, A, bad, overflow)) {
        unsigned long long* dst = P.accum + (size_t)RT_ACC_WORDS(real) * (size_t)rec.tp;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (A.hi[c]) atomicAdd(dst + c, (unsigned long long)A.hi[c]);
#if RT_F64
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (A.lo[c]) atomicAdd(dst + 3 + c, A.lo[c]);
#endif
        if (bad) atomicOr(P.nanflag + rec.tp, 1u);
      }
    }
  }
  if (overflow) atomicOr(P.status, 1);
}

typedef void (*list_fn)(KernelParams, const rt_adaptive_rec*, const int*, int, int, int);
// the instantiation of a variant's class: the render's (var, tex, media, mats, inst, leaf) with the
// workgroup size's field cleared; the lockstep BVH base has no list kernel
static list_fn list_kernel_of(int variant) {
  KernelClass cls = rt_class_of(RT_F64, variant);
  cls.narrow = false;
  return rt_with_class(cls, [](auto... k) -> list_fn {
    constexpr KernelClass c{decltype(k)::value...};
    if constexpr (rt_class_compiled(RT_F64, c) && !c.narrow && c.var != RT_VAR_BVH_LOCKSTEP)
      return rt_list_kernel<c.var, c.tex, c.media, c.mats, c.inst, c.leaf>;
    return nullptr;
  });
}

}  // namespace RT_NS

int rt_launch_list(const KernelParamsT<RT_NS::real>& p, int variant, const rt_adaptive_rec* list, const int* n_list,
                   int n_samples, int chunk, void* stream) {
  using namespace RT_NS;
  const long long pixels = (long long)p.tile_rows * p.cam.width;
  if (pixels <= 0 || n_samples <= 0) return 0;
  const list_fn fn = list_kernel_of(variant);
  if (!fn) return -1;
  // the ids a wave claims stay below 2^31: worst case every tile pixel with one-sample chunks, plus
  // one claim per wave of the grid behind the end
  const int resident = kLaneResident;    // the grid
  const int fill_lanes = 16 * resident;  // items to aim for: short chunks even out the lanes' path lengths
  const long long worst = (pixels * n_samples + kLaneBlock - 1) / kLaneBlock;
  const long long blocks = std::min<long long>(worst, resident / kLaneBlock);
  if (pixels * n_samples + (blocks + 1) * kLaneBlock > 0x7fffffffLL) return -1;
  const size_t lds = lane_stack_bytes(variant, p.stack_depth);
  hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(kLaneBlock), lds, (hipStream_t)stream, p, list, n_list, n_samples, chunk,
                     fill_lanes);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
