// rt_render_kernel.h — the persistent path-tracing megakernel, the fixed-point resolve and
// their launchers for ONE precision: included by rt_kernel.hip (RT_F64 0, float) and
// rt_kernel64.hip (RT_F64 1, binary64), each its own translation unit (built in parallel).
// The per-lane logic lives in rt_trace.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "rt_kernel_class.h"
#include "rt_trace.h"

namespace RT_NS {

// Diagnostic build only (make exp DEFS=-DRT_WAVE_STAMPS, tools/wave_stamps.py): per wave the
// wall clock (s_memrealtime, 100 MHz) at its start, when its grab first finds every queue spent
// (the queue has drained: from then on the wave only finishes the items it holds) and at its end,
// and its hardware id — the ramp and the tail of one launch, wave by wave.
#if defined(RT_WAVE_STAMPS)
#define RT_STAMP_WAVES 16384
static __device__ unsigned long long rt_stamp_buf[4 * RT_STAMP_WAVES];  // (one per translation unit)
#endif

namespace {

// Item claims.  A wave keeps a pool of consecutive item ids in SGPRs (wave-uniform state) and
// refills it with ONE returning atomicAdd of RT_POOL ids, so the global head word sees one
// atomic per RT_POOL claims instead of one per refilling wave-iteration (a single word saturates at
// ~88 returning atomics per microsecond, MI355X_MICROARCH.md "dequeue").  Lanes that need work
// take ids in lane order; ids are never dropped (a pool is contiguous and increasing, so once a
// lane draws an id >= n_items every later id is out of range too).
static_assert(RT_POOL >= 64, "a refill must cover every lane of a wave");
// The dynamic ids [offset, n_items) are split into RT_QUEUES contiguous ranges, each with its own
// head word (256 B apart): a wave starts on queue (wave % RT_QUEUES) and moves to the next one
// when its queue is spent, so each word sees 1 / RT_QUEUES of the refills.  Measured (kernel ms,
// 1 / 2 / 4 / 8 queues): README 0.315 / 0.282 / 0.285 / 0.29 (its cheap samples ran the single
// word near its returning-atomic rate), README on 2 GPUs 0.191 / 0.189 / 0.177 / 0.180, Cornell
// 3.455 / 3.42 / 3.42 / 3.43, Cornell's 8-GPU share 0.520 / 0.517 / 0.517 / 0.519.
#ifndef RT_QUEUES
#define RT_QUEUES 4
#endif
// How the queues split the dynamic ids.  Contiguous quarters (0, rounds 3-4) put the big items
// (the first ids) in the first queues and the small tail items in the last: the waves of a spent
// queue move on to the next, so the frame ENDED on the big items of the last queue to drain — the
// per-wave stamps of one binary64 Cornell launch (tools/wave_stamps.py, profiles/r5/) showed the
// queue drained at 4.78 ms and the last wave ending 1.30 ms later.  Interleaved pools (1): queue q
// serves pools q, q + RT_QUEUES, ... of RT_POOL ids, so every queue walks the ids in order and the
// tail items come last, as rt_host_plan_work intends.
#ifndef RT_QUEUE_INTERLEAVE
#define RT_QUEUE_INTERLEAVE 1
#endif
static_assert((RT_QUEUES & (RT_QUEUES - 1)) == 0 && RT_QUEUES <= 8, "RT_QUEUES: a power of two, at most 8 (workspace)");
// Per-wave commit aggregation.  Ids are pixel-major (rt_trace.h open_item), so the RT_POOL
// consecutive ids of one pool cover a few pixels: when a pool is opened the wave gives it one of
// its kSlots LDS slots (kPix pixels x RT_ACC_WORDS words, pixel-major like `accum`, plus a header:
// ids still open, first tile pixel; the item carries slot + 1, rt_trace.h ItemCtx).  A finished
// item adds its words to the slot with LDS atomics instead of 64-bit atomics to HBM and counts
// its id off; once a pool's ids are all committed the wave adds the slot's words to `accum` —
// consecutive addresses, one atomic per nonzero word per (pixel, pool) instead of per item — and
// frees the slot (lazily: when a new pool finds no free slot, and at the end).  A slot belongs to one wave
// (so no synchronisation beyond the wave's own LDS order); the ids of a pool are claimed by that
// wave only.  Pools the host did not qualify (a phase with few chunks per pixel, the pool that
// straddles the two item sizes) or that find every slot busy commit directly, as before.  Integer
// sums: the image is bit-identical either way.
// (keeping the item's pixel offset within the slot in its code, resolved at the item's start
// instead of one LDS read at its commit, measured no faster: Cornell f64 5.77 vs 5.74 ms)
// the 64-bit words of one aggregation slot (rt_kernel_class.h rt_class_agg_bytes: its LDS per wave)
template <int kSlots, int kPix>
struct AggGeom { static constexpr int kWords = kPix * RT_ACC_WORDS(real); };

// The work queue of the flat kernels re-reads its kernel-argument fields at each use; the BVH
// kernels' does in FP32 only (binary64 demo1 / pawn+fog -0.7 % with them held, Cornell's flat
// binary64 kernel +0.7 %: profiles/r4/kargs_phase_ab, r4/pp_ab)
#ifndef RT_KARGS_WORK_BVH
#define RT_KARGS_WORK_BVH (!RT_F64)
#endif
// kReread: the queue's kernel-argument fields re-read at each use (rt_trace.h RT_KARGS) or held
template <int kSlots, int kPix, bool kReread>
struct WaveWork {
  const KernelParams& P;
  // item claims: a pool of consecutive ids in SGPRs (wave-uniform state), refilled with ONE
  // returning atomicAdd of RT_POOL ids, so the head word sees one atomic per RT_POOL claims (a
  // single word saturates at ~88 returning atomics per microsecond, MI355X_MICROARCH.md
  // "dequeue").  Lanes that need work take ids in lane order; ids are never dropped (a pool is
  // contiguous and increasing, so once a lane draws an id >= n_items every later id is too).
  int pool;    // ids per pool: 1 << kp().pool_shift (the host's choice per launch, RT_POOL by default)
  int pool_base;
  int pool_left;
  int offset;  // ids [0, offset) are the waves' initial pools, handed out without atomics
  int queue;   // the queue this wave refills from
  int spent;   // queues found spent (RT_QUEUES: every id is claimed)
  int pool_slot;  // the current pool's slot (-1: direct commits)
  // aggregation: this wave's slots [kSlots][kWords] and header [open ids x kSlots, tplo x kSlots]
  unsigned long long* slots;
  int* hdr;
  unsigned free_mask;  // wave-uniform
#if defined(RT_WAVE_STAMPS)
  unsigned long long t_drain = 0;  // wall clock when every queue was first found spent
#endif
  // the kernel arguments re-read where used (rt_trace.h RT_KARGS): not held across the lane loop
  __device__ __forceinline__ const KernelParams& kp() const { return RT_KARGS_IF(kReread, P); }

  __device__ __forceinline__ WaveWork(const KernelParams& P_, int wave, int waves, unsigned long long* slots_)
      : P(P_), pool(1 << P_.pool_shift), pool_base(wave * pool), pool_left(pool), offset(waves * pool),
        queue(wave & (RT_QUEUES - 1)),
        spent(0), pool_slot(-1), slots(slots_),
        hdr(reinterpret_cast<int*>(slots_ + kSlots * AggGeom<kSlots, kPix>::kWords)),
        free_mask(kSlots > 0 ? (1u << kSlots) - 1u : 0u) {
#if defined(RT_NO_STATIC_POOLS)
    // (experiment: every pool from the queues, none by wave index)
    pool_left = 0;
    offset = 0;
#else
    // every wave starts with a static pool (its wave index x pool): at launch all resident
    // waves would otherwise queue up on the counter at once (~80 us at ~88 returning atomics per us)
    pool_slot = open_pool(pool_base, min(pool, P.n_items - pool_base));
#endif
  }

  // a slot for the pool of ids [b0, b0 + cnt) (wave-uniform), or -1: commit its items directly.
  // Slots are reclaimed here, lazily: when none is free, every slot whose ids are all committed
  // is flushed (so the commit path itself never waits on an LDS return or branches to a flush)
  __device__ __forceinline__ int open_pool(int b0, int cnt) {
    if (kSlots == 0 || cnt <= 0) return -1;
    const bool big = b0 < kp().big_items;
    if (big ? (!kp().agg_big || b0 + cnt > kp().big_items) : !kp().agg_small) return -1;
    if (free_mask == 0u) reclaim();
    if (free_mask == 0u) return -1;
    const int tplo = (int)fast_div((uint32_t)(big ? b0 : b0 - kp().big_items), big ? kp().div_big : kp().div_small);
    const int s = __builtin_ctz(free_mask);
    free_mask &= free_mask - 1u;
    hdr[s] = cnt;  // every active lane stores the same words
    hdr[kSlots + s] = tplo;
    return s;
  }
  __device__ __forceinline__ void reclaim() {
#pragma unroll 1
    for (int s = 0; s < kSlots; ++s)
      if (__builtin_amdgcn_readfirstlane(hdr[s]) == 0) flush(s);
  }
  // after the lane loop (every lane of the wave back): flush the slots still held
  __device__ __forceinline__ void finish() {
#pragma unroll 1
    for (int s = 0; s < kSlots; ++s)
      if (!((free_mask >> s) & 1u)) flush(s);
  }

  // wave-collective: a fresh item for lanes with need (n_items once every id is claimed), with
  // its pool's slot
  __device__ __forceinline__ int grab(bool need, int& slot) {
    slot = pool_slot;
    const unsigned long long m = __ballot(need);
    if (m == 0ull) return 0;
    const int lane = (int)__lane_id();
    const int cnt = (int)__popcll(m);
    const int rank = (int)__popcll(m & ((1ull << lane) - 1ull));
    if (pool_left >= cnt) {
      const int item = pool_base + rank;
      pool_base += cnt;
      pool_left -= cnt;
      return item;
    }
    // ranks [0, pool_left) drain the pool; the others are served by refills, in rank order
    const int n_items = kp().n_items;
    int item = rank < pool_left ? pool_base + rank : n_items;
    int first = pool_left, rest = cnt - pool_left;
    pool_left = 0;
    const int leader = __ffsll((unsigned long long)m) - 1;
    const int dyn = n_items - offset;
#if RT_QUEUE_INTERLEAVE
    const int n_pools = dyn > 0 ? (dyn + pool - 1) / pool : 0;
#else
    const int len = dyn > 0 ? (dyn + RT_QUEUES - 1) / RT_QUEUES : 0;
#endif
    while (rest > 0 && spent < RT_QUEUES) {
#if RT_QUEUE_INTERLEAVE
      // queue q hands out the dynamic pools q, q + RT_QUEUES, q + 2 RT_QUEUES, ... (one counter
      // increment per pool): the ids are claimed in (nearly) global order whatever queue a wave
      // draws from, so the frame ends with the last, smallest items
      int pk = 0;
      if (lane == leader) pk = atomicAdd(kp().counter + 64 * queue, 1);
      pk = __builtin_amdgcn_readfirstlane(__shfl(pk, leader));
      const int qs = offset, qlen = dyn;
      if (pk * RT_QUEUES + queue >= n_pools) {  // spent: the queue's next pool is past the last one
#else
      const int qs = offset + queue * len;
      const int qlen = min(len, n_items - qs);  // <= 0 for an empty last queue
      int base = 0;
      if (lane == leader) base = atomicAdd(kp().counter + 64 * queue, pool);
      base = __builtin_amdgcn_readfirstlane(__shfl(base, leader));
      if (base >= qlen) {  // spent: ids are only ever handed out below qlen
#endif
        queue = (queue + 1) & (RT_QUEUES - 1);
        ++spent;
#if defined(RT_WAVE_STAMPS)
        if (spent == RT_QUEUES && t_drain == 0) t_drain = wall_clock64();
#endif
        continue;
      }
#if RT_QUEUE_INTERLEAVE
      const int base = (pk * RT_QUEUES + queue) * pool;
#endif
      const int avail = min(pool, qlen - base);
      const int take = min(rest, avail);
      pool_slot = open_pool(qs + base, avail);
      if (rank >= first && rank < first + take) {
        item = qs + base + (rank - first);
        slot = pool_slot;
      }
      first += take;
      rest -= take;
      pool_base = qs + base + take;
      pool_left = avail - take;
      if (rest > 0) {  // the pool ended at the queue's end (interleaved: the last, short pool)
        queue = (queue + 1) & (RT_QUEUES - 1);
        ++spent;
      }
    }
    return item;
  }

  // wave-collective: lanes with c add their finished item's fixed-point sums (rt_trace.h Acc:
  // [hi.xyz] or [hi.xyz, lo.xyz]; zero words are skipped) to its pool's slot, or to `accum`
  __device__ __forceinline__ void direct(int tp, const Acc& A) const {
    unsigned long long* a = kp().accum + RT_ACC_WORDS(real) * (size_t)tp;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (A.hi[c]) atomicAdd(a + c, (unsigned long long)A.hi[c]);
#if RT_F64
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (A.lo[c]) atomicAdd(a + 3 + c, A.lo[c]);
#endif
  }
  // an item's tile pixel tagged with its slot code in bits 24-31 (rt_trace.h ItemCtx::tp): slot +
  // 1, or 0 for direct commits.  The code exists only in launches that aggregate (kp().agg_big |
  // kp().agg_small, set by the host for tiles below 2^24 pixels); elsewhere the word is the plain tile
  // pixel, whose bits 24-30 may be set (tiles up to 2^31 pixels), and commit must not decode it
  __device__ __forceinline__ bool aggregating() const { return kSlots > 0 && (kp().agg_big | kp().agg_small) != 0; }
  // an item's plain tile pixel (its slot code cleared; rt_trace.h steal_sample)
  __device__ __forceinline__ int untag(int tpk) const { return aggregating() ? (tpk & 0xffffff) : tpk; }
  __device__ __forceinline__ int tag(int tp, int slot) const {
    if (slot < 0) return tp;
    return tp | ((slot + 1) << 24);
  }
  template <class AccT>
  __device__ __forceinline__ void commit(bool c, int tpk, const AccT& acc, bool bad) {
    if (!c) return;
    const int code = aggregating() ? (int)((uint32_t)tpk >> 24) : 0;
    const int tp = code ? tpk & 0xffffff : tpk;
    const Acc A = acc_words(acc);
    if (code == 0) {
      direct(tp, A);
    } else {
      const int s = code - 1;
      unsigned long long* w = slots + s * AggGeom<kSlots, kPix>::kWords + (tp - hdr[kSlots + s]) * RT_ACC_WORDS(real);
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (A.hi[k]) lds_add(w + k, (unsigned long long)A.hi[k]);
#if RT_F64
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (A.lo[k]) lds_add(w + 3 + k, A.lo[k]);
#endif
      __hip_atomic_fetch_add(hdr + s, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // no return
    }
    if (bad) atomicOr(kp().nanflag + tp, 1u);
  }
  // The ring form (rt_trace.h lane_loop_flat_ring) commits every sample (64 wide at a refill:
  // flush_ring), so the slot's pixel is resolved where the id is opened, by the whole
  // wave: the code carries the slot + 1 in bits 24-26 and the pixel's offset within the slot in bits
  // 27-31 (tag_ring), and the commit adds the sample's words without reading the header or testing
  // them for zero (one exec region instead of seven)
  __device__ __forceinline__ int tag_ring(int tp, int slot) const {
    static_assert(kSlots <= 7 && kPix <= 32, "tag_ring: 3 bits of slot + 1, 5 bits of pixel offset");
    if (slot < 0) return tp;
    return (int)((uint32_t)tp | (uint32_t)((slot + 1) | ((tp - hdr[kSlots + slot]) << 3)) << 24);
  }
  // counts an id that has no sample (a padding row, a render without depth) off its pool's slot
  __device__ __forceinline__ void skip_ring(bool c, int tpk) {
    if (!c || !aggregating()) return;
    const int code = (int)((uint32_t)tpk >> 24) & 7;
    if (code) __hip_atomic_fetch_add(hdr + code - 1, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ __forceinline__ void commit_ring(int tpk, const Acc& A, bool bad) {
    const uint32_t code = aggregating() ? (uint32_t)tpk >> 24 : 0u;
    const int tp = code ? tpk & 0xffffff : tpk;
    if (code == 0u) {
      direct(tp, A);
    } else {
      const int s = (int)(code & 7u) - 1;
      unsigned long long* w = slots + s * AggGeom<kSlots, kPix>::kWords + (int)(code >> 3) * RT_ACC_WORDS(real);
#pragma unroll
      for (int k = 0; k < 3; ++k) lds_add(w + k, (unsigned long long)A.hi[k]);
#if RT_F64
#pragma unroll
      for (int k = 0; k < 3; ++k) lds_add(w + 3 + k, A.lo[k]);
#endif
      __hip_atomic_fetch_add(hdr + s, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // no return
    }
    if (bad) atomicOr(kp().nanflag + tp, 1u);
  }
  // add a closed slot's words to `accum` (consecutive pixels: consecutive addresses) and free it
  __device__ __forceinline__ void flush(int s) {
    constexpr int kW = AggGeom<kSlots, kPix>::kWords;
    const unsigned long long act = __ballot(true);
    const int k = (int)__popcll(act);
    const int r = (int)__popcll(act & ((1ull << __lane_id()) - 1ull));
    const int tplo = __builtin_amdgcn_readfirstlane(hdr[kSlots + s]);
    const long long g0 = (long long)tplo * RT_ACC_WORDS(real);
    const long long g_end = (long long)kp().tile_rows * kp().cam.width * RT_ACC_WORDS(real);
    unsigned long long* w = slots + s * kW;
    for (int j = r; j < kW; j += k) {
      const unsigned long long v = w[j];
      if (v != 0ull) {
        w[j] = 0ull;
        if (g0 + j < g_end) atomicAdd(kp().accum + g0 + j, v);
      }
    }
    free_mask |= 1u << s;
  }
};

}  // namespace

// One instantiation per kernel class (rt_kernel_class.h: the template parameters are KernelClass's
// fields; launch bound, occupancy floor, stack stride and LDS layout are its functions of them)
#ifndef RT_TU_NOLICM
#define RT_TU_NOLICM 0
#endif
template <int kVar, int kTex, int kMedia, bool kMats, bool kInst, int kLeaf, bool kNarrow = false>
__global__ __launch_bounds__(rt_class_block(RT_F64, KernelClass{kVar, kTex, kMedia, kMats, kInst, kLeaf, kNarrow}))
__attribute__((amdgpu_waves_per_eu(rt_class_waves(RT_F64, KernelClass{kVar, kTex, kMedia, kMats, kInst, kLeaf, kNarrow}))))
void rt_render_kernel(KernelParams P) {
  extern __shared__ int smem[];
#if defined(RT_WAVE_STAMPS)
  const unsigned long long t_start = wall_clock64();
#endif
  constexpr KernelClass kC{kVar, kTex, kMedia, kMats, kInst, kLeaf, kNarrow};
  constexpr int kSlots = rt_class_agg_slots(RT_F64, kC), kPix = rt_class_agg_pix(RT_F64, kC);
#if defined(RT_BLOCK_RUNTIME)  // (experiment: the stack stride from blockDim; profiles/r5/bigwg, r6/nondet)
  const int block = (int)blockDim.x;
#else
  constexpr int block = rt_class_block(RT_F64, kC);
#endif
  // (experiments, profiles/r6/nondet: one use of the launch-time workgroup size at a time)
#if defined(RT_BLOCK_RUNTIME_STACK)
  const int block_stack = (int)blockDim.x;
#else
  const int block_stack = block;
#endif
#if defined(RT_BLOCK_RUNTIME_NODES)
  const int block_nodes = (int)blockDim.x;
#else
  const int block_nodes = block;
#endif
#if defined(RT_BLOCK_RUNTIME_COPY)
  const int block_copy = (int)blockDim.x;
#else
  const int block_copy = block;
#endif
  constexpr int kAggBytes = rt_class_agg_bytes(RT_F64, kC);
  const int waves = (int)(gridDim.x * (blockDim.x / 64));
  // wave-uniform (readfirstlane: the compiler cannot tell that threadIdx.x / 64 is), so the work
  // state and the slot pointers below live in SGPRs
  const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
  const int wave = (int)blockIdx.x * (int)(blockDim.x / 64) + wave_in_block;
  int overflow;
  // LDS: the lanes' item sums [RT_ACC_WORDS][block] (rt_trace.h AccLds; BVH kernels), the waves'
  // commit-aggregation slots (kAggBytes each), then (BVH kernels) [stack_depth + 1][block]
  // stack words (the last row a spare write target) and the top P.lds_nodes BVH nodes (64 B each)
  using AccT = typename std::conditional<rt_class_acc_lds(RT_F64, kC), AccLds, Acc>::type;
  AccT acc;
  int* smem_rest = smem;
  if constexpr (rt_class_acc_lds(RT_F64, kC)) {
    acc = AccLds{reinterpret_cast<unsigned long long*>(smem) + threadIdx.x, (int)blockDim.x};
    smem_rest = smem + 2 * RT_ACC_WORDS(real) * (int)blockDim.x;
  }
  // this wave's slots, zeroed by the wave itself (nothing else touches them: no barrier)
  unsigned long long* agg = reinterpret_cast<unsigned long long*>(smem_rest) + kAggBytes / 8 * wave_in_block;
  smem_rest += kAggBytes / 4 * (int)(blockDim.x / 64);
  for (int i = (int)__lane_id(); i < kAggBytes / 8; i += 64) agg[i] = 0ull;
#if defined(RT_WAVE_STAMPS)
  // (vector stores from lane 0; waves beyond the buffer are not recorded)
#define RT_STAMP_END(work)                                                                        \
  if (__lane_id() == 0 && wave < RT_STAMP_WAVES) {                                                \
    rt_stamp_buf[4 * wave] = t_start;                                                             \
    rt_stamp_buf[4 * wave + 1] = work.t_drain;                                                    \
    rt_stamp_buf[4 * wave + 2] = wall_clock64();                                                  \
    rt_stamp_buf[4 * wave + 3] = (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (31 << 11)) << 32 | \
                                 (unsigned)__builtin_amdgcn_s_getreg((20 << 0) | (3 << 11));      \
  }
#else
#define RT_STAMP_END(work)
#endif
  if constexpr (kVar == RT_VAR_FLAT) {
    WaveWork<kSlots, kPix, true> work(P, wave, waves, agg);
    overflow = lane_loop_lockstep<true, kTex, kMedia != 0, kMats>(P, work, Trav{nullptr, 0, nullptr}, P.prims, acc);
    work.finish();
    RT_STAMP_END(work)
  } else {
    v4f* lds_nodes = reinterpret_cast<v4f*>(smem_rest + (P.stack_depth + 1) * block_nodes);
    const float4* src = reinterpret_cast<const float4*>(P.nodes);
    for (int i = threadIdx.x; i < 4 * P.lds_nodes; i += block_copy) {
      const float4 q = src[i];
      lds_nodes[i] = v4f{q.x, q.y, q.z, q.w};
    }
    __syncthreads();
    WaveWork<kSlots, kPix, RT_KARGS_WORK_BVH> work(P, wave, waves, agg);
    const Trav W{smem_rest + threadIdx.x, block_stack, lds_nodes};
    if constexpr (kVar == RT_VAR_BVH_LOCKSTEP)
      overflow = lane_loop_lockstep<false, kTex, kMedia != 0, kMats>(P, work, W, P.prims, acc);
    else
      overflow = lane_loop_bvh<kTex, kMedia, kMats, kInst, kLeaf>(P, work, W, P.prims, acc);
    work.finish();
    RT_STAMP_END(work)
  }
  if (overflow) atomicOr(P.status, 1);
}

// The ring kernel's translation unit.  The form that stores camera rays (FP32) is compiled with
// MachineLICM, as rt_ring_class's legacy kernel.  The form that traces the camera segments at the
// refill (RT_RING_PRIMARY_*; binary64) holds a second closest hit and shade while the other lanes'
// paths are live: with the pass's hoisted constants on top it spilled 44 VGPRs at the class's 5
// waves; without the pass it fits the 96 VGPRs with none
#define RT_RING_NOLICM (RT_F64 ? RT_RING_PRIMARY_F64 : RT_RING_PRIMARY_F32)
#if RT_TU_NOLICM == RT_RING_NOLICM
// The ring form of rt_ring_class's kernel (rt_trace.h lane_loop_flat_ring; launched when
// KernelParams::flat_ring): a one-wave workgroup at the class's occupancy floor.  LDS: the ring's
// rays, then this wave's aggregation slots (rt_kernel_class.h rt_ring_lds_bytes).
__global__ __launch_bounds__(RT_BLOCK) __attribute__((amdgpu_waves_per_eu(rt_class_waves(RT_F64, rt_ring_class()))))
void rt_render_kernel_ring(KernelParams P) {
  extern __shared__ int smem[];
  real* ring_od = reinterpret_cast<real*>(smem);
  uint32_t* ring_meta = reinterpret_cast<uint32_t*>(ring_od + rt_ring_reals(RT_F64) * RT_RING_LANES);
  unsigned long long* agg = reinterpret_cast<unsigned long long*>(ring_meta + rt_ring_words(RT_F64) * RT_RING_LANES);
  constexpr int kAggBytes = rt_ring_agg_bytes(RT_F64);
  for (int i = (int)__lane_id(); i < kAggBytes / 8; i += 64) agg[i] = 0ull;
  WaveWork<rt_ring_agg_slots(RT_F64), RT_RING_AGG_PIX, true> work(P, (int)blockIdx.x, (int)gridDim.x, agg);
  lane_loop_flat_ring(P, work, ring_od, ring_meta);
  work.finish();
}
#endif

#ifndef RT_KERNEL_ONLY  // (register probes of one instantiation: tools/reg_probe.sh)
#if !RT_TU_NOLICM  // (the main translation unit)
// mean over spp (Ray.hs:232) from the fixed-point sums; NaN where a sample was non-finite.  One
// thread per output word (blockIdx.y = the channel) and the FP32 scale from the host: the kernel
// needs at most 8 VGPRs.  The FP32 Cornell class (63 VGPRs at 8 waves per SIMD) takes every wave
// slot, so beside the next frame's render grid the resolve's waves start as that grid's waves end,
// not in registers it leaves free.  frame_rows > 0:
// `out` is the whole frame and tile row t goes to its global row (the rt_exec row interleave; rows
// past the image are padding and are skipped) — a multi-device scene's shards resolve straight into
// the first device's frame over xGMI instead of being gathered by copies afterwards
__global__ __launch_bounds__(256) void rt_resolve_kernel(const long long* __restrict__ accum,
                                                         const unsigned int* __restrict__ nanflag,
                                                         real* __restrict__ out, int n_pixels, int spp, double scale,
                                                         int width, int frame_rows, int n_shards, int shard,
                                                         int row_block) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pixels) return;
  size_t w = 3 * (size_t)i + blockIdx.y;
  if (frame_rows > 0) {
    const int t = i / width, px = i - t * width;
    const int g = ((t / row_block) * n_shards + shard) * row_block + t % row_block;
    if (g >= frame_rows) return;
    w = 3 * ((size_t)g * width + px) + blockIdx.y;
  }
  const bool bad = nanflag[i] != 0u;
#if RT_F64
  // (hi + lo 2^-32) 2^-32 / spp: the integer words are exact in binary64 (< 2^53), one rounding
  // for the sum, one for the mean
  (void)scale;
  const long long* a = accum + 6 * (size_t)i + blockIdx.y;
  const double sum = ((double)a[0] + (double)(unsigned long long)a[3] * (1.0 / RT_FIX_SCALE)) * (1.0 / RT_FIX_SCALE);
  out[w] = bad ? __builtin_nan("") : sum / (double)spp;
#else
  (void)spp;
  out[w] = bad ? __builtin_nanf("") : (float)((double)accum[3 * (size_t)i + blockIdx.y] * scale);  // scale = 2^-32 / spp
#endif
}
#endif

typedef void (*render_fn)(KernelParams);
// the instantiation of a variant's class (rt_kernel_class.h rt_class_of), or null when the other
// translation unit holds it (rt_class_nolicm); the units instantiate exactly the compiled classes
static render_fn render_kernel_this_tu(int variant) {
  return rt_with_class(rt_class_of(RT_F64, variant), [](auto... k) -> render_fn {
    constexpr KernelClass c{decltype(k)::value...};
    if constexpr (rt_class_compiled(RT_F64, c) && rt_class_nolicm(RT_F64, c) == (bool)RT_TU_NOLICM)
      return rt_render_kernel<c.var, c.tex, c.media, c.mats, c.inst, c.leaf, c.narrow>;
    return nullptr;
  });
}
// the kernels of the translation unit without MachineLICM (defined there)
render_fn render_kernel_nolicm(int variant);
// diagnostic builds: each translation unit's kernels count into that unit's own buffers; the
// main unit's readers add the other's (a wave's stamps come from one launch: the other is zero)
template <class T, size_t N>
static int diag_read(T (&buf)[N], unsigned long long* out, size_t n) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(buf), n * sizeof(T)) != hipSuccess) return -1;
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(buf)) != hipSuccess) return -1;
  return hipMemset(p, 0, sizeof(buf)) == hipSuccess ? 0 : -1;
}
int diag_read_nolicm(int which, unsigned long long* out, size_t n);  // 0: phase counters, 1: stamps
static int diag_read_this_tu(int which, unsigned long long* out, size_t n) {
  (void)which, (void)out, (void)n;
#if defined(RT_PHASE_PROF)
  if (which == 0) return diag_read(rt_prof_buf, out, n);
#endif
#if defined(RT_WAVE_STAMPS)
  if (which == 1) return diag_read(rt_stamp_buf, out, n);
#endif
  return -1;
}
#if RT_TU_NOLICM
int diag_read_nolicm(int which, unsigned long long* out, size_t n) { return diag_read_this_tu(which, out, n); }
#endif
static int diag_read_both(int which, unsigned long long* out, size_t n) {
  if (hipDeviceSynchronize() != hipSuccess || diag_read_this_tu(which, out, n)) return -1;
  unsigned long long* other = new unsigned long long[n];
  const int rc = diag_read_nolicm(which, other, n);
  for (size_t k = 0; k < n && rc == 0; ++k) out[k] += other[k];
  delete[] other;
  return rc;
}
// the ring kernel, from whichever unit holds it (RT_RING_NOLICM)
#if RT_RING_NOLICM
render_fn ring_kernel_nolicm();
#if RT_TU_NOLICM
render_fn ring_kernel_nolicm() { return rt_render_kernel_ring; }
#else
static render_fn ring_kernel_of() { return ring_kernel_nolicm(); }
#endif
#elif !RT_TU_NOLICM
static render_fn ring_kernel_of() { return rt_render_kernel_ring; }
#endif
#if RT_TU_NOLICM
render_fn render_kernel_nolicm(int variant) { return render_kernel_this_tu(variant); }
#else
static render_fn render_kernel_of(int variant) {
  const render_fn f = render_kernel_this_tu(variant);
  return f ? f : render_kernel_nolicm(variant);
}
#endif

#endif  // RT_KERNEL_ONLY
}  // namespace RT_NS
#if !defined(RT_KERNEL_ONLY) && !RT_TU_NOLICM  // (the launchers: in the main translation unit)

int rt_render_resident_blocks(const KernelParamsT<RT_NS::real>*, int device, int stack_depth, int variant,
                              int lds_nodes) {
  using namespace RT_NS;
  int per_cu = 0, cus = 0;
  const KernelClass c = rt_class_of(RT_F64, variant);
  size_t lds = rt_class_lds_bytes(RT_F64, c, stack_depth, lds_nodes);
  if (lds > 65536 && hipFuncSetAttribute((const void*)render_kernel_of(variant),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return -1;
  hipError_t e =
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, render_kernel_of(variant), rt_class_block(RT_F64, c), lds);
  if (e != hipSuccess) return -1;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return -1;
  if (per_cu < 1) per_cu = 1;
  return per_cu * cus;
}

int rt_launch_render(const KernelParamsT<RT_NS::real>& p, int grid_blocks, int variant, void* stream) {
  using namespace RT_NS;
  if (p.n_items <= 0 || grid_blocks <= 0) return 0;
  const KernelClass c = rt_class_of(RT_F64, variant);
  const int block = rt_class_block(RT_F64, c);
  long long need = ((long long)p.n_items + block - 1) / block;
  int grid = need < grid_blocks ? (int)need : grid_blocks;
  if (p.flat_ring) {  // the ring form's plan (rt_build.cpp rt_host_plan_ring): its kernel, or none
    if (!rt_class_has_ring(c)) return -1;
    hipLaunchKernelGGL(ring_kernel_of(), dim3(grid), dim3(block), rt_ring_lds_bytes(RT_F64), (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
  }
  size_t lds = rt_class_lds_bytes(RT_F64, c, p.stack_depth, p.lds_nodes);
  hipLaunchKernelGGL(render_kernel_of(variant), dim3(grid), dim3(block), lds, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

#if defined(RT_PHASE_PROF)
// diagnostic build: read (and zero) the phase counters of this precision's BVH kernel
int rt_prof_read_kernel(const KernelParamsT<RT_NS::real>*, unsigned long long* out, int n) {
  using namespace RT_NS;
  if (n > PF_N) n = PF_N;
  return diag_read_both(0, out, (size_t)n) == 0 ? n : -1;
}
#endif

#if defined(RT_WAVE_STAMPS)
// diagnostic build: read (and zero) this precision's per-wave stamps, 4 words per wave
int rt_stamps_read_kernel(const KernelParamsT<RT_NS::real>*, unsigned long long* out, int n_waves) {
  using namespace RT_NS;
  if (n_waves > RT_STAMP_WAVES) n_waves = RT_STAMP_WAVES;
  return diag_read_both(1, out, 4 * (size_t)n_waves) == 0 ? n_waves : -1;
}
#endif

int rt_launch_resolve(const KernelParamsT<RT_NS::real>& p, void* stream) {
  using namespace RT_NS;
  int n = p.tile_rows * p.cam.width;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(rt_resolve_kernel, dim3((n + 255) / 256, 3), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)p.accum, p.nanflag, p.out, n, p.cam.spp, 1.0 / (RT_FIX_SCALE * (double)p.cam.spp),
                     p.cam.width, p.out_frame_rows, p.n_shards, p.shard, p.row_block);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#endif  // RT_KERNEL_ONLY
