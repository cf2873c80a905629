// rt_order.hip — the order of a ray batch (include/rt.h rt_scene_ray_order): the
// batch's origin box, the coherence key of every record (rt_order.h, binary64, this unit is compiled
// with -ffp-contract=off) and a stable LSD radix sort of (key, index) pairs whose values are the order.
//
// The sort: 8-bit digits, four passes over the 32 key bits (30 of the key; RT_ORDER_KEY_LAST of the
// invalid records takes the two above), tiles of kTile = 4096 pairs per workgroup of 256 threads.  A
// pass is three kernels on the caller's stream:
//   hist     per tile, the count of every digit value -> hist[digit][tile]
//   scan     one workgroup per digit value: the exclusive prefix of its row over the tiles, the row's
//            total -> totals[digit]
//   scatter  per tile: the digit values' global bases (an exclusive scan of totals, 256 values,
//            redone by every workgroup) plus the row prefix, then the tile's pairs in 16 rounds of 256
//            consecutive pairs: a pair's slot is base + (pairs of its digit in earlier rounds) +
//            (in earlier waves of its round) + (in lower lanes of its wave).  The last is a match by
//            eight __ballot masks, the others are counts in LDS written by each match group's first
//            lane: no slot is claimed by an atomic, so a pair's position among equal digits is its
//            index order — the pass is stable and the order a pure function of the keys.
// The first pass takes the index as the value, the last writes only values, into the caller's
// order.  Pairs ping-pong between two buffers of the workspace; the caller's keys are only read.
// Every kernel is sized from n on the host; nothing is allocated or read back.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_internal.h"
#include "rt_order.h"

namespace {

constexpr int kBlock = 256;                // threads of every kernel here: 4 waves
constexpr int kWaves = kBlock / 64;
constexpr int kRounds = 16;                // rounds of kBlock consecutive pairs per tile
constexpr int kTile = kBlock * kRounds;    // pairs per workgroup per pass
constexpr int kDigitBits = 8, kDigits = 1 << kDigitBits;
constexpr int kPasses = 32 / kDigitBits;
constexpr int kBoxPer = 4;                 // records per thread of the box kernel
static_assert(kDigits == kBlock, "one thread per digit value in the scans");

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
long long tiles_of(long long n) { return (n + kTile - 1) / kTile; }

// the workspace of n records: keys of the records, two (key, value) buffers, hist, totals, the box
struct Layout {
  size_t keys, k[2], v[2], hist, totals, box, bytes;
};
Layout layout_of(long long n) {
  Layout L;
  const size_t col = up256((size_t)n * sizeof(uint32_t));
  L.keys = 0;
  L.k[0] = col, L.v[0] = 2 * col, L.k[1] = 3 * col, L.v[1] = 4 * col;
  L.hist = 5 * col;
  L.totals = L.hist + up256((size_t)tiles_of(n) * kDigits * sizeof(uint32_t));
  L.box = L.totals + kDigits * sizeof(uint32_t);
  L.bytes = L.box + 256;
  return L;
}

// ---- the batch box: min / max of the valid origins as maxima of order-preserving 64-bit codes
// (0: no value), box[a] = max of ~code(origin_a) (the minimum), box[3 + a] = max of code(origin_a)
__device__ __forceinline__ unsigned long long code_of(double x) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
  return b ^ ((b >> 63) ? ~0ull : 1ull << 63);
}
__device__ __forceinline__ double value_of(unsigned long long c) {
  return __builtin_bit_cast(double, (c >> 63) ? c ^ (1ull << 63) : ~c);
}
__device__ __forceinline__ void load_record(const char* __restrict__ rays, long long i, int stride, double* r) {
  const double* p = reinterpret_cast<const double*>(rays + (size_t)i * (size_t)stride);
#pragma unroll
  for (int c = 0; c < 6; ++c) r[c] = p[c];
}

__global__ __launch_bounds__(kBlock) void rt_order_box_kernel(const char* __restrict__ rays, long long n, int stride,
                                                             unsigned long long* __restrict__ box) {
  __shared__ unsigned long long red[kWaves][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long m[6] = {0, 0, 0, 0, 0, 0};
  const long long i0 = (long long)blockIdx.x * (kBlock * kBoxPer) + tid;
#pragma unroll
  for (int k = 0; k < kBoxPer; ++k) {
    const long long i = i0 + (long long)k * kBlock;
    if (i < n) {
      double r[6];
      load_record(rays, i, stride, r);
      if (rt_order_valid(r)) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const unsigned long long c = code_of(r[a]);
          m[a] = max(m[a], ~c);
          m[3 + a] = max(m[3 + a], c);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    for (int o = 32; o > 0; o >>= 1) m[c] = max(m[c], (unsigned long long)__shfl_xor(m[c], o));
    if (lane == 0) red[wave][c] = m[c];
  }
  __syncthreads();
  if (tid < 6) {
    unsigned long long v = red[0][tid];
    for (int w = 1; w < kWaves; ++w) v = max(v, red[w][tid]);
    if (v) atomicMax(box + tid, v);
  }
}

__global__ __launch_bounds__(kBlock) void rt_order_key_kernel(const char* __restrict__ rays, long long n, int stride,
                                                             const unsigned long long* __restrict__ box,
                                                             uint32_t* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double lo[3], s[3], r[6];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = value_of(~box[a]);
    s[a] = rt_order_scale(lo[a], value_of(box[3 + a]));
  }
  load_record(rays, i, stride, r);
  keys[i] = rt_order_key(r, lo, s);  // (a batch without a valid record: every key is RT_ORDER_KEY_LAST, the box is not read)
}

// ---- the sort

// the lanes of the wave whose pair is in range and has this lane's digit
__device__ __forceinline__ unsigned long long match_digit(uint32_t d, bool ok) {
  unsigned long long m = __ballot(ok);
#pragma unroll
  for (int b = 0; b < kDigitBits; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long s = __ballot(ok && bit);
    m &= bit ? s : ~s;
  }
  return m;
}
__device__ __forceinline__ int lanes_below(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// the inclusive prefix sum over the wave's lanes
__device__ __forceinline__ uint32_t wave_prefix(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}

__global__ __launch_bounds__(kBlock) void rt_order_hist_kernel(const uint32_t* __restrict__ keys, long long n, int tiles,
                                                              int shift, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kDigits];
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const long long tile0 = (long long)blockIdx.x * kTile;
  for (int r = 0; r < kRounds; ++r) {
    const long long i = tile0 + r * kBlock + tid;
    if (tile0 + r * kBlock >= n) break;  // (the whole workgroup)
    const bool ok = i < n;
    const uint32_t d = ok ? (keys[i] >> shift) & (kDigits - 1) : 0u;
    const unsigned long long m = match_digit(d, ok);
    if (ok && lanes_below(m) == 0) atomicAdd(&h[d], (uint32_t)__popcll(m));  // (a count: its order does not matter)
  }
  __syncthreads();
  hist[(size_t)tid * tiles + blockIdx.x] = h[tid];
}

// workgroup d: hist[d][*] -> its exclusive prefix, totals[d] = the row's sum
__global__ __launch_bounds__(kBlock) void rt_order_scan_kernel(uint32_t* __restrict__ hist, int tiles,
                                                              uint32_t* __restrict__ totals) {
  __shared__ uint32_t wsum[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t* row = hist + (size_t)blockIdx.x * tiles;
  uint32_t carry = 0;
  for (int t0 = 0; t0 < tiles; t0 += kBlock) {
    const int t = t0 + tid;
    const uint32_t v = t < tiles ? row[t] : 0u;
    const uint32_t inc = wave_prefix(v, lane);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t pre = 0, all = 0;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) pre += wsum[w];
      all += wsum[w];
    }
    if (t < tiles) row[t] = carry + pre + inc - v;
    carry += all;
    __syncthreads();
  }
  if (tid == 0) totals[blockIdx.x] = carry;
}

// kFirst: the value of pair i is i; kLast: only the values are written
template <bool kFirst, bool kLast>
__global__ __launch_bounds__(kBlock) void rt_order_scatter_kernel(const uint32_t* __restrict__ keys_in,
                                                                 const uint32_t* __restrict__ vals_in,
                                                                 uint32_t* __restrict__ keys_out,
                                                                 uint32_t* __restrict__ vals_out,
                                                                 const uint32_t* __restrict__ hist,
                                                                 const uint32_t* __restrict__ totals, long long n, int tiles,
                                                                 int shift) {
  __shared__ uint32_t base[kDigits];            // the next slot of every digit value for this tile
  __shared__ uint32_t wc[2][kWaves][kDigits];   // a round's counts per wave; two rounds' worth, zeroed in turn
  __shared__ uint32_t wsum[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  {
    const uint32_t t = totals[tid];
    const uint32_t inc = wave_prefix(t, lane);
    if (lane == 63) wsum[wave] = inc;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) wc[0][w][tid] = wc[1][w][tid] = 0;
    __syncthreads();
    uint32_t pre = 0;
    for (int w = 0; w < wave; ++w) pre += wsum[w];
    base[tid] = pre + inc - t + hist[(size_t)tid * tiles + blockIdx.x];
  }
  __syncthreads();
  const long long tile0 = (long long)blockIdx.x * kTile;
  for (int r = 0; r < kRounds; ++r) {
    if (tile0 + r * kBlock >= n) break;  // (the whole workgroup)
    const int b = r & 1;
    const long long i = tile0 + r * kBlock + tid;
    const bool ok = i < n;
    const uint32_t key = ok ? keys_in[i] : 0u;
    const uint32_t d = (key >> shift) & (kDigits - 1);
    const unsigned long long m = match_digit(d, ok);
    const int below = lanes_below(m);
    if (ok && below == 0) wc[b][wave][d] = (uint32_t)__popcll(m);
    __syncthreads();
    if (ok) {
      uint32_t slot = base[d] + (uint32_t)below;
      for (int w = 0; w < wave; ++w) slot += wc[b][w][d];
      if ((long long)slot < n) {  // (always: the counts are of the same keys)
        if constexpr (!kLast) keys_out[slot] = key;
        vals_out[slot] = kFirst ? (uint32_t)i : vals_in[i];
      }
    }
#pragma unroll
    for (int w = 0; w < kWaves; ++w) wc[b ^ 1][w][tid] = 0;  // (read last before this round's first barrier)
    __syncthreads();
    uint32_t add = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) add += wc[b][w][tid];
    base[tid] += add;  // (read next behind the next round's first barrier)
  }
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }

int sort_keys(const uint32_t* d_keys, long long n, uint32_t* d_order, char* ws, hipStream_t st) {
  const Layout L = layout_of(n);
  const int tiles = (int)tiles_of(n);
  uint32_t* hist = (uint32_t*)(ws + L.hist);
  uint32_t* totals = (uint32_t*)(ws + L.totals);
  const uint32_t* kin = d_keys;
  const uint32_t* vin = nullptr;
  for (int p = 0; p < kPasses; ++p) {
    const int shift = p * kDigitBits;
    uint32_t* kout = (uint32_t*)(ws + L.k[p & 1]);
    uint32_t* vout = p == kPasses - 1 ? d_order : (uint32_t*)(ws + L.v[p & 1]);
    hipLaunchKernelGGL(rt_order_hist_kernel, dim3(tiles), dim3(kBlock), 0, st, kin, n, tiles, shift, hist);
    hipLaunchKernelGGL(rt_order_scan_kernel, dim3(kDigits), dim3(kBlock), 0, st, hist, tiles, totals);
    if (p == 0)
      hipLaunchKernelGGL((rt_order_scatter_kernel<true, false>), dim3(tiles), dim3(kBlock), 0, st, kin, vin, kout, vout,
                         (const uint32_t*)hist, (const uint32_t*)totals, n, tiles, shift);
    else if (p == kPasses - 1)
      hipLaunchKernelGGL((rt_order_scatter_kernel<false, true>), dim3(tiles), dim3(kBlock), 0, st, kin, vin, kout, vout,
                         (const uint32_t*)hist, (const uint32_t*)totals, n, tiles, shift);
    else
      hipLaunchKernelGGL((rt_order_scatter_kernel<false, false>), dim3(tiles), dim3(kBlock), 0, st, kin, vin, kout, vout,
                         (const uint32_t*)hist, (const uint32_t*)totals, n, tiles, shift);
    if (launched()) return -1;
    kin = kout, vin = vout;
  }
  return 0;
}

}  // namespace

size_t rt_order_workspace_bytes(long long n) { return layout_of(n < 0 ? 0 : n).bytes; }
int rt_order_tile() { return kTile; }

int rt_launch_order_sort(const uint32_t* d_keys, long long n, uint32_t* d_order, void* d_ws, void* stream) {
  if (n <= 0) return 0;
  if (n > 0x7fffffffLL) return -1;
  return sort_keys(d_keys, n, d_order, (char*)d_ws, (hipStream_t)stream);
}

int rt_launch_ray_order(const void* d_rays, long long n, int stride, uint32_t* d_order, void* d_ws, void* stream) {
  if (n <= 0) return 0;
  if (n > 0x7fffffffLL) return -1;
  const Layout L = layout_of(n);
  char* ws = (char*)d_ws;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* box = (unsigned long long*)(ws + L.box);
  uint32_t* keys = (uint32_t*)(ws + L.keys);
  if (hipMemsetAsync(box, 0, 6 * sizeof(unsigned long long), st) != hipSuccess) return -1;
  const long long per = (long long)kBlock * kBoxPer;
  hipLaunchKernelGGL(rt_order_box_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(kBlock), 0, st, (const char*)d_rays, n,
                     stride, box);
  hipLaunchKernelGGL(rt_order_key_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                     (const char*)d_rays, n, stride, (const unsigned long long*)box, keys);
  if (launched()) return -1;
  return sort_keys(keys, n, d_order, ws, st);
}
