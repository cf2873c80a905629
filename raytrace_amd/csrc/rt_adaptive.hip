// rt_adaptive.hip — the film-side kernels of an adaptive pass (rt_adaptive.h): the count plane's
// fill, the selection (mask and count per workgroup, a scan across the workgroups, the ordered
// write), the merge of the listed pixels, and the resolve and noise estimate of a non-uniform film.
// All are bound by HBM traffic, like rt_film.hip's; the per-pixel arithmetic is rt_adaptive.h's and
// rt_film.h's, which a CPU program calls too.
#include <hip/hip_runtime.h>

#include "rt_adaptive.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
static_assert(RT_ADAPTIVE_TILE == kThreads, "a thread of the select kernels owns one pixel");

__global__ __launch_bounds__(kThreads) void rt_adaptive_init_kernel(uint2* __restrict__ counts, long long n_pixels,
                                                                    uint32_t N, uint32_t K, int width, int height,
                                                                    int n_shards, int shard, int row_block) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_pixels) return;
  const bool in = rt_adaptive_inside(i, width, height, n_shards, shard, row_block);
  counts[i] = in ? make_uint2(N, K) : make_uint2(0u, 0u);
}

// Selection, step 1: the predicate per pixel; a wave's ballot is its 64 pixels' mask (pixel order =
// lane order), its popcount the wave's count; thread 0 adds the workgroup's four counts.
template <int kW>
__global__ __launch_bounds__(kThreads) void rt_adaptive_mark_kernel(const long long* __restrict__ total,
                                                                    const unsigned int* __restrict__ flags,
                                                                    const double* __restrict__ q,
                                                                    const uint2* __restrict__ counts,
                                                                    long long n_pixels, int n_samples, double threshold,
                                                                    long long max_samples, int width, int height,
                                                                    int n_shards, int shard, int row_block,
                                                                    unsigned long long* __restrict__ masks,
                                                                    int* __restrict__ block_cnt) {
  __shared__ int wcnt[kWaves];
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  bool sel = false;
  if (i < n_pixels && rt_adaptive_inside(i, width, height, n_shards, shard, row_block)) {
    const long long* a = total + kW * i;
    const uint2 c = counts[i];
    sel = rt_adaptive_select(q[i], a[0], a[1], a[2], flags[i], c.x, c.y, n_samples, threshold, max_samples);
  }
  const unsigned long long m = __ballot(sel);
  const int wave = (int)(threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0) {
    masks[(size_t)blockIdx.x * kWaves + wave] = m;
    wcnt[wave] = (int)__popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int k = 0; k < kWaves; ++k) s += wcnt[k];
    block_cnt[blockIdx.x] = s;
  }
}

// Step 2, one workgroup: the exclusive scan of the workgroups' counts, kThreads at a time with a
// running carry (wave: shuffle-up scan; the four waves' totals through LDS), and the list length.
__global__ __launch_bounds__(kThreads) void rt_adaptive_scan_kernel(const int* __restrict__ block_cnt,
                                                                    int* __restrict__ block_off, int n_blocks,
                                                                    int* __restrict__ n_list) {
  __shared__ int wsum[kWaves];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  int carry = 0;
  for (int b0 = 0; b0 < n_blocks; b0 += kThreads) {
    const int b = b0 + (int)threadIdx.x;
    const int v = b < n_blocks ? block_cnt[b] : 0;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(inc, d);
      if (lane >= d) inc += u;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < kWaves; ++k) {
      if (k < wave) before += wsum[k];
      all += wsum[k];
    }
    if (b < n_blocks) block_off[b] = carry + before + inc - v;
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_list = carry;
}

// Step 3: the records in ascending tile-pixel order: a selected pixel's place is its workgroup's
// offset, the counts of the waves before its own, and the set bits of its wave's mask below its lane.
__global__ __launch_bounds__(kThreads) void rt_adaptive_write_kernel(const unsigned long long* __restrict__ masks,
                                                                     const int* __restrict__ block_off,
                                                                     const uint2* __restrict__ counts, long long n_pixels,
                                                                     rt_adaptive_rec* __restrict__ list) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const unsigned long long* bm = masks + (size_t)blockIdx.x * kWaves;
  const unsigned long long m = bm[wave];
  if (i >= n_pixels || !((m >> lane) & 1ull)) return;
  int at = block_off[blockIdx.x];
  for (int k = 0; k < wave; ++k) at += (int)__popcll(bm[k]);
  at += (int)__popcll(m & ((1ull << lane) - 1ull));
  rt_adaptive_rec r;
  r.tp = (int32_t)i;
  r.n = counts[i].x;
  list[at] = r;
}

// One thread per list entry (a pixel's words are 24 or 48 contiguous bytes; the list is ascending,
// so neighbouring threads touch neighbouring pixels)
template <int kW>
__global__ __launch_bounds__(kThreads) void rt_adaptive_merge_kernel(unsigned long long* __restrict__ total,
                                                                     unsigned int* __restrict__ flags,
                                                                     double* __restrict__ q, uint32_t* __restrict__ counts,
                                                                     const unsigned long long* __restrict__ pass,
                                                                     const unsigned int* __restrict__ pass_flags,
                                                                     const rt_adaptive_rec* __restrict__ list,
                                                                     const int* __restrict__ n_list, long long n_pixels,
                                                                     int n_samples) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= *n_list) return;
  const long long p = list[e].tp;
  if (p < 0 || p >= n_pixels) return;
  rt_adaptive_merge_pixel(total + kW * p, flags + p, q + p, counts + 2 * p, pass + kW * p, pass_flags[p], kW, n_samples);
}

template <class R>
__global__ __launch_bounds__(kThreads) void rt_adaptive_resolve_kernel(const long long* __restrict__ total,
                                                                       const unsigned int* __restrict__ flags,
                                                                       const uint2* __restrict__ counts,
                                                                       R* __restrict__ out, long long n_pixels) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_pixels) return;
  const int c = (int)blockIdx.y;
  const uint32_t N = counts[i].x;
  const bool bad = flags[i] != 0u;
  R v;
  if constexpr (sizeof(R) == 8) {
    const long long* a = total + 6 * i + c;
    v = bad ? __builtin_nan("") : N ? rt_adaptive_resolve64(a[0], (unsigned long long)a[3], N) : 0.0;
  } else {
    v = bad ? __builtin_nanf("") : N ? rt_adaptive_resolve32(total[3 * i + c], N) : 0.f;
  }
  out[3 * i + c] = v;
}

// rt_film.hip rt_film_noise_kernel with the pixel's own counts: the same workgroups, rounds and
// reduction order, so a film whose counts are all (N, K) gives the uniform kernel's figure
template <int kW>
__global__ __launch_bounds__(kThreads) void rt_adaptive_noise_kernel(const long long* __restrict__ total,
                                                                     const unsigned int* __restrict__ flags,
                                                                     const double* __restrict__ q,
                                                                     const uint2* __restrict__ counts,
                                                                     float* __restrict__ map,
                                                                     double* __restrict__ partial_sum,
                                                                     int* __restrict__ partial_cnt, long long n_pixels,
                                                                     int width, int height, int n_shards, int shard,
                                                                     int row_block) {
  __shared__ double wsum[kWaves];
  __shared__ int wcnt[kWaves];
  double s = 0.0;
  int c = 0;
  for (int round = 0; round < RT_FILM_TILE / kThreads; ++round) {
    const long long i = (long long)blockIdx.x * RT_FILM_TILE + round * kThreads + threadIdx.x;
    if (i >= n_pixels) break;
    double r = __builtin_nan("");
    if (rt_adaptive_inside(i, width, height, n_shards, shard, row_block) && flags[i] == 0u) {
      const long long* a = total + kW * i;
      const uint2 k = counts[i];
      r = rt_adaptive_rel_error(q[i], a[0], a[1], a[2], k.x, k.y);
      s += r * r;
      ++c;
    }
    if (map) map[i] = (float)r;
  }
  for (int m = 32; m >= 1; m >>= 1) {
    s += __shfl_xor(s, m);
    c += __shfl_xor(c, m);
  }
  if ((threadIdx.x & 63) == 0) {
    wsum[threadIdx.x >> 6] = s;
    wcnt[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ts = wsum[0];
    int tc = wcnt[0];
    for (int k = 1; k < kWaves; ++k) ts += wsum[k], tc += wcnt[k];
    partial_sum[blockIdx.x] = ts;
    partial_cnt[blockIdx.x] = tc;
  }
}

bool launched() { return hipGetLastError() == hipSuccess; }

}  // namespace

int rt_adaptive_launch_init(uint32_t* counts, long long n_pixels, uint32_t N, uint32_t K, int width, int height,
                            int n_shards, int shard, int row_block, void* stream) {
  if (n_pixels <= 0) return 0;
  hipLaunchKernelGGL(rt_adaptive_init_kernel, dim3(rt_adaptive_blocks(n_pixels)), dim3(kThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<uint2*>(counts), n_pixels, N, K, width, height, n_shards, shard, row_block);
  return launched() ? 0 : -1;
}

int rt_adaptive_launch_select(const unsigned long long* total, const unsigned int* flags, const double* q,
                              const uint32_t* counts, long long n_pixels, int acc_words, int n_samples, double threshold,
                              long long max_samples, int width, int height, int n_shards, int shard, int row_block,
                              void* scratch, rt_adaptive_rec* list, int* n_list, void* stream) {
  if (n_pixels <= 0) return -1;
  const int blocks = rt_adaptive_blocks(n_pixels);
  unsigned long long* masks = (unsigned long long*)scratch;
  int* block_cnt = (int*)(masks + (size_t)blocks * kWaves);
  int* block_off = block_cnt + blocks;
  const uint2* cn = reinterpret_cast<const uint2*>(counts);
  const long long* t = reinterpret_cast<const long long*>(total);
  const hipStream_t st = (hipStream_t)stream;
  auto mark = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kThreads), 0, st, t, flags, q, cn, n_pixels, n_samples, threshold,
                       max_samples, width, height, n_shards, shard, row_block, masks, block_cnt);
  };
  if (acc_words == 6)
    mark(rt_adaptive_mark_kernel<6>);
  else
    mark(rt_adaptive_mark_kernel<3>);
  hipLaunchKernelGGL(rt_adaptive_scan_kernel, dim3(1), dim3(kThreads), 0, st, block_cnt, block_off, blocks, n_list);
  hipLaunchKernelGGL(rt_adaptive_write_kernel, dim3(blocks), dim3(kThreads), 0, st, masks, block_off, cn, n_pixels, list);
  return launched() ? 0 : -1;
}

int rt_adaptive_launch_merge(unsigned long long* total, unsigned int* flags, double* q, uint32_t* counts,
                             const unsigned long long* pass, const unsigned int* pass_flags, const rt_adaptive_rec* list,
                             const int* n_list, long long n_pixels, int acc_words, int n_samples, void* stream) {
  if (n_pixels <= 0) return 0;
  const dim3 grid(rt_adaptive_blocks(n_pixels)), block(kThreads);
  if (acc_words == 6)
    hipLaunchKernelGGL(rt_adaptive_merge_kernel<6>, grid, block, 0, (hipStream_t)stream, total, flags, q, counts, pass,
                       pass_flags, list, n_list, n_pixels, n_samples);
  else
    hipLaunchKernelGGL(rt_adaptive_merge_kernel<3>, grid, block, 0, (hipStream_t)stream, total, flags, q, counts, pass,
                       pass_flags, list, n_list, n_pixels, n_samples);
  return launched() ? 0 : -1;
}

int rt_adaptive_launch_resolve(const unsigned long long* total, const unsigned int* flags, const uint32_t* counts, void* out,
                               long long n_pixels, int f32, void* stream) {
  if (n_pixels <= 0) return 0;
  const dim3 grid(rt_adaptive_blocks(n_pixels), 3), block(kThreads);
  const long long* t = reinterpret_cast<const long long*>(total);
  const uint2* cn = reinterpret_cast<const uint2*>(counts);
  if (f32)
    hipLaunchKernelGGL(rt_adaptive_resolve_kernel<float>, grid, block, 0, (hipStream_t)stream, t, flags, cn, (float*)out,
                       n_pixels);
  else
    hipLaunchKernelGGL(rt_adaptive_resolve_kernel<double>, grid, block, 0, (hipStream_t)stream, t, flags, cn, (double*)out,
                       n_pixels);
  return launched() ? 0 : -1;
}

int rt_adaptive_launch_noise(const unsigned long long* total, const unsigned int* flags, const double* q,
                             const uint32_t* counts, float* map, double* partial_sum, int* partial_cnt, long long n_pixels,
                             int acc_words, int width, int height, int n_shards, int shard, int row_block, void* stream) {
  if (n_pixels <= 0) return 0;
  const dim3 grid(rt_film_blocks(n_pixels)), block(kThreads);
  const long long* t = reinterpret_cast<const long long*>(total);
  const uint2* cn = reinterpret_cast<const uint2*>(counts);
  if (acc_words == 6)
    hipLaunchKernelGGL(rt_adaptive_noise_kernel<6>, grid, block, 0, (hipStream_t)stream, t, flags, q, cn, map, partial_sum,
                       partial_cnt, n_pixels, width, height, n_shards, shard, row_block);
  else
    hipLaunchKernelGGL(rt_adaptive_noise_kernel<3>, grid, block, 0, (hipStream_t)stream, t, flags, q, cn, map, partial_sum,
                       partial_cnt, n_pixels, width, height, n_shards, shard, row_block);
  return launched() ? 0 : -1;
}
