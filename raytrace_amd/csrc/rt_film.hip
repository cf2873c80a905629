// rt_film.hip — the progressive film's two kernels (rt_film.h): the merge of a rendered pass into
// the resident totals and the per-pixel noise estimate with its frame figure.  Both are bound by
// HBM traffic like the resolve (rt_render_kernel.h): per pixel the merge reads the pass words and
// reads and writes the totals, flags and q; the noise kernel reads the high words, flag and q.
#include <hip/hip_runtime.h>

#include "rt_film.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = RT_FILM_TILE;  // pixels per workgroup (two per thread)
static_assert(kTile == 2 * kThreads, "a thread owns one pixel pair");

// total += pass; flags |= pass flags; q += L^2 / n.  kW: RT_ACC_WORDS (3 FP32, 6 binary64).
// A workgroup owns kTile consecutive pixels = kTile kW consecutive words, an even count from an even
// word index: it walks them as 16-byte vectors, consecutive lanes on consecutive vectors, and keeps
// the pass words in LDS, where each thread then picks up its pixel pair's three high words (the
// 24- / 48-byte pixel stride never reaches HBM).  q goes as one double2 per thread, the flags as
// one uint4 per thread of the first two waves.
template <int kW>
__global__ __launch_bounds__(kThreads) void rt_film_merge_kernel(unsigned long long* __restrict__ total,
                                                                 unsigned int* __restrict__ flags,
                                                                 double* __restrict__ q,
                                                                 const unsigned long long* __restrict__ pass,
                                                                 const unsigned int* __restrict__ pass_flags,
                                                                 long long n_pixels, int n_samples) {
  __shared__ unsigned long long words[kTile * kW];
  const long long p0 = (long long)blockIdx.x * kTile;
  const int np = (int)(n_pixels - p0 < kTile ? n_pixels - p0 : kTile);  // pixels of this workgroup
  const long long w0 = p0 * kW;                                         // its first word (even)
  const int nw = np * kW;
  const ulonglong2* pv = reinterpret_cast<const ulonglong2*>(pass + w0);
  ulonglong2* tv = reinterpret_cast<ulonglong2*>(total + w0);
  for (int v = (int)threadIdx.x; 2 * v < nw; v += kThreads) {
    ulonglong2 a = pv[v];
    if (2 * v + 1 >= nw) a.y = 0ull;  // (an odd last word: what follows the pass sums is not a sum)
    ulonglong2 t = tv[v];
    t.x += a.x;
    t.y += a.y;
    tv[v] = t;
    words[2 * v] = a.x;
    words[2 * v + 1] = a.y;
  }
  if (4 * (int)threadIdx.x < np) {  // (the flag arrays are padded to whole vectors of zeros)
    const uint4 f = reinterpret_cast<const uint4*>(pass_flags + p0)[threadIdx.x];
    uint4* dst = reinterpret_cast<uint4*>(flags + p0) + threadIdx.x;
    uint4 g = *dst;
    g.x |= f.x, g.y |= f.y, g.z |= f.z, g.w |= f.w;
    *dst = g;
  }
  __syncthreads();
  const int i = 2 * (int)threadIdx.x;
  if (i < np) {
    double2* qv = reinterpret_cast<double2*>(q + p0) + threadIdx.x;
    double2 qq = *qv;
    const unsigned long long* a = words + i * kW;
    qq.x = rt_film_q_add(qq.x, rt_film_lum((long long)a[0], (long long)a[1], (long long)a[2]), n_samples);
    if (i + 1 < np)
      qq.y = rt_film_q_add(qq.y, rt_film_lum((long long)a[kW], (long long)a[kW + 1], (long long)a[kW + 2]), n_samples);
    *qv = qq;
  }
}

// Per pixel r (rt_film.h rt_film_rel_error), NaN for flagged pixels and a shard's padding rows; per
// workgroup the sum of r^2 and the count of the pixels that count, reduced in a fixed order (wave:
// xor butterfly, then the four waves' words in LDS added by thread 0), so the figure is the same
// from run to run.  One pixel per thread, two rounds per workgroup.
template <int kW>
__global__ __launch_bounds__(kThreads) void rt_film_noise_kernel(const long long* __restrict__ total,
                                                                 const unsigned int* __restrict__ flags,
                                                                 const double* __restrict__ q,
                                                                 float* __restrict__ map,
                                                                 double* __restrict__ partial_sum,
                                                                 int* __restrict__ partial_cnt, long long n_pixels,
                                                                 long long N, int K, int width, int height,
                                                                 int n_shards, int shard, int row_block) {
  __shared__ double wsum[kThreads / 64];
  __shared__ int wcnt[kThreads / 64];
  double s = 0.0;
  int c = 0;
  for (int round = 0; round < kTile / kThreads; ++round) {
    const long long i = (long long)blockIdx.x * kTile + round * kThreads + threadIdx.x;
    if (i >= n_pixels) break;
    const int t = (int)(i / width);
    const int g = ((t / row_block) * n_shards + shard) * row_block + t % row_block;
    double r = __builtin_nan("");
    if (g < height && flags[i] == 0u) {
      const long long* a = total + kW * i;
      r = rt_film_rel_error(q[i], rt_film_lum(a[0], a[1], a[2]), N, K);
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
    for (int k = 1; k < kThreads / 64; ++k) ts += wsum[k], tc += wcnt[k];
    partial_sum[blockIdx.x] = ts;
    partial_cnt[blockIdx.x] = tc;
  }
}

}  // namespace

int rt_film_launch_merge(unsigned long long* total, unsigned int* flags, double* q, const unsigned long long* pass,
                         const unsigned int* pass_flags, long long n_pixels, int acc_words, int n_samples,
                         void* stream) {
  if (n_pixels <= 0) return 0;
  const dim3 grid(rt_film_blocks(n_pixels)), block(kThreads);
  if (acc_words == 6)
    hipLaunchKernelGGL(rt_film_merge_kernel<6>, grid, block, 0, (hipStream_t)stream, total, flags, q, pass, pass_flags,
                       n_pixels, n_samples);
  else
    hipLaunchKernelGGL(rt_film_merge_kernel<3>, grid, block, 0, (hipStream_t)stream, total, flags, q, pass, pass_flags,
                       n_pixels, n_samples);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rt_film_launch_noise(const unsigned long long* total, const unsigned int* flags, const double* q, float* map,
                         double* partial_sum, int* partial_cnt, long long n_pixels, int acc_words, long long N, int K,
                         int width, int height, int n_shards, int shard, int row_block, void* stream) {
  if (n_pixels <= 0) return 0;
  const dim3 grid(rt_film_blocks(n_pixels)), block(kThreads);
  const long long* t = reinterpret_cast<const long long*>(total);
  if (acc_words == 6)
    hipLaunchKernelGGL(rt_film_noise_kernel<6>, grid, block, 0, (hipStream_t)stream, t, flags, q, map, partial_sum,
                       partial_cnt, n_pixels, N, K, width, height, n_shards, shard, row_block);
  else
    hipLaunchKernelGGL(rt_film_noise_kernel<3>, grid, block, 0, (hipStream_t)stream, t, flags, q, map, partial_sum,
                       partial_cnt, n_pixels, N, K, width, height, n_shards, shard, row_block);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
