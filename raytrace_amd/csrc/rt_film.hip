// rt_film.hip — the progressive film's kernels (rt_film.h): the merge of a rendered pass into the
// resident totals (of a film's own tile, or of a shard's tile into the rows of a multi-device
// film's frame) and the per-pixel noise estimate with its frame figure.  All are bound by
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

// The merge of a SHARD's pass into the rows of a whole frame (a multi-device film, rt_api.hip): tile
// row block blockIdx.y of shard (n_shards, shard, row_block) is a contiguous run of pixels in the
// tile and in the frame (rt_film_block_span); blockIdx.x walks it in runs of kTile pixels, so a
// workgroup never spans two blocks, and the workgroups of a padding block (or behind a block that
// `height` cuts short) have nothing to do.  Per pixel exactly what rt_film_merge_kernel does.  Several
// shards' merges may run at once into one frame (one stream each), so no access leaves the
// workgroup's own pixels: no vector straddles their end, odd last elements go as scalars.
// kVec: every run starts on a pixel index that is a multiple of 4 in the tile and in the frame
// (row_block * width is one) — 16-byte vectors as in rt_film_merge_kernel, consecutive lanes on
// consecutive vectors, the pass words staged in LDS for the luminance, q as double2, the flags as
// uint4.  Otherwise (with kW = 3 every second block then starts on an odd word) the scalar form:
// a thread per pixel, word by word.
template <int kW, bool kVec>
__global__ __launch_bounds__(kThreads) void rt_film_merge_rows_kernel(unsigned long long* __restrict__ total,
                                                                      unsigned int* __restrict__ flags,
                                                                      double* __restrict__ q,
                                                                      const unsigned long long* __restrict__ pass,
                                                                      const unsigned int* __restrict__ pass_flags,
                                                                      int width, int height, int n_shards, int shard,
                                                                      int row_block, int n_samples) {
  const rt_film_span s = rt_film_block_span((int)blockIdx.y, width, height, n_shards, shard, row_block);
  const long long off = (long long)blockIdx.x * kTile;  // this workgroup's first pixel of the block
  if (off >= s.n_pixels) return;                        // (uniform: before any barrier)
  const int np = (int)(s.n_pixels - off < kTile ? s.n_pixels - off : kTile);
  const long long tp0 = s.tile_pixel + off, fp0 = s.frame_pixel + off;
  if constexpr (kVec) {
    __shared__ unsigned long long words[kTile * kW];
    const int nw = np * kW;
    const unsigned long long* pw = pass + tp0 * kW;
    unsigned long long* tw = total + fp0 * kW;
    const ulonglong2* pv = reinterpret_cast<const ulonglong2*>(pw);
    ulonglong2* tv = reinterpret_cast<ulonglong2*>(tw);
    for (int v = (int)threadIdx.x; 2 * v + 1 < nw; v += kThreads) {
      const ulonglong2 a = pv[v];
      ulonglong2 t = tv[v];
      t.x += a.x;
      t.y += a.y;
      tv[v] = t;
      words[2 * v] = a.x;
      words[2 * v + 1] = a.y;
    }
    if ((nw & 1) && threadIdx.x == 0) {  // an odd last word (kW = 3, an odd pixel count)
      const unsigned long long a = pw[nw - 1];
      tw[nw - 1] += a;
      words[nw - 1] = a;
    }
    const int f0 = 4 * (int)threadIdx.x;
    if (f0 + 3 < np) {
      const uint4 f = reinterpret_cast<const uint4*>(pass_flags + tp0)[threadIdx.x];
      uint4* dst = reinterpret_cast<uint4*>(flags + fp0) + threadIdx.x;
      uint4 g = *dst;
      g.x |= f.x, g.y |= f.y, g.z |= f.z, g.w |= f.w;
      *dst = g;
    } else {
      for (int i = f0; i < np; ++i) flags[fp0 + i] |= pass_flags[tp0 + i];
    }
    __syncthreads();
    const int i = 2 * (int)threadIdx.x;
    const unsigned long long* a = words + i * kW;
    if (i + 1 < np) {
      double2* qv = reinterpret_cast<double2*>(q + fp0) + threadIdx.x;
      double2 qq = *qv;
      qq.x = rt_film_q_add(qq.x, rt_film_lum((long long)a[0], (long long)a[1], (long long)a[2]), n_samples);
      qq.y = rt_film_q_add(qq.y, rt_film_lum((long long)a[kW], (long long)a[kW + 1], (long long)a[kW + 2]), n_samples);
      *qv = qq;
    } else if (i < np) {
      q[fp0 + i] = rt_film_q_add(q[fp0 + i], rt_film_lum((long long)a[0], (long long)a[1], (long long)a[2]), n_samples);
    }
  } else {
    for (int i = (int)threadIdx.x; i < np; i += kThreads) {
      const unsigned long long* a = pass + (tp0 + i) * kW;
      unsigned long long* t = total + (fp0 + i) * kW;
      unsigned long long w[kW];
#pragma unroll
      for (int c = 0; c < kW; ++c) {
        w[c] = a[c];
        t[c] += w[c];
      }
      flags[fp0 + i] |= pass_flags[tp0 + i];
      q[fp0 + i] = rt_film_q_add(q[fp0 + i], rt_film_lum((long long)w[0], (long long)w[1], (long long)w[2]), n_samples);
    }
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

int rt_film_launch_merge_rows(unsigned long long* total, unsigned int* flags, double* q, const unsigned long long* pass,
                              const unsigned int* pass_flags, int width, int height, int tile_rows, int n_shards, int shard,
                              int row_block, int acc_words, int n_samples, void* stream) {
  if (width <= 0 || height <= 0 || tile_rows <= 0 || n_shards < 1 || shard < 0 || shard >= n_shards || row_block < 1) return -1;
  // one shard: its tile is the frame, one block of `height` rows from pixel 0 (always aligned)
  if (n_shards == 1) row_block = tile_rows = height;
  if (tile_rows % row_block) return -1;
  const long long block_pixels = (long long)row_block * width;
  const bool vec = n_shards == 1 || block_pixels % 4 == 0;
  const dim3 grid(rt_film_blocks(block_pixels), tile_rows / row_block), block(kThreads);
  if (grid.y > 65535u) return -1;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, total, flags, q, pass, pass_flags, width, height, n_shards,
                       shard, row_block, n_samples);
  };
  if (acc_words == 6)
    vec ? launch(rt_film_merge_rows_kernel<6, true>) : launch(rt_film_merge_rows_kernel<6, false>);
  else
    vec ? launch(rt_film_merge_rows_kernel<3, true>) : launch(rt_film_merge_rows_kernel<3, false>);
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
