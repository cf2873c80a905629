// rt_film.h — the progressive film: per-pixel arithmetic (host and device, so a CPU program can
// call exactly what the kernels run) and the launchers of rt_film.hip.  Not part of the public
// ABI (include/rt.h rt_film_*; rt_api_film.hip holds the film's state and entry points).
//
// A film keeps, per tile pixel, the TOTAL fixed-point sums of every sample added so far (the
// render workspace's layout: RT_ACC_WORDS int64 words, rt_internal.h), the NaN flag and one
// binary64 word q.  A pass renders samples [N, N + n) into a zeroed pass workspace (the render
// kernel with KernelParams::sample0 = N) and rt_film_merge_kernel folds it into the totals:
//   total[w] += pass[w]            exact int64 adds: the totals are those of ONE render of N + n
//   flag     |= pass flag
//   L         = (double)(pass_hi[R] + pass_hi[G] + pass_hi[B])       (one int64 sum, one rounding)
//   q        += L * L / n          binary64, IEEE division, no contraction
// so that with T = (double)(total_hi[R] + total_hi[G] + total_hi[B]) after K passes of N samples
//   q - T * T / N = sum_k n_k (m_k - M)^2,   m_k = L_k / n_k,  M = T / N,
// whose expectation is (K - 1) sigma^2 for ANY batch sizes (batch means): the per-sample variance
// estimate v, the standard error of the pixel mean se = sqrt(v / N), and the relative error r
// against the mean, floored at one 8-bit code per channel (3 / 256 summed over RGB).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RT_FILM_FN __host__ __device__ inline
#else
#define RT_FILM_FN inline
#endif
#include <cmath>

#define RT_FILM_MAX_SAMPLES (1 << 24)  // total samples of a film at most (int64 sums, binary64 L: no overflow)
#define RT_FILM_FLOOR (3.0 / 256.0)    // one 8-bit code per channel: below it a relative error cannot be shown
#define RT_FILM_UNSCALE (1.0 / 4294967296.0)  // 2^-32: the fixed-point sums' unit (rt_internal.h RT_FIX_SCALE)

// The expressions below must round as written (the numpy twin raytrace_amd.film.noise_from_sums
// runs the same sequence): no fused multiply-add
#if defined(__clang__)
#define RT_FILM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RT_FILM_NO_CONTRACT  // (GCC: build with -ffp-contract=off)
#endif

// a pass's (or the totals') luminance word: the three high words added as integers, then rounded once
RT_FILM_FN double rt_film_lum(long long r, long long g, long long b) { return (double)(r + g + b); }

// q after a pass of n samples whose luminance word is L
RT_FILM_FN double rt_film_q_add(double q, double L, int n) {
  RT_FILM_NO_CONTRACT
  const double sq = L * L;
  const double per = sq / (double)n;
  return q + per;
}

// per-sample variance of the luminance word by batch means (fixed-point units squared)
RT_FILM_FN double rt_film_variance(double q, double T, long long N, int K) {
  RT_FILM_NO_CONTRACT
  const double tt = T * T;
  const double d = q - tt / (double)N;
  return (d > 0.0 ? d : 0.0) / (double)(K - 1);
}

// relative standard error of the pixel's mean luminance (R + G + B of the linear mean)
RT_FILM_FN double rt_film_rel_error(double q, double T, long long N, int K) {
  RT_FILM_NO_CONTRACT
  const double v = rt_film_variance(q, T, N, K);
  const double se = sqrt(v / (double)N) * RT_FILM_UNSCALE;
  const double M = T / (double)N * RT_FILM_UNSCALE;
  return se / (M > RT_FILM_FLOOR ? M : RT_FILM_FLOOR);
}

// A shard's row block inside its tile and inside the whole frame (the rt_exec interleave,
// include/rt.h rt_shard_row: tile row t is global row ((t / row_block) n_shards + shard) row_block +
// t % row_block).  Tile block b is a contiguous run of pixels in both: it starts at tile pixel
// b row_block width and at frame pixel (b n_shards + shard) row_block width.  n_pixels counts the
// rows that lie inside the frame: the last block may be cut short by `height`, a padding block has 0.
struct rt_film_span {
  long long tile_pixel, frame_pixel;
  int n_pixels;
};
RT_FILM_FN rt_film_span rt_film_block_span(int b, int width, int height, int n_shards, int shard, int row_block) {
  const long long g0 = ((long long)b * n_shards + shard) * row_block;  // the block's first global row
  const long long left = (long long)height - g0;
  const int rows = left <= 0 ? 0 : (left < row_block ? (int)left : row_block);
  rt_film_span s;
  s.tile_pixel = (long long)b * row_block * width;
  s.frame_pixel = g0 * width;
  s.n_pixels = rows * width;
  return s;
}

// ---- launchers (rt_film.hip); device pointers, asynchronous on `stream`, 0 or -1
// pixels per workgroup of both kernels (one partial of the noise figure per workgroup)
#define RT_FILM_TILE 512
inline int rt_film_blocks(long long n_pixels) { return (int)((n_pixels + RT_FILM_TILE - 1) / RT_FILM_TILE); }
// Buffers: every array starts 16-byte aligned; `total` and `q` have 16 bytes, the flag arrays up
// to a multiple of 16 bytes, of zeroed slack behind their n_pixels entries (vector accesses)
int rt_film_launch_merge(unsigned long long* total, unsigned int* flags, double* q, const unsigned long long* pass,
                         const unsigned int* pass_flags, long long n_pixels, int acc_words, int n_samples,
                         void* stream);
// The merge of shard (n_shards, shard, row_block)'s pass (pass / pass_flags: its tile of tile_rows =
// rt_shard_rows rows) into the totals of a whole width x height frame (total / flags / q), block by
// block through rt_film_block_span.  It touches the frame pixels of the shard's rows and nothing
// else (no slack is needed or written), so merges of different shards into one frame may overlap.
int rt_film_launch_merge_rows(unsigned long long* total, unsigned int* flags, double* q, const unsigned long long* pass,
                              const unsigned int* pass_flags, int width, int height, int tile_rows, int n_shards, int shard,
                              int row_block, int acc_words, int n_samples, void* stream);
// map (float per tile pixel) may be null; partial_sum / partial_cnt: rt_film_blocks(n_pixels)
// entries, the sum of r^2 and the number of pixels that count per workgroup, to be added in index
// order.  Tile rows whose global row (the rt_exec interleave) is >= height are padding
int rt_film_launch_noise(const unsigned long long* total, const unsigned int* flags, const double* q, float* map,
                         double* partial_sum, int* partial_cnt, long long n_pixels, int acc_words, long long N, int K,
                         int width, int height, int n_shards, int shard, int row_block, void* stream);
