// rt_adaptive.h — adaptive film passes: per-pixel arithmetic (host and device, as rt_film.h's, so a
// CPU program calls exactly what the kernels run) and the launchers of rt_adaptive.hip.  Not part of
// the public ABI (include/rt.h rt_adaptive_*; rt_api_film.hip holds the state and the entry points).
//
// A film becomes NON-UNIFORM at its first adaptive pass: it gains a count plane, two uint32 per tile
// pixel, the pixel's samples N_p and passes K_p (a shard's padding rows hold (0, 0)).  A pass of n
// samples with threshold t and cap `max`:
//   select   a pixel that counts (inside the frame, not NaN-flagged) is selected iff
//            rt_film_rel_error(q_p, T_p, N_p, K_p) > t   (binary64; t < 0: every counting pixel)
//            and N_p + n <= max; the selected pixels' {tile pixel, N_p} in ascending tile-pixel order
//   render   samples [N_p, N_p + n) of each selected pixel summed into the zeroed pass workspace
//            (rt_list.h: the render's own streams, so the words are a uniform render's)
//   merge    per selected pixel what rt_film_merge_kernel does per pixel, with the pixel's counts:
//            total += pass, flag |= pass flag, q = rt_film_q_add(q, L, n), (N_p, K_p) += (n, 1)
// Unselected pixels are not touched.  Sums are integers keyed by (pixel, sample index), so pixel p
// at N_p samples is bit for bit pixel p of a uniform film at N_p, whatever the others hold, and the
// batch-means estimator (rt_film.h) holds per pixel with its own (N_p, K_p).
#pragma once
#include "rt_film.h"

// one entry of the selection list
struct rt_adaptive_rec {
  int32_t tp;   // tile pixel
  uint32_t n;   // N_p before the pass: the pixel's first new sample
};

// tile pixel tp of shard (n_shards, shard, row_block) lies inside a frame of `height` rows (the
// rt_exec row interleave, rt_film.hip rt_film_noise_kernel)
RT_FILM_FN bool rt_adaptive_inside(long long tp, int width, int height, int n_shards, int shard, int row_block) {
  const int t = (int)(tp / width);
  const int g = ((t / row_block) * n_shards + shard) * row_block + t % row_block;
  return g < height;
}

// the pixel's relative error with its own counts: what rt_film_noise maps, before the cast to float
RT_FILM_FN double rt_adaptive_rel_error(double q, long long hr, long long hg, long long hb, uint32_t N, uint32_t K) {
  return rt_film_rel_error(q, rt_film_lum(hr, hg, hb), (long long)N, (int)K);
}

// the select predicate of a pixel that lies inside the frame; hr, hg, hb: its totals' high words
RT_FILM_FN bool rt_adaptive_select(double q, long long hr, long long hg, long long hb, unsigned flag, uint32_t N, uint32_t K,
                                   int n, double threshold, long long max_samples) {
  if (flag != 0u || K < 2u) return false;
  if ((long long)N + n > max_samples) return false;
  return threshold < 0.0 || rt_adaptive_rel_error(q, hr, hg, hb, N, K) > threshold;
}

// the merge of one selected pixel: kW words of pass sums at `pass` into `total`, the flag, q and the
// counts (cnt[0] = N_p, cnt[1] = K_p)
RT_FILM_FN void rt_adaptive_merge_pixel(unsigned long long* total, unsigned int* flag, double* q, uint32_t* cnt,
                                        const unsigned long long* pass, unsigned int pass_flag, int kW, int n) {
  for (int c = 0; c < kW; ++c) total[c] += pass[c];
  *flag |= pass_flag;
  *q = rt_film_q_add(*q, rt_film_lum((long long)pass[0], (long long)pass[1], (long long)pass[2]), n);
  cnt[0] += (uint32_t)n;
  cnt[1] += 1u;
}

// resolve with counts: rt_render_kernel.h rt_resolve_kernel's operation sequence with the pixel's N_p
RT_FILM_FN double rt_adaptive_resolve64(long long hi, unsigned long long lo, uint32_t N) {
  RT_FILM_NO_CONTRACT
  const double sum = ((double)hi + (double)lo * RT_FILM_UNSCALE) * RT_FILM_UNSCALE;
  return sum / (double)N;
}
RT_FILM_FN float rt_adaptive_resolve32(long long hi, uint32_t N) {
  RT_FILM_NO_CONTRACT
  return (float)((double)hi * (1.0 / (4294967296.0 * (double)N)));
}

// ---- launchers (rt_adaptive.hip); device pointers, asynchronous on `stream`, 0 or -1
#define RT_ADAPTIVE_TILE 256  // pixels per workgroup of the select kernels
inline int rt_adaptive_blocks(long long n_pixels) { return (int)((n_pixels + RT_ADAPTIVE_TILE - 1) / RT_ADAPTIVE_TILE); }
// the scratch of a select: per wave of the tile its 64-bit selection mask, per workgroup its count and offset
inline size_t rt_adaptive_scratch_bytes(long long n_pixels) {
  const size_t b = (size_t)rt_adaptive_blocks(n_pixels);
  return b * (RT_ADAPTIVE_TILE / 64) * sizeof(unsigned long long) + 2 * b * sizeof(int);
}
// counts[p] = (N, K) inside the frame, (0, 0) on a shard's padding rows
int rt_adaptive_launch_init(uint32_t* counts, long long n_pixels, uint32_t N, uint32_t K, int width, int height,
                            int n_shards, int shard, int row_block, void* stream);
// the selection list (ascending tile pixels) and *n_list; scratch: rt_adaptive_scratch_bytes, 8-byte aligned
int rt_adaptive_launch_select(const unsigned long long* total, const unsigned int* flags, const double* q,
                              const uint32_t* counts, long long n_pixels, int acc_words, int n_samples, double threshold,
                              long long max_samples, int width, int height, int n_shards, int shard, int row_block,
                              void* scratch, rt_adaptive_rec* list, int* n_list, void* stream);
// the merge of the listed pixels' pass words; a worst-case grid (n_pixels threads) whose threads
// beyond *n_list exit at once
int rt_adaptive_launch_merge(unsigned long long* total, unsigned int* flags, double* q, uint32_t* counts,
                             const unsigned long long* pass, const unsigned int* pass_flags, const rt_adaptive_rec* list,
                             const int* n_list, long long n_pixels, int acc_words, int n_samples, void* stream);
// out: 3 reals per tile pixel (float with f32), NaN where flagged; a pixel without samples (a padding row) 0
int rt_adaptive_launch_resolve(const unsigned long long* total, const unsigned int* flags, const uint32_t* counts, void* out,
                               long long n_pixels, int f32, void* stream);
// as rt_film_launch_noise with the pixels' own counts (the same partials in the same order)
int rt_adaptive_launch_noise(const unsigned long long* total, const unsigned int* flags, const double* q,
                             const uint32_t* counts, float* map, double* partial_sum, int* partial_cnt, long long n_pixels,
                             int acc_words, int width, int height, int n_shards, int shard, int row_block, void* stream);
