// merge_rows.cpp — TEST TOOLING (tests/test_multi_film_host.py): the row map of a multi-device
// film's merge (raytrace_amd/csrc/rt_film.h rt_film_block_span, the function
// rt_film_merge_rows_kernel runs) on the host.
//
//   merge_rows map <librt_amd.so>
//     rt_film_block_span against a plain loop over the library's rt_shard_row / rt_shard_rows, for
//     height in {1, 7, 8, 50} x width in {1, 9, 50} x row_block in {1, 3, 4} x n_shards in {1, 2, 3, 5},
//     every shard: each tile pixel of a span lies where rt_shard_row puts its row, every frame pixel
//     is the target of exactly one (shard, tile pixel), padding rows target nothing.  Prints
//     "ok <pixels checked>" or the first mismatch.
//
//   merge_rows merge <in> <out>
//     The merge restated for the host: the kernel's per-pixel functions (rt_film_lum, rt_film_q_add)
//     driven by rt_film_block_span over shard tiles.
//     input : int64 kW, width, height, row_block, n_shards, K, sizes[K]; then per pass, per shard:
//             int64 sums[tile_rows * width * kW], uint32 flags[tile_rows * width]
//             (tile_rows: height when n_shards = 1, else ceil(ceil(height / row_block) / n_shards) row_block)
//     output: int64 total[height * width * kW], uint32 flags[height * width], double q[height * width]
// Build: g++ -std=c++17 -ffp-contract=off merge_rows.cpp -ldl
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/rt.h"
#include "../../raytrace_amd/csrc/rt_film.h"

static int check_map(const char* lib) {
  void* h = dlopen(lib, RTLD_NOW | RTLD_LOCAL);
  if (!h) return std::printf("dlopen: %s\n", dlerror()), 1;
  auto shard_rows = (int (*)(int32_t, const rt_exec*))dlsym(h, "rt_shard_rows");
  auto shard_row = (int (*)(int32_t, const rt_exec*))dlsym(h, "rt_shard_row");
  if (!shard_rows || !shard_row) return std::printf("rt_shard_rows / rt_shard_row not found\n"), 1;
  long long checked = 0;
  for (int height : {1, 7, 8, 50})
    for (int width : {1, 9, 50})
      for (int row_block : {1, 3, 4})
        for (int n_shards : {1, 2, 3, 5}) {
          std::vector<int> hits((size_t)height * width, 0);
          for (int shard = 0; shard < n_shards; ++shard) {
            rt_exec ex;
            std::memset(&ex, 0, sizeof ex);
            ex.n_shards = n_shards, ex.shard = shard, ex.row_block = row_block;
            const int tile_rows = shard_rows(height, &ex);
            // (one shard: the tile is the image, its last block cut short; else whole blocks)
            if (tile_rows <= 0 || (n_shards > 1 && tile_rows % row_block))
              return std::printf("rt_shard_rows(%d) = %d (row_block %d)\n", height, tile_rows, row_block), 1;
            std::vector<char> covered((size_t)tile_rows * width, 0);
            for (int b = 0; b < (tile_rows + row_block - 1) / row_block; ++b) {
              const rt_film_span s = rt_film_block_span(b, width, height, n_shards, shard, row_block);
              if (s.n_pixels < 0 || s.n_pixels % width || s.tile_pixel + s.n_pixels > (long long)tile_rows * width)
                return std::printf("span out of the tile: h %d w %d rb %d shard %d/%d block %d\n", height, width, row_block,
                                   shard, n_shards, b), 1;
              for (int i = 0; i < s.n_pixels; ++i) {
                const long long tp = s.tile_pixel + i, fp = s.frame_pixel + i;
                const int g = shard_row((int)(tp / width), &ex);  // the plain map: tile row -> global row
                if (g >= height || fp != (long long)g * width + tp % width || fp < 0 || fp >= (long long)height * width)
                  return std::printf("h %d w %d rb %d shard %d/%d: tile pixel %lld -> frame pixel %lld, row %d\n", height,
                                     width, row_block, shard, n_shards, tp, fp, g), 1;
                covered[(size_t)tp] = 1;
                ++hits[(size_t)fp];
                ++checked;
              }
            }
            for (int t = 0; t < tile_rows; ++t)  // exactly the rows inside the frame are covered
              for (int x = 0; x < width; ++x)
                if ((shard_row(t, &ex) < height) != (covered[(size_t)t * width + x] != 0))
                  return std::printf("h %d w %d rb %d shard %d/%d: tile row %d (global %d) covered %d\n", height, width,
                                     row_block, shard, n_shards, t, shard_row(t, &ex), covered[(size_t)t * width + x]), 1;
          }
          for (size_t p = 0; p < hits.size(); ++p)
            if (hits[p] != 1)
              return std::printf("h %d w %d rb %d n %d: frame pixel %zu is the target of %d tile pixels\n", height, width,
                                 row_block, n_shards, p, hits[p]), 1;
        }
  std::printf("ok %lld\n", checked);
  return 0;
}

template <class T>
static bool read_n(FILE* f, std::vector<T>& v) { return std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

static int merge(const char* src, const char* dst) {
  FILE* in = std::fopen(src, "rb");
  if (!in) return 2;
  long long hd[6];
  if (std::fread(hd, 8, 6, in) != 6) return 2;
  const int kW = (int)hd[0], width = (int)hd[1], height = (int)hd[2], row_block = (int)hd[3], n_shards = (int)hd[4];
  const long long K = hd[5];
  if ((kW != 3 && kW != 6) || width < 1 || height < 1 || row_block < 1 || n_shards < 1 || K < 1 || K > 64) return 2;
  std::vector<long long> sizes((size_t)K);
  if (!read_n(in, sizes)) return 2;
  const int blocks = (height + row_block - 1) / row_block;
  const int tile_rows = n_shards == 1 ? height : (blocks + n_shards - 1) / n_shards * row_block;
  const int rb = n_shards == 1 ? height : row_block;  // (one shard: the tile is the frame, one block)
  const size_t n = (size_t)height * width, tn = (size_t)tile_rows * width;
  std::vector<long long> total(n * kW, 0), pass(tn * kW);
  std::vector<unsigned> flags(n, 0u), pflags(tn);
  std::vector<double> q(n, 0.0);
  for (long long k = 0; k < K; ++k)
    for (int shard = 0; shard < n_shards; ++shard) {
      if (!read_n(in, pass) || !read_n(in, pflags)) return 2;
      for (int b = 0; b < tile_rows / rb; ++b) {
        const rt_film_span s = rt_film_block_span(b, width, height, n_shards, shard, rb);
        for (int i = 0; i < s.n_pixels; ++i) {  // what rt_film_merge_rows_kernel does per pixel
          const long long* a = &pass[(size_t)(s.tile_pixel + i) * kW];
          long long* t = &total[(size_t)(s.frame_pixel + i) * kW];
          for (int c = 0; c < kW; ++c) t[c] += a[c];
          flags[(size_t)(s.frame_pixel + i)] |= pflags[(size_t)(s.tile_pixel + i)];
          double& qq = q[(size_t)(s.frame_pixel + i)];
          qq = rt_film_q_add(qq, rt_film_lum(a[0], a[1], a[2]), (int)sizes[(size_t)k]);
        }
      }
    }
  std::fclose(in);
  FILE* out = std::fopen(dst, "wb");
  if (!out) return 2;
  std::fwrite(total.data(), 8, total.size(), out);
  std::fwrite(flags.data(), 4, flags.size(), out);
  std::fwrite(q.data(), 8, q.size(), out);
  std::fclose(out);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "map")) return check_map(argv[2]);
  if (argc == 4 && !std::strcmp(argv[1], "merge")) return merge(argv[2], argv[3]);
  return 2;
}
