// pixel_math.cpp — TEST TOOLING (tests/test_film_host.py): the film's per-pixel functions
// (raytrace_amd/csrc/rt_film.h, the text the merge and noise kernels run) on the host, over pass
// sums read from a file, so that raytrace_amd.film.noise_from_sums can be checked against them.
//   input : int64 K, int64 n_pixels, int64 sizes[K], int64 sums[K][n_pixels][3]
//   output: double q[n_pixels], double v[n_pixels], double r[n_pixels]
// Build: g++ -std=c++17 -ffp-contract=off pixel_math.cpp
#include <cstdio>
#include <vector>

#include "../../raytrace_amd/csrc/rt_film.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  long long K = 0, n = 0;
  if (std::fread(&K, 8, 1, in) != 1 || std::fread(&n, 8, 1, in) != 1 || K < 2 || K > 64 || n < 0) return 2;
  std::vector<long long> sizes(K), sums((size_t)(K * n * 3));
  if (std::fread(sizes.data(), 8, K, in) != (size_t)K || std::fread(sums.data(), 8, sums.size(), in) != sums.size())
    return 2;
  std::fclose(in);
  long long N = 0;
  for (long long s : sizes) N += s;
  std::vector<double> q(n, 0.0), v(n), r(n);
  for (long long i = 0; i < n; ++i) {
    long long total[3] = {0, 0, 0};
    for (long long k = 0; k < K; ++k) {  // what rt_film_merge_kernel does per pass
      const long long* a = &sums[(size_t)((k * n + i) * 3)];
      for (int c = 0; c < 3; ++c) total[c] += a[c];
      q[i] = rt_film_q_add(q[i], rt_film_lum(a[0], a[1], a[2]), (int)sizes[k]);
    }
    const double T = rt_film_lum(total[0], total[1], total[2]);  // rt_film_noise_kernel
    v[i] = rt_film_variance(q[i], T, N, (int)K);
    r[i] = rt_film_rel_error(q[i], T, N, (int)K);
  }
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  std::fwrite(q.data(), 8, n, out);
  std::fwrite(v.data(), 8, n, out);
  std::fwrite(r.data(), 8, n, out);
  std::fclose(out);
  return 0;
}
