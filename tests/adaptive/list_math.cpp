// list_math.cpp — TEST TOOLING (tests/test_adaptive_host.py): the adaptive passes' per-pixel functions
// (raytrace_amd/csrc/rt_adaptive.h, the text the select, merge, resolve and noise kernels run) on
// the host, over a film state read from a file.
//   input : int64 n_pixels, kW (3 or 6), n (the pass's samples), max_samples; double threshold;
//           uint64 total[n_pixels][kW]; uint32 flags[n_pixels]; double q[n_pixels];
//           uint32 counts[n_pixels][2]; uint64 pass[n_pixels][kW]; uint32 pass_flags[n_pixels];
//           uint8 listed[n_pixels] (a selection for the merge check)
//   output: double r[n_pixels] (noise with counts); uint8 selected[n_pixels] (the select predicate)
// and checked here (exit status 1 and a line on stderr otherwise):
//   - the merge of the listed pixels equals the whole-frame merge (rt_film.h's steps, as
//     rt_film_merge_kernel runs them) on those pixels plus their counts' step, and leaves every
//     other pixel's bytes as they were;
//   - the resolve with counts equals the uniform resolve's operation sequence, bit for bit.
// Build: g++ -std=c++17 -ffp-contract=off list_math.cpp
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raytrace_amd/csrc/rt_adaptive.h"

template <class T>
static bool rd(FILE* in, std::vector<T>& v) {
  return std::fread(v.data(), sizeof(T), v.size(), in) == v.size();
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  long long head[4];
  double threshold = 0;
  if (std::fread(head, 8, 4, in) != 4 || std::fread(&threshold, 8, 1, in) != 1) return 2;
  const long long np = head[0], kW = head[1], n = head[2], max_samples = head[3];
  if (np < 0 || np > (1 << 24) || (kW != 3 && kW != 6) || n <= 0) return 2;
  std::vector<unsigned long long> total(np * kW), pass(np * kW);
  std::vector<unsigned> flags(np), pass_flags(np);
  std::vector<double> q(np);
  std::vector<uint32_t> counts(2 * np);
  std::vector<unsigned char> listed(np);
  if (!rd(in, total) || !rd(in, flags) || !rd(in, q) || !rd(in, counts) || !rd(in, pass) || !rd(in, pass_flags) ||
      !rd(in, listed))
    return 2;
  std::fclose(in);

  // noise with counts and the select predicate, for the numpy twin
  std::vector<double> r(np);
  std::vector<unsigned char> sel(np);
  for (long long i = 0; i < np; ++i) {
    const long long* a = (const long long*)&total[i * kW];
    r[i] = rt_adaptive_rel_error(q[i], a[0], a[1], a[2], counts[2 * i], counts[2 * i + 1]);
    sel[i] = rt_adaptive_select(q[i], a[0], a[1], a[2], flags[i], counts[2 * i], counts[2 * i + 1], (int)n, threshold,
                                max_samples);
  }

  // the list merge against the whole-frame merge
  std::vector<rt_adaptive_rec> list;
  for (long long i = 0; i < np; ++i)
    if (listed[i]) list.push_back(rt_adaptive_rec{(int32_t)i, counts[2 * i]});
  std::vector<unsigned long long> t2 = total;
  std::vector<unsigned> f2 = flags;
  std::vector<double> q2 = q;
  std::vector<uint32_t> c2 = counts;
  for (const rt_adaptive_rec& e : list) {
    const long long p = e.tp;
    rt_adaptive_merge_pixel(&t2[p * kW], &f2[p], &q2[p], &c2[2 * p], &pass[p * kW], pass_flags[p], (int)kW, (int)n);
  }
  for (long long i = 0; i < np; ++i) {
    std::vector<unsigned long long> wt(total.begin() + i * kW, total.begin() + (i + 1) * kW);
    unsigned wf = flags[i];
    double wq = q[i];
    uint32_t wc[2] = {counts[2 * i], counts[2 * i + 1]};
    if (listed[i]) {  // rt_film_merge_kernel's steps for one pixel
      for (int c = 0; c < kW; ++c) wt[c] += pass[i * kW + c];
      wf |= pass_flags[i];
      wq = rt_film_q_add(wq, rt_film_lum((long long)pass[i * kW], (long long)pass[i * kW + 1], (long long)pass[i * kW + 2]),
                         (int)n);
      wc[0] += (uint32_t)n, wc[1] += 1u;
    }
    if (std::memcmp(wt.data(), &t2[i * kW], 8 * kW) || wf != f2[i] || std::memcmp(&wq, &q2[i], 8) ||
        std::memcmp(wc, &c2[2 * i], 8)) {
      std::fprintf(stderr, "merge: pixel %lld (%s) differs\n", i, listed[i] ? "listed" : "not listed");
      return 1;
    }
  }

  // resolve with counts at uniform counts N against the uniform resolve (rt_render_kernel.h
  // rt_resolve_kernel; tests/kernel_emu emu_body.h), for a few N
  const uint32_t Ns[] = {1u, 3u, 8u, 16u, 1000u, 1u << 24};
  for (uint32_t N : Ns)
    for (long long i = 0; i < np; ++i)
      for (int c = 0; c < 3; ++c) {
        const long long hi = (long long)total[i * kW + c];
        const unsigned long long lo = kW == 6 ? total[i * kW + 3 + c] : 0ull;
        const double sum = ((double)hi + (double)lo * (1.0 / 4294967296.0)) * (1.0 / 4294967296.0);
        const double want64 = sum / (double)N;
        const double scale = 1.0 / (4294967296.0 * (double)N);
        const float want32 = (float)((double)hi * scale);
        const double got64 = rt_adaptive_resolve64(hi, lo, N);
        const float got32 = rt_adaptive_resolve32(hi, N);
        if (std::memcmp(&want64, &got64, 8) || std::memcmp(&want32, &got32, 4)) {
          std::fprintf(stderr, "resolve: pixel %lld channel %d N %u differs\n", i, c, N);
          return 1;
        }
      }

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  std::fwrite(r.data(), 8, np, out);
  std::fwrite(sel.data(), 1, np, out);
  std::fclose(out);
  std::printf("ok %zu listed\n", list.size());
  return 0;
}
