// dn_host.cpp — TEST TOOLING: the denoiser's per-pixel functions (raytrace_amd/csrc/rt_denoise.h,
// the text the kernels of rt_denoise.hip run) compiled for the host as a stand-alone program, so
// tests/test_denoise_host.py can compare them bit for bit with the numpy twin and run them under
// AddressSanitizer / UBSan.  usage: dn_host <in> <out>
//   in : int32 W, H, levels, k, n_feat, K, fw (8: high feature words only, 16: with low words),
//        n_albedo (0: no remodulation albedo); int64 N; double sigma_z, sigma_l, sigma_a, eps_n, eps_z, eps_l;
//        int64 S[W H fw 3 / 8] (the film's sum words: 3, or 6 with their low words); double q[W H];
//        int64 F[W H fw]; int64 F2[W H fw] if n_albedo > 0; uint32 flags[W H]
//   out: double rgb[W H 3] (e b+ after `levels` levels; NaN where flagged)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../raytrace_amd/csrc/rt_denoise.h"

namespace {

struct HostSrc {
  const std::vector<double>*ev, *guide;
  const std::vector<uint32_t>* flags;
  long long n;
  int W;
  size_t at(int x, int y) const { return (size_t)y * W + x; }
  double e(int c, int x, int y) const { return ev->at(c * n + at(x, y)); }
  double v(int x, int y) const { return ev->at(3 * n + at(x, y)); }
  double gn(int c, int x, int y) const { return guide->at(c * n + at(x, y)); }
  double gz(int x, int y) const { return guide->at(3 * n + at(x, y)); }
  double gc(int x, int y) const { return guide->at(4 * n + at(x, y)); }
  double ga(int c, int x, int y) const { return guide->at((5 + c) * n + at(x, y)); }
  bool flag(int x, int y) const { return flags->at(at(x, y)) != 0u; }
};

template <class T>
bool get(FILE* f, T* p, size_t count) {
  return fread(p, sizeof(T), count, f) == count;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hd[8];
  int64_t N;
  double pr[6];
  if (!get(f, hd, 8) || !get(f, &N, 1) || !get(f, pr, 6)) return 3;
  const int W = hd[0], H = hd[1], n_feat = hd[4], K = hd[5], fw = hd[6], n_albedo = hd[7];
  rt_denoise_params P;
  rt_dn_defaults(&P);
  P.levels = hd[2], P.k = hd[3];
  P.sigma_z = pr[0], P.sigma_l = pr[1], P.sigma_a = pr[2], P.eps_n = pr[3], P.eps_z = pr[4], P.eps_l = pr[5];
  if (W < 1 || H < 1 || W > 4096 || H > 4096 || !rt_dn_params_ok(&P) || n_feat < 1 || K < 2 || N < K ||
      (fw != 8 && fw != 16) || n_albedo < 0)
    return 3;
  const long long n = (long long)W * H;
  const int sw = fw == 16 ? 6 : 3;
  std::vector<long long> S(sw * n), F(fw * n), F2(n_albedo > 0 ? fw * n : 0);
  std::vector<double> q(n);
  std::vector<uint32_t> flags(n);
  if (!get(f, S.data(), S.size()) || !get(f, q.data(), q.size()) || !get(f, F.data(), F.size()) ||
      !get(f, F2.data(), F2.size()) ||
      !get(f, flags.data(), flags.size()))
    return 3;
  fclose(f);
  std::vector<double> ev[2] = {std::vector<double>(RT_DN_EV_PLANES * n), std::vector<double>(RT_DN_EV_PLANES * n)};
  std::vector<double> guide(RT_DN_GUIDE_PLANES * n);
  for (long long i = 0; i < n; ++i) {
    const rt_dn_inputs r = rt_dn_prepare(&S[sw * i], fw == 16 ? &S[sw * i + 3] : nullptr, q[i], N, K, &F[fw * i],
                                         fw == 16 ? &F[fw * i + 8] : nullptr, n_feat, n_albedo > 0 ? &F2[fw * i] : nullptr,
                                         n_albedo > 0 && fw == 16 ? &F2[fw * i + 8] : nullptr, n_albedo);
    for (int c = 0; c < 3; ++c)
      ev[0][c * n + i] = r.e[c], guide[c * n + i] = r.n[c], guide[(5 + c) * n + i] = r.ap[c], guide[(8 + c) * n + i] = r.bp[c];
    ev[0][3 * n + i] = r.v;
    guide[3 * n + i] = r.z, guide[4 * n + i] = r.cov;
  }
  int cur = 0;
  for (int l = 0; l < P.levels; ++l, cur ^= 1) {
    const HostSrc src{&ev[cur], &guide, &flags, n, W};
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        double oe[3], ov;
        rt_dn_filter(src, P, x, y, W, H, 1 << l, oe, ov);
        const long long i = (long long)y * W + x;
        for (int c = 0; c < 3; ++c) ev[cur ^ 1][c * n + i] = oe[c];
        ev[cur ^ 1][3 * n + i] = ov;
      }
  }
  std::vector<double> out(3 * n);
  for (long long i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) out[3 * i + c] = flags[i] ? std::nan("") : ev[cur][c * n + i] * guide[(8 + c) * n + i];
  FILE* g = fopen(argv[2], "wb");
  if (!g || fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) return 4;
  fclose(g);
  return 0;
}
