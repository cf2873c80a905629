// rt_denoise.h — the film's variance-guided denoiser: per-pixel arithmetic (host and device, so a
// CPU program can call exactly what the kernels of rt_denoise.hip run) and the launchers.  Not part
// of the public ABI (include/rt.h rt_denoise_*; rt_api_film.hip holds the buffers and the entry points).
//
// An edge-stopping a-trous wavelet filter (5 x 5 B3-spline taps at step 2^i per level) of the film's
// mean colour demodulated by the first-hit albedo, guided by the first-hit normal and depth
// (rt_features.h) and by the film's own variance estimate (rt_film.h).  Everything is binary64
// whatever the film's precision, written with + - x / sqrt, min / max and comparisons only, never
// contracted, and summed in one fixed order, so that raytrace_amd.denoise.denoise_reference (numpy)
// gives the same bits.  That is why the edge-stopping functions are rational, not exponentials.
//
// Per pixel, with N samples in K passes, the film's sum words S (and, in a binary64 film, their low
// words S': the image's own mean, rt_render_kernel.h rt_resolve_kernel), its estimator word q, and the
// n_feat feature samples' words F (rt_features.h: albedo RGB, normal xyz, depth sum, hit count; each
// real a high word F and, in a binary64 film, a low word F' with the next 32 bits, 0 in an FP32 film):
//   c  = f(S) / N                                  mean colour, the film's image
//   f(F) = ((double)F + (double)F' 2^-32) 2^-32    a feature sum (one rounding, as the resolve's)
//   a  = f(F_albedo) / n_feat                      a+ = max(a, 1/256) per channel
//   n  = f(F_normal) / n_feat
//   z  = f(F_depth) / hits (0 without hits)        cov = hits / n_feat
//   e  = c / a+                                    the demodulated colour;  l = (e_R + e_G) + e_B
//   v  = rt_film_variance(q, T, N, K) / N 2^-64 / m^2,  m = max(((a_R + a_G) + a_B) / 3, 1/256)
//        (T: the high words' luminance word, as the film's noise estimate)
// Level i (step s = 2^i) replaces (e, v) at pixel p by
//   e' = sum_q w e_q / sum_q w,   v' = sum_q w^2 v_q / (sum_q w)^2,   w = (((h w_n) w_z) w_a) w_l
// over the 25 taps q = p + s (dx, dy), dy = -2..2 outer, dx = -2..2 inner, in that order from 0.0;
// taps outside the frame and NaN-flagged taps are skipped; a NaN-flagged centre keeps (e, v).
//   h   = k[dx] k[dy],  k = (1/16, 1/4, 3/8, 1/4, 1/16)
//   w_n = (max(0, n_p . n_q) / max(sqrt(|n_p|^2 |n_q|^2), eps_n))^(2^k) by k squarings; 1 when both
//         |n|^2 < eps_n (featureless: misses, media), 0 when exactly one is
//   w_z = 1 / (1 + (|z_p - z_q| / (sigma_z max(z_p, z_q, eps_z)))^2); 1 when both cov = 0, 0 when one is
//   w_a = 1 / (1 + ((r_R^2 + r_G^2) + r_B^2) / sigma_a^2),  r = (a+_p - a+_q) / max(a+_p, a+_q) per channel: the
//         albedo as a guide, in w_z's relative form.  A pixel an emitter's edge crosses has an albedo
//         between the emitter's and the wall's; without this weight its quiet e (the colour and the
//         albedo of the same samples carry the same coverage noise) is mixed with the wall's, because
//         the film's variance of c, large there, opens w_l (profiles/denoise/README.md)
//   w_l = 1 / (1 + (l_p - l_q)^2 / (sigma_l^2 g_p + eps_l)),  g_p = the (1 2 1) x (1 2 1) weighted mean
//         of the level's input v over the 3 x 3 unit-step neighbours in the frame that are not
//         NaN-flagged (dy outer, dx inner; the centre always counts)
// The output is e_final b+ per channel, in the film's dtype; NaN for NaN-flagged pixels, as the image.
// b+ = max(b, 1/256) is the REMODULATION albedo: b = f(F2_albedo) / n_albedo from a second feature
// buffer of more samples (rt_denoise_albedo, 64 by default) where there is one, else a.  Dividing by
// the albedo of the film's own first samples cancels the coverage noise they share; multiplying by a
// better estimate of the same albedo then removes it from the output instead of putting it back.
#pragma once
#include <stdint.h>

#include "../../include/rt.h"
#include "rt_film.h"

#define RT_DN_FN RT_FILM_FN
#define RT_DN_NO_CONTRACT RT_FILM_NO_CONTRACT
#define RT_DN_ALBEDO_FLOOR (1.0 / 256.0)
#define RT_DN_UNSCALE2 (RT_FILM_UNSCALE * RT_FILM_UNSCALE)  // 2^-64
#define RT_FEAT_WORDS 8  // per pixel: albedo RGB, normal xyz, depth sum (2^-32 units), hit count
// ... and the buffer's words per pixel: those, then in a binary64 film their low words (the last unused)
constexpr int rt_feat_words(bool f64) { return f64 ? 2 * RT_FEAT_WORDS : RT_FEAT_WORDS; }

RT_DN_FN double rt_dn_max(double a, double b) { return a > b ? a : b; }

// the level-0 inputs of one pixel from the film's words and the feature words
struct rt_dn_inputs {
  double e[3], v, ap[3], n[3], z, cov, bp[3];
};
// a fixed-point sum: high word k of F and, where Flo is not null, its low word (a binary64 film's)
RT_DN_FN double rt_dn_feature_sum(const long long* F, const long long* Flo, int k) {
  RT_DN_NO_CONTRACT
  const double lo = Flo ? (double)(unsigned long long)Flo[k] : 0.0;
  return ((double)F[k] + lo * RT_FILM_UNSCALE) * RT_FILM_UNSCALE;
}
// S: the film's 3 high sum words; Slo: their low words (a binary64 film's) or null
RT_DN_FN rt_dn_inputs rt_dn_prepare(const long long* S, const long long* Slo, double q, long long N, int K,
                                    const long long* F, const long long* Flo, int n_feat,
                                    const long long* F2 = nullptr, const long long* F2lo = nullptr, int n_albedo = 0) {
  RT_DN_NO_CONTRACT
  rt_dn_inputs r;
  double a[3];
  for (int c = 0; c < 3; ++c) {
    const double mean = rt_dn_feature_sum(S, Slo, c) / (double)N;
    a[c] = rt_dn_feature_sum(F, Flo, c) / (double)n_feat;
    r.ap[c] = rt_dn_max(a[c], RT_DN_ALBEDO_FLOOR);
    r.e[c] = mean / r.ap[c];
    r.n[c] = rt_dn_feature_sum(F, Flo, 3 + c) / (double)n_feat;
    r.bp[c] = F2 ? rt_dn_max(rt_dn_feature_sum(F2, F2lo, c) / (double)n_albedo, RT_DN_ALBEDO_FLOOR) : r.ap[c];
  }
  const double var = rt_film_variance(q, rt_film_lum(S[0], S[1], S[2]), N, K);
  const double vm = var / (double)N * RT_DN_UNSCALE2;
  const double m = rt_dn_max(((a[0] + a[1]) + a[2]) / 3.0, RT_DN_ALBEDO_FLOOR);
  r.v = vm / (m * m);
  const long long hits = F[7];
  r.z = hits > 0 ? rt_dn_feature_sum(F, Flo, 6) / (double)hits : 0.0;
  r.cov = (double)hits / (double)n_feat;
  return r;
}

// the guides of a pixel as the weights read them
struct rt_dn_guide {
  double n[3], nn, z, cov, ap[3];
};
RT_DN_FN double rt_dn_nn(const double* n) {
  RT_DN_NO_CONTRACT
  return (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
}
RT_DN_FN double rt_dn_lum(const double* e) { return (e[0] + e[1]) + e[2]; }

// w = (((h w_n) w_z) w_a) w_l of centre p and tap q; lden = sigma_l^2 g_p + eps_l
RT_DN_FN double rt_dn_weight(const rt_denoise_params& P, double h, const rt_dn_guide& p, double lp, double lden,
                             const rt_dn_guide& q, double lq) {
  RT_DN_NO_CONTRACT
  double wn;
  const bool fp = p.nn < P.eps_n, fq = q.nn < P.eps_n;
  if (fp && fq) {
    wn = 1.0;
  } else if (fp || fq) {
    wn = 0.0;
  } else {
    const double d = (p.n[0] * q.n[0] + p.n[1] * q.n[1]) + p.n[2] * q.n[2];
    wn = rt_dn_max(0.0, d) / rt_dn_max(sqrt(p.nn * q.nn), P.eps_n);
    for (int k = 0; k < P.k; ++k) wn = wn * wn;
  }
  double wz;
  const bool cp = p.cov > 0.0, cq = q.cov > 0.0;
  if (!cp && !cq) {
    wz = 1.0;
  } else if (!cp || !cq) {
    wz = 0.0;
  } else {
    const double dz = p.z > q.z ? p.z - q.z : q.z - p.z;
    const double r = dz / (P.sigma_z * rt_dn_max(rt_dn_max(p.z, q.z), P.eps_z));
    wz = 1.0 / (1.0 + r * r);
  }
  double ra[3];
  for (int c = 0; c < 3; ++c) ra[c] = (p.ap[c] - q.ap[c]) / rt_dn_max(p.ap[c], q.ap[c]);
  const double wa = 1.0 / (1.0 + ((ra[0] * ra[0] + ra[1] * ra[1]) + ra[2] * ra[2]) / (P.sigma_a * P.sigma_a));
  const double dl = lp - lq;
  const double wl = 1.0 / (1.0 + dl * dl / lden);
  return (((h * wn) * wz) * wa) * wl;
}

// One level at pixel (x, y) of a W x H frame.  Src gives the level's input and the guides:
//   double e(int c, int x, int y), v(x, y), gn(int c, x, y), gz(x, y), gc(x, y), ga(int c, x, y) (a+);
//   bool flag(x, y)
template <class Src>
RT_DN_FN void rt_dn_filter(const Src& S, const rt_denoise_params& P, int x, int y, int W, int H, int step, double* out_e,
                           double& out_v) {
  RT_DN_NO_CONTRACT
  double ep[3] = {S.e(0, x, y), S.e(1, x, y), S.e(2, x, y)};
  if (S.flag(x, y)) {
    out_e[0] = ep[0], out_e[1] = ep[1], out_e[2] = ep[2];
    out_v = S.v(x, y);
    return;
  }
  // g: the prefiltered variance
  double gs = 0.0, gw = 0.0;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx, qy = y + dy;
      if (qx < 0 || qx >= W || qy < 0 || qy >= H || S.flag(qx, qy)) continue;
      const double k = (double)((2 - (dx < 0 ? -dx : dx)) * (2 - (dy < 0 ? -dy : dy)));  // 1 2 1 / 2 4 2 / 1 2 1
      gs = gs + k * S.v(qx, qy);
      gw = gw + k;
    }
  const double g = gs / gw;
  const double lden = (P.sigma_l * P.sigma_l) * g + P.eps_l;
  rt_dn_guide gp;
  for (int c = 0; c < 3; ++c) gp.n[c] = S.gn(c, x, y), gp.ap[c] = S.ga(c, x, y);
  gp.nn = rt_dn_nn(gp.n);
  gp.z = S.gz(x, y);
  gp.cov = S.gc(x, y);
  const double lp = rt_dn_lum(ep);
  const double kern[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
  double sw = 0.0, sv = 0.0, se[3] = {0.0, 0.0, 0.0};
  for (int dy = -2; dy <= 2; ++dy)
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = x + dx * step, qy = y + dy * step;
      if (qx < 0 || qx >= W || qy < 0 || qy >= H || S.flag(qx, qy)) continue;
      rt_dn_guide gq;
      for (int c = 0; c < 3; ++c) gq.n[c] = S.gn(c, qx, qy), gq.ap[c] = S.ga(c, qx, qy);
      gq.nn = rt_dn_nn(gq.n);
      gq.z = S.gz(qx, qy);
      gq.cov = S.gc(qx, qy);
      const double eq[3] = {S.e(0, qx, qy), S.e(1, qx, qy), S.e(2, qx, qy)};
      const double w = rt_dn_weight(P, kern[dx + 2] * kern[dy + 2], gp, lp, lden, gq, rt_dn_lum(eq));
      sw = sw + w;
      for (int c = 0; c < 3; ++c) se[c] = se[c] + w * eq[c];
      sv = sv + (w * w) * S.v(qx, qy);
    }
  for (int c = 0; c < 3; ++c) out_e[c] = se[c] / sw;
  out_v = sv / (sw * sw);
}

// the shipped parameters (profiles/denoise/README.md: the quality record was measured with these)
inline void rt_dn_defaults(rt_denoise_params* p) {
  p->levels = 5;
  p->k = 5;
  p->sigma_z = 0.1;
  p->sigma_l = 4.0;
  p->sigma_a = 0.1;  // (sigma_z's value: the same relative form, the same role)
  p->eps_n = 1e-6;
  p->eps_z = 1e-6;
  p->eps_l = 1e-10;
}
inline bool rt_dn_params_ok(const rt_denoise_params* p) {
  return p->levels >= 1 && p->levels <= 8 && p->k >= 0 && p->k <= 16 && p->sigma_z > 0.0 && p->sigma_l > 0.0 && p->sigma_a > 0.0 &&
         p->eps_n > 0.0 && p->eps_z > 0.0 && p->eps_l > 0.0;
}

// ---- launchers (rt_denoise.hip); device pointers, asynchronous on `stream`, 0 or -1.
// Planes of n_pixels doubles each: ev[4] (e RGB, v), guide[11] (n xyz, z, cov, a+ RGB, b+ RGB).
#define RT_DN_EV_PLANES 4
#define RT_DN_GUIDE_PLANES 11
int rt_denoise_launch_prepare(const unsigned long long* total, const double* q, const long long* feat, double* ev,
                              double* guide, long long n_pixels, int acc_words, long long N, int K, int n_feat,
                              const long long* feat2_or_null, int n_albedo, void* stream);
// one level: ev_in -> ev_out (different buffers); steps 1 and 2 read their halo through LDS
int rt_denoise_launch_level(const double* ev_in, double* ev_out, const double* guide, const unsigned int* flags,
                            const rt_denoise_params* p, int width, int height, int step, void* stream);
// out (width x height x 3 of float or double) = e b+, NaN where flagged
int rt_denoise_launch_finish(const double* ev, const double* guide, const unsigned int* flags, void* out, int out_f32,
                             long long n_pixels, void* stream);
