// rt_denoise.hip — the denoiser's kernels (rt_denoise.h holds the per-pixel arithmetic and the
// definitions): prepare (film words + feature words -> demodulated colour, variance, guides), one
// launch per a-trous level over ping-pong buffers, finish (x albedo, to the film's dtype).
// Everything is binary64 and compiled without contraction (the Makefile adds -ffp-contract=off for
// this unit on top of the functions' own pragmas): the numpy twin must get the same bits.
//
// Layout: planes of n_pixels doubles (ev: e_R e_G e_B v; guide: n_x n_y n_z z cov, a+ RGB, b+ RGB), so
// the 64 lanes of a wave, on 64 consecutive pixels of a row, read 512 contiguous bytes per plane.
// A level's workgroup is a 64 x 4 pixel tile, one thread per pixel.  Steps 1 and 2 stage the
// tile's (e, v, flag) with its halo of 2 step pixels in LDS (68 x 8 / 72 x 12 pixels, 20 / 31 KB):
// each staged value is read by up to 25 + 9 taps.  The guides are read from memory at every step
// (eight more planes would not fit two workgroups per CU), and so is everything at steps >= 4, whose
// halo (>= 8 pixels a side) is larger than the tile: at a preview's size the planes (600 x 600: 35 MB
// in all) sit in the 256 MB memory-side cache, the taps of neighbouring lanes are neighbouring
// addresses, and the kernel is bound by its binary64 divisions, not by those loads
// (profiles/denoise/README.md).  No MFMA: the weights are data-dependent per tap.
#include <hip/hip_runtime.h>

#include "rt_denoise.h"

namespace {

constexpr int kTileW = 64, kTileH = 4, kThreads = kTileW * kTileH;

template <int kW>
__global__ __launch_bounds__(256) void rt_denoise_prepare_kernel(const long long* __restrict__ total,
                                                                 const double* __restrict__ q,
                                                                 const long long* __restrict__ feat,
                                                                 double* __restrict__ ev, double* __restrict__ guide,
                                                                 long long n, long long N, int K, int n_feat,
                                                                 const long long* __restrict__ feat2, int n_albedo) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long* S = total + kW * i;
  // (kW == 6: a binary64 film, whose feature words have their low words behind them)
  const long long* F = feat + (kW == 6 ? 2 : 1) * RT_FEAT_WORDS * i;
  const long long* F2 = feat2 ? feat2 + (kW == 6 ? 2 : 1) * RT_FEAT_WORDS * i : nullptr;
  const rt_dn_inputs r = rt_dn_prepare(S, kW == 6 ? S + 3 : nullptr, q[i], N, K, F, kW == 6 ? F + RT_FEAT_WORDS : nullptr, n_feat,
                                       F2, F2 && kW == 6 ? F2 + RT_FEAT_WORDS : nullptr, n_albedo);
  ev[i] = r.e[0], ev[n + i] = r.e[1], ev[2 * n + i] = r.e[2], ev[3 * n + i] = r.v;
  guide[i] = r.n[0], guide[n + i] = r.n[1], guide[2 * n + i] = r.n[2];
  guide[3 * n + i] = r.z, guide[4 * n + i] = r.cov;
  guide[5 * n + i] = r.ap[0], guide[6 * n + i] = r.ap[1], guide[7 * n + i] = r.ap[2];
  guide[8 * n + i] = r.bp[0], guide[9 * n + i] = r.bp[1], guide[10 * n + i] = r.bp[2];
}

// the guides, from memory
struct GuideSrc {
  const double* g;
  long long n;
  int W;
  __device__ double gn(int c, int x, int y) const { return g[c * n + (long long)y * W + x]; }
  __device__ double gz(int x, int y) const { return g[3 * n + (long long)y * W + x]; }
  __device__ double gc(int x, int y) const { return g[4 * n + (long long)y * W + x]; }
  __device__ double ga(int c, int x, int y) const { return g[(5 + c) * n + (long long)y * W + x]; }
};
// the level's input from memory (steps >= 4)
struct GlobalSrc : GuideSrc {
  const double* ev;
  const unsigned int* flags;
  __device__ double e(int c, int x, int y) const { return ev[c * n + (long long)y * W + x]; }
  __device__ double v(int x, int y) const { return ev[3 * n + (long long)y * W + x]; }
  __device__ bool flag(int x, int y) const { return flags[(long long)y * W + x] != 0u; }
};
// ... from the workgroup's LDS tile [plane][row][column], origin (x0, y0) in the frame
template <int kPitch, int kRows>
struct LdsSrc : GuideSrc {
  const double* t;
  const unsigned int* f;
  int x0, y0;
  __device__ int at(int x, int y) const { return (y - y0) * kPitch + (x - x0); }
  __device__ double e(int c, int x, int y) const { return t[c * kPitch * kRows + at(x, y)]; }
  __device__ double v(int x, int y) const { return t[3 * kPitch * kRows + at(x, y)]; }
  __device__ bool flag(int x, int y) const { return f[at(x, y)] != 0u; }
};

// kStep 1, 2: the LDS kernels; 0: any step, from memory
template <int kStep>
__global__ __launch_bounds__(kThreads) void rt_denoise_level_kernel(const double* __restrict__ ev_in,
                                                                    double* __restrict__ ev_out,
                                                                    const double* __restrict__ guide,
                                                                    const unsigned int* __restrict__ flags,
                                                                    rt_denoise_params P, int W, int H, int step) {
  const long long n = (long long)W * H;
  const int bx = (int)blockIdx.x * kTileW, by = (int)blockIdx.y * kTileH;
  const int x = bx + (int)(threadIdx.x % kTileW), y = by + (int)(threadIdx.x / kTileW);
  double oe[3], ov;
  if constexpr (kStep > 0) {
    constexpr int kHalo = 2 * kStep, kPitch = kTileW + 2 * kHalo, kRows = kTileH + 2 * kHalo;
    __shared__ double tile[4 * kPitch * kRows];
    __shared__ unsigned int tflag[kPitch * kRows];
    for (int k = (int)threadIdx.x; k < kPitch * kRows; k += kThreads) {
      const int ty = k / kPitch, tx = k - ty * kPitch;
      const int gx = bx - kHalo + tx, gy = by - kHalo + ty;
      const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
      const long long g = (long long)gy * W + gx;
#pragma unroll
      for (int c = 0; c < 4; ++c) tile[c * kPitch * kRows + k] = in ? ev_in[c * n + g] : 0.0;
      tflag[k] = in ? flags[g] : 1u;
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    LdsSrc<kPitch, kRows> S;
    S.g = guide, S.n = n, S.W = W, S.t = tile, S.f = tflag, S.x0 = bx - kHalo, S.y0 = by - kHalo;
    rt_dn_filter(S, P, x, y, W, H, kStep, oe, ov);
  } else {
    if (x >= W || y >= H) return;
    GlobalSrc S;
    S.g = guide, S.n = n, S.W = W, S.ev = ev_in, S.flags = flags;
    rt_dn_filter(S, P, x, y, W, H, step, oe, ov);
  }
  const long long i = (long long)y * W + x;
  ev_out[i] = oe[0], ev_out[n + i] = oe[1], ev_out[2 * n + i] = oe[2], ev_out[3 * n + i] = ov;
}

template <class T>
__global__ __launch_bounds__(256) void rt_denoise_finish_kernel(const double* __restrict__ ev,
                                                                const double* __restrict__ guide,
                                                                const unsigned int* __restrict__ flags,
                                                                T* __restrict__ out, long long n) {
  RT_DN_NO_CONTRACT
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool bad = flags[i] != 0u;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double val = ev[c * n + i] * guide[(8 + c) * n + i];
    out[3 * i + c] = bad ? (T)__builtin_nan("") : (T)val;
  }
}

}  // namespace

int rt_denoise_launch_prepare(const unsigned long long* total, const double* q, const long long* feat, double* ev,
                              double* guide, long long n_pixels, int acc_words, long long N, int K, int n_feat,
                              const long long* feat2, int n_albedo, void* stream) {
  if (n_pixels <= 0) return 0;
  const dim3 grid((unsigned)((n_pixels + 255) / 256)), block(256);
  const long long* t = reinterpret_cast<const long long*>(total);
  if (acc_words == 6)
    hipLaunchKernelGGL(rt_denoise_prepare_kernel<6>, grid, block, 0, (hipStream_t)stream, t, q, feat, ev, guide, n_pixels,
                       N, K, n_feat, feat2, n_albedo);
  else
    hipLaunchKernelGGL(rt_denoise_prepare_kernel<3>, grid, block, 0, (hipStream_t)stream, t, q, feat, ev, guide, n_pixels,
                       N, K, n_feat, feat2, n_albedo);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rt_denoise_launch_level(const double* ev_in, double* ev_out, const double* guide, const unsigned int* flags,
                            const rt_denoise_params* p, int width, int height, int step, void* stream) {
  if (width <= 0 || height <= 0) return 0;
  const dim3 grid((unsigned)((width + kTileW - 1) / kTileW), (unsigned)((height + kTileH - 1) / kTileH)), block(kThreads);
  if (grid.y > 65535u) return -1;
  hipStream_t st = (hipStream_t)stream;
  if (step == 1)
    hipLaunchKernelGGL(rt_denoise_level_kernel<1>, grid, block, 0, st, ev_in, ev_out, guide, flags, *p, width, height, step);
  else if (step == 2)
    hipLaunchKernelGGL(rt_denoise_level_kernel<2>, grid, block, 0, st, ev_in, ev_out, guide, flags, *p, width, height, step);
  else
    hipLaunchKernelGGL(rt_denoise_level_kernel<0>, grid, block, 0, st, ev_in, ev_out, guide, flags, *p, width, height, step);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rt_denoise_launch_finish(const double* ev, const double* guide, const unsigned int* flags, void* out, int out_f32,
                             long long n_pixels, void* stream) {
  if (n_pixels <= 0) return 0;
  const dim3 grid((unsigned)((n_pixels + 255) / 256)), block(256);
  if (out_f32)
    hipLaunchKernelGGL(rt_denoise_finish_kernel<float>, grid, block, 0, (hipStream_t)stream, ev, guide, flags, (float*)out,
                       n_pixels);
  else
    hipLaunchKernelGGL(rt_denoise_finish_kernel<double>, grid, block, 0, (hipStream_t)stream, ev, guide, flags,
                       (double*)out, n_pixels);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
