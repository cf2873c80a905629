// item_cover.cpp — TEST TOOLING (tests/test_film_host.py): the work items of a launch that starts
// at sample `sample0` cover samples [sample0, sample0 + spp) of every image pixel exactly once and
// give a shard's padding rows nothing.  The kernel's own open_item (rt_trace.h, compiled for the
// host as tests/kernel_emu does) over every item id of the host's own plan (rt_host_plan_work),
// with one item size (the BVH kernels' decode) and with two (the flat kernels').
// Build: g++ -std=c++17 -ffp-contract=off item_cover.cpp <csrc>/rt_build.cpp <csrc>/rt_bvh.cpp
#define RT_HOST_EMU 1
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/rt.h"
#include "../../raytrace_amd/csrc/rt_internal.h"
#include "../../raytrace_amd/csrc/rt_kernel_class.h"
#define RT_F64 1
#include "../../raytrace_amd/csrc/rt_trace.h"

namespace rt_emu {
thread_local long long counters[4];
}

namespace {

struct Layout {
  int width, height, n_shards, shard, row_block;
};

int g_failures = 0;
bool g_expect_two = false;  // the plan under test must have big items (spp >= 17)
long long g_items = 0;

template <bool kTwoSizes>
void check(const Layout& L, int sample0, int spp, long long resident_lanes, bool lone) {
  rtk64::KernelParams P = {};
  rt_exec ex = {};
  ex.n_shards = L.n_shards;
  ex.shard = L.shard;
  ex.row_block = L.row_block;
  P.cam.width = L.width;
  P.cam.height = L.height;
  P.cam.spp = spp;
  P.cam.max_depth = 4;
  P.n_shards = L.n_shards;
  P.shard = L.shard;
  P.row_block = L.row_block;
  P.tile_rows = rt_host_shard_rows(L.height, &ex);
  P.sample0 = sample0;
  rt_host_plan_work(P, resident_lanes, kTwoSizes, lone);
  const int tile_pixels = P.tile_rows * L.width;
  std::vector<int> seen((size_t)tile_pixels * spp, 0);
  auto bad = [&](const char* what, int item, int a, int b) {
    if (++g_failures <= 10)
      std::printf("FAIL %s: two_sizes %d width %d height %d shard %d/%d sample0 %d spp %d (chunk %d big %d x %d) item %d: %d %d\n",
                  what, (int)kTwoSizes, L.width, L.height, L.shard, L.n_shards, sample0, spp, P.chunk, P.big_chunk,
                  P.n_big_chunks, item, a, b);
  };
  for (int item = 0; item < P.n_items; ++item) {
    rtk64::ItemCtx I{-1, 0, 0, 0u, 0u};
    const bool ok = rtk64::open_item<kTwoSizes>(P, item, I);
    ++g_items;
    if (I.tp < 0 || I.tp >= tile_pixels) {
      bad("tile pixel out of range", item, I.tp, tile_pixels);
      continue;
    }
    const int tr = I.tp / L.width, px = I.tp % L.width;
    const int gy = ((tr / L.row_block) * L.n_shards + L.shard) * L.row_block + tr % L.row_block;
    if (ok != (I.sample < I.s_end)) bad("return value", item, I.sample, I.s_end);
    if (gy >= L.height) {
      if (ok) bad("a padding row got samples", item, I.sample, I.s_end);
      continue;
    }
    if (I.pix != (uint32_t)(gy * L.width + px) || I.pxgy != ((uint32_t)gy << 16 | (uint32_t)px))
      bad("global pixel", item, (int)I.pix, gy * L.width + px);
    for (int s = I.sample; s < I.s_end; ++s) {
      if (s < sample0 || s >= sample0 + spp)
        bad("sample outside [sample0, sample0 + spp)", item, s, sample0);
      else
        ++seen[(size_t)I.tp * spp + (s - sample0)];
    }
  }
  for (int tp = 0; tp < tile_pixels; ++tp) {
    const int tr = tp / L.width;
    const int gy = ((tr / L.row_block) * L.n_shards + L.shard) * L.row_block + tr % L.row_block;
    for (int s = 0; s < spp; ++s) {
      const int want = gy < L.height ? 1 : 0;
      if (seen[(size_t)tp * spp + s] != want) bad("coverage count", -1, tp, seen[(size_t)tp * spp + s]);
    }
  }
  if (kTwoSizes && g_expect_two && spp >= 17 && P.n_big_chunks == 0) bad("the plan has one item size", -1, P.chunk, P.big_chunk);
}

}  // namespace

int main() {
  const Layout layouts[] = {{5, 7, 1, 0, 4}, {6, 10, 3, 1, 4}, {6, 10, 3, 2, 4}};  // the last two: padding rows
  const int sample0s[] = {0, 1, 37}, spps[] = {1, 3, 17, 64};
  // one item size: the BVH kernels' plan (its default chunk, then 16-sample items: few resident lanes)
  for (const Layout& L : layouts)
    for (int s0 : sample0s)
      for (int spp : spps) {
        check<false>(L, s0, spp, 4096, false);
        check<false>(L, s0, spp, 1, true);
        check<true>(L, s0, spp, 4, true);  // the flat kernels' decode under the planner's own choice
        check<true>(L, s0, spp, 4, false);
      }
  // two item sizes, as tests/test_gpu.py forces them: big items of at most 5 samples, a tail of 3-sample items
  g_expect_two = true;
  setenv("RT_AMD_EXPERIMENTS", "1", 1);
  setenv("RT_AMD_CHUNK", "3", 1);
  setenv("RT_AMD_BIG_CHUNK", "5", 1);
  setenv("RT_AMD_TAIL_SAMPLES", "3", 1);
  for (const Layout& L : layouts)
    for (int s0 : sample0s)
      for (int spp : spps) check<true>(L, s0, spp, 4096, true);
  if (g_failures) {
    std::printf("%d failures\n", g_failures);
    return 1;
  }
  std::printf("ok %lld items\n", g_items);
  return 0;
}
