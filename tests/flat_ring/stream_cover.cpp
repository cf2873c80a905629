// stream_cover.cpp — TEST TOOLING (tests/test_flat_ring_host.py): the ring form's plan
// (rt_build.cpp rt_host_plan_ring) makes every item id ONE sample of a wave-owned linear stream,
// id = tile pixel x spp + k (pixel-major, sample-minor).  The kernel's own open_item (rt_trace.h,
// compiled for the host as tests/kernel_emu does) over every id of the plan: each (pixel, sample)
// of the shard exactly once, sample = sample0 + k, nothing on a padding row, nothing at all without
// depth; and a pool of consecutive ids spans no more pixels than an aggregation slot holds whenever
// the plan aggregates.
// Build: g++ -std=c++17 -ffp-contract=off stream_cover.cpp <csrc>/rt_build.cpp <csrc>/rt_bvh.cpp
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

struct Case {
  int width, height, spp, n_shards, shard, row_block, sample0, max_depth;
  bool lone;
};

int g_failures = 0;
long long g_ids = 0;

rtk64::KernelParams params(const Case& c) {
  rtk64::KernelParams P = {};
  rt_exec ex = {};
  ex.n_shards = c.n_shards;
  ex.shard = c.shard;
  ex.row_block = c.row_block;
  P.cam.width = c.width;
  P.cam.height = c.height;
  P.cam.spp = c.spp;
  P.cam.max_depth = c.max_depth;
  P.n_shards = c.n_shards;
  P.shard = c.shard;
  P.row_block = c.row_block;
  P.tile_rows = rt_host_shard_rows(c.height, &ex);
  P.sample0 = c.sample0;
  rt_host_plan_work(P, 4096, true, c.lone);
  return P;
}

void check(const Case& c) {
  rtk64::KernelParams P = params(c);
  auto bad = [&](const char* what, long long id, long long a, long long b) {
    if (++g_failures <= 10)
      std::printf("FAIL %s: %dx%d spp %d shard %d/%d row_block %d sample0 %d depth %d id %lld: %lld %lld\n", what, c.width,
                  c.height, c.spp, c.shard, c.n_shards, c.row_block, c.sample0, c.max_depth, id, a, b);
  };
  if (!rt_host_plan_ring(P, RT_VAR_FLAT, c.lone) || P.flat_ring != 1) return bad("no ring plan", -1, P.flat_ring, 0);
  const int tile_pixels = P.tile_rows * c.width;
  if (P.n_items != tile_pixels * c.spp || P.big_items != 0 || P.chunk != 1 || P.n_chunks != c.spp)
    return bad("plan members", -1, P.n_items, (long long)tile_pixels * c.spp);
  const int pool = 1 << P.pool_shift;
  if (pool < 64) bad("a refill must cover every lane of a wave", -1, pool, 64);
  std::vector<int> seen((size_t)tile_pixels * c.spp, 0);
  int pool_lo = 0, pool_hi = -1;
  for (int id = 0; id < P.n_items; ++id) {
    rtk64::ItemCtx I{-1, 0, 0, 0u, 0u};
    const bool ok = rtk64::open_item<true>(P, id, I);
    ++g_ids;
    const int tp = id / c.spp, k = id % c.spp;
    if (I.tp != tp) {
      bad("tile pixel", id, I.tp, tp);
      continue;
    }
    // a pool of consecutive ids [b, b + pool): its pixel span against the slot (rt_render_kernel.h WaveWork)
    if (id % pool == 0) pool_lo = tp;
    pool_hi = tp;
    if (P.agg_small && pool_hi - pool_lo + 1 > RT_RING_AGG_PIX) bad("pool wider than a slot", id, pool_lo, pool_hi);
    const int tr = tp / c.width, px = tp % c.width;
    const int gy = ((tr / c.row_block) * c.n_shards + c.shard) * c.row_block + tr % c.row_block;
    if (gy >= c.height || c.max_depth <= 0) {
      if (ok) bad("a sample on a padding row or without depth", id, gy, c.max_depth);
      continue;
    }
    if (!ok) bad("no sample", id, I.sample, I.s_end);
    if (I.pix != (uint32_t)(gy * c.width + px) || I.pxgy != ((uint32_t)gy << 16 | (uint32_t)px))
      bad("global pixel", id, (long long)I.pix, gy * c.width + px);
    if (I.sample != c.sample0 + k || I.s_end != I.sample + 1) bad("sample", id, I.sample, c.sample0 + k);
    ++seen[(size_t)tp * c.spp + k];
  }
  for (int tp = 0; tp < tile_pixels; ++tp) {
    const int tr = tp / c.width;
    const int gy = ((tr / c.row_block) * c.n_shards + c.shard) * c.row_block + tr % c.row_block;
    const int want = gy < c.height && c.max_depth > 0 ? 1 : 0;
    for (int k = 0; k < c.spp; ++k)
      if (seen[(size_t)tp * c.spp + k] != want) bad("coverage count", -1, tp, seen[(size_t)tp * c.spp + k]);
  }
}

}  // namespace

int main() {
  const int sizes[2][2] = {{7, 5}, {16, 9}}, spps[] = {1, 3, 63, 64, 65, 130};
  for (const auto& wh : sizes)
    for (int spp : spps)
      for (int lone = 0; lone < 2; ++lone) {
        check(Case{wh[0], wh[1], spp, 1, 0, 4, 0, 8, lone != 0});
        check(Case{wh[0], wh[1], spp, 1, 0, 4, 0, 1, lone != 0});  // every lane pops every iteration
        check(Case{wh[0], wh[1], spp, 1, 0, 4, 0, 0, lone != 0});  // black: no samples
        check(Case{wh[0], wh[1], spp, 1, 0, 4, 41, 8, lone != 0}); // a later film pass
        for (int shard = 0; shard < 3; ++shard)                    // 5 or 9 rows in 3 shards of 2-row blocks: padding rows
          check(Case{wh[0], wh[1], spp, 3, shard, 2, spp, 8, lone != 0});
      }
  // 144 random (width, height, spp, shards, row_block, sample0) tuples (a fixed LCG)
  unsigned long long s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&](int n) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (int)((s >> 33) % (unsigned)n);
  };
  for (int k = 0; k < 144; ++k) {
    Case c;
    c.width = 1 + rnd(40);
    c.height = 1 + rnd(30);
    c.spp = 1 + rnd(k % 3 == 0 ? 300 : 20);
    c.n_shards = 1 + rnd(5);
    c.shard = rnd(c.n_shards);
    c.row_block = 1 + rnd(6);
    c.sample0 = k % 2 ? rnd(1000) : 0;
    c.max_depth = 1 + rnd(8);
    c.lone = rnd(2) != 0;
    check(c);
  }
  // the classes without a ring form, an image whose samples do not fit an item id, and the knob
  {
    const Case c{7, 5, 3, 1, 0, 4, 0, 8, false};
    rtk64::KernelParams P = params(c);
    const int n_items = P.n_items;
    for (int v : {RT_VAR_FLAT | RT_VAR_MATS, RT_VAR_FLAT | RT_VAR_TEX, RT_VAR_FLAT | RT_VAR_MEDIA, RT_VAR_FLAT | RT_VAR_NOISE,
                  RT_VAR_BVH, RT_VAR_BVH_LOCKSTEP})
      if (rt_host_plan_ring(P, v, false) || P.flat_ring || P.n_items != n_items) {
        ++g_failures;
        std::printf("FAIL variant %d got the ring plan\n", v);
      }
    Case big = c;
    big.width = 40000, big.height = 30000, big.spp = 2;
    rtk64::KernelParams Q = params(big);
    if (rt_host_plan_ring(Q, RT_VAR_FLAT, false) || Q.flat_ring) ++g_failures, std::printf("FAIL 2.4e9 samples got the ring plan\n");
    setenv("RT_AMD_EXPERIMENTS", "1", 1);
    setenv("RT_AMD_FLAT_RING", "0", 1);
    if (rt_host_plan_ring(P, RT_VAR_FLAT, false) || P.flat_ring) ++g_failures, std::printf("FAIL RT_AMD_FLAT_RING=0 got the ring plan\n");
    setenv("RT_AMD_FLAT_RING", "1", 1);
    if (!rt_host_plan_ring(P, RT_VAR_FLAT, false) || !P.flat_ring) ++g_failures, std::printf("FAIL RT_AMD_FLAT_RING=1 got no ring plan\n");
  }
  if (g_failures) {
    std::printf("%d failures\n", g_failures);
    return 1;
  }
  std::printf("ok %lld ids\n", g_ids);
  return 0;
}
