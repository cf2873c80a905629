// rt_kernel_class.h — the one table from a variant code (rt_internal.h RT_VAR_*) to the render
// kernel's class and its launch shape: occupancy floor, workgroup size, LDS layout, slot geometry,
// translation unit.  The kernel (rt_render_kernel.h) applies these functions to its own template
// arguments and the host to rt_class_of(f64, variant).  Plain C++17: the host emulator includes it too.
#pragma once
#include <stddef.h>
#include <type_traits>
#include "rt_internal.h"

// The seven template parameters of rt_render_kernel, in that order.
//  var: RT_VAR_FLAT: every primitive set is one flat leaf, its records read with wave-uniform
//    addresses (scalar loads, scalar-cache resident); lockstep loop.  RT_VAR_BVH / _LOCKSTEP: BVH
//    scenes; dynamic LDS = the lanes' traversal stacks [depth][lane], then the top staged nodes.
//    The default decouples traversal from shading per lane (rt_trace.h lane_loop_bvh); the lockstep
//    loop runs every query of a segment with the whole wave (experiments; bit-identical images).
//  tex: 0 constant textures, 1 some material reads a non-constant texture, 2 noise textures too
//  media: 0 none; 1 the media queries chained in the traversal loop; 2 the media events in the
//    shading phase (RT_VAR_MEDIA_LATE; rt_trace.h media_events_late)
//  mats: materials beyond lightSource / pitchBlack / lambertian;  inst: two-level instancing
//  leaf: the leaf class (0 generic, 1 triangles, 2 spheres; rt_trace.h trav_round)
//  narrow: the 1024-lane class at 512 lanes, for a scene whose stacks do not fit one 1024-lane
//    workgroup's LDS (RT_VAR_NARROW)
// Non-constant textures, noise textures, media and the further materials are compiled only into
// the instantiations of scenes that use them (inlined everywhere they raise the register
// allocation of every scene's kernel: the Cornell box is 4.8 % faster without the unused media code)
struct KernelClass {
  int var, tex, media; bool mats, inst; int leaf; bool narrow;
};

// Register budget: occupancy floor (waves per SIMD), per kernel class and precision — the knobs
// below and rt_class_waves, each entry measured against its neighbours (DESIGN_HISTORY
// §1a, §4).  Since round 6 every entry also keeps its class free of VGPR spills (tools/spill_gate.py
// fails the build otherwise): the binary64 full-material BVH classes, the binary64 instanced
// full-material class, the FP32 full-material generic-leaf class and the FP32 instanced media-chain
// classes each run one wave less than their round-5 entries.
#ifndef RT_WAVES_FLAT
#define RT_WAVES_FLAT 7
#endif
#ifndef RT_WAVES_FLAT_NOISE
#define RT_WAVES_FLAT_NOISE 5
#endif
#ifndef RT_WAVES_BVH
#define RT_WAVES_BVH 5
#endif
// knobs for the lightest instantiations (constant textures; BVH: no media).  The flat kernel with
// constant textures runs 8 waves since round 4: with the kernel arguments re-read per iteration
// (rt_trace.h RT_KARGS) and shade's unconditional ray update it needs 64 VGPRs without spills
// (Cornell FP32 3.162 -> 3.075 ms against 7 waves, profiles/r4/unc_ab); round 3's 8-wave build
// spilled 6 VGPRs and gained nothing
#ifndef RT_WAVES_FLAT_TEX0
#define RT_WAVES_FLAT_TEX0 8
#endif
#ifndef RT_WAVES_BVH_LITE
#define RT_WAVES_BVH_LITE 6  // 80 VGPRs once the item sums moved to LDS: bunny-Cornell 107.2 -> 100.6 ms at 6 (profiles/r3/slim)
#endif
// binary64: every real is a register pair, so the same code needs about twice the VGPRs; the
// lightest instantiations (constant textures, no media, no materials beyond the diffuse ones)
// keep more waves
#ifndef RT_WAVES64_FLAT_LITE
#define RT_WAVES64_FLAT_LITE 5  // 96 VGPRs, no spills (round 4): Cornell binary64 5.442 -> 5.315 ms against 4
#endif
#ifndef RT_WAVES64_FLAT
#define RT_WAVES64_FLAT 4  // 100 VGPRs without MachineLICM (round 4: 2, with it 195 VGPRs; readme 0.65 -> 0.46 ms)
#endif
#ifndef RT_WAVES64_BVH_LITE
#define RT_WAVES64_BVH_LITE 4  // 163 ms bunny-Cornell vs 180 at 3 once the BVH nodes were tested in FP32 (profiles/r2/waves64)
#endif
#ifndef RT_WAVES64_BVH
#define RT_WAVES64_BVH 4  // demo1 69.9 ms vs 76.6 at 3 (profiles/r2/waves64); textured scenes, instances
#endif
#ifndef RT_WAVES64_BVH_MATS
// constant textures, the full material set (demo1).  Round 5 ran it at 5 (57.0 -> 56.4 ms), where
// every leaf class of it spilled 4-14 VGPRs; round 6 keeps every dispatchable kernel spill-free
// (tools/spill_gate.py), so 4
#define RT_WAVES64_BVH_MATS 4
#endif
#ifndef RT_WAVES64_BVH_MEDIA
#define RT_WAVES64_BVH_MEDIA 3  // the media chain kernels (pawn+fog 641 ms at 3, 883 at 4), instanced with textures / media
#endif
#ifndef RT_WAVES64_BVH_INST_MATS
#define RT_WAVES64_BVH_INST_MATS 3  // instances with the full material set: 1 VGPR spilled at 4
#endif
#ifndef RT_WAVES64_BVH_MEDIA_LATE
#define RT_WAVES64_BVH_MEDIA_LATE 4  // media events in the shading phase (media 2): pawn+fog 508 -> 476 ms
#endif
#ifndef RT_WAVES_BVH_MEDIA_LATE
// FP32 pawn+fog: 310.7 -> 302 ms at 7 against 5 (profiles/r5/licm); 6, in two 768-lane workgroups
// per CU, stages 520 of its 631 surface nodes per copy against 120 at 7: 302.7 -> 276.1 ms (4:
// 318, 8: 297; profiles/r5/occ)
#define RT_WAVES_BVH_MEDIA_LATE 6
#endif
#ifndef RT_WAVES_BVH_MATS
#define RT_WAVES_BVH_MATS 8  // FP32 BVH, constant textures, the full material set, no media (demo1 39.7 -> 39.25 ms)
#endif
#ifndef RT_WAVES_BVH_MATS_GENERIC
#define RT_WAVES_BVH_MATS_GENERIC 7  // ... with generic leaves: 4 VGPRs spilled at 8
#endif
#ifndef RT_WAVES_BVH_INST_CHAIN
#define RT_WAVES_BVH_INST_CHAIN 4  // FP32 instances with the media query chain: 2-25 VGPRs spilled at 5
#endif
constexpr int rt_class_waves(bool f64, KernelClass c) {
  const bool tex0 = c.tex == 0;
  if (f64) {
    if (c.var == RT_VAR_FLAT) return tex0 && !c.media && !c.mats ? RT_WAVES64_FLAT_LITE : RT_WAVES64_FLAT;
    if (c.inst && (!tex0 || c.media)) return RT_WAVES64_BVH_MEDIA;
    if (c.inst && c.mats) return RT_WAVES64_BVH_INST_MATS;
    if (c.media) return c.media == 2 ? RT_WAVES64_BVH_MEDIA_LATE : RT_WAVES64_BVH_MEDIA;
    if (tex0 && !c.mats) return RT_WAVES64_BVH_LITE;
    return tex0 && !c.inst ? RT_WAVES64_BVH_MATS : RT_WAVES64_BVH;
  }
  if (c.var == RT_VAR_FLAT) return c.tex == 2 ? RT_WAVES_FLAT_NOISE : tex0 ? RT_WAVES_FLAT_TEX0 : RT_WAVES_FLAT;
  if (c.media == 2) return c.inst ? RT_WAVES_BVH : RT_WAVES_BVH_MEDIA_LATE;
  if (c.media == 1 && c.inst) return RT_WAVES_BVH_INST_CHAIN;
  if (tex0 && !c.media && c.mats && !c.inst) return c.leaf == 0 ? RT_WAVES_BVH_MATS_GENERIC : RT_WAVES_BVH_MATS;
  return tex0 && !c.media ? RT_WAVES_BVH_LITE : RT_WAVES_BVH;
}

// BVH workgroup size of a kernel class: each workgroup stages its own LDS copy of the top BVH
// nodes, so the fewer workgroups share a CU the more nodes each copy holds (pawn+fog and demo1
// gain 6-13 % from staging).  The largest workgroup whose waves split evenly over the
// CU's 4 SIMDs at the kernel's occupancy W (waves per SIMD): W = 3 -> 768 threads (one per CU),
// 4 -> 1024 (one), 6 -> 768 (two), 8 -> 1024 (two); W = 5 / 7 keep 256.  Round 5 (profiles/r5/
// bigwg): W = 4 at 1024 instead of 512 stages all of pawn+fog's surface nodes (binary64 476.5 ->
// 428.1 ms; bunny even); W = 8 at 1024 instead of 256, FP32 demo1 39.35 -> 37.7 ms; 640 / 896
// threads at W = 5 / 7 do not split evenly (10 / 14 waves per workgroup over 4 SIMDs): demo1
// binary64 +36 %, pawn+fog FP32 +22 %, one workgroup per CU fits.  RT_BIG_WG=0: 256 everywhere.
#ifndef RT_BIG_WG
#define RT_BIG_WG 1
#endif
constexpr int rt_class_block_wide(bool f64, KernelClass c) {
  if (c.var == RT_VAR_FLAT) return RT_BLOCK;
  const int w = rt_class_waves(f64, c);
  return RT_BIG_WG && (w == 3 || w == 6) ? 768 : RT_BIG_WG && (w == 4 || w == 8) ? 1024 : RT_BLOCK_BVH;
}
// the classes with a 512-lane twin (narrow: a deep BVH's render), and the launch bound / stack stride
constexpr bool rt_class_has_twin(bool f64, KernelClass c) { return rt_class_block_wide(f64, c) == 1024; }
constexpr int rt_class_block(bool f64, KernelClass c) { return c.narrow ? 512 : rt_class_block_wide(f64, c); }

// Where the lanes' item sums live (rt_trace.h Acc / AccLds).  Same-box A/B against registers
// (profiles/r3/slim): in LDS they free the VGPRs that let the FP32 BVH kernel without media run 6
// waves per SIMD (bunny-Cornell 107.2 -> 100.6 ms) and trim the binary64 BVH kernels (bunny 162.7
// -> 157.6, pawn+fog 643 -> 631); the flat kernels, which read their scene with scalar loads that
// share the LDS return counter, lose 2-3.5 % (Cornell f64 6.12 -> 6.33) and the FP32 media kernel
// 2.8 %, so those keep registers.  -DRT_ACC_IN_LDS=0 keeps registers everywhere.
#ifndef RT_ACC_IN_LDS
#define RT_ACC_IN_LDS 1
#endif
constexpr bool rt_class_acc_lds(bool f64, KernelClass c) {
  return RT_ACC_IN_LDS && c.var != RT_VAR_FLAT && (f64 || !c.media);
}

// commit-aggregation slots per wave and pixels per slot of a kernel class (rt_internal.h RT_AGG_*;
// rt_render_kernel.h WaveWork).  The wide slots: every binary64 flat class, and the FP32 flat
// classes without media
constexpr bool rt_class_agg_wide(bool f64, KernelClass c) { return f64 || c.media == 0; }
constexpr int rt_class_agg_slots(bool f64, KernelClass c) {
  return c.var != RT_VAR_FLAT ? RT_AGG_SLOTS_BVH : rt_class_agg_wide(f64, c) ? RT_AGG_SLOTS_FLAT_F64 : RT_AGG_SLOTS_FLAT;
}
constexpr int rt_class_agg_pix(bool f64, KernelClass c) {
  return c.var != RT_VAR_FLAT ? RT_AGG_PIX_BVH : rt_class_agg_wide(f64, c) ? RT_AGG_PIX_FLAT_F64 : RT_AGG_PIX_FLAT;
}
static_assert(RT_AGG_SLOTS_FLAT < 255 && RT_AGG_SLOTS_FLAT_F64 < 255 && RT_AGG_SLOTS_BVH < 255,
              "slot + 1 must fit the 8 bits of rt_trace.h ItemCtx::tp");
constexpr int rt_acc_words(bool f64) { return f64 ? RT_ACC_WORDS(double) : RT_ACC_WORDS(float); }
// LDS of the aggregation slots per wave: slots x pix x RT_ACC_WORDS 64-bit words + 2 header ints per slot
constexpr int rt_class_agg_bytes(bool f64, KernelClass c) {
  return rt_class_agg_slots(f64, c) * (rt_class_agg_pix(f64, c) * rt_acc_words(f64) * 8 + 2 * 4);
}
// LDS besides the stacks and the staged nodes: the lanes' item sums and the aggregation slots
constexpr size_t rt_class_fixed_lds(bool f64, KernelClass c) {
  const size_t block = (size_t)rt_class_block(f64, c);
  return (rt_class_acc_lds(f64, c) ? rt_acc_words(f64) * 8 * block : 0) + rt_class_agg_bytes(f64, c) * (block / 64);
}
// ... and all of it: [stack_depth + 1][block] stack words and lds_nodes staged nodes of 64 B (BVH)
constexpr size_t rt_class_lds_bytes(bool f64, KernelClass c, int stack_depth, int lds_nodes) {
  return rt_class_fixed_lds(f64, c) +
         (c.var == RT_VAR_FLAT ? 0 : (size_t)(stack_depth + 1) * rt_class_block(f64, c) * sizeof(int) + (size_t)lds_nodes * 64);
}

// The ring form of the flat lane loop (rt_render_kernel.h rt_render_kernel_ring, rt_trace.h
// lane_loop_flat_ring): one class has it, in both precisions — flat, constant textures, the diffuse
// materials, no media (the Cornell box) — as a kernel of its own beside the class's legacy one, at
// the class's occupancy.  LDS of its one-wave workgroup: the ring's 64 rays (6 reals and 4 words
// each; 7 and 5 where the refill traces the camera segments, rt_ring_primary), then the aggregation
// slots (rt_internal.h RT_RING_*); never more than the legacy kernel's.
constexpr KernelClass rt_ring_class() { return KernelClass{RT_VAR_FLAT, 0, 0, false, false, 0, false}; }
constexpr bool rt_class_has_ring(KernelClass c) {
  return c.var == RT_VAR_FLAT && c.tex == 0 && c.media == 0 && !c.mats && !c.inst;
}
constexpr int rt_ring_agg_slots(bool f64) { return f64 ? RT_RING_AGG_SLOTS_F64 : RT_RING_AGG_SLOTS_F32; }
constexpr int rt_ring_agg_bytes(bool f64) { return rt_ring_agg_slots(f64) * (RT_RING_AGG_PIX * rt_acc_words(f64) * 8 + 2 * 4); }
// (an entry of the form that traces the camera segments at the refill, rt_internal.h
// RT_RING_PRIMARY_*: one more real, the scatter's weight, and one more word, leaf left and primitive)
constexpr bool rt_ring_primary(bool f64) { return f64 ? RT_RING_PRIMARY_F64 != 0 : RT_RING_PRIMARY_F32 != 0; }
constexpr int rt_ring_reals(bool f64) { return rt_ring_primary(f64) ? 7 : 6; }
constexpr int rt_ring_words(bool f64) { return rt_ring_primary(f64) ? 5 : 4; }
constexpr int rt_ring_ray_bytes(bool f64) { return RT_RING_LANES * (rt_ring_reals(f64) * (f64 ? 8 : 4) + rt_ring_words(f64) * 4); }
constexpr size_t rt_ring_lds_bytes(bool f64) { return (size_t)rt_ring_ray_bytes(f64) + rt_ring_agg_bytes(f64); }
static_assert(RT_BLOCK == RT_RING_LANES, "the ring belongs to a one-wave workgroup");
static_assert(rt_ring_lds_bytes(false) <= rt_class_fixed_lds(false, rt_ring_class()) &&
                  rt_ring_lds_bytes(true) <= rt_class_fixed_lds(true, rt_ring_class()),
              "the ring form's LDS must not exceed the legacy kernel's (same workgroups per CU)");

// Kernels built without MachineLICM (rt_kernel_nl.hip / rt_kernel64_nl.hip, compiled with
// -mllvm -disable-machine-licm): the pass hoists the loop's binary64 constants (log, sincos and
// texture polynomial coefficients, ...) out of the persistent lane loop into ~20-90 VGPRs, so the
// heavier kernels sat at 2-3 waves or spilled (readme binary64 195 VGPRs -> 100: 0.65 -> 0.46 ms;
// pawn+fog binary64 107 instead of 128 + spills).  The lightest kernels keep it: the Cornell box
// (flat, constant textures, the diffuse materials) is 1.3 % slower without it and the bunny even
// (profiles/r5/licm).  Every instantiation lives in exactly one of the two translation units.
#ifndef RT_NOLICM_FLAT_LITE
#define RT_NOLICM_FLAT_LITE 0  // (experiments: the binary64 Cornell kernel without MachineLICM too)
#endif
#ifndef RT_NOLICM_BVH_LITE
#define RT_NOLICM_BVH_LITE 0  // (experiments: the bunny class without MachineLICM too)
#endif
constexpr bool rt_class_nolicm(bool f64, KernelClass c) {
  const bool heavy = c.tex != 0 || c.media != 0 || c.mats;
  return c.var == RT_VAR_FLAT ? f64 && (RT_NOLICM_FLAT_LITE || heavy) : RT_NOLICM_BVH_LITE || heavy || c.inst;
}

// Which classes exist.  The media events run in the shading phase (media 2) in the decoupled
// kernel only; one-class leaves: the decoupled kernel without instances, and with media triangle
// leaves with constant textures only (pawn+fog; -DRT_LEAF_MEDIA=0: none)
#ifndef RT_LEAF_MEDIA
#define RT_LEAF_MEDIA 1
#endif
constexpr bool rt_media_late_compiled(int var) { return var == RT_VAR_BVH; }
constexpr bool rt_leaf_compiled(int var, int tex, int media, bool inst, int leaf) {
  if (leaf == 0) return true;
  if (var != RT_VAR_BVH || inst) return false;
  return media ? RT_LEAF_MEDIA && tex == 0 && leaf == 1 : true;
}
constexpr bool rt_class_compiled(bool f64, KernelClass c) {
  if (c.var == RT_VAR_BVH_LOCKSTEP && !RT_LOCKSTEP_KERNELS) return false;
  if (c.var != RT_VAR_BVH && c.inst) return false;
  if (c.media == 2 && !rt_media_late_compiled(c.var)) return false;
  return rt_leaf_compiled(c.var, c.tex, c.media, c.inst, c.leaf) && (!c.narrow || rt_class_has_twin(f64, c));
}

// The class of a variant code (base variant | RT_VAR_* flags), the only decode of the flags: the
// kernel the dispatch returns and the shape the host launches it with.  Two-level instancing is
// compiled into the decoupled BVH kernel only, and the lockstep base runs the decoupled kernel
// where the lockstep kernels are not built (RT_LOCKSTEP_KERNELS); the media mode and the leaf
// class follow the code's own base, and a flag whose class does not exist keeps the generic one.
constexpr KernelClass rt_class_of(bool f64, int variant) {
  const int base = variant & RT_VAR_BASE;
  KernelClass c{};
  c.inst = (variant & RT_VAR_INST) != 0;
  c.var = c.inst || (base == RT_VAR_BVH_LOCKSTEP && !RT_LOCKSTEP_KERNELS) ? RT_VAR_BVH : base;
  c.tex = (variant & RT_VAR_NOISE) ? 2 : (variant & RT_VAR_TEX) ? 1 : 0;
  c.media = !(variant & RT_VAR_MEDIA) ? 0 : (variant & RT_VAR_MEDIA_LATE) && rt_media_late_compiled(base) ? 2 : 1;
  c.mats = (variant & RT_VAR_MATS) != 0;
  const int leaf = (variant & RT_VAR_LEAF_TRI) ? 1 : (variant & RT_VAR_LEAF_SPHERE) ? 2 : 0;
  c.leaf = rt_leaf_compiled(base, c.tex, c.media, c.inst, leaf) ? leaf : 0;
  c.narrow = (variant & RT_VAR_NARROW) && rt_class_has_twin(f64, c);
  return c;
}

// p(f64, class of every variant code: 0..2047 whose base is a variant) in both precisions
constexpr bool rt_every_class(bool (*p)(bool, KernelClass)) {
  for (int v = 0; v < 2 * RT_VAR_NARROW; ++v)
    if ((v & RT_VAR_BASE) != RT_VAR_BASE && !(p(false, rt_class_of(false, v)) && p(true, rt_class_of(true, v))))
      return false;
  return true;
}
static_assert(rt_every_class(rt_class_compiled), "rt_class_of names a class that is not compiled");
// rt_build.cpp rt_host_variant sends a BVH deeper than RT_WIDE_STACK_ROWS stack rows to the narrow
// twin: that many rows fit one 1024-lane workgroup beside its item sums and slots (binary64: 48 +
// 15.5 B per lane) in the CU's 160 KB of LDS less the 1 KB granule rt_api.hip ensure_precision
// keeps free; the FP32 classes take the same rule
constexpr bool rt_wide_rows_fit(bool f64, KernelClass c) {
  return !rt_class_has_twin(f64, c) || rt_class_lds_bytes(f64, c, RT_WIDE_STACK_ROWS - 1, 0) <= 163840 - 1024;
}
static_assert(rt_every_class(rt_wide_rows_fit), "RT_WIDE_STACK_ROWS stack rows must fit a 1024-lane workgroup's LDS");

// rt_lift<N>(v, f): f(std::integral_constant<int, v>) for a run-time v in [0, N)
template <int N, class F>
auto rt_lift(int v, F f) {
  if constexpr (N == 1) return f(std::integral_constant<int, 0>{});
  else if (v >= N - 1) return f(std::integral_constant<int, N - 1>{});
  else return rt_lift<N - 1>(v, f);
}
// f(seven integral constants: the fields of c), the one dispatch from a run-time class to template
// arguments: `constexpr KernelClass k{decltype(args)::value...}` inside f
template <int I = 0, class F, class... K>
auto rt_with_class(KernelClass c, F f, K... k) {
  constexpr int kRange[7] = {3, 3, 3, 2, 2, 3, 2};
  const int field[7] = {c.var, c.tex, c.media, c.mats, c.inst, c.leaf, c.narrow};
  if constexpr (I == 7) return f(k...);
  else return rt_lift<kRange[I]>(field[I], [&](auto x) { return rt_with_class<I + 1>(c, f, k..., x); });
}
