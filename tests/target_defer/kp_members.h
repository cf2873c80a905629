// kp_members.h — TEST TOOLING: the members of KernelParamsT<R> in declaration order, one X(member)
// each (td_probe.cpp: their byte offsets; tests/kernel_emu/rt_emu.cpp: their values)
#pragma once
#define RT_TD_KP_MEMBERS(X)                                                                                            \
  X(nodes) X(prims) X(prim_shade) X(prim_uv) X(mats) X(texs) X(motions) X(uvframes) X(texels) X(perlin_perm)          \
  X(perlin_grad) X(flat_recs) X(boxes) X(instances) X(out) X(status) X(accum) X(nanflag) X(counter) X(chunk)          \
  X(n_chunks) X(n_items) X(big_chunk) X(n_big_chunks) X(big_items) X(small_start) X(div_big) X(div_small) X(agg_big)  \
  X(agg_small) X(pool_shift) X(stack_depth) X(lds_nodes) X(trav_exit_pct) X(leaf_exit_pct) X(n_prims) X(surface_root) \
  X(surface_prefix) X(n_media) X(n_targets) X(rem_prob) X(media) X(flat_sets) X(targets) X(cam) X(key0) X(key1)       \
  X(n_shards) X(shard) X(row_block) X(tile_rows) X(out_frame_rows) X(div_width) X(div_block) X(sample0)               \
  X(target_defer) X(target_rec) X(cam_defocus)
