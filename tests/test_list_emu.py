"""The per-pixel path body of the adaptive passes (raytrace_amd/csrc/rt_list.h path_sample) against the
render's lane loops, both compiled for the host (tests/list_emu, tests/kernel_emu): a pixel's samples
[0, n) through path_sample give the render's mean at n samples per pixel BIT FOR BIT, in both
precisions, for every kernel class the scenes of tests/test_render_params.py reach (flat with and
without the deferred redirect pdf, textures, a BVH with the full material set, media in the shading
phase, instancing) and for a whole frame and a shard.  And the first-hit feature body (rt_features.h)
against the path body: its albedo is the emitter twin's render at depth 1."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from raytrace_amd import denoise, scenes
from test_render_params import LAYOUTS, SCENES, scene

sys.path.insert(0, os.path.join(ROOT, "tests", "list_emu"))
import list_emu  # noqa: E402

NAMES = [n for n in SCENES if n != "cornell_192"]  # the 12-pixel scenes


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.fixture(scope="module")
def reference(emu_mod):
    """(name, precision, layout, spp) -> the lane loops' render, computed once"""
    cache = {}

    def get(name, precision, layout, spp):
        key = (name, precision, layout, spp)
        if key not in cache:
            cs, flat, seed = scene(name)
            n_shards, shard, row_block = LAYOUTS[layout]
            cache[key] = emu_mod.render(cs.replace(cs_samplesPerPixel=spp), flat, seed, n_shards, shard, row_block,
                                        precision=precision)
            cache[key].setflags(write=False)
        return cache[key]
    return get


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_uniform_counts_are_the_render(reference, name, precision, layout):
    cs, flat, seed = scene(name)
    n_shards, shard, row_block = LAYOUTS[layout]
    ref = reference(name, precision, layout, 20)
    got = list_emu.render(cs, flat, seed, 20, precision, n_shards, shard, row_block)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert np.isfinite(ref).all() and ref.max() > 0
    assert np.array_equal(bits(got), bits(ref)), f"{int((bits(got) != bits(ref)).any(-1).sum())} pixels differ"


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_checkerboard_counts_are_each_pixels_own_render(reference, name, precision, layout):
    cs, flat, seed = scene(name)
    n_shards, shard, row_block = LAYOUTS[layout]
    ref8, ref20 = reference(name, precision, layout, 8), reference(name, precision, layout, 20)
    rows, width = ref8.shape[:2]
    board = (np.add.outer(np.arange(rows), np.arange(width)) & 1).astype(bool)
    counts = np.where(board, 20, 8).astype(np.uint32)
    got = list_emu.render(cs, flat, seed, counts, precision, n_shards, shard, row_block)
    want = np.where(board[..., None], ref20, ref8)
    assert not np.array_equal(bits(ref8), bits(ref20))
    assert np.array_equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).any(-1).sum())} pixels differ"


# ---- the feature body against the path body (tests/feature_emu): both run rt_lane.h's segment 0

def _tree(name):
    cs, world, seed = SCENES[name]()
    return cs.replace(cs_aspectRatio=1.7), world, seed


TWIN_SCENES = {name: (lambda name=name: _tree(name)) for name in ["cornell", "cornell_noisy", "readme", "demo1", "pawn_fog"]}
TWIN_SCENES.update({name: (lambda name=name: getattr(scenes, name)(width=12, spp=4))
                    for name in ["instance_gallery", "noise_test", "box_gallery", "bunny_cornell"]})


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", list(TWIN_SCENES))
def test_feature_albedo_is_the_emitter_twin_at_depth_1(name, precision, layout):
    """The feature body's albedo at 4 samples is the path body's 4-sample render of the emitter twin
    (every material replaced by an emitter of its albedo) at recursion depth 1, BIT FOR BIT: the same
    primary rays, first events (surface, medium, instance), uvs and textures, so segment 0 of the two
    bodies is one function — media and instancing included."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "feature_emu"))
    import feature_emu
    cs, world, seed = TWIN_SCENES[name]()
    n_shards, shard, row_block = LAYOUTS[layout]
    words = feature_emu.features(cs, world, seed, 4, precision, n_shards, shard, row_block)
    dtype = np.float64 if precision == "f64" else np.float32
    albedo = denoise.features_from_words(words, 4)["albedo"].astype(dtype)
    twin = list_emu.render(cs.replace(cs_maxRecursionDepth=1), denoise.emitter_twin(world), seed, 4, precision, n_shards,
                           shard, row_block)
    for img in (albedo, twin):
        assert np.isfinite(img).all() and img.any() and len(np.unique(img)) > 1
    assert albedo.shape == twin.shape and albedo.dtype == twin.dtype
    assert np.array_equal(bits(albedo), bits(twin)), f"{int((bits(albedo) != bits(twin)).any(-1).sum())} pixels differ"
