"""The per-pixel path body of the adaptive passes (raytrace_amd/csrc/rt_list.h path_sample) against the
render's lane loops, both compiled for the host (tests/list_emu, tests/kernel_emu): a pixel's samples
[0, n) through path_sample give the render's mean at n samples per pixel BIT FOR BIT, in both
precisions, for every kernel class the scenes of tests/test_render_params.py reach (flat with and
without the deferred redirect pdf, textures, a BVH with the full material set, media in the shading
phase, instancing) and for a whole frame and a shard."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
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
