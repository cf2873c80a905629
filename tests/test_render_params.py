"""The kernel arguments of a render pinned member by member (no GPU needed).

tests/golden/render_params.json holds, for every case below, each member of the KernelParams the
host emulator's render() hands the lane loop (tests/kernel_emu rt_emu_render_params): numbers exactly,
pointers as null or not.  It was recorded while the emulator still filled the struct by hand, with
target_defer / target_rec as its lane loop then matched them (tests/golden/make_render_params.py), and
is never regenerated from the code under test: the one fill function the library and the emulator
share (rt_build.cpp rt_host_render_params) has to reproduce every member.

Every scene is rendered 12 pixels wide and 7 rows high at 20 samples, once whole and once as shard
1 of 3 in row blocks of 4 (rows 4-6 and one padding row).  With the emulator's 4096 resident lanes
an image of 84 pixels gets one item size; "cornell_192" (192 pixels wide) is there for the plan with two."""
import functools
import json
import os

import pytest

import raytrace_amd as R
from raytrace_amd import scenes
from raytrace_amd.camera import image_height
from raytrace_amd.scene import FlatScene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_params.json")


def _instanced():
    """a ground sphere and one six-sphere object placed twice (two-level traversal)"""
    grey = R.lambertian(R.constantTexture(0.5))
    obj = R.group([grey << R.sphere((i % 3, i // 3, 0), 0.3) for i in range(6)])
    world = R.group([grey << R.sphere((0, -1000, 0), 990),
                     R.mirror(R.constantTexture(0.9)) << R.transform(R.translate((10, 0, 0)) @ R.rotateY(0.5), obj),
                     R.transform(R.translate((-10, 0, 2)), obj)])
    return scenes.readme_scene(width=12, spp=20)[0], R.flatten(world, instance_min=4), R.mkStdGen(3)


SCENES = {
    "cornell": lambda: scenes.cornell_box(width=12, spp=20),                      # its one target matches
    "cornell_noisy": lambda: scenes.cornell_box(width=12, spp=20, redirect=False),  # no redirect target
    "readme": lambda: scenes.readme_scene(width=12, spp=20),
    "demo1": lambda: scenes.demo1(width=12, spp=20),                             # a BVH, no media
    "pawn_fog": lambda: scenes.pawn_fog(width=12, spp=20),                       # media in the shading phase
    "instanced": _instanced,
    "cornell_192": lambda: scenes.cornell_box(width=192, spp=20),                  # big and small items
}
LAYOUTS = {"whole": (1, 0, 4), "shard1of3": (3, 1, 4)}
KNOBS = ["RT_AMD_TARGET_DEFER=0", "RT_AMD_VARIANT=0"]  # (on the Cornell box: neither defers)


@functools.lru_cache(maxsize=None)
def scene(name):
    cs, world, seed = SCENES[name]()
    cs = cs.replace(cs_aspectRatio=1.7)
    assert image_height(cs) == 7 or name == "cornell_192"
    return cs, world if isinstance(world, FlatScene) else R.flatten(world), seed


def cases():
    """case id -> (scene, precision, layout, knob or None)"""
    out = {}
    for name in SCENES:
        for precision in ("f64", "f32"):
            for layout in (["whole"] if name == "cornell_192" else LAYOUTS):
                out[f"{name}-{precision}-{layout}"] = (name, precision, layout, None)
                if name == "cornell":
                    for k in KNOBS:
                        out[f"{name}-{precision}-{layout}+{k}"] = (name, precision, layout, k)
    return out


def params(emu, name, precision, layout):
    cs, flat, seed = scene(name)
    n_shards, shard, row_block = LAYOUTS[layout]
    return emu.render_params(cs, flat, seed, n_shards, shard, row_block, precision=precision)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", list(cases()))
def test_render_params_are_the_recorded_ones(emu_mod, request, golden, case):
    name, precision, layout, knob = cases()[case]
    if knob:
        request.getfixturevalue("knobs").setenv(*knob.split("="))
    got, want = params(emu_mod, name, precision, layout), golden[case]
    assert list(got) == list(want), "members in declaration order"
    # (repr: -0.0 is not 0.0)
    differ = [k for k in want if [repr(x) for x in got[k]] != [repr(x) for x in want[k]]]
    assert not differ, {k: (got[k], want[k]) for k in differ}


def test_recorded_cases_reach_their_paths(golden):
    assert set(golden) == set(cases())
    one = lambda case, k: golden[case][k][0]
    for p in ("f64", "f32"):
        assert (one(f"cornell-{p}-whole", "target_defer"), one(f"cornell-{p}-whole", "target_rec") >= 0) == (1, True)
        for other in ("cornell_noisy", "readme", "demo1", "pawn_fog", "instanced"):
            assert (one(f"{other}-{p}-whole", "target_defer"), one(f"{other}-{p}-whole", "target_rec")) == (0, -1)
        for k in KNOBS:
            for layout in LAYOUTS:
                assert one(f"cornell-{p}-{layout}+{k}", "target_defer") == 0
        assert one(f"cornell-{p}-whole", "n_big_chunks") == 0 and one(f"cornell_192-{p}-whole", "n_big_chunks") > 0
        assert one(f"cornell-{p}-shard1of3", "tile_rows") == 4 and one(f"cornell-{p}-whole", "tile_rows") == 7
        assert one(f"demo1-{p}-whole", "surface_prefix") == 1 and one(f"demo1-{p}-whole", "n_media") == 0
        assert one(f"pawn_fog-{p}-whole", "n_media") == 2 and one(f"instanced-{p}-whole", "instances") == 1
