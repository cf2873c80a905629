"""The host scene builder (rt_build.cpp rt_host_build_scene) pinned byte for byte (no GPU needed).

tests/golden/host_scene.json holds, for every scene below, one (length, FNV-1a) pair per array of
HostScene in both precisions (tests/kernel_emu rt_emu_scene_digest), and for every single-defect
scene the return code and message.  It was recorded from the builder as it stood before it was split
into stages (tests/golden/make_host_scene.py) and is never regenerated from the code under test: a
restructured builder has to reproduce every record, and the first error it reports for a scene,
exactly."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import raytrace_amd as R
from raytrace_amd import _lib, scenes
from raytrace_amd import scene as S
from raytrace_amd.perlin import perlin_record

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_scene.json")

PROJECT = ["cornell_box", "readme_scene", "demo1", "demo2", "bunny_cornell", "pawn_test", "pawn_fog",
           "bunny_instances", "instance_gallery", "noise_test", "box_gallery"]
KNOB_SCENES = ["bunny_cornell", "pawn_fog"]
KNOBS = ["RT_AMD_NO_PREFIX=1", "RT_AMD_NO_BOX=1", "RT_AMD_NO_ALIAS=1", "RT_AMD_LEAF_MAX=7", "RT_AMD_PREFIX_AREA=0.9",
         "RT_AMD_PREFIX_SHRINK=0.5", "RT_AMD_LEAF_EXIT_PCT=90", "RT_AMD_TRAV_PCT=10"]


@functools.lru_cache(maxsize=None)
def project_scene(name):
    # the host build does not depend on the image size
    return R.flatten(getattr(scenes, name)(width=8, spp=1)[1])


# ------------------------------------------------------------------ hand-made scenes
def _grey(v=0.5):
    return R.lambertian(R.constantTexture(v))


def _spheres(n, r=0.3):
    """n small spheres on a 7 x 7 x k lattice"""
    return [_grey(0.1 + 0.01 * i) << R.sphere((i % 7, (i // 7) % 7, i // 49), r) for i in range(n)]


def _empty():
    z = np.zeros
    return S.FlatScene(z(0, S.PRIM_DTYPE), z(0, S.MEDIUM_DTYPE), z(0, S.MATERIAL_DTYPE), z(0, S.TEXTURE_DTYPE),
                       z(0, S.MOTION_DTYPE), z(0, S.UVFRAME_DTYPE), 0)


def _wall_and(n):
    """n surface primitives, one of them a wall quad far larger than the rest"""
    return R.group([_grey() << R.parallelogram((-50, -50, -5), (100, 0, 0), (0, 100, 0))] + _spheres(n - 1))


def _moving_quad():
    return R.group([
        _grey() << R.sphere((0, 0, 0), 1),
        _grey() << R.parallelogram((2, 0, 0), (1, 0, 0), (0, 1, 0)),
        _grey() << R.moving((0, 0, 0), (0, 0.5, 0), R.parallelogram((4, 0, 0), (1, 0, 0), (0, 1, 0))),
        _grey() << R.triangle(((6, 0, 0), (0, 0)), ((7, 0, 0), (1, 0)), ((6, 1, 0), (0, 1))),
    ])


def _degenerate():
    # u parallel to v: the frame is NaN and the stored normal zero (never hit)
    return R.group([_grey() << R.parallelogram((0, 0, 0), (1, 2, 3), (2, 4, 6)), _grey() << R.sphere((5, 0, 0), 1)])


def _split_cuboid():
    """A cuboid whose six faces reach the surface prefix (a BVH scene), three of them 40 depth-first
    leaves after the others: the 5-bit span filter refuses the box group."""
    faces = [_grey() << f for f in R.cuboid(R.fromCorners((-20, -20, -20), (30, 30, 30))).children]
    return R.group(faces[:3] + _spheres(40) + faces[3:] + _spheres(10, r=0.2))


def _fog_cloud():
    cloud = R.bvhTree(_spheres(40))
    fog = R.isotropic(R.constantTexture(1)) << R.constantMedium(0.05, R.sphere((3, 3, 0), 30))
    return R.group([cloud, fog])


def _instanced_twice():
    obj = R.group(_spheres(6))  # the leaves carry their own materials
    world = R.group([_grey() << R.sphere((0, -1000, 0), 990),
                     R.mirror(R.constantTexture(0.9)) << R.transform(R.translate((10, 0, 0)) @ R.rotateY(0.5), obj),
                     R.transform(R.translate((-10, 0, 2)), obj)])
    return R.flatten(world, instance_min=4)


HAND_MADE = {
    "empty": _empty,
    "spheres_32": lambda: R.group(_spheres(32)),  # RT_FLAT_MAX: one flat leaf
    "spheres_33": lambda: R.group(_spheres(33)),  # a BVH
    "wall_48": lambda: _wall_and(48),             # RT_FLAT_MAX + RT_PREFIX_MAX: no prefix
    "wall_49": lambda: _wall_and(49),             # the prefix takes the wall
    "moving_quad": _moving_quad,
    "degenerate_quad": _degenerate,
    "split_cuboid": _split_cuboid,
    "fog_cloud": _fog_cloud,
    "instanced_twice": _instanced_twice,
}
# what each hand-made scene is there to reach, in emu.scene_info's terms
HAND_MADE_INFO = {
    "empty": dict(n_prims=0, n_nodes=0, flat=1),
    "spheres_32": dict(n_prims=32, n_nodes=0, flat=1),
    "spheres_33": dict(n_prims=33, flat=0, prefix=0, leaf_kind=2),
    "wall_48": dict(n_prims=48, flat=0, prefix=0),
    "wall_49": dict(n_prims=49, flat=0, prefix=1),
    "moving_quad": dict(n_prims=4, flat=1),
    "degenerate_quad": dict(n_prims=2, flat=1),
    "split_cuboid": dict(n_prims=56, flat=0, prefix=6, boxes=0),
    "fog_cloud": dict(n_prims=41, flat=0, leaf_kind=2),
    "instanced_twice": dict(n_prims=7, flat=0),
}


def digest_cases():
    """(case id, scene thunk, knob or None) of every recorded digest"""
    out = [(n, functools.partial(project_scene, n), None) for n in PROJECT]
    out += [(n, fn, None) for n, fn in HAND_MADE.items()]
    out += [(f"{n}+{k}", functools.partial(project_scene, n), k) for n in KNOB_SCENES for k in KNOBS]
    return out


# ------------------------------------------------------------------ single-defect scenes
def small_cornell():
    return R.flatten(scenes.cornell_box(width=8, spp=1)[1])


def _set(table, i, field, value, sub=None):
    def f(flat):
        rec = getattr(flat, table)
        if sub is None:
            rec[field][i] = value
        else:
            rec[field][i][sub] = value
    return f


def _media(density, material):
    def f(flat):
        flat.media = np.zeros(1, S.MEDIUM_DTYPE)
        flat.media[0] = (density, material, 99)
    return f


def _noise(perm_entry=None):
    def f(flat):
        flat.textures["kind"][0] = 3
        if perm_entry is not None:
            flat.perlin = perlin_record().copy()
            flat.perlin[0]["perm"][1][5] = perm_entry
    return f


def _image_past_texels(flat):
    flat.textures["kind"][0] = 2
    flat.textures["nu"][0] = flat.textures["nv"][0] = 4
    flat.textures["image"][0] = 0


def _bad_motion(flat):
    flat.motions = np.zeros(1, S.MOTION_DTYPE)
    flat.motions["v1"][0][1] = np.inf
    flat.prims["motion"][3] = 0


def _instance(blas=0, material=0, m=None, leaf=3, leaf_set=-1, leaf_material=None):
    """one placement; primitive `leaf` becomes a leaf of instanced object -1 - leaf_set"""
    def f(flat):
        flat.instances = np.zeros(1, S.INSTANCE_DTYPE)
        flat.instances[0]["blas"] = blas
        flat.instances[0]["material"] = material
        flat.instances[0]["m"] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] if m is None else m
        if leaf is not None:
            flat.prims["set"][leaf] = leaf_set
            if leaf_material is not None:
                flat.prims["material"][leaf] = leaf_material
    return f


def _both(*fs):
    def f(flat):
        for g in fs:
            g(flat)
    return f


def _deep_chain(flat):
    """Spheres whose size and spacing double along x: the binned SAH peels them off a few at a time.
    One chain of 100 is ~40 levels deep; a second one as an instanced object under a placement in
    the first adds its own levels (surface + 1 + object + 1 = 76 > RT_STACK_DEPTH)."""
    n = 100
    prims = np.zeros(2 * n, S.PRIM_DTYPE)
    prims["motion"] = prims["uvframe"] = -1
    prims["gid"] = prims["order"] = np.arange(2 * n)
    prims["set"][n:] = -1
    for i in range(2 * n):
        prims["p"][i][:4] = (2.0 ** (i % n), 0, 0, 0.4 * 2.0 ** (i % n))
    flat.prims = prims
    _instance(leaf=None)(flat)

_SCALE2 = [2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0]
# id -> (edit of the FlatScene or None, edit of the rt_scene struct or None)
DEFECTS = {
    "negative_count": (None, lambda sc: setattr(sc, "n_motions", -1)),
    "null_array": (None, lambda sc: setattr(sc, "materials", None)),
    "too_many_media": (lambda flat: setattr(flat, "media", np.zeros(9, S.MEDIUM_DTYPE)), None),
    "texture_kind": (_set("textures", 0, "kind", 7), None),
    "texture_colour": (_set("textures", 1, "c0", np.inf, sub=1), None),
    "image_past_texels": (_image_past_texels, None),
    "noise_without_perlin": (_noise(), None),
    "perlin_entry_256": (_noise(256), None),
    "material_kind": (_set("materials", 1, "kind", 10), None),
    "material_texture": (_set("materials", 1, "texture", 1000), None),
    "medium_density_0": (_media(0.0, 0), None),
    "medium_material": (_media(1.0, 1000), None),
    "prim_kind": (_set("prims", 3, "kind", 3), None),
    "prim_set": (_set("prims", 3, "set", 5), None),
    "surface_without_material": (_set("prims", 3, "material", -1), None),
    "motion_index": (_set("prims", 3, "motion", 0), None),
    "geometry_nan": (_set("prims", 3, "p", np.nan, sub=2), None),
    "motion_inf": (_bad_motion, None),
    "medium_empty_boundary": (_media(1.0, 0), None),
    "instance_of_no_object": (_instance(leaf=None), None),
    "instance_of_empty_object": (_instance(blas=0, leaf_set=-2), None),
    "instance_not_rigid": (_instance(m=_SCALE2), None),
    "instance_leaf_without_material": (_instance(material=-1, leaf_material=-1), None),
    "bvh_too_deep": (_deep_chain, None),
    # the order of the checks is behaviour: the placements are checked before the primitives
    "instance_not_rigid_and_prim_kind": (_both(_instance(m=_SCALE2), _set("prims", 5, "kind", 3)), None),
}


def defect_result(emu, name):
    """(rc, message) of the host build of the small Cornell box with one field spoiled"""
    edit_flat, edit_struct = DEFECTS[name]
    flat = small_cornell()
    if edit_flat:
        edit_flat(flat)
    sc = _lib.scene_struct(flat)
    if edit_struct:
        edit_struct(sc)
    info = np.zeros(8, np.int32)
    rc = emu.lib().rt_emu_scene_info(ctypes.byref(sc), info.ctypes.data_as(ctypes.c_void_p))
    return [int(rc), emu.lib().rt_emu_last_error().decode()]


# ------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case,scene,knob", digest_cases(), ids=[c[0] for c in digest_cases()])
def test_host_scene_is_byte_identical(emu_mod, knobs, golden, case, scene, knob):
    if knob:
        knobs.setenv(*knob.split("="))
    rc, err, got = emu_mod.scene_digest(scene())
    assert (rc, err) == (0, "")
    want = golden["digests"][case]
    assert list(got) == emu_mod.DIGEST_ITEMS == list(want)
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, {k: (got[k], want[k]) for k in differ}


# knobs that cannot change a scene's build: pawn_fog has no parallelograms (no boxes), and its
# surface set has no large primitive, no outlier even at half the shrink (no prefix)
NO_EFFECT = {("pawn_fog", "RT_AMD_NO_BOX=1"), ("pawn_fog", "RT_AMD_NO_PREFIX=1"), ("pawn_fog", "RT_AMD_PREFIX_AREA=0.9"),
             ("pawn_fog", "RT_AMD_PREFIX_SHRINK=0.5"), ("bunny_cornell", "RT_AMD_NO_ALIAS=1")}


def test_knob_runs_differ_from_the_plain_build(golden):
    # every recorded knob run reached the code it is there for
    for n in KNOB_SCENES:
        for k in KNOBS:
            if (n, k) in NO_EFFECT:
                assert golden["digests"][f"{n}+{k}"] == golden["digests"][n]
            else:
                assert golden["digests"][f"{n}+{k}"] != golden["digests"][n], (n, k)


@pytest.mark.parametrize("name", list(HAND_MADE))
def test_hand_made_scenes_reach_their_paths(emu_mod, name):
    info = emu_mod.scene_info(HAND_MADE[name]())
    assert {k: info[k] for k in HAND_MADE_INFO[name]} == HAND_MADE_INFO[name]


@pytest.mark.parametrize("name", list(DEFECTS))
def test_error_exits(emu_mod, golden, name):
    assert defect_result(emu_mod, name) == golden["errors"][name]


def test_every_defect_is_refused(golden):
    assert set(golden["errors"]) == set(DEFECTS)
    assert all(rc < 0 and msg for rc, msg in golden["errors"].values())
    assert golden["errors"]["instance_not_rigid_and_prim_kind"] == golden["errors"]["instance_not_rigid"]
