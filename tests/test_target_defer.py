"""The deferred redirect pdf of the diffuse flat kernels (rt_build.cpp rt_host_render_params,
rt_trace.h lane_loop_lockstep / closest_flat / mixture_scatter; KernelParams::target_defer).

When the scene's one redirect target is, bit for bit, a static parallelogram of the flat surface
set whose material ends the path, the scatter leaves the target's term of the mixture pdf to the
next segment's test of that record.  Every draw and every branch stay the same; only the rounding
order of the throughput factor changes.  So the bars are those of tests/test_gpu.py against the
oracle's Philox mode (binary64: >= 99.9 % of pixels within 1e-9 relative, the worst pixel within
2 L / spp; FP32: >= 99 % within 1e-3, the worst within 4 L / spp; the mean within 5e-3), the same
bars between the two orders, and the emulator-against-device bar of
test_gpu.py::test_gpu_matches_kernel_emulator between the host emulator and the device.

CPU tests run the host emulator (the same rt_trace.h); the GPU tests the library.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, pixel_agreement

import raytrace_amd as R  # noqa: E402
from raytrace_amd import _lib, scenes  # noqa: E402
from raytrace_amd.core import V3, degrees, fromCorners, mkStdGen  # noqa: E402
from raytrace_amd.geometry import (constantMedium, cuboid, group, parallelogram, rotateY, sphere, transform,  # noqa: E402
                                   translate)
from raytrace_amd.material import constantTexture, isotropic, lambertian, lightSource  # noqa: E402
from raytrace_amd.ray import assemble_shards, render_shard  # noqa: E402
from raytrace_amd.scene import flatten  # noqa: E402

PRECISIONS = ["f64", "f32"]
LMAX = 15.0  # the light's emission: the largest radiance of one sample
LIGHT_Q, LIGHT_U, LIGHT_V = V3(343, 554, 332), V3(-130, 0, 0), V3(0, 0, -105)


def box(light=None, extra=(), targets=None, width=32, spp=16, depth=50, **cam):
    """The Cornell box of scenes.cornell_box with its light replaced by `light` (a Geometry; default
    the reference's quad), `extra` objects added and `targets` as the redirect targets (default the
    reference's: the light's parallelogram with probability 0.25)."""
    walls, white = scenes.cornell_walls()
    emit = lightSource(constantTexture(V3(LMAX, LMAX, LMAX)))
    walls[2] = light if light is not None else emit << parallelogram(LIGHT_Q, LIGHT_U, LIGHT_V)
    blocks = [
        transform(translate(V3(265, 0, 295)) @ rotateY(degrees(15)),
                  white << cuboid(fromCorners(V3(0, 0, 0), V3(165, 330, 165)))),
        transform(translate(V3(130, 0, 65)) @ rotateY(degrees(-18)),
                  white << cuboid(fromCorners(V3(0, 0, 0), V3(165, 165, 165)))),
    ]
    cs = scenes.cornell_settings(width, spp, depth).replace(**cam)
    if targets is not None:
        cs = cs.replace(cs_redirectTargets=list(targets))
    return cs, group(walls + blocks + list(extra)), mkStdGen(234)


def emit():
    return lightSource(constantTexture(V3(LMAX, LMAX, LMAX)))


def white():
    return lambertian(constantTexture(V3(0.73, 0.73, 0.73)))


def up32(x):
    """x moved one FP32 ulp up: another number in both precisions the records are uploaded in."""
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


# A lambertian quad that is a target.  A scatter ON it that draws the target gets a direction in the
# quad's own plane, so the reference's `pdf1 <= 0` (Ray.hs:198) is decided by the last bit of the
# hit point there, and the device (FMA contraction, refined hardware reciprocals) and the IEEE host
# may part: the reference's algorithm, whatever the pdf's order.  With probability p for the target
# a fraction ~p of the bounces lands on the quad and p of those draw it again, p^2 of all bounces:
# at p = 0.25 that is ~3000 such draws in a 32 x 32 x 16 image, and 2-3 of its 1024 binary64 pixels
# differ between device and emulator (on the scatter's own target loop; the quad's size does not
# matter, the target draws the rays to it).  p = 0.02 leaves ~20 such draws.
SHELF = (V3(200, 300, 200), V3(150, 0, 0), V3(0, 0, 150))
SHELF_P = 0.02
LAMP = (V3(213, 500, 227), V3(343, 554, 332))  # a light-emitting cuboid: its bottom face is the target
LAMP_FACE = (LAMP[0], V3(130.0, 0.0, 0.0), V3(0.0, 0.0, 105.0))

# name -> (scene builder, the host defers)
SCENES = {
    "cornell": (lambda **k: box(**k), True),
    # the light's parallelogram written from its other diagonal's vectors swapped: the same surface,
    # another record (the normal and the two edge vectors trade places), so no match — and, the
    # plane test being symmetric in them, the same image as the matched scene's old path
    "swapped": (lambda **k: box(light=emit() << parallelogram(LIGHT_Q, LIGHT_V, LIGHT_U), **k), False),
    "ulp": (lambda **k: box(targets=[(0.25, V3(up32(343), 554, 332), LIGHT_U, LIGHT_V)], **k), False),
    "two_targets": (lambda **k: box(targets=[(0.25, LIGHT_Q, LIGHT_U, LIGHT_V),
                                             (0.1, V3(200, 250, 200), V3(100, 0, 0), V3(0, 0, 100))], **k), False),
    "lambertian_target": (lambda **k: box(extra=[white() << parallelogram(*SHELF)], targets=[(SHELF_P,) + SHELF], **k),
                          False),
    # the lamp's bottom face as geometry.cuboid writes it, parallelogram((xmin, ymin, zmin), dx, dz):
    # inside the cuboid's box group it must not match; the same parallelogram as a lone quad does
    # (lamp_face_alone), so it is the box group that keeps the first from deferring
    "box_group_target": (lambda **k: box(light=emit() << cuboid(fromCorners(*LAMP)), targets=[(0.25,) + LAMP_FACE], **k),
                         False),
    "lamp_face_alone": (lambda **k: box(light=emit() << parallelogram(*LAMP_FACE), targets=[(0.25,) + LAMP_FACE], **k),
                        True),
    "medium": (lambda **k: box(extra=[isotropic(constantTexture(1)) << constantMedium(0.002, sphere(V3(278, 278, 278), 150))],
                               **k), False),
}
# first-bounce edge cases of the matched scene (16 x 16 at 8 spp: they go wrong there or not at all)
EDGES = {
    # every primary ray ends on the light: no scatter precedes it, no pdf factor may apply
    "at_the_light": dict(cs_center=V3(278, 150, 250), cs_lookAt=V3(278, 554, 279.5), cs_vfov=0.15),
    "depth1": dict(depth=1),
    "depth2": dict(depth=2),
    "full_prob": dict(targets=[(1.0, LIGHT_Q, LIGHT_U, LIGHT_V)]),  # remProb = 0: the pdf is the target's term alone
}
# the light (and the target on it) 2^-14 = 6.1e-5 above the floor: closer to that wall than the rays'
# tmin, 1e-4, so most rays leaving the floor below it pass through it — yet the target's pdf term,
# which knows no tmin, counts it.  (At the floor, y = 0, FP32 still resolves the gap; under the
# ceiling, y = 555, it is one ulp and FP32 paths part from the oracle's whatever the pdf's order.)
NEAR_Y = 2.0 ** -14
NEAR = dict(light=None, targets=[(0.25, V3(343, NEAR_Y, 332), LIGHT_U, LIGHT_V)])


def edge_scene(name):
    if name == "near_wall":
        return box(light=emit() << parallelogram(V3(343, NEAR_Y, 332), LIGHT_U, LIGHT_V), targets=NEAR["targets"],
                   width=16, spp=8)
    return box(width=16, spp=8, **EDGES[name])


ALL_EDGES = list(EDGES) + ["near_wall"]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(settings, world, seed), built once."""
    return edge_scene(name[5:]) if name.startswith("edge:") else SCENES[name][0]()


_PROBE = None


def probe():
    """tests/target_defer/td_probe.cpp (host code: the builder and its match), built once."""
    global _PROBE
    if _PROBE is None:
        import subprocess
        d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "target_defer")
        subprocess.run(["make", "-C", d, "-s"], check=True)
        _PROBE = ctypes.CDLL(os.path.join(d, "_build", "librt_td_probe.so"))
        _PROBE.rt_td_last_error.restype = ctypes.c_char_p
    return _PROBE


def host_match(emu_mod, name, precision):
    """(target_defer, target_rec) the host chooses for the scene's render in this precision."""
    cs, world, _ = scene(name)
    flat = flatten(world)
    out = (ctypes.c_int * 2)()
    csx, scx = _lib.camera_struct(cs), _lib.scene_struct(flat)
    rc = probe().rt_td_target_match(ctypes.byref(csx), ctypes.byref(scx), ctypes.c_int(precision == "f64"), out)
    assert rc == 0, probe().rt_td_last_error()
    return out[0], out[1]


_REF = {}


def oracle_ref(oracle_mod, name):
    """The oracle's Philox-mode render: computed once per scene, read-only."""
    if name not in _REF:
        cs, flat, seed = scene(name)
        ref = oracle_mod.render(cs, flat, seed, mode=oracle_mod.RNG_PHILOX)
        ref.setflags(write=False)
        _REF[name] = ref
    return _REF[name]


_EMU = {}


def emu_render(emu_mod, name, precision):
    """The host emulator's render with no knobs set: computed once, read-only."""
    if (name, precision) not in _EMU:
        cs, flat, seed = scene(name)
        img = emu_mod.render(cs, flat, seed, precision=precision)
        img.setflags(write=False)
        _EMU[name, precision] = img
    return _EMU[name, precision]


def assert_bars(img, ref, precision, spp, what):
    """tests/test_gpu.py's per-pixel, worst-pixel and mean bars (no 8 x 8 block bar: its floor is a
    property of the full-size published image)."""
    assert img.shape == ref.shape and np.isfinite(img).all(), what
    d = np.abs(img.astype(np.float64) - ref)
    if precision == "f64":
        rel = (d / np.maximum(np.abs(ref), 1e-3)).max(-1)
        frac = float((rel <= 1e-9).mean())
        print(what, "f64 within 1e-9:", frac, "max abs:", float(d.max()))
        assert frac >= 0.999, (what, frac)
        assert d.max() <= 2 * LMAX / spp, (what, float(d.max()))
    else:
        rel = (d / np.maximum(np.abs(ref), 1.0)).max(-1)
        frac = float((rel < 1e-3).mean())
        print(what, "f32 within 1e-3:", frac, "max abs:", float(d.max()))
        assert frac >= 0.99, (what, frac)
        assert d.max() <= 4 * LMAX / spp + 1e-3, (what, float(d.max()))
    np.testing.assert_allclose(img.reshape(-1, 3).mean(0), ref.reshape(-1, 3).mean(0), rtol=5e-3, atol=1e-6)


# ------------------------------------------------------------------ host

def test_appended_kernel_params_keep_every_earlier_offset(emu_mod):
    """KernelParams grows at its end only: every member of the struct before this change sits at the
    byte offset it had (tests/golden/kernel_params_offsets.json, from the earlier header), in both
    precisions, and the new members follow the old last one."""
    with open(os.path.join(GOLDEN, "kernel_params_offsets.json")) as f:
        want = json.load(f)
    for f64, key in ((0, "f32"), (1, "f64")):
        n = probe().rt_td_params_offsets(f64, None, None, 0)
        off = (ctypes.c_longlong * n)()
        names = (ctypes.c_char_p * n)()
        assert probe().rt_td_params_offsets(f64, off, names, n) == n
        got = {names[i].decode(): int(off[i]) for i in range(n)}
        old = dict(want[key])
        old_size = old.pop("sizeof")
        assert list(got)[:len(old)] == list(old), "members in declaration order"
        assert {k: got[k] for k in old} == old
        new = [k for k in got if k not in old and k != "sizeof"]
        assert new == ["target_defer", "target_rec", "cam_defocus"]
        assert all(got[k] >= got["sample0"] + 4 for k in new) and got["sizeof"] >= old_size


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(SCENES))
def test_host_matches_only_the_safe_case(emu_mod, name, precision):
    defer, rec = host_match(emu_mod, name, precision)
    assert bool(defer) == SCENES[name][1], (name, defer, rec)
    assert (rec >= 0) == bool(defer)
    if name == "box_group_target":  # the lamp really is a box group (the walls, the two blocks, the lamp)
        assert emu_mod.scene_info(scene(name)[1])["boxes"] == emu_mod.scene_info(scene("cornell")[1])["boxes"] + 1


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ALL_EDGES)
def test_host_matches_the_edge_scenes(emu_mod, name, precision):
    assert host_match(emu_mod, "edge:" + name, precision)[0] == 1


def test_knob_and_pinned_variant_leave_the_old_path(knobs, emu_mod):
    assert host_match(emu_mod, "cornell", "f64")[0] == 1  # (the experiments switch alone changes nothing)
    knobs.setenv("RT_AMD_TARGET_DEFER", "0")
    assert host_match(emu_mod, "cornell", "f64") == (0, -1)
    knobs.setenv("RT_AMD_TARGET_DEFER", "1")
    assert host_match(emu_mod, "cornell", "f64")[0] == 1
    knobs.setenv("RT_AMD_VARIANT", "0")
    assert host_match(emu_mod, "cornell", "f64") == (0, -1)


# ------------------------------------------------------------------ emulator against the oracle

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(SCENES))
def test_emulator_matches_oracle(emu_mod, oracle_mod, name, precision):
    """32 x 32 at 16 spp: the matched scene (deferred) and every scene that must not defer."""
    img = emu_render(emu_mod, name, precision)
    assert_bars(img, oracle_ref(oracle_mod, name), precision, 16, name)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ALL_EDGES)
def test_emulator_edge_cases_match_oracle(emu_mod, oracle_mod, name, precision):
    img = emu_render(emu_mod, "edge:" + name, precision)
    assert_bars(img, oracle_ref(oracle_mod, "edge:" + name), precision, 8, name)
    if name == "at_the_light":  # every sample is the light's emission, exactly
        assert np.array_equal(img, np.full_like(img, LMAX))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_fallback_is_the_old_path(knobs, emu_mod, oracle_mod, precision):
    """RT_AMD_TARGET_DEFER=0 on the matched scene: within the bars of the deferred render and of the
    oracle, and bit-identical to the render of the scene whose light is the same parallelogram
    written with its edge vectors swapped — a record the target does not match, so a render that
    cannot defer."""
    deferred = emu_render(emu_mod, "cornell", precision)
    unmatched = emu_render(emu_mod, "swapped", precision)
    knobs.setenv("RT_AMD_TARGET_DEFER", "0")
    cs, flat, seed = scene("cornell")
    old = emu_mod.render(cs, flat, seed, precision=precision)
    assert_bars(old, oracle_ref(oracle_mod, "cornell"), precision, 16, "old path")
    assert_bars(deferred, old.astype(np.float64), precision, 16, "deferred against old")
    assert np.array_equal(old, unmatched)
    assert not np.array_equal(old, deferred)  # (the deferred order does round differently: it ran)


# ------------------------------------------------------------------ device

@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    return torch


_DEV = {}


def dev_render(name, precision):
    if (name, precision) not in _DEV:
        cs, flat, seed = scene(name)
        img = R.raytrace(cs, flat, seed, precision=precision)
        img.setflags(write=False)
        _DEV[name, precision] = img
    return _DEV[name, precision]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(SCENES) + ["edge:" + e for e in ALL_EDGES])
def test_device_matches_emulator(gpu, emu_mod, name, precision):
    """Every scene of this file, deferring or not, on the device against the emulator."""
    a, b = dev_render(name, precision), emu_render(emu_mod, name, precision)
    assert np.isfinite(a).all()
    if precision == "f64":
        rel = (np.abs(a - b) / np.maximum(np.abs(b), 1e-3)).max(-1)
        print(name, "f64 within 1e-9 of the emulator:", float((rel <= 1e-9).mean()))
        assert (rel <= 1e-9).mean() >= 0.999
    else:
        print(name, "f32 within 1e-4 of the emulator:", pixel_agreement(a, b, 1e-4))
        assert pixel_agreement(a, b, 1e-4) > 0.99


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_old_path_and_repeats(knobs, gpu, precision):
    """Repeated renders are bit-identical; the knob's old path is the unmatched scene's image, bit for
    bit, and differs from the deferred one by rounding only."""
    cs, flat, seed = scene("cornell")
    first = dev_render("cornell", precision)
    for _ in range(2):
        assert np.array_equal(R.raytrace(cs, flat, seed, precision=precision), first)
    knobs.setenv("RT_AMD_TARGET_DEFER", "0")
    old = R.raytrace(cs, flat, seed, precision=precision)
    assert np.array_equal(old, dev_render("swapped", precision))
    assert not np.array_equal(old, first)
    assert pixel_agreement(first, old.astype(np.float64), 1e-9 if precision == "f64" else 1e-3) >= 0.99


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_shards_are_bit_identical(gpu, precision):
    cs, flat, seed = scene("cornell")
    want = dev_render("cornell", precision)
    for n in (1, 2, 3):
        tiles = [render_shard(cs, flat, seed, n, k, 4, precision=precision) for k in range(n)]
        assert np.array_equal(assemble_shards(tiles, 32, 4), want), n


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("width,passes", [(32, (7, 9)), (8, (150, 150))])
def test_film_in_two_passes_equals_one_shot(gpu, width, passes, precision):
    """The carried pdf term does not leak across samples, passes or stolen samples: 32 x 32 in passes
    of 7 and 9 samples (3-sample tail items), and 8 x 8 in two passes of 150, where the queue drains
    at once and most samples are stolen from another lane's item."""
    cs, world, seed = box(width=width, spp=sum(passes))
    flat = flatten(world)
    want = R.raytrace(cs, flat, seed, precision=precision)
    with R.Film(flat, cs, seed, precision=precision) as f:
        for n in passes:
            f.add(n)
        img = f.image()
    assert np.array_equal(img, want, equal_nan=True) and img.mean() > 0
