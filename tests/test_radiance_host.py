"""The radiance-query body (raytrace_amd/csrc/rt_radiance.h: path_from_ray, the record prologue, the
camera-ray body, the resolve) compiled for the host (tests/radiance_emu), without a GPU: against the
per-pixel path body (tests/list_emu, which the render's lane loops and the oracle pin) on its own
camera rays, against closed forms, its keying, malformed rays, the ABI and a sanitizer build."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT
import raytrace_amd as R
from raytrace_amd import _lib
from raytrace_amd import radiance as rad
from raytrace_amd.camera import lerpYBackground
from raytrace_amd.radiance import PATH_RAY_DTYPE, RADIANCE_DTYPE
from test_render_params import SCENES, scene

sys.path.insert(0, os.path.join(ROOT, "tests", "list_emu"))
sys.path.insert(0, os.path.join(ROOT, "tests", "radiance_emu"))
import list_emu  # noqa: E402
import radiance_emu as RE  # noqa: E402

NAMES = [n for n in SCENES if n != "cornell_192"]  # the 12 x 7 scenes: every kernel class
PRECISIONS = ["f64", "f32"]
EPS = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}    # one rounding of the precision, relative
FIX = {"f64": 2.0 ** -64, "f32": 2.0 ** -32}    # one step of the precision's fixed-point sums


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def settings(depth=8, background=(0.25, 0.5, 1.0)):
    return R.defaultCameraSettings(cs_imageWidth=4, cs_aspectRatio=1.0, cs_samplesPerPixel=1, cs_maxRecursionDepth=depth,
                                   cs_background=background)


def sphere_and_light():
    """a lambertian sphere of albedo 0.5 at the origin and an emitter of (0.5, 2, 0.25) at z = 5: all dyadic"""
    return R.group([R.lambertian(R.constantTexture(0.5)) << R.sphere((0, 0, 0), 1.0),
                    R.lightSource(R.constantTexture((0.5, 2.0, 0.25))) << R.parallelogram((-1, -1, 5), (2, 0, 0), (0, 2, 0))])


# ---- 1. the emulator against the list emulator
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", NAMES)
def test_own_camera_rays_give_the_list_emulators_image(name, precision):
    """Three accumulated one-sample calls, sample0 = 0, 1, 2, each on the emulator's own camera rays of
    that sample: rgb is list_emu's image at counts of 3 bit for bit (list_emu resolves the sums of
    path_sample with the count; a flagged pixel is NaN in both), every ray holds 3 samples."""
    cs, flat, seed = scene(name)
    ref = list_emu.render(cs, flat, seed, 3, precision)
    work = None
    for k in range(3):
        rays = RE.camera_rays(cs, flat, seed, k, precision)
        assert (rays["sample0"] == k).all() and (rays["stream"] == np.arange(len(rays))).all()
        assert np.allclose(np.linalg.norm(rays["dir"], axis=1), 1.0, atol=1e-6) and ((rays["time"] >= 0) & (rays["time"] < 1)).all()
        out, work = RE.radiance(cs, flat, seed, rays, 1, precision, unit_dir=True, work=work)
    rgb = out["rgb"].astype(ref.dtype).reshape(ref.shape)
    assert np.array_equal(bits(rgb), bits(ref)), f"{int((bits(rgb) != bits(ref)).any(-1).sum())} pixels differ"
    assert (out["samples"] == 3).all() and ((work[:, -1] >> np.uint64(32)) == 3).all()
    flagged = (work[:, -1] & np.uint64(0xffffffff)) != 0
    assert (out["status"] == np.where(flagged, 2, 1)).all() and (np.isnan(rgb).any(-1).ravel() == flagged).all()
    assert np.isfinite(ref).all() and ref.max() > 0


# ---- 2. closed forms
@pytest.mark.parametrize("precision", PRECISIONS)
def test_emitter_miss_and_depth_closed_forms(precision):
    world = sphere_and_light()
    rays = rad.make_path_rays([(0, 0, 3), (0, 5, 0), (0, 0, -4)], [(0, 0, 2), (0, 3, 0), (0, 0, 1)])
    for samples in (1, 3, 7):
        out, work = RE.radiance(settings(), world, 7, rays, samples, precision)
        assert (out["status"] == 1).all() and (out["samples"] == samples).all()
        assert (out["rgb"][0] == (0.5, 2.0, 0.25)).all()   # the emission, exactly, for any sample count
        assert (out["rgb"][1] == (0.25, 0.5, 1.0)).all()   # a miss: the constant background, exactly
    out0, _ = RE.radiance(settings(depth=0), world, 7, rays, 4, precision)
    assert (out0["rgb"] == 0).all() and (out0["samples"] == 4).all() and (out0["status"] == 1).all()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_lerp_background_closed_form(precision):
    """A miss under RT_BG_LERP_Y is (1 - a) c0 + a c1, a = 0.5 (d.y + 1), of the direction the kernel
    sees (unit_dir: the record's bits, rounded to the precision).  a, 1 - a, the two products and the
    sum are at most four roundings of the precision on a value no larger than the larger colour
    (the two terms are convex weights of it), plus one truncation step of the fixed-point sums."""
    c0, c1 = np.array((1.0, 0.75, 0.5)), np.array((0.25, 0.5, 2.0))
    cs = settings(background=lerpYBackground(tuple(c0), tuple(c1)))
    rng = np.random.default_rng(5)
    d = rng.normal(size=(64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if precision == "f32":
        d = d.astype(np.float32).astype(np.float64)
    rays = rad.make_path_rays((0, 50, 0), d)
    out, _ = RE.radiance(cs, sphere_and_light(), 3, rays, 1, precision, unit_dir=True)
    a = 0.5 * (d[:, 1:2] + 1.0)
    want = (1.0 - a) * c0 + a * c1
    bar = 4 * EPS[precision] * max(c0.max(), c1.max()) + FIX[precision]
    err = np.abs(out["rgb"] - want).max()
    print(f"lerp background {precision}: worst error {err:.3e}, bar {bar:.3e}")
    assert (out["status"] == 1).all() and err <= bar


@pytest.mark.parametrize("precision", PRECISIONS)
def test_lone_lambertian_sphere_closed_form(precision):
    """A lone convex lambertian sphere of albedo a under a constant background c: a path scatters once
    (throughput a pdf1 rcp(pdf1)) and leaves, so the radiance is a c at depth >= 2 and 0 at depth 1.
    Roundings: rcp(pdf1) (one, correctly rounded on the host), its product with pdf1 (one), the product
    with a (one) and with c (one): four roundings of the precision relative to a c, plus one
    truncation step of the fixed-point sums per sample."""
    a, c = 0.5, np.array((0.25, 0.5, 1.0))
    world = R.lambertian(R.constantTexture(a)) << R.sphere((0, 0, 0), 1.0)
    rng = np.random.default_rng(11)
    o = rng.normal(size=(32, 3))
    o = 4.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    rays = rad.make_path_rays(o, -o + 0.2 * rng.normal(size=(32, 3)))
    out, _ = RE.radiance(settings(depth=4, background=tuple(c)), world, 9, rays, 16, precision)
    bar = 4 * EPS[precision] * a * c.max() + FIX[precision]
    err = np.abs(out["rgb"] - a * c).max()
    print(f"lambertian sphere {precision}: worst error {err:.3e}, bar {bar:.3e}")
    assert (out["status"] == 1).all() and err <= bar
    out1, _ = RE.radiance(settings(depth=1, background=tuple(c)), world, 9, rays, 16, precision)
    assert (out1["rgb"] == 0).all() and (out1["status"] == 1).all()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_media_events_fire(precision):
    """Rays through a constantMedium: on the emulator's camera rays the result is list_emu's image
    (the chain of test 1, whose path body runs the media events), and it differs from the same rays'
    result without the medium, which is the constant background exactly."""
    c = (0.25, 0.5, 1.0)
    fog = R.isotropic(R.constantTexture(0.5)) << R.constantMedium(0.8, R.sphere((0, 0, -3), 1.0))
    cs = R.defaultCameraSettings(cs_imageWidth=6, cs_aspectRatio=1.5, cs_samplesPerPixel=1, cs_maxRecursionDepth=6,
                                 cs_background=c, cs_vfov=0.3, cs_center=(0, 0, 0), cs_lookAt=(0, 0, -1))
    far = R.lambertian(R.constantTexture(0.5)) << R.sphere((0, -1000, 0), 1.0)   # (a surface out of every ray's way)
    rays = RE.camera_rays(cs, R.group([fog, far]), 5, 0, precision)
    out, _ = RE.radiance(cs, R.group([fog, far]), 5, rays, 8, precision, unit_dir=True)
    # (samples 0..7 of one call use camera ray 0 for every sample: only sample 0 is list_emu's path)
    one, _ = RE.radiance(cs, R.group([fog, far]), 5, rays, 1, precision, unit_dir=True)
    ref1 = list_emu.render(cs, R.group([fog, far]), 5, 1, precision)
    assert np.array_equal(bits(one["rgb"].astype(ref1.dtype).reshape(ref1.shape)), bits(ref1))
    clear, _ = RE.radiance(cs, far, 5, rays, 8, precision, unit_dir=True)
    assert (clear["rgb"] == c).all()
    assert (np.abs(out["rgb"] - clear["rgb"]).max(-1) > 1e-3).mean() > 0.5 and (out["status"] == 1).all()


# ---- 3. keying
@pytest.mark.parametrize("precision", PRECISIONS)
def test_results_are_keyed_by_the_record(precision):
    cs, flat, seed = scene("cornell")
    rays = RE.camera_rays(cs, flat, seed, 0, precision).copy()
    rays["sample0"] = 3
    out, work = RE.radiance(cs, flat, seed, rays, 4, precision, unit_dir=True)
    perm = np.random.default_rng(2).permutation(len(rays))
    outp, workp = RE.radiance(cs, flat, seed, rays[perm], 4, precision, unit_dir=True)
    assert outp.tobytes() == out[perm].tobytes() and workp.tobytes() == work[perm].tobytes()
    twice = np.concatenate([rays[40:44], rays[40:44]])
    out2, _ = RE.radiance(cs, flat, seed, twice, 4, precision, unit_dir=True)
    assert out2[:4].tobytes() == out2[4:].tobytes() == out[40:44].tobytes()
    lit = out["rgb"].max(-1) > 0   # rays that scatter inside the box
    assert lit.sum() >= 20
    for field, value in (("stream", rays["stream"] + 1000), ("sample0", 4)):
        other = rays.copy()
        other[field] = value
        o, _ = RE.radiance(cs, flat, seed, other, 4, precision, unit_dir=True)
        assert ((o["rgb"] != out["rgb"]).any(-1) & lit).sum() >= lit.sum() // 2, field
    o, _ = RE.radiance(cs, flat, R.mkStdGen(12345), rays, 4, precision, unit_dir=True)
    assert ((o["rgb"] != out["rgb"]).any(-1) & lit).sum() >= lit.sum() // 2


# ---- 4. malformed rays
@pytest.mark.parametrize("precision", PRECISIONS)
def test_malformed_rays_are_flagged_and_touch_nothing(precision):
    world = sphere_and_light()
    good = rad.make_path_rays([(0, 0, 3), (0, 5, 0), (0, 0, -4)] * 3, [(0, 0, 2), (0, 3, 0), (0, 0, 1)] * 3)[:8]
    rays = good.copy()
    rays["origin"][1, 0] = np.nan
    rays["dir"][2, 1] = np.inf
    rays["dir"][3] = 0.0
    rays["time"][4] = -0.1
    rays["time"][5] = 1.5
    rays["time"][6] = np.nan
    bad = np.zeros(8, bool)
    bad[1:7] = True
    ref, ref_work = RE.radiance(settings(), world, 7, good, 3, precision)
    out, work = RE.radiance(settings(), world, 7, rays, 3, precision)
    assert (out["status"][bad] == -1).all() and (out["rgb"][bad] == 0).all() and (out["samples"][bad] == 0).all()
    assert (work[bad] == 0).all()
    assert out[~bad].tobytes() == ref[~bad].tobytes() and work[~bad].tobytes() == ref_work[~bad].tobytes()
    # accumulating: a malformed ray's workspace words stay what they were
    out2, work2 = RE.radiance(settings(), world, 7, rays, 2, precision, work=ref_work)
    assert work2[bad].tobytes() == ref_work[bad].tobytes() and (out2["status"][bad] == -1).all()
    assert (out2["samples"][~bad] == 5).all() and (out2["samples"][bad] == 3).all()
    # time 0 and time 1 are well formed
    edge = good[:2].copy()
    edge["time"] = (0.0, 1.0)
    assert (RE.radiance(settings(), world, 7, edge, 1, precision)[0]["status"] == 1).all()


# ---- 5. ABI
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "rt.h"
#define S(T) printf(#T " %zu\n", sizeof(T))
#define O(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  S(rt_path_ray); O(rt_path_ray, origin); O(rt_path_ray, dir); O(rt_path_ray, time); O(rt_path_ray, stream);
  O(rt_path_ray, sample0);
  S(rt_radiance); O(rt_radiance, rgb); O(rt_radiance, status); O(rt_radiance, samples);
  printf("RT_ABI_VERSION %d\nRT_RADIANCE_UNIT_DIR %d\nRT_RADIANCE_ACCUMULATE %d\n", RT_ABI_VERSION, RT_RADIANCE_UNIT_DIR,
         RT_RADIANCE_ACCUMULATE);
  return 0;
}
"""
NEW_SYMBOLS = ["rt_scene_radiance_workspace_bytes", "rt_scene_radiance_async", "rt_scene_radiance", "rt_scene_radiance_status",
               "rt_scene_camera_rays_async", "rt_scene_camera_rays"]


def test_record_layouts_symbols_and_haskell_offsets():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write(LAYOUT_C)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src], check=True)
        got = dict(line.rsplit(" ", 1) for line in subprocess.run([exe], capture_output=True, text=True,
                                                                  check=True).stdout.splitlines())
    got = {k: int(v) for k, v in got.items()}
    assert got["rt_path_ray"] == PATH_RAY_DTYPE.itemsize == 64 and got["rt_radiance"] == RADIANCE_DTYPE.itemsize == 32
    for st, dt in (("rt_path_ray", PATH_RAY_DTYPE), ("rt_radiance", RADIANCE_DTYPE)):
        for f in dt.names:
            assert got[f"{st}.{f}"] == dt.fields[f][1], (st, f)
    assert got["RT_ABI_VERSION"] == 6 == _lib.ABI_VERSION
    assert got["RT_RADIANCE_UNIT_DIR"] == _lib.RT_RADIANCE_UNIT_DIR and got["RT_RADIANCE_ACCUMULATE"] == _lib.RT_RADIANCE_ACCUMULATE
    assert "#define RT_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "rt.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (rt_\w+)", nm))
    assert set(NEW_SYMBOLS) <= exported and set(NEW_SYMBOLS) <= set(_lib.EXPORTED + _lib.SIZE_FUNCTIONS)
    hs = open(os.path.join(ROOT, "hs", "Graphics", "Ray", "Device.hs")).read()
    decl = {(s, f): int(v) for s, f, v in re.findall(r"^-- LAYOUT (\w+)(?:\.(\w+))? (\d+)$", hs, flags=re.M)}
    for key, v in got.items():
        if key.startswith(("rt_path_ray", "rt_radiance")):
            st, _, f = key.partition(".")
            assert decl[(st, f)] == v, key
    assert "radianceMany" in hs and "cameraRays" in hs and '"rt_scene_radiance"' in hs and '"rt_scene_camera_rays"' in hs
    L = _lib.load()
    assert L.rt_scene_radiance_workspace_bytes(5, 0) == rad.workspace_bytes(5, "f64") == 5 * 7 * 8 + 16
    assert L.rt_scene_radiance_workspace_bytes(5, _lib.RT_EXEC_F32) == rad.workspace_bytes(5, "f32") == 5 * 4 * 8 + 16


def test_argument_checks_need_no_device():
    """Null arguments, n < 0, n_samples <= 0, unknown flags, a device list and ids beyond the range are
    RT_E_INVALID before the scene handle is ever dereferenced (a made-up handle is never read)."""
    import ctypes
    L = _lib.load()
    cs = _lib.camera_struct(settings())
    ex = _lib.exec_struct()
    buf = np.zeros(64, np.uint8).ctypes.data_as(ctypes.c_void_p)
    assert L.rt_scene_radiance(None, ctypes.byref(ex), ctypes.byref(cs), 0, buf, buf, None, 1, 1, 0) == _lib.RT_E_INVALID
    assert b"null scene" in L.rt_last_error()
    assert L.rt_scene_radiance_async(None, ctypes.byref(ex), ctypes.byref(cs), 0, buf, buf, buf, 1, 1, 0, None) == _lib.RT_E_INVALID
    assert L.rt_scene_camera_rays(None, ctypes.byref(ex), ctypes.byref(cs), 0, 0, buf) == _lib.RT_E_INVALID
    assert L.rt_scene_camera_rays_async(None, ctypes.byref(ex), ctypes.byref(cs), 0, 0, buf, None) == _lib.RT_E_INVALID
    with pytest.raises(ValueError):
        rad.make_path_rays(np.zeros((2, 2, 3)), (0, 0, 1))
    r = rad.make_path_rays(np.zeros((5, 3)), (0, 0, 1), time=0.5)
    assert (r["stream"] == np.arange(5)).all() and (r["sample0"] == 0).all() and (r["time"] == 0.5).all()


# ---- 6. sanitizers
def test_radiance_body_under_sanitizers():
    """tests/radiance_emu's stand-alone program (its own main; address and undefined-behaviour
    sanitizers linked in, nothing preloaded) drives the emulator and the argument checks over the
    closed forms and the malformed rays above."""
    here = os.path.join(ROOT, "tests", "radiance_emu")
    subprocess.run(["make", "-C", here, "-s", "san"], check=True)
    p = subprocess.run([os.path.join(here, "_build", "radiance_san")], capture_output=True, text=True)
    assert p.returncode == 0 and "radiance_san: 0 failed" in p.stdout, p.stdout + p.stderr
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr
