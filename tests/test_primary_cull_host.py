"""The screen rectangles of the ring loop's camera segments (rt_build.cpp rt_host_cull_rects) on the
host, without a GPU.

tests/primary_cull/cull_rects.cpp is built once over rt_build.cpp and rt_trace.h under RT_HOST_EMU
(g++ -ffp-contract=off) and run per scene and camera, in both precisions.  For every box group and
static parallelogram with a rectangle it sweeps the frame with camera rays made as camera_ray_flat
makes them (through each pixel's four footprint corners and 16 jittered points) and tests them against
that record alone with test_box<true> / isect_plane<1> (cull_body.h):

- no pixel outside the rectangle has a valid candidate (what the kernel's skip relies on);
- the rectangle, cut to the frame, lies within 2 pixels of the tight bounding rectangle of the pixels
  that have one, so that empty culling ("every pixel" everywhere) cannot pass;
- the rectangle is "every pixel" exactly when the camera has a defocus disk or a corner of the record
  is not strictly in front of the camera: every record of the defocus camera, the room's box group
  for the camera inside it, the tall box for the camera beside it.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from raytrace_amd import scenes
from raytrace_amd.camera import image_height
from raytrace_amd.core import V3
from raytrace_amd.scene import flatten

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "primary_cull")
CSRC = os.path.join(os.path.dirname(SRC), os.pardir, "raytrace_amd", "csrc")

SCENES = {"cornell": scenes.cornell_box, "box_gallery": scenes.box_gallery}
SIZES = {"40x30": (40, 30), "64x64": (64, 64)}
CAMERAS = {
    "inside": dict(cs_center=V3(278, 278, 20), cs_lookAt=V3(278, 278, 555)),
    "corner_behind": dict(cs_center=V3(255, 200, 350), cs_lookAt=V3(455, 200, 450)),
    "defocus": dict(cs_defocusAngle=0.02, cs_focusDist=1000.0),
}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("primary_cull")
    exe = str(d / "cull_rects")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-o", exe, os.path.join(SRC, "cull_rects.cpp"),
                    os.path.join(CSRC, "rt_build.cpp"), os.path.join(CSRC, "rt_bvh.cpp"), "-lm", "-pthread"], check=True)
    files = {}
    for name, make in SCENES.items():
        flat = flatten(make()[1])
        assert not (len(flat.media) or len(flat.motions) or len(flat.uvframes) or len(flat.texels))
        path = str(d / f"{name}.scene")
        with open(path, "wb") as f:
            f.write(np.array([len(flat.prims), len(flat.materials), len(flat.textures)], np.int32).tobytes())
            for a in (flat.prims, flat.materials, flat.textures):
                f.write(np.ascontiguousarray(a).tobytes())
        files[name] = path
    return exe, files


def run(program, scene, size, **camera):
    exe, files = program
    w, h = SIZES[size]
    cs = SCENES[scene]()[0].replace(cs_imageWidth=w, cs_aspectRatio=w / h, **camera)
    assert image_height(cs) == h
    args = [exe, files[scene], str(w), repr(w / h), *map(repr, map(float, cs.cs_center)),
            *map(repr, map(float, cs.cs_lookAt)), repr(float(cs.cs_vfov)), repr(float(cs.cs_defocusAngle)),
            repr(float(cs.cs_focusDist))]
    r = subprocess.run(args, capture_output=True, text=True)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and not [ln for ln in lines if not ln.startswith("ok ")], r.stdout + r.stderr
    recs = [dict(re.findall(r"(\w+)=(\S+)", ln), prec=ln.split()[1], kind=ln.split()[2], j=int(ln.split()[3]))
            for ln in lines if " box " in ln or " quad " in ln]
    assert {r["prec"] for r in recs} == {"f32", "f64"}
    return recs


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("scene", list(SCENES))
def test_rectangles_hold_every_hit_and_are_tight(program, scene, size):
    recs = run(program, scene, size)
    # the Cornell walls' box group, the scene's other boxes, the light: each has a real rectangle
    assert len([r for r in recs if r["prec"] == "f64" and r["kind"] == "box"]) >= 3
    assert len([r for r in recs if r["prec"] == "f64" and r["kind"] == "quad"]) >= 1
    assert all(r["all"] == "0" and r["want_all"] == "0" for r in recs)
    # ... and the inner boxes and the light cover a small part of the frame (the room: all of it)
    w, h = SIZES[size]
    small = 0
    for r in recs:
        x0, x1, y0, y1 = map(int, re.match(r"(\d+)\.\.(-?\d+),(\d+)\.\.(-?\d+)", r["rect"]).groups())
        small += (x1 - x0 + 1) * (y1 - y0 + 1) * 3 <= w * h
    assert small >= len(recs) // 2


@pytest.mark.parametrize("camera", list(CAMERAS))
def test_special_cameras_get_every_pixel(program, camera):
    recs = run(program, "cornell", "40x30", **CAMERAS[camera])
    everything = [r for r in recs if r["all"] == "1"]
    assert all(r["all"] == r["want_all"] for r in recs)
    if camera == "defocus":
        assert len(everything) == len(recs)
    else:
        assert [r for r in everything if r["kind"] == "box"]
