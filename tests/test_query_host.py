"""The ray queries (include/rt.h rt_scene_cast) without a GPU: the per-ray body's host build
(tests/query_emu: raytrace_amd/csrc/rt_query.h over rt_trace.h) against closed forms and against the
long-double evaluator tests/query_ref.py under the bars of tests/query_cases.py, the same body as a
stand-alone program under AddressSanitizer / UBSan, and the C ABI's records, symbols and argument checks."""
import ctypes
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "query_emu"))
import query_cases as QC  # noqa: E402
import query_emu as QE  # noqa: E402
import raytrace_amd as R  # noqa: E402
from raytrace_amd import _lib  # noqa: E402
from raytrace_amd.query import HIT_DTYPE, RAY_DTYPE, make_rays  # noqa: E402

PRECISIONS = ["f64", "f32"]
GREY = R.lambertian(R.constantTexture(0.5))
RED = R.metal(0.1, R.constantTexture(R.V3(0.9, 0.1, 0.1)))


def eps_of(precision):
    return float(np.finfo(np.float64 if precision == "f64" else np.float32).eps)


def cast(world, o, d, precision, tmin=1e-4, tmax=np.inf, time=0.0, **kw):
    hits, _ = QE.cast(world, make_rays(o, d, tmin, tmax, time), precision, **kw)
    return hits


# ---- 1. closed forms
@pytest.mark.parametrize("precision", PRECISIONS)
def test_sphere_closed_forms(precision):
    """A sphere of radius 2 at (1, 2, 3) seen from outside along -z (front hit, t = 3, normal +z) and from
    its centre (the far root: t = r, front == 0, the normal faces the ray); uv at points away from the
    seam and the poles: sphereUV(n) = (atan2(n.x, n.z) / 2 pi + 1/2, acos(-n.y) / pi)."""
    e = eps_of(precision)
    world = GREY << R.sphere((1, 2, 3), 2)
    h = cast(world, [(1, 2, 8), (1, 2, 3), (1, 2, 3), (6, 2, 3)], [(0, 0, -2), (0, 0, 1), (1, 0, 0), (-1, 0, 0)], precision)
    assert (h["hit"] == 1).all()
    np.testing.assert_allclose(h["t"], [3, 2, 2, 3], rtol=8 * e)
    np.testing.assert_allclose(h["point"], [(1, 2, 5), (1, 2, 5), (3, 2, 3), (3, 2, 3)], atol=32 * e)
    np.testing.assert_allclose(h["normal"], [(0, 0, 1), (0, 0, -1), (-1, 0, 0), (1, 0, 0)], atol=8 * e)
    assert h["front"].tolist() == [1, 0, 0, 1]
    # outward normals (0,0,1), (0,0,1), (1,0,0), (1,0,0): u = 1/2, 1/2, 3/4, 3/4; v = 1/2
    np.testing.assert_allclose(h["uv"], [(0.5, 0.5), (0.5, 0.5), (0.75, 0.5), (0.75, 0.5)], atol=8 * e)
    assert (h["leaf"] == 0).all() and (h["instance"] == -1).all() and (h["material"] == 0).all()
    # a ray that starts inside, off-centre, hits the far root from behind
    h = cast(world, [(1, 2, 4)], [(0, 0, 1)], precision)
    assert h["hit"][0] == 1 and h["front"][0] == 0 and abs(h["t"][0] - 1) <= 8 * e
    # an oblique outward normal: (0.6, 0, 0.8) -> u = atan2(0.6, 0.8) / 2 pi + 1/2
    h = cast(world, [(1 + 0.6 * 5, 2, 3 + 0.8 * 5)], [(-0.6, 0, -0.8)], precision)
    assert abs(h["uv"][0, 0] - (math.atan2(0.6, 0.8) / (2 * math.pi) + 0.5)) <= 16 * e and abs(h["t"][0] - 3) <= 16 * e


@pytest.mark.parametrize("precision", PRECISIONS)
def test_plane_shape_closed_forms(precision):
    """A parallelogram and a triangle (with its own texture coordinates): front and back hits, t, the
    facing normal, and uv exactly at chosen points (a = 1/4, b = 1/2 are exact in both precisions)."""
    e = eps_of(precision)
    quad = GREY << R.parallelogram((0, 0, 0), (4, 0, 0), (0, 2, 0))  # normal +z
    h = cast(quad, [(1, 1, 3), (1, 1, -3), (5, 1, 3)], [(0, 0, -1), (0, 0, 3), (0, 0, -1)], precision)
    assert h["hit"].tolist() == [1, 1, 0] and h["front"][:2].tolist() == [1, 0]
    assert (h["t"][:2] == 3).all() and h["t"][2] == np.inf
    assert h["normal"][:2].tolist() == [[0, 0, 1], [0, 0, -1]]
    assert h["uv"][:2].tolist() == [[0.25, 0.5], [0.25, 0.5]]
    assert h["point"][:2].tolist() == [[1, 1, 0], [1, 1, 0]]
    tri = RED << R.triangle(((0, 0, 0), (0, 0)), ((4, 0, 0), (1, 0)), ((0, 4, 0), (0.5, 1)))
    h = cast(tri, [(1, 2, 2), (1, 2, -2), (3, 3, 2)], [(0, 0, -1), (0, 0, 1), (0, 0, -1)], precision)
    assert h["hit"].tolist() == [1, 1, 0] and h["front"][:2].tolist() == [1, 0]
    np.testing.assert_allclose(h["t"][:2], 2, rtol=4 * e)
    # a = 1/4, b = 1/2: uv = 1/4 (0, 0) + 1/4 (1, 0) + 1/2 (0.5, 1) = (0.5, 0.5)
    np.testing.assert_allclose(h["uv"][:2], [(0.5, 0.5)] * 2, atol=4 * e)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_cuboid_closed_forms(precision):
    """A cuboid (six parallelograms, a box group in the kernel): from outside the entry face is hit on
    its front side; from inside the exit face is hit from behind (front == 0, the normal turned to face
    the ray); leaf is the face's position in `cuboid`'s list (front, back, left, right, top, bottom)."""
    e = eps_of(precision)
    box = GREY << R.cuboid(((0, 2), (0, 3), (0, 4)))
    h = cast(box, [(1, 1, 9), (1, 1, 1), (-5, 1, 1), (1, 1, 1)], [(0, 0, -1), (0, 0, 1), (1, 0, 0), (0, -1, 0)], precision)
    assert (h["hit"] == 1).all()
    np.testing.assert_allclose(h["t"], [5, 3, 5, 1], rtol=8 * e)
    assert h["leaf"].tolist() == [0, 0, 2, 5]  # front (z = zmax), front again from inside, left, bottom
    assert h["front"].tolist() == [1, 0, 1, 0]
    np.testing.assert_allclose(h["normal"], [(0, 0, 1), (0, 0, -1), (-1, 0, 0), (0, 1, 0)], atol=4 * e)
    np.testing.assert_allclose(h["uv"][0], (0.5, 1 / 3), atol=8 * e)


# ---- 2. interval semantics
@pytest.mark.parametrize("precision", PRECISIONS)
def test_interval_is_open_at_both_ends(precision):
    """A sphere's near root at t0 = 3 (far root 7), all values exact in both precisions."""
    world = GREY << R.sphere((0, 0, -5), 2)
    up = {"f64": np.nextafter(3.0, 4.0), "f32": float(np.nextafter(np.float32(3), np.float32(4)))}[precision]
    dn = {"f64": np.nextafter(3.0, 2.0), "f32": float(np.nextafter(np.float32(3), np.float32(2)))}[precision]
    tmin = [1e-4, 1e-4, dn, 3.0, 0.0, 0.0, 3.0]
    tmax = [up, 3.0, np.inf, np.inf, np.inf, 8.0, 7.0]
    h = cast(world, [(0, 0, 0)] * 7, [(0, 0, -1)] * 7, precision, tmin=np.array(tmin), tmax=np.array(tmax))
    assert h["hit"].tolist() == [1, 0, 1, 1, 1, 1, 0]
    assert h["t"].tolist() == [3, np.inf, 3, 7, 3, 3, np.inf]  # tmin == t0 finds the far root instead
    assert h["front"][3] == 0 and h["front"][0] == 1


# ---- 3. malformed rays
@pytest.mark.parametrize("precision", PRECISIONS)
def test_malformed_rays_are_flagged_and_neighbours_correct(precision):
    world = GREY << R.sphere((0, 0, -5), 2)
    rays = make_rays([(0, 0, 0)] * 15, [(0, 0, -1)] * 15)
    bad = {1: ("origin", (np.nan, 0, 0)), 3: ("dir", (0, 0, 0)), 5: ("tmin", -1e-9), 7: ("tmax", 1e-4), 9: ("time", 1.5),
           10: ("time", -0.25), 11: ("dir", (0, np.inf, 0)), 12: ("tmax", np.nan), 13: ("tmax", 5e-5)}
    for i, (f, v) in bad.items():
        rays[f][i] = v
    for any_hit in (False, True):
        h, _ = QE.cast(world, rays, precision, any_hit=any_hit)
        want = np.array([-1 if i in bad else 1 for i in range(15)])
        assert (h["hit"] == want).all(), h["hit"]
        assert (h["t"][want == 1] == 3).all()


# ---- 4. the host build against query_ref
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", QC.SCENES)
def test_host_build_against_reference(name, precision):
    """512 rays per scene under the bars of tests/query_cases.py (its docstring has the excluded shares
    measured with this evaluator: cornell_box 3.12 % / 3.71 % at m = 1e-6 / 1e-3, box_gallery 1.17 / 1.56,
    demo1 0 / 0.20, bunny_cornell 0 / 0.59, pawn_instances 0 / 0.20, demo1_moving 0 / 0.39; the cap is 5 %).
    Worst error over bar measured on the host build, binary64 / FP32: t 0.046 / 0.040, point 0.032 / 0.029,
    uv 0.031 / 0.029; | |n|^2 - 1 | at most 2.4 eps, plane normals within 1.1 eps."""
    hits, variant = QE.cast(QC.world_of(name), QC.ray_records(name), precision)
    if name == "pawn_instances":
        assert variant & QC.RT_VAR_INST and len(QC.flat_of(name).instances) == 3
    if name in ("cornell_box",):
        assert (variant & QC.RT_VAR_BASE) == 0  # the flat class
    QC.check_against_ref(hits, name, precision, variant)


# ---- 5. time
@pytest.mark.parametrize("precision", PRECISIONS)
def test_moving_sphere_follows_time(precision):
    """moving v0 v1 at time 0, 1/2 and 1: the sphere sits at c + (1 - time) v0 + time v1, with time kept
    in 24 bits (floor(time 2^24) / 2^24; a time of 1 is 1 - 2^-24)."""
    e = eps_of(precision)
    world = GREY << R.moving((0, 0, 0), (0, 0, -4), R.sphere((0, 0, -5), 1))
    times = np.array([0.0, 0.5, 1.0, 0.5 + 2.0 ** -25])
    h = cast(world, [(0, 0, 0)] * 4, [(0, 0, -1)] * 4, precision, time=times)
    q = np.minimum(np.floor(times * 2 ** 24), 2 ** 24 - 1) / 2 ** 24
    want = 4 + 4 * q
    assert (h["hit"] == 1).all()
    np.testing.assert_allclose(h["t"], want, rtol=8 * e)
    assert want[2] == 8 - 4 * 2.0 ** -24 and want[3] == want[1]  # the documented quantisation
    if precision == "f64":
        assert h["t"][2] < 8 and h["t"][3] == h["t"][1]


# ---- 6. any-hit, 7. no-UV
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", QC.SCENES)
def test_any_hit_and_no_uv(name, precision):
    rays = QC.ray_records(name)
    rays["tmax"][::3] = 0.75 * float(np.abs(np.array(QC.leaves_of(name).box)).max())  # finite ends too
    world = QC.world_of(name)
    full, _ = QE.cast(world, rays, precision)
    anyh, _ = QE.cast(world, rays, precision, any_hit=True)
    assert (anyh["hit"] == full["hit"]).all()
    h = full["hit"] == 1
    assert h.any() and (~h).any()
    assert ((anyh["t"] > rays["tmin"]) & (anyh["t"] < rays["tmax"]) & (anyh["t"] >= full["t"]))[h].all()
    nouv, _ = QE.cast(world, rays, precision, uv=False)
    assert (nouv["uv"] == 0).all()
    for f in HIT_DTYPE.names:
        if f != "uv":
            assert nouv[f].tobytes() == full[f].tobytes(), f


def test_stack_overflow_path_on_host_build(knobs):
    """Fewer stack rows than the BVH needs (the test knob RT_AMD_CAST_STACK, as the device's cast reads
    it): the defined error path, RT_E_STACK, and nothing of the kind without the knob."""
    world, rays = QC.deep_scene(), QC.deep_rays()
    for precision in PRECISIONS:
        hits, _, rc = QE.cast(world, rays, precision, want_rc=True)
        assert rc == 0 and (hits["hit"] == 1).sum() > 20
    knobs.setenv("RT_AMD_CAST_STACK", "2")
    for precision in PRECISIONS:
        assert QE.cast(world, rays, precision, want_rc=True)[2] == _lib.RT_E_STACK


# ---- 8. the per-ray body under AddressSanitizer / UBSan, as a stand-alone program
def test_query_body_under_sanitizers(tmp_path):
    emu_dir = os.path.join(ROOT, "tests", "query_emu")
    r = subprocess.run(["make", "-C", emu_dir, "-s", "-j4", "_build/query_host_san"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    exe = os.path.join(emu_dir, "_build", "query_host_san")
    rng = np.random.default_rng(5)
    n = 300
    o = rng.uniform(-9, 9, (n, 3)) * [1, 0.3, 1] + [0, 3, 0]
    tgt = rng.uniform(-7, 7, (n, 3)) * [1, 0.1, 1]
    rays = make_rays(o, tgt - o, time=rng.integers(0, 2 ** 24, n) / 2.0 ** 24)
    rays["dir"][7] = 0
    rays["origin"][9] = np.nan
    rays["tmax"][11:40] = 6.0
    rays_path, hits_path = str(tmp_path / "rays.bin"), str(tmp_path / "hits.bin")
    rays.tofile(rays_path)
    for n_small, flat in ((0, True), (81, False)):  # the flat class; a sphere BVH with a prefix and motion
        for f64 in (1, 0):
            for flags in (1, 0, 3):
                r = subprocess.run([exe, rays_path, hits_path, str(f64), str(flags), str(n_small)], capture_output=True, text=True)
                assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
                variant = int(r.stdout.split()[-1])
                assert ((variant & 3) == 0) == flat
                hits = np.fromfile(hits_path, HIT_DTYPE)
                assert len(hits) == n and hits["hit"][7] == -1 and hits["hit"][9] == -1
                assert (hits["hit"] == 1).sum() > n // 4


# ---- 9. ABI
C_LAYOUT = r"""
#include <stdio.h>
#include <stddef.h>
#include "rt.h"
#define P(T) printf(#T " %zu\n", sizeof(T))
#define O(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  P(rt_ray); O(rt_ray, origin); O(rt_ray, dir); O(rt_ray, tmin); O(rt_ray, tmax); O(rt_ray, time); O(rt_ray, reserved);
  P(rt_hit); O(rt_hit, t); O(rt_hit, point); O(rt_hit, normal); O(rt_hit, uv); O(rt_hit, hit); O(rt_hit, front);
  O(rt_hit, leaf); O(rt_hit, instance); O(rt_hit, material); O(rt_hit, reserved);
  printf("flags %d %d\n", RT_QUERY_UV, RT_QUERY_ANY_HIT);
  return 0;
}
"""
RAY_OFFSETS = dict(origin=0, dir=24, tmin=48, tmax=56, time=64, reserved=72)
HIT_OFFSETS = dict(t=0, point=8, normal=32, uv=56, hit=72, front=76, leaf=80, instance=84, material=88, reserved=92)


def test_record_layouts_and_symbols():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write(C_LAYOUT)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    lines = out.strip().splitlines()
    assert lines[-1] == f"flags {_lib.RT_QUERY_UV} {_lib.RT_QUERY_ANY_HIT}" == "flags 1 2"
    c = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in lines[:-1])}
    assert c["rt_ray"] == 80 == RAY_DTYPE.itemsize == ctypes.sizeof(_lib.RtRay)
    assert c["rt_hit"] == 96 == HIT_DTYPE.itemsize == ctypes.sizeof(_lib.RtHit)
    for f, off in RAY_OFFSETS.items():
        assert c[f"rt_ray.{f}"] == off == RAY_DTYPE.fields[f][1] == getattr(_lib.RtRay, f).offset, f
    for f, off in HIT_OFFSETS.items():
        assert c[f"rt_hit.{f}"] == off == HIT_DTYPE.fields[f][1] == getattr(_lib.RtHit, f).offset, f
    L = _lib.load()
    for name in ("rt_scene_cast", "rt_scene_cast_async", "rt_scene_cast_status"):
        assert name in _lib.EXPORTED and hasattr(L, name)


def test_argument_checks_need_no_device():
    """Null arguments and a negative count are RT_E_INVALID before any device call (the scene handle
    is never dereferenced: a dummy non-null value stands for it), with rt_last_error naming the
    argument; unknown flags and a device list likewise."""
    L = _lib.load()
    ex = _lib.exec_struct()
    rays, hits = np.zeros(2, RAY_DTYPE), np.zeros(2, HIT_DTYPE)
    rp, hp, exp = rays.ctypes.data, hits.ctypes.data, ctypes.byref(ex)
    s = ctypes.c_void_p(rp)  # non-null; the checks below return before it is read
    P = ctypes.c_void_p
    for args, msg in [((None, exp, P(rp), P(hp), 2, 0), b"scene"), ((s, None, P(rp), P(hp), 2, 0), b"rt_exec"),
                      ((s, exp, None, P(hp), 2, 0), b"ray"), ((s, exp, P(rp), None, 2, 0), b"hit"),
                      ((s, exp, P(rp), P(hp), -1, 0), b"negative"), ((s, exp, P(rp), P(hp), 2, 4), b"flags")]:
        assert L.rt_scene_cast(*args) == _lib.RT_E_INVALID and msg in L.rt_last_error(), (msg, L.rt_last_error())
        assert L.rt_scene_cast_async(*args, None) == _lib.RT_E_INVALID and msg in L.rt_last_error(), msg
    assert L.rt_scene_cast(s, exp, P(rp), P(hp), 0, 0) == _lib.RT_OK
    assert L.rt_scene_cast_async(s, exp, P(rp), P(hp), 0, 3, None) == _lib.RT_OK
    assert L.rt_scene_cast_status(None, None) == _lib.RT_E_INVALID
    lst = _lib.exec_struct(devices=[0])
    assert L.rt_scene_cast(s, ctypes.byref(lst), P(rp), P(hp), 2, 0) == _lib.RT_E_INVALID and b"n_devices" in L.rt_last_error()


def test_python_front_end_without_a_device():
    """make_rays broadcasts, the dtypes are exported, and a cast fails loudly without a GPU."""
    r = make_rays((0, 0, 0), np.zeros((5, 3)) + (0, 0, 1), tmax=np.arange(5) + 1.0)
    assert r.shape == (5,) and r["tmax"].tolist() == [1, 2, 3, 4, 5] and (r["tmin"] == 1e-4).all()
    assert R.RAY_DTYPE is RAY_DTYPE and R.HIT_DTYPE is HIT_DTYPE
    with pytest.raises(ValueError):
        make_rays(np.zeros((2, 2, 3)), (0, 0, 1))
    flat = R.flatten(QC.world_of("cornell_box"))
    assert len(flat.material_objects) == len(flat.materials)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(R.RtDeviceError):
            R.cast(QC.world_of("cornell_box"), (278, 278, -800), (0, 0, 1))
