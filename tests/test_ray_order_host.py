"""Ray orders without a GPU (include/rt.h rt_scene_ray_order): the host twin of the
coherence key (rt_build.cpp rt_host_ray_order, from rt_order.h) against a numpy twin written from the
formula, its stable order against numpy's stable argsort, the new entry points' refusals before any
device call, and the host twin under AddressSanitizer / UBSan as a stand-alone program."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ray_order_cases as OC  # noqa: E402
from raytrace_amd import _lib, scenes  # noqa: E402
from raytrace_amd.query import HIT_DTYPE, RAY_DTYPE  # noqa: E402
from raytrace_amd.radiance import PATH_RAY_DTYPE, RADIANCE_DTYPE  # noqa: E402

P = ctypes.c_void_p
SAN_SRC = os.path.join(ROOT, "tests", "ray_order", "order_san.cpp")
CSRC = os.path.join(ROOT, "raytrace_amd", "csrc")


def host_order(recs, kind):
    L = _lib.load()
    n = len(recs)
    keys, order = np.full(n + 4, 0xA5A5A5A5, np.uint32), np.full(n + 4, 0xA5A5A5A5, np.uint32)
    recs = np.ascontiguousarray(recs)
    assert L.rt_host_ray_order(P(recs.ctypes.data), n, kind, P(keys.ctypes.data), P(order.ctypes.data)) == _lib.RT_OK
    assert (keys[n:] == 0xA5A5A5A5).all() and (order[n:] == 0xA5A5A5A5).all()
    return keys[:n].copy(), order[:n].copy()


# ---- 1. / 2. keys against the twin, the order against a stable argsort
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", OC.BATCHES)
def test_keys_and_order_against_numpy_twin(name, kind):
    o, d = OC.batch(name)
    keys, order = host_order(OC.records(name, kind), kind)
    want = OC.twin_keys(o, d)
    assert keys.dtype == want.dtype and (keys == want).all(), np.flatnonzero(keys != want)[:8]
    assert (order == np.argsort(want, kind="stable").astype(np.uint32)).all()
    ok = keys != OC.KEY_LAST
    assert (keys[ok] < 1 << 30).all()
    distinct = len(np.unique(keys))
    print(f"{name}: {len(keys)} rays, {distinct} distinct keys, {int((~ok).sum())} invalid")
    if name in OC.SCENE_BATCHES:
        assert ok.all() and distinct >= 4000  # (ties are the other batches' business)
    if name == "one_origin":  # every origin bit is constant: the direction's 12 bits alone vary
        assert ok.all() and (keys >> 12 == keys[0] >> 12).all() and 2000 <= distinct < OC.N_BATCH
    if name == "none_valid":
        assert (~ok).all() and (order == np.arange(len(order))).all()
    if name in ("edges", "degenerate_axis"):
        bo, bd = OC.bad_records()
        assert int((~ok).sum()) == len(bo)
        assert (order[-len(bo):] == np.flatnonzero(~ok)).all()  # invalid rays last, in index order
    if name == "degenerate_axis":  # the constant axis is cell 0: bits 1, 4, ... of the origin part are clear
        assert ((keys[ok] >> 12) & 0o222222 == 0).all()


def test_edge_batch_reaches_the_cell_boundaries():
    """The edge batch holds lo + k (hi - lo) / 64 on every axis; on the axes where that product is exact
    (x: 1/16 steps, z: 1/8 steps) the formula puts it in cell min(k, 63) and the value just below it
    one cell lower wherever the subtraction keeps the difference: the inputs sit on the boundaries."""
    o, d = OC.batch("edges")
    lo, hi = np.array([-1.0, 2.0, 0.5]), np.array([3.0, 2.75, 8.5])
    k = np.arange(65)
    grid = lo + k[:, None] * (hi - lo) / 64
    have = {tuple(r) for r in o[np.isfinite(o).all(1)]}
    assert all(tuple(g) in have for g in grid)
    c = OC.cell((grid - lo) * (64.0 / (hi - lo)))
    assert (c[:, 0] == np.minimum(k, 63)).all() and (c[:, 2] == np.minimum(k, 63)).all()
    below = np.nextafter(grid[1:], -np.inf)
    assert all(tuple(b) in have for b in below)
    cb = OC.cell((below - lo) * (64.0 / (hi - lo)))
    for a in (0, 2):  # (where |below| < |lo| the subtraction may round back onto the boundary)
        lower = cb[:, a] == k[:-1]
        assert (lower | (cb[:, a] == np.minimum(k[1:], 63))).all() and lower.any()
    seams = OC.seam_directions()
    assert len(seams) > 60 and (np.abs(seams).sum(1) > 0).all()


# ---- 3. refusals before any device call
def test_argument_checks_need_no_device():
    L = _lib.load()
    ex = _lib.exec_struct()
    lst = _lib.exec_struct(devices=[0])
    cs = _lib.camera_struct(scenes.cornell_box()[0])
    rays, hits = np.zeros(2, RAY_DTYPE), np.zeros(2, HIT_DTYPE)
    prays, out = np.zeros(2, PATH_RAY_DTYPE), np.zeros(2, RADIANCE_DTYPE)
    order, work = np.arange(2, dtype=np.uint32), np.zeros(64, np.uint64)
    rp, hp, pp, up, op, wp = (P(a.ctypes.data) for a in (rays, hits, prays, out, order, work))
    s = P(rays.ctypes.data)  # non-null; the checks below return before it is read
    exp, lstp, csp = ctypes.byref(ex), ctypes.byref(lst), ctypes.byref(cs)
    big = 1 << 31

    def refused(fn, args, msg):
        assert fn(*args) == _lib.RT_E_INVALID and msg in L.rt_last_error(), (fn.__name__, msg, L.rt_last_error())

    # the order calls
    for args, msg in [((None, rp, 2, 0, op), b"scene"), ((s, None, 2, 0, op), b"ray"), ((s, rp, 2, 0, None), b"order"),
                      ((s, rp, -1, 0, op), b"negative"), ((s, rp, big, 0, op), b"2^31"), ((s, rp, 2, 2, op), b"kind"),
                      ((s, rp, 2, -1, op), b"kind")]:
        refused(L.rt_scene_ray_order, args, msg)
        refused(L.rt_scene_ray_order_async, (*args, wp, None), msg)
    refused(L.rt_scene_ray_order_async, (s, rp, 2, 0, op, None, None), b"workspace")
    assert L.rt_scene_ray_order(s, rp, 0, 0, op) == _lib.RT_OK
    assert L.rt_scene_ray_order_async(s, pp, 0, 1, op, wp, None) == _lib.RT_OK
    assert L.rt_ray_order_workspace_bytes(0) > 0
    assert L.rt_ray_order_workspace_bytes(1 << 20) >= 4 * 4 * (1 << 20)
    # the ordered casts
    for args, msg in [((None, exp, rp, hp, 2, 0), b"scene"), ((s, None, rp, hp, 2, 0), b"rt_exec"),
                      ((s, exp, None, hp, 2, 0), b"ray"), ((s, exp, rp, None, 2, 0), b"hit"),
                      ((s, exp, rp, hp, -1, 0), b"negative"), ((s, exp, rp, hp, big, 0), b"2^31"),
                      ((s, exp, rp, hp, 2, 4), b"flags"), ((s, lstp, rp, hp, 2, 0), b"n_devices")]:
        refused(L.rt_scene_cast_ordered, (*args, op), msg)
        refused(L.rt_scene_cast_ordered, (*args, None), msg)
        refused(L.rt_scene_cast_ordered_async, (*args, op, None), msg)
    refused(L.rt_scene_cast_ordered_async, (s, exp, rp, hp, 2, 0, None, None), b"order")
    assert L.rt_scene_cast_ordered(s, exp, rp, hp, 0, 0, None) == _lib.RT_OK
    assert L.rt_scene_cast_ordered_async(s, exp, rp, hp, 0, 3, op, None) == _lib.RT_OK
    # the ordered radiance queries
    for args, msg in [((None, exp, csp, 1, pp, up, wp, 2, 1, 0), b"scene"), ((s, None, csp, 1, pp, up, wp, 2, 1, 0), b"rt_exec"),
                      ((s, exp, None, 1, pp, up, wp, 2, 1, 0), b"camera"), ((s, exp, csp, 1, None, up, wp, 2, 1, 0), b"ray"),
                      ((s, exp, csp, 1, pp, None, wp, 2, 1, 0), b"result"), ((s, exp, csp, 1, pp, up, wp, -1, 1, 0), b"negative"),
                      ((s, exp, csp, 1, pp, up, wp, big, 1, 0), b"item ids"), ((s, exp, csp, 1, pp, up, wp, 2, 0, 0), b"n_samples"),
                      ((s, exp, csp, 1, pp, up, wp, 2, 1, 4), b"flags"), ((s, lstp, csp, 1, pp, up, wp, 2, 1, 0), b"n_devices")]:
        refused(L.rt_scene_radiance_ordered, (*args, op), msg)
        refused(L.rt_scene_radiance_ordered, (*args, None), msg)
        refused(L.rt_scene_radiance_ordered_async, (*args, op, None), msg)
    refused(L.rt_scene_radiance_ordered_async, (s, exp, csp, 1, pp, up, wp, 2, 1, 0, None, None), b"order")
    refused(L.rt_scene_radiance_ordered_async, (s, exp, csp, 1, pp, up, None, 2, 1, 0, op, None), b"workspace")
    assert L.rt_scene_radiance_ordered(s, exp, csp, 1, pp, up, wp, 0, 1, 0, None) == _lib.RT_OK
    assert L.rt_scene_radiance_ordered_async(s, exp, csp, 1, pp, up, wp, 0, 1, 0, op, None) == _lib.RT_OK
    # a host order that is no permutation: refused before the device is touched
    for bad in ([0, 0], [0, 2], [1, 0xFFFFFFFF]):
        b = np.array(bad, np.uint32)
        refused(L.rt_scene_cast_ordered, (s, exp, rp, hp, 2, 0, P(b.ctypes.data)), b"permutation")
        refused(L.rt_scene_radiance_ordered, (s, exp, csp, 1, pp, up, wp, 2, 1, 0, P(b.ctypes.data)), b"permutation")
    # the host twin's own refusals
    assert L.rt_host_ray_order(rp, -1, 0, None, None) == _lib.RT_E_INVALID
    assert L.rt_host_ray_order(rp, big, 0, None, None) == _lib.RT_E_INVALID
    assert L.rt_host_ray_order(rp, 2, 7, None, None) == _lib.RT_E_INVALID
    assert L.rt_host_ray_order(None, 2, 0, None, None) == _lib.RT_E_INVALID
    assert L.rt_host_ray_order(None, 0, 0, None, None) == _lib.RT_OK


def test_names_in_header_library_and_binding():
    names = ["rt_scene_ray_order_async", "rt_scene_ray_order", "rt_scene_cast_ordered_async", "rt_scene_cast_ordered",
             "rt_scene_radiance_ordered_async", "rt_scene_radiance_ordered"]
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "rt.h")).read()
    for n in names:
        assert n in _lib.EXPORTED and hasattr(L, n) and n + "(" in header, n
    assert "rt_ray_order_workspace_bytes" in _lib.SIZE_FUNCTIONS and "rt_ray_order_workspace_bytes(" in header
    assert "rt_host_ray_order" not in header and "rt_order_sort_keys_async" not in header
    assert _lib.RT_ORDER_RAYS == 0 and _lib.RT_ORDER_PATH_RAYS == 1
    assert "#define RT_ORDER_RAYS 0" in header and "#define RT_ORDER_PATH_RAYS 1" in header
    assert L.rt_abi_version() == 6


def test_python_front_end_without_a_device():
    import inspect
    import raytrace_amd as R
    from raytrace_amd import query, radiance
    for fn, names in [(R.DeviceScene.cast, ("reorder", "order")), (R.DeviceScene.radiance, ("reorder", "order")),
                      (R.DeviceScene.cast_async, ("order_ptr",)), (R.DeviceScene.radiance_async, ("order_ptr",)),
                      (query.cast_records, ("reorder", "order")), (radiance.radiance_records, ("reorder", "order"))]:
        sig = inspect.signature(fn).parameters
        for n in names:
            assert n in sig and sig[n].default in (False, None, 0), (fn, n)
    assert hasattr(R.DeviceScene, "ray_order") and hasattr(R.DeviceScene, "ray_order_async")
    with pytest.raises(ValueError):
        query.order_arg(np.arange(3), 4)
    assert query.order_arg([1, 0], 2).dtype == np.uint32


# ---- 4. the host twin under AddressSanitizer / UBSan, a stand-alone program
def test_host_twin_under_sanitizers(tmp_path):
    exe = str(tmp_path / "order_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
                        "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SAN_SRC,
                        os.path.join(CSRC, "rt_build.cpp"), os.path.join(CSRC, "rt_bvh.cpp"), "-lm", "-pthread"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    for name in OC.EDGE_BATCHES + ["one_origin"]:
        for kind in (0, 1):
            recs = OC.records(name, kind)
            src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
            with open(src, "wb") as f:
                f.write(np.array([len(recs), kind], np.int64).tobytes())
                f.write(np.ascontiguousarray(recs).tobytes())
            r = subprocess.run([exe, src, dst], capture_output=True, text=True)
            assert r.returncode == 0 and r.stdout.startswith("ok ") and "ERROR" not in r.stderr and \
                "runtime error" not in r.stderr, (name, kind, r.stdout[-500:], r.stderr[-4000:])
            got = np.fromfile(dst, np.uint32)
            want = OC.twin_keys(*OC.batch(name))
            assert (got[:len(recs)] == want).all(), (name, kind)
            assert (got[len(recs):] == np.argsort(want, kind="stable")).all(), (name, kind)
