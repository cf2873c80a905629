"""The ray queries (include/rt.h rt_scene_cast, DeviceScene.cast) on the GPU: the device against the
host build of the same body (tests/query_emu) and against the long-double evaluator tests/query_ref.py
under the bars of tests/query_cases.py; the launch shape, determinism, any-hit and no-UV, coexistence
with a film, and the traversal-stack error path."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "query_emu"))
import query_cases as QC  # noqa: E402
import query_emu as QE  # noqa: E402
import raytrace_amd as R  # noqa: E402
from raytrace_amd import _lib, query, scenes  # noqa: E402
from raytrace_amd.query import HIT_DTYPE, RAY_DTYPE  # noqa: E402

PRECISIONS = ["f64", "f32"]
INT_FIELDS = ("hit", "leaf", "front", "instance", "material")
REAL_FIELDS = ("t", "point", "normal", "uv")


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    return torch


@functools.lru_cache(None)
def device_scene(name):
    return R.DeviceScene(QC.flat_of(name))


@functools.lru_cache(None)
def device_hits(name, precision):
    return query.cast_records(device_scene(name), QC.ray_records(name), precision)


@functools.lru_cache(None)
def host_hits(name, precision):
    return QE.cast(QC.flat_of(name), QC.ray_records(name), precision)


def cast_on_stream(torch, scene, rays, precision="f64", guard=0, **kw):
    """rt_scene_cast_async on a stream of the caller's, from and to torch device buffers; `guard` extra
    hit records behind the output, pre-filled with 0xA5 bytes.  Returns (hits, guard bytes)."""
    n = len(rays)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1).copy()).cuda()
    d_hits = torch.full(((n + guard) * HIT_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the fill above ran on the default stream
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        scene.cast_async(d_rays.data_ptr(), d_hits.data_ptr(), n, st.cuda_stream, precision=precision, **kw)
    st.synchronize()
    out = d_hits.cpu().numpy()
    return out[:n * HIT_DTYPE.itemsize].view(HIT_DTYPE).copy(), out[n * HIT_DTYPE.itemsize:]


# ---- 1. the device against the host build
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", QC.SCENES)
def test_device_matches_host_build(gpu, name, precision):
    """The integer fields are equal on included rays; binary64 reals within 1e-9 relative on the
    max(|ref|, 1e-3) scale for at least 99.9 % of included rays (the bar of
    test_device_guides_match_host_build); FP32 within the query_ref bars."""
    dev = device_hits(name, precision)
    host, variant = host_hits(name, precision)
    _, inc, _ = QC.reference(name, precision)
    for f in INT_FIELDS:
        assert (dev[f] == host[f])[inc].all(), (f, np.flatnonzero((dev[f] != host[f]) & inc)[:8])
    if precision == "f64":
        h = inc & (host["hit"] == 1)
        bad = np.zeros(len(dev), bool)
        for f in REAL_FIELDS:
            a, b = dev[f].reshape(len(dev), -1)[h], host[f].reshape(len(dev), -1)[h]
            bad[h] |= (np.abs(a - b) > 1e-9 * np.maximum(np.abs(b), 1e-3)).any(1)
        share = float(bad[h].mean())
        print(f"{name}: binary64 device vs host build, {100 * share:.3f} % of included hits beyond 1e-9")
        assert share <= 0.001, share
    else:
        QC.check_against_ref(dev, name, precision, variant)


# ---- 2. the device against query_ref directly
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["cornell_box", "pawn_instances"])
def test_device_against_reference(gpu, name, precision):
    QC.check_against_ref(device_hits(name, precision), name, precision, host_hits(name, precision)[1])


# ---- 3. launch shape
@pytest.mark.parametrize("precision", PRECISIONS)
def test_launch_shape_prefixes_and_guard(gpu, precision):
    """n = 1, 63, 64, 65 and 1000 rays: every shorter call's result is, byte for byte, the prefix of
    the 1000-ray result, and four hit records of guard bytes behind d_hits are untouched."""
    name = "bunny_cornell"
    rays = QC.ray_records(name, 1000)
    scene = device_scene(name)
    full, g = cast_on_stream(gpu, scene, rays, precision, guard=4)
    assert (g == 0xA5).all() and len(g) == 4 * HIT_DTYPE.itemsize
    assert (full["hit"] == 1).sum() > 500
    for n in (1, 63, 64, 65):
        part, g = cast_on_stream(gpu, scene, rays[:n], precision, guard=4)
        assert (g == 0xA5).all()
        assert part.tobytes() == full[:n].tobytes(), n


# ---- 4. determinism
@pytest.mark.parametrize("name", ["cornell_box", "pawn_instances"])
def test_casts_are_deterministic_sync_and_async(gpu, name):
    for precision in PRECISIONS:
        sync = device_hits(name, precision)
        asyn, _ = cast_on_stream(gpu, device_scene(name), QC.ray_records(name), precision)
        assert sync.tobytes() == asyn.tobytes()
        assert not device_scene(name).cast_overflowed()


# ---- 5. any-hit and no-UV
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", QC.SCENES)
def test_any_hit_and_no_uv_on_device(gpu, name, precision):
    rays = QC.ray_records(name)
    rays["tmax"][::3] = 0.75 * float(np.abs(np.array(QC.leaves_of(name).box)).max())
    scene = device_scene(name)
    full = query.cast_records(scene, rays, precision)
    anyh = query.cast_records(scene, rays, precision, any_hit=True)
    assert (anyh["hit"] == full["hit"]).all()
    h = full["hit"] == 1
    assert h.any() and (~h).any()
    assert ((anyh["t"] > rays["tmin"]) & (anyh["t"] < rays["tmax"]) & (anyh["t"] >= full["t"]))[h].all()
    nouv = query.cast_records(scene, rays, precision, uv=False)
    assert (nouv["uv"] == 0).all()
    for f in HIT_DTYPE.names:
        if f != "uv":
            assert nouv[f].tobytes() == full[f].tobytes(), f


def test_python_cast_dict_and_malformed_rays(gpu):
    """DeviceScene.cast: broadcasting, the dict's fields, misses at t = inf, a malformed ray flagged
    invalid with its neighbours correct, `materials` mapping the index back, and the one-shot form."""
    world = QC.world_of("cornell_box")
    scene = device_scene("cornell_box")
    d = np.array([(0, 0, 1), (0, 0, 1), (0, 0, 0), (0, 0, -1)], float)
    h = scene.cast((30, 540, -800), d)
    assert h["hit"].tolist() == [True, True, False, False] and h["valid"].tolist() == [True, True, False, True]
    assert h["t"][3] == np.inf and h["t"][2] == np.inf
    assert abs(h["t"][0] - 1355) < 1e-9  # through the open front, above the blocks, to the back wall at z = 555
    assert np.abs(h["normal"][0] - (0, 0, -1)).max() == 0 and np.abs(h["point"][0] - (30, 540, 555)).max() < 1e-9
    assert scene.materials[h["material"][0]].kind == R.lambertian(R.constantTexture(0.5)).kind
    one = R.cast(world, (30, 540, -800), d, precision="f32")
    assert one["hit"].tolist() == h["hit"].tolist() and abs(one["t"][0] - 1355) < 1e-3


# ---- 6. coexistence with a film
def test_cast_between_film_passes(gpu):
    cs, world, seed = scenes.cornell_box(spp=1, width=32)
    scene = R.DeviceScene(world)
    rays = QC.ray_records("cornell_box")
    before = query.cast_records(scene, rays, "f64")
    a = R.Film(scene, cs, seed)
    a.add(2)
    between = query.cast_records(scene, rays, "f64")
    between32 = query.cast_records(scene, rays, "f32")
    state = a.add(3).state()
    after = query.cast_records(scene, rays, "f64")
    b = R.Film(R.DeviceScene(world), cs, seed)
    assert b.add(2).add(3).state().tobytes() == state.tobytes()
    assert before.tobytes() == between.tobytes() == after.tobytes()
    assert (between32["hit"] == between["hit"]).mean() > 0.95


# ---- 7. the traversal-stack error path
def test_stack_overflow_is_reported(gpu, knobs):
    """The library sizes a cast's traversal stacks by the scene's own BVH depth (a scene deeper than the
    64 rows the kernels accept is refused when it is built, with RT_E_STACK), so an overflow needs fewer
    rows than the scene's depth: the experiment knob RT_AMD_CAST_STACK gives a cast 2.  The sync call
    then returns RT_E_STACK, rt_scene_cast_status reports and clears the async call's word, and the
    same casts without the knob overflow nothing and agree with the host build."""
    world = QC.deep_scene()
    scene = R.DeviceScene(world)
    assert scene.stats()["max_stack"] >= 20
    n = 256
    rays = QC.deep_rays(n)
    good = query.cast_records(scene, rays, "f64")
    host, _ = QE.cast(world, rays, "f64")
    assert (good["hit"] == host["hit"]).all() and (good["leaf"] == host["leaf"]).all()
    knobs.setenv("RT_AMD_CAST_STACK", "2")
    hits = np.zeros(n, HIT_DTYPE)
    for precision in PRECISIONS:
        ex = _lib.exec_struct(precision=precision)
        rc = scene._lib.rt_scene_cast(scene.handle, ctypes.byref(ex), rays.ctypes.data_as(ctypes.c_void_p),
                                      hits.ctypes.data_as(ctypes.c_void_p), n, 1)
        assert rc == _lib.RT_E_STACK and b"stack" in scene._lib.rt_last_error()
        assert not scene.cast_overflowed()  # the synchronous call's word is its own
        cast_on_stream(gpu, scene, rays, precision)
        assert scene.cast_overflowed() and not scene.cast_overflowed()
    knobs.delenv("RT_AMD_CAST_STACK")
    again, _ = cast_on_stream(gpu, scene, rays, "f64")
    assert again.tobytes() == good.tobytes() and not scene.cast_overflowed()
