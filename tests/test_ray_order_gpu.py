"""Ray orders on the GPU (include/rt.h rt_scene_ray_order, rt_scene_cast_ordered,
rt_scene_radiance_ordered): the radix sort alone against numpy's stable argsort, the
device's keys and order against the host twin, and the ordered queries against the unordered ones
byte for byte — only the grouping of rays into waves may differ."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tests"))
import query_cases as QC  # noqa: E402
import ray_order_cases as OC  # noqa: E402
import raytrace_amd as R  # noqa: E402
from raytrace_amd import _lib, query  # noqa: E402
from raytrace_amd import radiance as rad  # noqa: E402
from raytrace_amd.query import HIT_DTYPE  # noqa: E402
from raytrace_amd.radiance import RADIANCE_DTYPE  # noqa: E402
from test_adaptive_gpu import PRECISIONS, scene  # noqa: E402

P = ctypes.c_void_p
GUARD = 256


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    return torch


def to_device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def guarded(torch, nbytes):
    """nbytes + GUARD bytes of 0xA5 on the device"""
    return torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")


# ---- 5. the sort alone
def tile():
    return int(_lib.load().rt_ray_order_tile())


def sort_sizes():
    T = tile()
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17, 257 * T + 1]


def key_set(kind, n, rng):
    if kind == "all_equal":
        return np.full(n, 0x2ABCDEF1, np.uint32)
    if kind == "ascending":
        return (np.arange(n, dtype=np.uint64) * ((1 << 30) // max(n, 1))).astype(np.uint32)
    if kind == "descending":
        return key_set("ascending", n, rng)[::-1].copy()
    if kind == "top_digit":
        return (rng.integers(0, 64, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00C0FFEE)
    if kind == "bottom_digit":
        return rng.integers(0, 256, n).astype(np.uint32) | np.uint32(0x15A5A500)
    if kind == "all_but_one":
        k = np.full(n, 0x0D15EA5E, np.uint32)
        if n:
            k[int(rng.integers(0, n))] ^= np.uint32(0x00003100)  # (another value of the second digit)
        return k
    if kind == "random30":
        return rng.integers(0, 1 << 30, n).astype(np.uint32)
    if kind == "random_with_last":
        k = rng.integers(0, 1 << 30, n).astype(np.uint32)
        k[rng.random(n) < 0.1] = OC.KEY_LAST
        return k
    raise KeyError(kind)


KEY_SETS = ["all_equal", "ascending", "descending", "top_digit", "bottom_digit", "all_but_one", "random30", "random_with_last"]


def device_sort(torch, keys):
    """rt_order_sort_keys_async on a stream of the caller's: (order, keys after, guards intact)"""
    L = _lib.load()
    n = len(keys)
    d_keys = to_device(torch, keys) if n else torch.zeros(4, dtype=torch.uint8, device="cuda")
    ws_bytes = int(L.rt_ray_order_workspace_bytes(n))
    d_order, d_ws = guarded(torch, 4 * n), guarded(torch, ws_bytes)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        rc = L.rt_order_sort_keys_async(0, P(d_keys.data_ptr()), n, P(d_order.data_ptr()), P(d_ws.data_ptr()), P(st.cuda_stream))
    st.synchronize()
    assert rc == _lib.RT_OK, L.rt_last_error()
    order = d_order.cpu().numpy()
    intact = bool((order[4 * n:] == 0xA5).all() and (d_ws[ws_bytes:].cpu().numpy() == 0xA5).all())
    after = d_keys.cpu().numpy()[:4 * n].view(np.uint32)
    return order[:4 * n].view(np.uint32).copy(), after, intact


@pytest.mark.parametrize("kind", KEY_SETS)
def test_sort_is_numpys_stable_argsort(gpu, kind):
    """Every size at which a tail tile, a wave boundary or the scan across tiles (more than 256 of
    them) can go wrong; guard bytes behind the order and the workspace, the keys unchanged, and two
    runs of every case equal byte for byte."""
    assert tile() % 64 == 0 and tile() >= 256
    rng = np.random.default_rng(KEY_SETS.index(kind) + 100)
    for n in sort_sizes():
        keys = key_set(kind, n, rng)
        want = np.argsort(keys, kind="stable").astype(np.uint32)
        a, after, intact = device_sort(gpu, keys)
        assert intact, (kind, n)
        assert (after == keys).all(), (kind, n)
        assert (a == want).all(), (kind, n, np.flatnonzero(a != want)[:8])
        b, _, intact = device_sort(gpu, keys)
        assert intact and a.tobytes() == b.tobytes(), (kind, n)


# ---- 6. the device's order against the host twin
@functools.lru_cache(None)
def cornell():
    return R.DeviceScene(QC.flat_of("cornell_box"))


def device_order(torch, recs, kind):
    L = _lib.load()
    n = len(recs)
    d_rays = to_device(torch, recs) if n else torch.zeros(4, dtype=torch.uint8, device="cuda")
    ws_bytes = int(L.rt_ray_order_workspace_bytes(n))
    d_order, d_ws = guarded(torch, 4 * n), guarded(torch, ws_bytes)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        cornell().ray_order_async(d_rays.data_ptr(), n, d_order.data_ptr(), d_ws.data_ptr(), st.cuda_stream, path_rays=kind == 1)
    st.synchronize()
    order = d_order.cpu().numpy()
    assert (order[4 * n:] == 0xA5).all() and (d_ws[ws_bytes:].cpu().numpy() == 0xA5).all()
    keys = d_ws.cpu().numpy()[:4 * n].view(np.uint32).copy()  # (the workspace starts with the records' keys)
    return order[:4 * n].view(np.uint32).copy(), keys, d_order


def host_order(recs, kind):
    L = _lib.load()
    n = len(recs)
    keys, order = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    recs = np.ascontiguousarray(recs)
    assert L.rt_host_ray_order(P(recs.ctypes.data), n, kind, P(keys.ctypes.data), P(order.ctypes.data)) == _lib.RT_OK
    return keys, order


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", OC.BATCHES)
def test_device_order_is_the_host_twins(gpu, name, kind):
    recs = OC.records(name, kind)
    order, keys, _ = device_order(gpu, recs, kind)
    hkeys, horder = host_order(recs, kind)
    assert (keys == hkeys).all(), np.flatnonzero(keys != hkeys)[:8]
    assert (order == horder).all(), np.flatnonzero(order != horder)[:8]
    assert (np.sort(order) == np.arange(len(recs))).all()
    if len(recs) and kind == 0:  # the synchronous form
        assert (cornell().ray_order(*OC.batch(name)) == horder).all()


# ---- 7. ordered casts
CAST_SCENES = ["cornell_box", "bunny_cornell", "pawn_instances", "demo1_moving"]


@functools.lru_cache(None)
def device_scene(name):
    return R.DeviceScene(QC.flat_of(name))


@functools.lru_cache(None)
def cast_rays(name, n):
    rays = QC.ray_records(name, n).copy()
    rays["dir"][5] = 0.0
    rays["origin"][n // 2, 1] = np.nan
    rays["tmax"][n - 3] = -1.0  # (malformed for a cast, valid for the key)
    rays.setflags(write=False)
    return rays


def cast_on_stream(torch, sc, d_rays, n, precision, d_order=None, **kw):
    d_hits = guarded(torch, n * HIT_DTYPE.itemsize)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        sc.cast_async(d_rays.data_ptr(), d_hits.data_ptr(), n, st.cuda_stream, precision=precision,
                      order_ptr=d_order.data_ptr() if d_order is not None else 0, **kw)
    st.synchronize()
    out = d_hits.cpu().numpy()
    assert (out[n * HIT_DTYPE.itemsize:] == 0xA5).all()
    return out[:n * HIT_DTYPE.itemsize].view(HIT_DTYPE).copy()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [512, 4099])
@pytest.mark.parametrize("name", CAST_SCENES)
def test_ordered_cast_is_the_unordered_cast(gpu, name, n, precision):
    sc = device_scene(name)
    rays = cast_rays(name, n)
    bad = np.array([5, n // 2, n - 3])
    d_rays = to_device(gpu, rays)
    want = cast_on_stream(gpu, sc, d_rays, n, precision)
    want_any = cast_on_stream(gpu, sc, d_rays, n, precision, any_hit=True)
    assert (want["hit"][bad] == -1).all() and (want["hit"] == 1).sum() > n // 8
    rng = np.random.default_rng(n)
    own, _, d_own = device_order(gpu, rays, 0)
    orders = {"own": own, "arange": np.arange(n, dtype=np.uint32), "reversed": np.arange(n, dtype=np.uint32)[::-1].copy(),
              "random": rng.permutation(n).astype(np.uint32)}
    assert (np.sort(own) == np.arange(n)).all() and (own != orders["arange"]).any()
    for label, order in orders.items():
        d_order = d_own if label == "own" else to_device(gpu, order)
        got = cast_on_stream(gpu, sc, d_rays, n, precision, d_order)
        assert got.tobytes() == want.tobytes(), (label, np.flatnonzero(got["t"] != want["t"])[:8])
        assert (got["hit"][bad] == -1).all()
        got_any = cast_on_stream(gpu, sc, d_rays, n, precision, d_order, any_hit=True)
        assert (got_any["hit"] == want_any["hit"]).all(), label
    # entries that are no record's index: exactly those records' slots keep their bytes
    order = orders["random"].copy()
    at = rng.choice(n, 7, replace=False)
    skipped = order[at].copy()
    order[at] = [n, n + 5, 0xFFFFFFFF, n, 1 << 31, n + 64, 0x80000001]
    got = cast_on_stream(gpu, sc, d_rays, n, precision, to_device(gpu, order))
    raw, ref = got.view(np.uint8).reshape(n, -1), want.view(np.uint8).reshape(n, -1)
    keep = np.ones(n, bool)
    keep[skipped] = False
    assert (raw[skipped] == 0xA5).all() and raw[keep].tobytes() == ref[keep].tobytes()


# ---- 8. ordered radiance queries
RADIANCE_SCENES = ["cornell", "instanced", "pawn_fog"]  # flat, a triangle BVH (instanced), media


class Buffers:
    def __init__(self, torch, rays, precision):
        self.torch, self.n, self.precision = torch, len(rays), precision
        self.out_bytes = self.n * RADIANCE_DTYPE.itemsize
        self.work_bytes = rad.workspace_bytes(self.n, precision)
        self.d_rays = to_device(torch, rays)
        self.d_out, self.d_work = guarded(torch, self.out_bytes), guarded(torch, self.work_bytes)
        torch.cuda.synchronize()
        self.stream = torch.cuda.Stream()

    def run(self, sc, cs, seed, samples, d_order=None, accumulate=False):
        with self.torch.cuda.stream(self.stream):
            sc.radiance_async(self.d_rays.data_ptr(), self.d_out.data_ptr(), self.d_work.data_ptr(), self.n, samples, cs, seed,
                              self.stream.cuda_stream, accumulate=accumulate, unit_dir=True, precision=self.precision,
                              order_ptr=d_order.data_ptr() if d_order is not None else 0)
        self.stream.synchronize()
        out, work = self.d_out.cpu().numpy(), self.d_work.cpu().numpy()
        assert (out[self.out_bytes:] == 0xA5).all() and (work[self.work_bytes:] == 0xA5).all()
        words = self.n * rad.workspace_words(self.precision) * 8
        return out[:self.out_bytes].tobytes(), work[:words].tobytes()


@functools.lru_cache(None)
def radiance_scene(name):
    return R.DeviceScene(scene(name)[1])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", RADIANCE_SCENES)
def test_ordered_radiance_is_the_unordered_query(gpu, knobs, name, precision):
    cs, _, seed = scene(name)
    sc = radiance_scene(name)
    rays = sc.camera_rays(cs, seed, 0, precision)
    rng = np.random.default_rng(17)
    rays = rays[rng.permutation(len(rays))].copy()
    rays["dir"][9] = 0.0  # a malformed record among them
    n = len(rays)
    own, _, d_own = device_order(gpu, rays, 1)
    assert (np.sort(own) == np.arange(n)).all()
    d_rand = to_device(gpu, rng.permutation(n).astype(np.uint32))
    for samples, chunk in ((3, None), (5, "2")):
        if chunk:
            knobs.setenv("RT_AMD_RADIANCE_CHUNK", chunk)
        want = Buffers(gpu, rays, precision).run(sc, cs, seed, samples)
        out = np.frombuffer(want[0], RADIANCE_DTYPE)
        assert out["status"][9] == -1 and (np.delete(out["samples"], 9) == samples).all() and out["rgb"].max() > 0
        for d_order in (d_own, d_rand):
            assert Buffers(gpu, rays, precision).run(sc, cs, seed, samples, d_order) == want, (samples, chunk)
        # accumulate: an ordered call after an unordered one is two unordered calls
        later = rays.copy()
        later["sample0"] += samples
        two = Buffers(gpu, rays, precision)
        two.run(sc, cs, seed, samples)
        two.d_rays.copy_(to_device(gpu, later))
        want2 = two.run(sc, cs, seed, samples, accumulate=True)
        mixed = Buffers(gpu, rays, precision)
        mixed.run(sc, cs, seed, samples)
        mixed.d_rays.copy_(to_device(gpu, later))
        assert mixed.run(sc, cs, seed, samples, d_own, accumulate=True) == want2, (samples, chunk)
        if chunk:
            knobs.delenv("RT_AMD_RADIANCE_CHUNK")
    # an order with entries >= n: those rays get nothing, the others their result
    order = own.copy()
    at = rng.choice(n, 5, replace=False)
    skipped = order[at].copy()
    order[at] = [n, 0xFFFFFFFF, n + 1, 1 << 31, n]
    got = np.frombuffer(Buffers(gpu, rays, precision).run(sc, cs, seed, 3, to_device(gpu, order))[0], RADIANCE_DTYPE)
    ref = np.frombuffer(Buffers(gpu, rays, precision).run(sc, cs, seed, 3)[0], RADIANCE_DTYPE)
    keep = np.ones(n, bool)
    keep[skipped] = False
    assert got[keep].tobytes() == ref[keep].tobytes() and (got["samples"][skipped] == 0).all()


# ---- 9. the Python surface
def same_dict(a, b):
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_python_surface(gpu, precision):
    name = "bunny_cornell"
    sc = device_scene(name)
    o, d = QC.rays_of(name, 1000)[:2]
    plain = sc.cast(o, d, precision=precision)
    assert plain["hit"].sum() > 300
    assert same_dict(sc.cast(o, d, precision=precision, reorder=True), plain)
    order = sc.ray_order(o, d)
    assert order.dtype == np.uint32 and (np.sort(order) == np.arange(1000)).all()
    assert (order == host_order(query.make_rays(o, d), 0)[1]).all()
    assert same_dict(sc.cast(o, d, precision=precision, order=order), plain)
    assert (sc.cast(o, d, tmax=500.0, any_hit=True, precision=precision, order=order)["hit"] ==
            sc.cast(o, d, tmax=500.0, any_hit=True, precision=precision)["hit"]).all()  # (any hit: only `hit` is specified)
    cs, _, seed = scene("cornell")
    rs = radiance_scene("cornell")
    rays = rs.camera_rays(cs, seed, 0, precision)
    ro, rd = rays["origin"], rays["dir"] * 3.0
    rgb, info = rs.radiance(ro, rd, cs, seed, samples=4, precision=precision)
    for kw in (dict(reorder=True), dict(order=rs.ray_order(ro, rd))):
        rgb2, info2 = rs.radiance(ro, rd, cs, seed, samples=4, precision=precision, **kw)
        assert rgb2.tobytes() == rgb.tobytes() and same_dict(info2, info), kw
    # the synchronous C form refuses an order that is no permutation
    with pytest.raises(R.RtInvalid):
        sc.cast(o, d, precision=precision, order=np.zeros(1000, np.uint32))
    with pytest.raises(R.RtInvalid):
        rs.radiance(ro, rd, cs, seed, precision=precision, order=np.full(len(ro), len(ro), np.uint32))


# ---- 10. a synchronous ordered query that accumulates onto a host workspace
@pytest.mark.parametrize("precision", PRECISIONS)
def test_sync_ordered_radiance_accumulates_onto_a_host_workspace(gpu, precision):
    """rt_scene_radiance_ordered with RT_RADIANCE_ACCUMULATE and a host workspace: the call uploads
    the caller's words, adds onto them in the order's sequence and returns them.  Two calls of 2
    samples (the second with sample0 advanced by 2, over the first one's words), plain, with an order
    computed on the device and with a host order (the reversed permutation), give one another's records
    and workspace words bit for bit, and those of one plain call of 4 samples.  130 rays: two full waves
    and two lanes."""
    cs, _, seed = scene("cornell")
    sc = radiance_scene("cornell")
    n = 130
    rays = sc.camera_rays(cs, seed, 0, precision)
    rays = rays[np.random.default_rng(5).permutation(len(rays))[:n]].copy()
    later = rays.copy()
    later["sample0"] += 2

    def records(recs, samples, **kw):
        return rad.radiance_records(sc, recs, cs, seed, samples, precision, unit_dir=True, **kw)

    want_out, want_work = records(rays, 4)
    assert (want_out["samples"] == 4).all() and want_out["rgb"].max() > 0
    for kw in (dict(), dict(reorder=True), dict(order=np.arange(n - 1, -1, -1, dtype=np.uint32))):
        _, first = records(rays, 2, **kw)
        out, work = records(later, 2, work=first, **kw)
        assert out.tobytes() == want_out.tobytes() and work.tobytes() == want_work.tobytes(), kw
