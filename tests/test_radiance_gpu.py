"""The radiance queries (include/rt.h rt_scene_radiance, DeviceScene.radiance) on the GPU: the pin to
the film (the device's own camera rays return the film's sums bit for bit), the device against the
host build of the same body (tests/radiance_emu), determinism and chunking, few rays with many
samples and the guard regions, coexistence with a film and a cast, and the refusals."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "radiance_emu"))
import query_cases as QC  # noqa: E402
import radiance_emu as RE  # noqa: E402
import raytrace_amd as R  # noqa: E402
from raytrace_amd import _lib, film, query  # noqa: E402
from raytrace_amd import radiance as rad  # noqa: E402
from raytrace_amd.radiance import PATH_RAY_DTYPE, RADIANCE_DTYPE  # noqa: E402
from raytrace_amd.ray import _seed64  # noqa: E402
from test_adaptive_gpu import PRECISIONS, SCENES, scene  # noqa: E402

K = 3  # samples of the pin


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    return torch


@functools.lru_cache(None)
def device_scene(name):
    return R.DeviceScene(scene(name)[1])


@functools.lru_cache(None)
def device_camera_rays(name, precision, sample):
    cs, _, seed = scene(name)
    rays = device_scene(name).camera_rays(cs, seed, sample, precision)
    rays.setflags(write=False)
    return rays


class Buffers:
    """Device buffers of one query: rays, results and workspace, the last two followed by `guard`
    bytes of 0xA5."""

    def __init__(self, torch, rays, precision, guard=0):
        self.torch, self.n, self.precision, self.guard = torch, len(rays), precision, guard
        self.out_bytes = self.n * RADIANCE_DTYPE.itemsize
        self.work_bytes = rad.workspace_bytes(self.n, precision)
        self.d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).cuda()
        self.d_out = torch.full((self.out_bytes + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        self.d_work = torch.full((self.work_bytes + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # the fills above ran on the default stream
        self.stream = torch.cuda.Stream()

    def set_rays(self, rays):
        assert len(rays) == self.n
        self.d_rays.copy_(self.torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()))
        self.torch.cuda.synchronize()

    def run(self, sc, cs, seed, samples, accumulate=False, unit_dir=False):
        with self.torch.cuda.stream(self.stream):
            sc.radiance_async(self.d_rays.data_ptr(), self.d_out.data_ptr(), self.d_work.data_ptr(), self.n, samples, cs, seed,
                              self.stream.cuda_stream, accumulate=accumulate, unit_dir=unit_dir, precision=self.precision)
        self.stream.synchronize()
        return self

    def out(self):
        return self.d_out.cpu().numpy()[:self.out_bytes].view(RADIANCE_DTYPE).copy()

    def work(self):
        w = self.d_work.cpu().numpy()[:self.n * rad.workspace_words(self.precision) * 8].view(np.uint64)
        return w.reshape(self.n, rad.workspace_words(self.precision)).copy()

    def guards(self):
        return self.d_out.cpu().numpy()[self.out_bytes:], self.d_work.cpu().numpy()[self.work_bytes:]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---- 1. the pin
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(SCENES))
def test_camera_rays_return_the_film(gpu, name, precision):
    """camera_rays(sample k) traced with one sample each, unit_dir, accumulated over k = 0..2: the
    workspace's sums and flags are the state of a film of the same scene and seed after add(3), and
    rgb is its image, bit for bit."""
    cs, flat, seed = scene(name)
    sc = device_scene(name)
    with R.Film(sc, cs, seed, precision=precision) as f:
        f.add(K)
        st = film.unpack_state(f.state().copy())
        image = f.image()
    b = Buffers(gpu, device_camera_rays(name, precision, 0), precision)
    for k in range(K):
        rays = device_camera_rays(name, precision, k)
        assert (rays["sample0"] == k).all() and (rays["stream"] == np.arange(len(rays))).all()
        b.set_rays(rays)
        b.run(sc, cs, seed, 1, accumulate=k > 0, unit_dir=True)
    out, work = b.out(), b.work()
    words = rad.workspace_words(precision) - 1
    n = len(out)
    assert n == st["sums"].shape[0] * st["sums"].shape[1] == 24 * 14
    assert np.array_equal(work[:, :words].view(np.int64), st["sums"].reshape(n, words)), "sums differ from the film's"
    assert np.array_equal((work[:, words] & np.uint64(0xffffffff)).astype(np.uint32), st["flags"].reshape(n))
    assert ((work[:, words] >> np.uint64(32)) == K).all() and (out["samples"] == K).all()
    assert (out["status"] == np.where(st["flags"].reshape(n) != 0, 2, 1)).all()
    rgb = out["rgb"].astype(image.dtype).reshape(image.shape)
    assert np.array_equal(bits(rgb), bits(image)), f"{int((bits(rgb) != bits(image)).any(-1).sum())} pixels differ"
    assert np.isfinite(image).all() and image.max() > 0


# ---- 2. the device against the host build
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(SCENES))
def test_device_matches_host_build(gpu, name, precision):
    """On the device's own camera rays of sample 0, two samples per ray: status and count are the host
    build's; binary64 reals within 1e-9 relative on the max(|ref|, 1e-3) scale for at least 99.9 % of
    the rays (tests/test_query_gpu.py test_device_matches_host_build's bar); FP32 against the
    BINARY64 host build under the guide-buffer tests' bars (tests/test_denoise_gpu.py assert_bars:
    at least 99 % within 1e-3, relative above 1, the worst within 4 L / spp + 1e-3, L the largest
    reference value or 1)."""
    cs, flat, seed = scene(name)
    spp = 2
    rays = device_camera_rays(name, precision, 0)
    dev = Buffers(gpu, rays, precision).run(device_scene(name), cs, seed, spp, unit_dir=True).out()
    host, _ = RE.radiance(cs, flat, seed, rays, spp, "f64", unit_dir=True)
    assert (dev["status"] == host["status"]).all() and (dev["samples"] == host["samples"]).all() and (dev["samples"] == spp).all()
    d = np.abs(dev["rgb"] - host["rgb"])
    if precision == "f64":
        share = float(((d / np.maximum(np.abs(host["rgb"]), 1e-3)).max(-1) > 1e-9).mean())
        print(f"{name}: binary64 device vs host build, {100 * share:.3f} % of rays beyond 1e-9, worst {d.max():.3e}")
        assert share <= 0.001, share
    else:
        lmax = max(1.0, float(host["rgb"].max()))
        frac = float(((d / np.maximum(np.abs(host["rgb"]), 1.0)).max(-1) < 1e-3).mean())
        print(f"{name}: FP32 device vs binary64 host build, fraction within 1e-3 {frac:.4f}, worst {d.max():.3e}")
        assert frac >= 0.99, frac
        assert d.max() <= 4 * lmax / spp + 1e-3, float(d.max())


# ---- 3. determinism and chunking
@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunking_and_repeats_give_identical_bytes(gpu, knobs, precision):
    """200 rays (not a multiple of 64) at 8 samples: samples per item of 1, 3 and 8 against the launcher's
    own choice and that choice twice — results and workspace words byte for byte."""
    name = "pawn_fog"
    cs, flat, seed = scene(name)
    rays = device_camera_rays(name, precision, 0)[:200]
    sc = device_scene(name)

    def run():
        b = Buffers(gpu, rays, precision).run(sc, cs, seed, 8, unit_dir=True)
        return b.out().tobytes(), b.work().tobytes()
    base = run()
    assert run() == base
    for chunk in ("1", "3", "8"):
        knobs.setenv("RT_AMD_RADIANCE_CHUNK", chunk)
        assert run() == base, chunk
    knobs.delenv("RT_AMD_RADIANCE_CHUNK")
    out = np.frombuffer(base[0], RADIANCE_DTYPE)
    assert (out["samples"] == 8).all() and (out["status"] == 1).all() and out["rgb"].max() > 0


# ---- 4. few rays, many samples
@pytest.mark.parametrize("precision", PRECISIONS)
def test_few_rays_many_samples_and_guards(gpu, knobs, precision):
    """Four rays at 512 samples in the launcher's own chunking equal the same call as 2048 one-sample
    items (chunk 1) and two accumulated calls of 256 samples, byte for byte; the guard regions of 0xA5
    bytes behind d_out and behind the workspace stay intact."""
    name = "cornell"
    cs, flat, seed = scene(name)
    rays = device_camera_rays(name, precision, 0)[[130, 180, 200, 224]]  # (pixels that see the inside of the box)
    sc = device_scene(name)
    a = Buffers(gpu, rays, precision, guard=256).run(sc, cs, seed, 512, unit_dir=True)
    knobs.setenv("RT_AMD_RADIANCE_CHUNK", "1")
    b = Buffers(gpu, rays, precision, guard=256).run(sc, cs, seed, 512, unit_dir=True)
    knobs.delenv("RT_AMD_RADIANCE_CHUNK")
    assert a.out().tobytes() == b.out().tobytes() and a.work().tobytes() == b.work().tobytes()
    for buf in (a, b):
        go, gw = buf.guards()
        assert len(go) == len(gw) == 256 and (go == 0xA5).all() and (gw == 0xA5).all()
    out = a.out()
    assert (out["samples"] == 512).all() and (out["status"] == 1).all() and (out["rgb"].max(-1) > 0).all()
    # two accumulated calls of 256 samples are the one call of 512
    half = rays.copy()
    c = Buffers(gpu, half, precision).run(sc, cs, seed, 256, unit_dir=True)
    half["sample0"] = 256
    c.set_rays(half)
    c.run(sc, cs, seed, 256, accumulate=True, unit_dir=True)
    assert c.work().tobytes() == a.work().tobytes() and c.out().tobytes() == out.tobytes()


# ---- 5. coexistence
def test_film_cast_and_radiance_leave_each_other_alone(gpu):
    """A film pass, a cast and a radiance query on one scene and one stream, in two orders: each
    result is what it is alone."""
    name, precision = "demo1", "f64"
    cs, flat, seed = scene(name)
    sc = device_scene(name)
    rays = device_camera_rays(name, precision, 0)
    qrays = query.make_rays(rays["origin"], rays["dir"])
    alone_rad = Buffers(gpu, rays, precision).run(sc, cs, seed, 2, unit_dir=True).out().tobytes()
    alone_hits = query.cast_records(sc, qrays, precision).tobytes()
    with R.Film(sc, cs, seed, precision=precision) as f:
        alone_state = f.add(2).state().tobytes()
    for order in ("film-cast-radiance", "radiance-cast-film"):
        b = Buffers(gpu, rays, precision)
        d_q = gpu.from_numpy(qrays.view(np.uint8).reshape(-1).copy()).cuda()
        d_h = gpu.zeros(len(qrays) * query.HIT_DTYPE.itemsize, dtype=gpu.uint8, device="cuda")
        gpu.cuda.synchronize()
        with R.Film(sc, cs, seed, precision=precision) as f:
            with gpu.cuda.stream(b.stream):
                steps = {"film": lambda: f.add(2, b.stream.cuda_stream),
                         "cast": lambda: sc.cast_async(d_q.data_ptr(), d_h.data_ptr(), len(qrays), b.stream.cuda_stream,
                                                       precision=precision),
                         "radiance": lambda: sc.radiance_async(b.d_rays.data_ptr(), b.d_out.data_ptr(), b.d_work.data_ptr(),
                                                               b.n, 2, cs, seed, b.stream.cuda_stream, unit_dir=True,
                                                               precision=precision)}
                for s in order.split("-"):
                    steps[s]()
            b.stream.synchronize()
            assert f.state().tobytes() == alone_state, order
        assert b.out().tobytes() == alone_rad, order
        assert d_h.cpu().numpy().tobytes() == alone_hits, order
    assert not sc.radiance_overflowed() and not sc.cast_overflowed()


# ---- 6. errors
def test_refusals_and_stack_overflow(gpu, knobs):
    """Null arguments, n < 0, n_samples <= 0, a device list, n x n_samples beyond the id range and
    unknown flags are RT_E_INVALID; n == 0 is a no-op; with two stack rows (the experiment knob
    RT_AMD_RADIANCE_STACK, as RT_AMD_CAST_STACK) the synchronous call returns RT_E_STACK and
    rt_scene_radiance_status reports and clears the asynchronous call's word."""
    name = "cornell"
    cs, flat, seed = scene(name)
    sc = device_scene(name)
    L = sc._lib
    c = _lib.camera_struct(cs)
    ex = _lib.exec_struct()
    rays = np.ascontiguousarray(device_camera_rays(name, "f64", 0)[:8])
    out = np.zeros(8, RADIANCE_DTYPE)
    rp, op = rays.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)

    def call(h=sc.handle, e=ex, cam=c, r=rp, o=op, n=8, ns=1, flags=0):
        return L.rt_scene_radiance(h, ctypes.byref(e) if e is not None else None, ctypes.byref(cam) if cam is not None else None,
                                   _seed64(seed), r, o, None, n, ns, flags)
    assert call() == 0 and (out["status"] == 1).all()
    for kw in (dict(h=None), dict(e=None), dict(cam=None), dict(r=None), dict(o=None), dict(n=-1), dict(ns=0), dict(ns=-3),
               dict(flags=4), dict(e=_lib.exec_struct(devices=[0])), dict(n=1 << 22, ns=1 << 10), dict(ns=(1 << 24) + 1)):
        assert call(**kw) == _lib.RT_E_INVALID, kw
    before = out.copy()
    assert call(n=0) == 0 and out.tobytes() == before.tobytes()
    assert L.rt_scene_radiance_async(sc.handle, ctypes.byref(ex), ctypes.byref(c), _seed64(seed), rp, op, None, 8, 1, 0,
                                     None) == _lib.RT_E_INVALID  # (a null workspace)
    assert L.rt_scene_camera_rays(sc.handle, ctypes.byref(ex), ctypes.byref(c), _seed64(seed), -1, rp) == _lib.RT_E_INVALID
    assert L.rt_scene_radiance_workspace_bytes(10, 0) == 10 * 7 * 8 + 16
    assert L.rt_scene_radiance_workspace_bytes(10, _lib.RT_EXEC_F32) == 10 * 4 * 8 + 16
    # the traversal-stack word
    deep = R.DeviceScene(QC.deep_scene())
    assert deep.stats()["max_stack"] >= 20
    q = QC.deep_rays(256)
    drays = rad.make_path_rays(q["origin"], q["dir"])
    cs = R.defaultCameraSettings(cs_maxRecursionDepth=4)  # (no redirect targets: the scene has no emitter)
    c = _lib.camera_struct(cs)
    good, _ = rad.radiance_records(deep, drays, cs, seed, 1)
    host, _ = RE.radiance(cs, QC.deep_scene(), seed, drays, 1, "f64")
    assert (good["status"] == 1).all() and (good["status"] == host["status"]).all()
    knobs.setenv("RT_AMD_RADIANCE_STACK", "2")
    res = np.zeros(256, RADIANCE_DTYPE)
    for precision in PRECISIONS:
        e = _lib.exec_struct(precision=precision)
        rc = L.rt_scene_radiance(deep.handle, ctypes.byref(e), ctypes.byref(c), _seed64(seed), drays.ctypes.data_as(ctypes.c_void_p),
                                 res.ctypes.data_as(ctypes.c_void_p), None, 256, 1, 0)
        assert rc == _lib.RT_E_STACK and b"stack" in L.rt_last_error()
        assert not deep.radiance_overflowed()  # the synchronous call's word is its own
        Buffers(gpu, drays, precision).run(deep, cs, seed, 1)
        assert deep.radiance_overflowed() and not deep.radiance_overflowed()
    knobs.delenv("RT_AMD_RADIANCE_STACK")
    again = Buffers(gpu, drays, "f64").run(deep, cs, seed, 1).out()
    assert again.tobytes() == good.tobytes() and not deep.radiance_overflowed()
    deep.close()
