"""Every dispatchable kernel class once on the GPU (MI355X), on the scenes of tests/class_scenes.py.

rt_kernel_class.h compiles 72 FP32 and 91 binary64 render kernels, and per class (without the 512-lane
twins) a list kernel, a radiance kernel with its ordered twin and, for the classes without the full
material set, a feature kernel.  Each is launched here on a scene that dispatches to it by its own
properties (tests/test_class_sweep_host.py proves that on the host) and held to the check the suite
already has for that kernel family on a handful of scenes:

  a. render      48 x 32 x 4 spp against the FP64 oracle (test_gpu.assert_parity); rt_stats.kernel_block
                 is the class's workgroup size (512 for a twin); a second render is bit-identical
  b. list        24 x 14: add(2), add(2), add_where(2, t) against uniform films, bit for bit
                 (test_adaptive_gpu test_selected_pixels_are_a_uniform_film_at_their_count)
  c. radiance    24 x 14: camera_rays(k), k = 0..2, accumulated, are the film after add(3), bit for bit
                 (test_radiance_gpu test_camera_rays_return_the_film); then in the device's own ray order
  d. features    40 px, n_feat 4: albedo against the oracle's emitter twin, normal, depth and coverage
                 against the binary64 host build (test_denoise_gpu's bars and numbers)

Scenes, device scenes and reference frames are made once per class."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, record_measure

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tests", "feature_emu"))
import class_scenes as CS  # noqa: E402
import raytrace_amd as R  # noqa: E402
import test_adaptive_gpu as TA  # noqa: E402
from raytrace_amd import _lib, denoise, film, query  # noqa: E402
from raytrace_amd import radiance as rad  # noqa: E402
from raytrace_amd.radiance import RADIANCE_DTYPE  # noqa: E402
from raytrace_amd.scene import flatten  # noqa: E402
from test_class_sweep_host import oracle_frame  # noqa: E402
from test_denoise_gpu import N_FEAT, assert_bars  # noqa: E402
from test_gpu import assert_parity  # noqa: E402

RENDER_CASES = CS.all_cases()
WIDE_CASES = [(c, p) for c, p in RENDER_CASES if not c[5]]      # list and radiance kernels: no twins
FEATURE_CASES = [(c, p) for c, p in WIDE_CASES if not c[3]]     # feature kernels: mats cleared


def ids(cases):
    return [f"{CS.class_id(c)}-{p}" for c, p in cases]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    return torch


@functools.lru_cache(maxsize=None)
def flat_of(cls):
    return flatten(CS.scene_of(cls)[1])


@functools.lru_cache(maxsize=None)
def device_scene(cls):
    return R.DeviceScene(flat_of(cls))


def small(cls, width=24, height=14):
    cs, _, seed, _ = CS.scene_of(cls)
    return cs.replace(cs_imageWidth=width, cs_aspectRatio=width / height, cs_samplesPerPixel=1), seed


# ---- a. the render kernel
@pytest.mark.parametrize("cls,precision", RENDER_CASES, ids=ids(RENDER_CASES))
def test_render_matches_oracle(gpu, oracle_mod, emu_mod, cls, precision):
    cs, _, seed, lmax = CS.scene_of(cls)
    ref = oracle_frame(cls)
    st = {}
    img = R.raytrace(cs, flat_of(cls), seed, precision=precision, stats=st)
    want_block = CS.enumerated_classes(precision)[cls][1]
    assert st["kernel_block"] == want_block, (st, want_block)  # the intended kernel ran
    assert want_block == 512 if cls[5] else want_block != 512
    d = np.abs(img.astype(np.float64) - ref)
    rel = (d / np.maximum(np.abs(ref), 1e-3 if precision == "f64" else 1.0)).max(-1)
    share = float((rel <= 1e-9).mean() if precision == "f64" else (rel < 1e-3).mean())
    print(f"{CS.class_id(cls)} {precision}: share {share:.4f}, worst {d.max():.3e}, block {st['kernel_block']}")
    record_measure("class_sweep", dict(test="render", cls=CS.class_id(cls), precision=precision, share=share,
                                       worst=float(d.max()), block=st["kernel_block"], kernel_ms=st["kernel_ms"]))
    assert_parity(img, ref, precision, CS.need32(cls), None, CS.class_id(cls), CS.SPP, lmax)
    again = R.raytrace(cs, flat_of(cls), seed, precision=precision)
    assert np.array_equal(img, again, equal_nan=True), float(np.nanmax(np.abs(img - again)))


# ---- b. the list kernel
@functools.lru_cache(maxsize=None)
def uniform(cls, precision, passes):
    cs, seed = small(cls)
    with R.Film(device_scene(cls), cs, seed, precision=precision) as f:
        for n in passes:
            f.add(n)
        st = TA.snapshot(f)
    for a in st.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return st


@pytest.mark.parametrize("cls,precision", WIDE_CASES, ids=ids(WIDE_CASES))
def test_list_kernel_selected_pixels_are_a_uniform_film(gpu, cls, precision):
    cs, seed = small(cls)
    with R.Film(device_scene(cls), cs, seed, precision=precision) as f:
        f.add(2).add(2)
        before = TA.snapshot(f)
        r, counting = TA.rel_error(before)
        t = TA.median_threshold(r, counting)
        f.add_where(2, t)
        want_sel = np.flatnonzero(((r > t) & counting).ravel())
        assert np.array_equal(f.selection(), want_sel)
        assert 0.25 * r.size <= len(want_sel) <= 0.75 * r.size, (len(want_sel), r.size)
        after = TA.snapshot(f)
    sel = np.zeros(r.size, bool)
    sel[want_sel] = True
    sel = sel.reshape(r.shape)
    TA.assert_pixels_equal(after, uniform(cls, precision, (2, 2, 2)), sel, "selected")
    TA.assert_pixels_equal(after, uniform(cls, precision, (2, 2)), ~sel, "not selected")
    TA.assert_pixels_equal(after, before, ~sel, "not selected, before")
    assert np.isfinite(after["image"]).all() and after["image"].mean() > 0
    record_measure("class_sweep", dict(test="list", cls=CS.class_id(cls), precision=precision,
                                       selected=len(want_sel) / r.size))


# ---- c. the radiance kernels
K = 3


def to_device(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def accumulate_camera_rays(torch, sc, cs, seed, precision, ordered):
    """camera_rays(k), one sample each, accumulated over k < K (in the device's own order of each
    batch when `ordered`): (results, workspace words) as host arrays, guard bytes checked."""
    rays = [sc.camera_rays(cs, seed, k, precision) for k in range(K)]
    n = len(rays[0])
    out_bytes, work_bytes = n * RADIANCE_DTYPE.itemsize, rad.workspace_bytes(n, precision)
    d_out = torch.full((out_bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    d_work = torch.full((work_bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    for k in range(K):
        assert (rays[k]["sample0"] == k).all()
        d_rays = to_device(torch, rays[k])
        d_order = None
        if ordered:
            order = query.ray_order_records(sc, rays[k])
            assert (np.sort(order) == np.arange(n)).all()
            d_order = to_device(torch, order.astype(np.uint32))
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            sc.radiance_async(d_rays.data_ptr(), d_out.data_ptr(), d_work.data_ptr(), n, 1, cs, seed, stream.cuda_stream,
                              accumulate=k > 0, unit_dir=True, precision=precision,
                              order_ptr=d_order.data_ptr() if d_order is not None else 0)
        stream.synchronize()
    out, work = d_out.cpu().numpy(), d_work.cpu().numpy()
    assert (out[out_bytes:] == 0xA5).all() and (work[work_bytes:] == 0xA5).all()
    words = rad.workspace_words(precision)
    return out[:out_bytes].view(RADIANCE_DTYPE).copy(), work[:n * words * 8].view(np.uint64).reshape(n, words).copy()


@pytest.mark.parametrize("cls,precision", WIDE_CASES, ids=ids(WIDE_CASES))
def test_radiance_kernels_return_the_film(gpu, cls, precision):
    cs, seed = small(cls)
    sc = device_scene(cls)
    with R.Film(sc, cs, seed, precision=precision) as f:
        f.add(K)
        st = film.unpack_state(f.state().copy())
        image = f.image()
    out, work = accumulate_camera_rays(gpu, sc, cs, seed, precision, ordered=False)
    words = rad.workspace_words(precision) - 1
    n = len(out)
    assert n == 24 * 14
    assert np.array_equal(work[:, :words].view(np.int64), st["sums"].reshape(n, words)), "sums differ from the film's"
    assert np.array_equal((work[:, words] & np.uint64(0xffffffff)).astype(np.uint32), st["flags"].reshape(n))
    assert ((work[:, words] >> np.uint64(32)) == K).all() and (out["samples"] == K).all()
    assert (out["status"] == np.where(st["flags"].reshape(n) != 0, 2, 1)).all()
    rgb = out["rgb"].astype(image.dtype).reshape(image.shape)
    assert TA.bits_equal(rgb, image), "rgb differs from the film's image"
    assert np.isfinite(image).all() and image.max() > 0
    out_o, work_o = accumulate_camera_rays(gpu, sc, cs, seed, precision, ordered=True)
    assert out_o.tobytes() == out.tobytes() and work_o.tobytes() == work.tobytes(), "the ordered twin differs"


# ---- d. the feature kernel
FEATURE_WIDTH = 40


def feature_scene(cls):
    cs, world, seed, _ = CS.scene_of(cls)
    return cs.replace(cs_imageWidth=FEATURE_WIDTH, cs_samplesPerPixel=N_FEAT), world, seed


@functools.lru_cache(maxsize=None)
def feature_refs(cls):
    """(the oracle's render of the emitter twin, the binary64 host build's features), once per class"""
    import feature_emu
    import oracle
    cs, world, seed = feature_scene(cls)
    albedo = oracle.render(cs, denoise.emitter_twin(world), seed, mode=oracle.RNG_PHILOX)
    host = denoise.features_from_words(feature_emu.features(cs, world, seed, N_FEAT, precision="f64"), N_FEAT)
    return albedo, host


@pytest.mark.parametrize("cls,precision", FEATURE_CASES, ids=ids(FEATURE_CASES))
def test_feature_kernel(gpu, oracle_mod, cls, precision):
    cs, world, seed = feature_scene(cls)
    albedo, host = feature_refs(cls)
    with R.Film(device_scene(cls), cs, seed, precision=precision) as f:
        got = f.features(N_FEAT)
    what = CS.class_id(cls)
    assert_bars(got["albedo"], albedo, precision, what + " albedo", N_FEAT, max(1.0, float(albedo.max())))
    assert_bars(got["normal"], host["normal"], precision, what + " normal", N_FEAT, 1.0, mean=False)
    scale = max(float(host["depth"].max()), 1.0)
    assert_bars(got["depth"][..., None] / scale, host["depth"][..., None] / scale, precision, what + " depth", N_FEAT, 1.0,
                mean=False)
    assert_bars(got["coverage"][..., None], host["coverage"][..., None], precision, what + " coverage", N_FEAT, 1.0,
                mean=False)
    assert 0.0 < host["coverage"].mean() < 1.0  # hits and misses
