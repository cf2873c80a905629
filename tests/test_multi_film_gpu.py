"""The multi-device film on the GPU (include/rt.h rt_multi_film_*, raytrace_amd.film.MultiFilm).

Passes are exact integer sums keyed by global pixel and sample index, so every comparison is bit for
bit (np.array_equal / byte equality), and the comparand is always the existing single-device path
(R.raytrace, R.Film), never the multi film itself.  Devices are [0] x n (several shards on one GPU,
each on its own stream) unless a test says otherwise; RT_AMD_COPY_SHARDS puts shards on the path a
device without peer access takes.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raytrace_amd as R  # noqa: E402
from raytrace_amd import _lib, scenes  # noqa: E402
from raytrace_amd.scene import flatten  # noqa: E402

SCENES = {"cornell": (scenes.cornell_box, 50), "bunny_cornell": (scenes.bunny_cornell, 40),
          "pawn_fog": (scenes.pawn_fog, 40)}
PASSES = [1, 7, 3, 16, 5]
PRECISIONS = ["f64", "f32"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    return torch


@functools.lru_cache(maxsize=None)
def scene(name, width=None):
    """(settings, flattened world, seed) of a test scene, built once."""
    fn, w = SCENES[name]
    cs, world, seed = fn(width=width or w, spp=1)
    return cs, flatten(world), seed


@functools.lru_cache(maxsize=None)
def one_shot(name, spp, precision, width=None):
    """The reference image: one single-device render of `spp` samples (computed once, read-only)."""
    cs, flat, seed = scene(name, width)
    img = R.raytrace(cs.replace(cs_samplesPerPixel=spp), flat, seed, precision=precision)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def plain_film(name, passes, precision, width=None, row_block=4):
    """The reference state: what a plain one-device Film holds after `passes` (computed once):
    its saved state, noise figure and noise map (None before two passes)."""
    cs, flat, seed = scene(name, width)
    with R.Film(flat, cs, seed, precision=precision, row_block=row_block) as f:
        for n in passes:
            f.add(n)
        out = dict(state=f.state(), noise=f.noise() if len(passes) > 1 else None,
                   noise_map=f.noise_map() if len(passes) > 1 else None)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def multi_film(name, precision, devices, width=None, **kw):
    cs, flat, seed = scene(name, width)
    return R.MultiFilm(flat, cs, seed, devices=devices, precision=precision, **kw)


def check_against_single_device(f, name, passes, precision, width=None, row_block=4):
    """Items 1 and 2: the image is the one-shot render's, the state (header, sums, flags, q), the
    noise figure and the noise map are a plain film's after the same passes."""
    for n in passes:
        f.add(n)
    assert (f.spp, f.passes) == (sum(passes), len(passes))
    img = f.image()
    want = one_shot(name, sum(passes), precision, width)
    assert img.dtype == want.dtype and img.shape == want.shape
    assert np.array_equal(img, want, equal_nan=True)
    assert np.isfinite(img).all() and img.mean() > 0
    ref = plain_film(name, tuple(passes), precision, width, row_block)
    assert f.state().tobytes() == ref["state"].tobytes()
    assert f.noise() == ref["noise"]
    assert np.array_equal(f.noise_map(), ref["noise_map"], equal_nan=True)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(SCENES))
def test_passes_and_state_equal_the_single_device(gpu, name, precision):
    """Passes of 1, 7, 3, 16 and 5 samples on three shards against one render of 32 and a plain film:
    flat, BVH and media kernels.  Cornell at width 50 has 13 row blocks: tiles with padding rows."""
    with multi_film(name, precision, [0, 0, 0]) as f:
        assert f.shape == one_shot(name, 32, precision).shape
        check_against_single_device(f, name, PASSES, precision)
        assert f.copied_passes == 0  # (one GPU: every shard merges directly)


@pytest.mark.parametrize("mask,copied", [("-1", 3), ("2", 1)])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_copied_shards(knobs, gpu, precision, mask, copied):
    """RT_AMD_COPY_SHARDS: every shard, or shard 1 alone beside two direct ones, goes through the
    staging copy and the merge on the first device; the film counts the passes that did."""
    knobs.setenv("RT_AMD_COPY_SHARDS", mask)
    with multi_film("cornell", precision, [0, 0, 0]) as f:
        check_against_single_device(f, "cornell", PASSES, precision)
        assert f.copied_passes == copied * len(PASSES)


@pytest.mark.parametrize("mask", [None, "-1"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_resolve_on_a_caller_stream_between_adds(knobs, gpu, precision, mask):
    """The preview loop add; resolve(S); add; resolve(S) on a stream of the caller's, with no
    rt_multi_film_frame in between: each resolve follows the merges of the passes before it, and the
    next pass's merges follow the resolve.  Every image equals the one-shot render's."""
    if mask:
        knobs.setenv("RT_AMD_COPY_SHARDS", mask)
    L = _lib.load()
    stream = gpu.cuda.Stream()
    dt = gpu.float64 if precision == "f64" else gpu.float32
    sizes = [4, 4, 8, 16]
    with multi_film("cornell", precision, [0, 0, 0]) as f:
        outs = [gpu.zeros(f.shape, dtype=dt, device="cuda:0") for _ in sizes]
        for n, out in zip(sizes, outs):
            f.add(n)
            _lib.check(L.rt_film_resolve(f.handle, out.data_ptr(), stream.cuda_stream))
        stream.synchronize()
        total = 0
        for n, out in zip(sizes, outs):
            total += n
            assert np.array_equal(out.cpu().numpy(), one_shot("cornell", total, precision), equal_nan=True), total
        assert np.array_equal(f.image(), one_shot("cornell", total, precision), equal_nan=True)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_unaligned_blocks(gpu, precision):
    """Width 9 in blocks of 3 rows on two shards: 27 pixels per block, so in FP32 every second block
    starts on an odd word and on a pixel index that is no multiple of 4 (the merge's scalar form)."""
    with multi_film("cornell", precision, [0, 0], width=9, row_block=3) as f:
        check_against_single_device(f, "cornell", [2, 3], precision, width=9, row_block=3)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_more_devices_than_blocks(gpu, precision):
    """Width 8: two 4-row blocks on three shards; the third holds only padding rows."""
    with multi_film("cornell", precision, [0, 0, 0], width=8) as f:
        check_against_single_device(f, "cornell", [2, 3], precision, width=8)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_device_list(gpu, precision):
    """A list of one device: one shard, the whole frame as one block."""
    with multi_film("cornell", precision, [0], width=37) as f:
        check_against_single_device(f, "cornell", [4, 4], precision, width=37)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_states_move_between_device_counts(gpu, precision):
    cs, flat, seed = scene("cornell")
    want16, want8 = one_shot("cornell", 16, precision), one_shot("cornell", 8, precision)
    with multi_film("cornell", precision, [0, 0, 0]) as f:
        state = f.add(4).add(4).state()
        with R.Film(flat, cs, seed, precision=precision) as g:  # three shards -> one device
            assert g.restore(state).spp == 8 and g.passes == 2
            assert np.array_equal(g.add(8).image(), want16, equal_nan=True)
        assert (f.reset().spp, f.passes) == (0, 0)
        assert np.array_equal(f.add(8).image(), want8, equal_nan=True)
    plain = plain_film("cornell", (4, 4), precision)["state"]
    assert state.tobytes() == plain.tobytes()
    with multi_film("cornell", precision, [0, 0]) as h:  # one device -> two shards
        assert h.restore(plain).spp == 8 and h.passes == 2
        assert np.array_equal(h.add(8).image(), want16, equal_nan=True)
        with pytest.raises(R.RtInvalid, match="does not match"):
            h.restore(plain_film("cornell", (4, 4), precision, 37)["state"])
        assert h.spp == 16


@pytest.mark.parametrize("precision", PRECISIONS)
def test_denoiser_on_the_frame(gpu, precision):
    """denoised() with the default parameters (8-sample features, 64-sample albedo) and features(8)
    equal a plain film's."""
    cs, flat, seed = scene("cornell")
    with R.Film(flat, cs, seed, precision=precision) as g:
        want, want_feat, want_albedo = g.add(4).add(4).denoised(), g.features(8), g.albedo(64)
    with multi_film("cornell", precision, [0, 0, 0]) as f:
        got, feat = f.add(4).add(4).denoised(), f.features(8)
        assert np.array_equal(f.albedo(64), want_albedo) and want_albedo.mean() > 0
    assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True) and np.isfinite(got).all()
    assert sorted(feat) == sorted(want_feat)
    for k in feat:
        assert np.array_equal(feat[k], want_feat[k], equal_nan=True), k


@pytest.mark.parametrize("precision", PRECISIONS)
def test_raytrace_until_on_a_device_list(gpu, precision):
    cs, flat, seed = scene("cornell")
    for noise in (0.0, 1e9):  # runs to max_spp; stops at the first check
        want, want_info = R.raytrace_until(cs, flat, seed, noise, batch=4, max_spp=16, precision=precision)
        img, info = R.raytrace_until(cs, flat, seed, noise, batch=4, max_spp=16, precision=precision, devices=[0, 0])
        assert info == want_info and np.array_equal(img, want, equal_nan=True)
    assert np.array_equal(want, one_shot("cornell", 8, precision), equal_nan=True)
    want, want_info = R.raytrace_until(cs, flat, seed, 0.0, batch=4, max_spp=8, precision=precision, denoise=True)
    img, info = R.raytrace_until(cs, flat, seed, 0.0, batch=4, max_spp=8, precision=precision, denoise=True, devices=[0, 0])
    assert np.array_equal(img, want, equal_nan=True) and np.array_equal(info.pop("raw"), want_info.pop("raw"), equal_nan=True)
    assert info == want_info


def test_refusals(gpu):
    cs, flat, seed = scene("cornell")
    L = _lib.load()
    multi = R.MultiDeviceScene(flat, [0, 0])
    try:
        with R.MultiFilm(multi, cs, seed) as f:  # (a caller's scene: the film leaves it open)
            f.add(2)
            state = f.state()
            buf = np.ascontiguousarray(state)
            for call, rc in (("add", L.rt_film_add(f.handle, 1, None)), ("reset", L.rt_film_reset(f.handle)),
                             ("load", L.rt_film_load(f.handle, buf.ctypes.data_as(ctypes.c_void_p), buf.size)),
                             ("destroy", L.rt_film_destroy(f.handle))):
                assert rc == _lib.RT_E_INVALID, call
                with pytest.raises(R.RtInvalid, match="frame"):
                    _lib.check(rc)
            assert f.spp == 2 and np.array_equal(f.image(), one_shot("cornell", 2, "f64"), equal_nan=True)
            for n in (0, -3, R.film.MAX_SAMPLES):
                with pytest.raises(R.RtInvalid):
                    f.add(n)
            with pytest.raises(R.RtInvalid):
                R.MultiFilm(multi, cs, seed, devices=[0])
        # ex.n_shards = 2 at create
        c, ex, h = _lib.camera_struct(cs), _lib.exec_struct(), ctypes.c_void_p()
        ex.n_shards = 2
        rc = L.rt_multi_film_create(multi.handle, ctypes.byref(c), 1, ctypes.byref(ex), ctypes.byref(h))
        assert rc == _lib.RT_E_INVALID and h.value is None
        with pytest.raises(R.RtInvalid, match="n_shards"):
            _lib.check(rc)
        enc = _lib.exec_struct(encode="srgb")
        assert L.rt_multi_film_create(multi.handle, ctypes.byref(c), 1, ctypes.byref(enc), ctypes.byref(h)) == _lib.RT_E_INVALID
        # the scene still renders, and a film that is not owned behaves as before
        assert np.array_equal(multi.render(cs.replace(cs_samplesPerPixel=2), seed), one_shot("cornell", 2, "f64"), equal_nan=True)
    finally:
        multi.close()
    with R.Film(flat, cs, seed) as g:
        assert np.array_equal(g.add(1).add(1).image(), one_shot("cornell", 2, "f64"), equal_nan=True)
        assert g.reset().spp == 0 and g.restore(state).spp == 2


@pytest.mark.parametrize("precision", PRECISIONS)
def test_distinct_gpus(gpu, precision):
    """Two different GPUs: the peer merge into the first device's frame."""
    if gpu.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    with multi_film("cornell", precision, [0, 1]) as f:
        check_against_single_device(f, "cornell", PASSES, precision)
