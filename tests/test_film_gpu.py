"""The progressive film on the GPU (include/rt.h rt_film_*, raytrace_amd.film).

The sample index is a word of the Philox counter and the per-pixel sums are integers, so every
comparison of a film against the one-shot render of the same sample count is bit for bit
(np.array_equal).  The noise estimate is compared with its numpy restatement
(film.noise_from_sums) on the pass sums recovered from the saved states: 4 ulp per pixel (the same
operation sequence; float32 ulps, the map's type), and the frame figure against math.fsum to
n_pixels 2^-53 relative (the device adds n_pixels terms in a fixed tree).
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from conftest import record_measure

pytestmark = pytest.mark.gpu

import raytrace_amd as R  # noqa: E402
from raytrace_amd import _lib, film, scenes  # noqa: E402
from raytrace_amd.ray import assemble_shards  # noqa: E402
from raytrace_amd.scene import flatten  # noqa: E402

SCENES = {"cornell": (scenes.cornell_box, 48), "bunny_cornell": (scenes.bunny_cornell, 40),
          "pawn_fog": (scenes.pawn_fog, 40)}
PASSES = [1, 7, 3, 16, 5]


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
    """The reference of every comparison: one render of `spp` samples (computed once, read-only)."""
    cs, flat, seed = scene(name, width)
    img = R.raytrace(cs.replace(cs_samplesPerPixel=spp), flat, seed, precision=precision)
    img.setflags(write=False)
    return img


def new_film(name, precision, width=None, **kw):
    cs, flat, seed = scene(name, width)
    return R.Film(flat, cs, seed, precision=precision, **kw)


def ulps32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def pass_sums(states):
    """Per-pass RGB sums (K, rows, width, 3) from the states saved after each pass."""
    hi = [film.unpack_state(s)["sums"][..., :3] for s in states]
    return np.stack([hi[0]] + [b - a for a, b in zip(hi, hi[1:])])


KNOBS = {"default": {}, "two_sizes": {"RT_AMD_CHUNK": "3", "RT_AMD_BIG_CHUNK": "5", "RT_AMD_TAIL_SAMPLES": "3"},
         "no_agg": {"RT_AMD_AGG": "0"}}


@pytest.mark.parametrize("mode", list(KNOBS))
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", list(SCENES))
def test_passes_equal_the_one_shot_render(knobs, gpu, name, precision, mode):
    """Passes of 1, 7, 3, 16 and 5 samples against one render of 32: flat, BVH and media kernels, both
    precisions; with two item sizes forced (big items of 5 samples, a tail of 3-sample items) and
    with every item committed directly (no LDS aggregation)."""
    want = one_shot(name, sum(PASSES), precision)
    for k, v in KNOBS[mode].items():
        knobs.setenv(k, v)
    with new_film(name, precision) as f:
        for n in PASSES:
            f.add(n)
        assert (f.spp, f.passes) == (sum(PASSES), len(PASSES))
        img = f.image()
    assert img.dtype == want.dtype and img.shape == want.shape
    assert np.array_equal(img, want, equal_nan=True)
    assert np.isfinite(img).all() and img.mean() > 0


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_passes_in_the_stealing_regime(gpu, precision):
    """8 x 8 pixels, two passes of 300 samples against 600: the queue drains at once and most samples
    are rendered by lanes that took them from another lane's item (absolute sample indices move)."""
    want = one_shot("cornell", 600, precision, 8)
    with new_film("cornell", precision, 8) as f:
        img = f.add(300).add(300).image()
    assert np.array_equal(img, want, equal_nan=True) and img.mean() > 0


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_intermediate_images_equal_the_one_shot_renders(gpu, precision):
    with new_film("cornell", precision) as f:
        total = 0
        for n in PASSES:
            total += n
            assert np.array_equal(f.add(n).image(), one_shot("cornell", total, precision), equal_nan=True), total
        f.reset()
        assert (f.spp, f.passes) == (0, 0)
        assert np.array_equal(f.add(8).image(), one_shot("cornell", 8, precision), equal_nan=True)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_shard_films_assemble_to_the_image(gpu, precision):
    """Width 50 in 3 shards of 4-row blocks: 13 blocks, so 20-row tiles with padding rows.  The
    tiles of three films equal the one-shot image; padding rows are NaN in the noise map."""
    want = one_shot("cornell", 8, precision, 50)
    h = want.shape[0]
    tiles, maps = [], []
    for r in range(3):
        with new_film("cornell", precision, 50, n_shards=3, shard=r, row_block=4) as f:
            f.add(4).add(4)
            tiles.append(f.image())
            maps.append(f.noise_map())
            assert math.isfinite(f.noise())
    assert tiles[0].shape == (20, 50, 3)
    assert np.array_equal(assemble_shards(tiles, h, 4), want, equal_nan=True)
    n_pad = 0
    for r in range(3):
        pad = R.ray.shard_row_index(h, 3, r, 4) >= h
        n_pad += int(pad.sum())
        assert np.isnan(maps[r][pad]).all() and np.isfinite(maps[r][~pad]).all()
    assert n_pad == 3 * 20 - h > 0


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_noise_matches_the_numpy_estimator(gpu, precision):
    sizes = [2, 5, 1, 8, 4]
    with new_film("cornell", precision) as f, new_film("cornell", precision) as g:
        states = []
        for n in sizes:
            states.append(f.add(n).state())
            g.add(n)
        got_map, got = f.noise_map(), f.noise()
        assert got == g.noise()  # bitwise: a fixed reduction order, no floating-point atomics
        assert np.array_equal(got_map, g.noise_map())
        q = film.unpack_state(states[-1])["q"]
    want = film.noise_from_sums(pass_sums(states), sizes)
    worst = float(ulps32(got_map, want["r"]).max())
    n_pix = got_map.size
    rel = abs(got - want["noise"]) / want["noise"]
    q_ulps = float((np.abs(q - want["q"]) / np.spacing(np.maximum(q, want["q"]))).max())
    record_measure("film", dict(test="noise_matches", precision=precision, noise=got, numpy_noise=want["noise"],
                                rel=rel, map_ulps32=worst, q_ulps=q_ulps))
    assert np.isfinite(got_map).all() and got > 0
    assert q_ulps <= 4
    assert worst <= 4
    assert rel <= n_pix * 2.0 ** -53


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_noise_falls_with_the_sample_count(gpu, precision):
    """Equal passes of 4 samples: the figure after 16 passes is below the figure after 4 (the
    1 / sqrt(N) law predicts half; only the decrease is asserted)."""
    with new_film("cornell", precision) as f:
        for _ in range(4):
            f.add(4)
        n4 = f.noise()
        for _ in range(12):
            f.add(4)
        n16 = f.noise()
    record_measure("film", dict(test="noise_falls", precision=precision, noise_4x4=n4, noise_16x4=n16, ratio=n16 / n4))
    assert 0 < n16 < n4


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_save_and_load_resume_exactly(gpu, precision):
    """4 + 4 samples in one film against 4, save, a fresh film, load, 4: images and noise maps
    bitwise equal, and the image the one-shot's at 8.  Width 37: an odd pixel count (the merge's
    vector tail).  A state of another width, precision or seed is refused."""
    w = 37
    with new_film("cornell", precision, w) as a:
        img_a, map_a = a.add(4).add(4).image(), a.noise_map()
    with new_film("cornell", precision, w) as b:
        state = b.add(4).state()
    assert state.dtype == np.uint8 and film.unpack_state(state)["header"]["samples"] == 4
    with new_film("cornell", precision, w) as c:
        c.restore(state)
        assert (c.spp, c.passes) == (4, 1)
        img_c, map_c = c.add(4).image(), c.noise_map()
        state8 = c.state()
    assert np.array_equal(img_a, img_c, equal_nan=True) and np.array_equal(map_a, map_c, equal_nan=True)
    assert np.array_equal(img_a, one_shot("cornell", 8, precision, w), equal_nan=True)
    other = "f32" if precision == "f64" else "f64"
    for kw in (dict(width=w + 1), dict(width=w, precision=other)):
        with new_film("cornell", kw.get("precision", precision), kw["width"]) as d:
            with pytest.raises(R.RtInvalid, match="does not match"):
                d.restore(state)
            assert d.spp == 0
    cs, flat, seed = scene("cornell", w)
    with R.Film(flat, cs, 12345, precision=precision) as e:
        with pytest.raises(R.RtInvalid, match="does not match"):
            e.restore(state)
        with pytest.raises(R.RtInvalid):
            e.restore(state8[:-8])
        with pytest.raises(R.RtInvalid):
            e.restore(np.zeros(16, np.uint8))


def test_raytrace_until(gpu):
    cs, flat, seed = scene("cornell")
    # a bar no frame meets: runs to max_spp (the last pass cut to fit)
    img, info = R.raytrace_until(cs, flat, seed, 0.0, batch=5, max_spp=11)
    assert (info["spp"], info["passes"], info["converged"]) == (11, 3, False)
    assert np.array_equal(img, one_shot("cornell", 11, "f64"), equal_nan=True)
    # max_spp defaults to the settings' sample count
    img, info = R.raytrace_until(cs.replace(cs_samplesPerPixel=8), flat, seed, 0.0, batch=4, precision="f32")
    assert info["spp"] == 8 and np.array_equal(img, one_shot("cornell", 8, "f32"), equal_nan=True)
    # a bar every frame meets: stops at the first check, after two passes
    img, info = R.raytrace_until(cs, flat, seed, 1e9, batch=4, max_spp=64)
    assert (info["spp"], info["passes"], info["converged"]) == (8, 2, True) and info["noise"] <= 1e9
    assert np.array_equal(img, one_shot("cornell", 8, "f64"), equal_nan=True)


def test_invalid_film_calls(gpu):
    cs, flat, seed = scene("cornell")
    dev = R.DeviceScene(flat)
    try:
        with R.Film(dev, cs, seed) as f:  # (a caller's DeviceScene: the film leaves it open)
            with pytest.raises(R.RtInvalid, match="two passes"):
                f.noise()
            with pytest.raises(R.RtInvalid):
                f.image()  # no samples yet
            for n in (0, -3, film.MAX_SAMPLES + 1):
                with pytest.raises(R.RtInvalid):
                    f.add(n)
            f.add(2)
            with pytest.raises(R.RtInvalid, match="two passes"):
                f.noise_map()
            assert f.info() == dict(samples=2, passes=1, width=48, rows=48, nan_pixels=0, f32=False)
            assert np.array_equal(f.image(), one_shot("cornell", 2, "f64"), equal_nan=True)
        # a film lives on one device: an rt_exec with a device list is refused
        L = _lib.load()
        c, ex, h = _lib.camera_struct(cs), _lib.exec_struct(devices=[0]), ctypes.c_void_p()
        assert L.rt_film_create(dev.handle, ctypes.byref(c), 1, ctypes.byref(ex), ctypes.byref(h)) == _lib.RT_E_INVALID
        assert b"n_devices" in L.rt_last_error() and h.value is None
        # the scene still renders after its film is gone
        with R.Film(dev, cs, seed, precision="f32") as g:
            assert np.array_equal(g.add(1).add(1).image(), one_shot("cornell", 2, "f32"), equal_nan=True)
    finally:
        dev.close()
