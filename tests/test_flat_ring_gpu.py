"""The ring form of the flat lane loop (rt_trace.h lane_loop_flat_ring) against the legacy loop
(RT_AMD_FLAT_RING=0) on the GPU.

Both render every (pixel, sample) pair once with the same Philox counters and add the same
fixed-point words, so every comparison is of bytes.  The scene is the Cornell box (the one class
with a ring form) cut down to a few pixels; the shapes sit where the ring can go wrong: sample
counts around the 64-lane refill, a stream range that crosses pixels, depth 1 (every lane pops in
every iteration) and 0 (no sample at all), padding rows, a later film pass, two streams.  The legacy
render of each shape is made once and shared.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raytrace_amd as R  # noqa: E402
from raytrace_amd import _lib, scenes  # noqa: E402
from raytrace_amd.camera import image_height  # noqa: E402
from raytrace_amd.ray import DeviceScene, render_shard  # noqa: E402
from raytrace_amd.scene import flatten  # noqa: E402

SIZES = {"7x5": (7, 5), "16x9": (16, 9)}
SPPS = [1, 3, 63, 64, 65, 130]
PRECISIONS = ["f64", "f32"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    return torch


@functools.lru_cache(maxsize=None)
def scene(size, spp, depth=50):
    w, h = SIZES[size]
    cs, world, seed = scenes.cornell_box(spp=spp, depth=depth, width=w)
    cs = cs.replace(cs_aspectRatio=w / h)
    assert image_height(cs) == h
    return cs, flatten(world), seed


def render(size, spp, precision, depth=50):
    cs, flat, seed = scene(size, spp, depth)
    return R.raytrace(cs, flat, seed, precision=precision)


_legacy = {}


def legacy(knobs, key, fn):
    """fn() under RT_AMD_FLAT_RING=0, once per key (read-only afterwards)"""
    if key not in _legacy:
        knobs.setenv("RT_AMD_FLAT_RING", "0")
        img = fn()
        knobs.delenv("RT_AMD_FLAT_RING")
        img.setflags(write=False)
        _legacy[key] = img
    return _legacy[key]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("size", list(SIZES))
def test_ring_equals_the_legacy_loop(knobs, gpu, size, spp, precision):
    want = legacy(knobs, (size, spp, precision), lambda: render(size, spp, precision))
    img = render(size, spp, precision)
    assert same(img, want)
    assert np.isfinite(img).all() and img.mean() > 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("depth", [1, 0])
def test_depth_one_and_none(knobs, gpu, depth, precision):
    """depth 1: every path ends at its first hit, so every lane pops a ray in every iteration and the
    ring refills every iteration; depth 0: no id has a sample, the image is black"""
    want = legacy(knobs, ("16x9", 65, precision, depth), lambda: render("16x9", 65, precision, depth))
    img = render("16x9", 65, precision, depth)
    assert same(img, want)
    assert (img.max() > 0) == (depth > 0)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_shards_with_padding_rows(knobs, gpu, precision):
    """5 rows in 3 shards of 2-row blocks: shards 0 and 1 hold 2 rows, shard 2 one row and a padding row"""
    cs, flat, seed = scene("7x5", 65)
    for shard in range(3):
        fn = lambda: render_shard(cs, flat, seed, 3, shard, row_block=2, precision=precision)  # noqa: E731
        want = legacy(knobs, ("shard", shard, precision), fn)
        tile = fn()
        assert tile.shape == (2, 7, 3) and same(tile, want)
    assert not _legacy[("shard", 2, precision)][1].any()  # (the padding row)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_film_passes_equal_one_render(knobs, gpu, precision):
    """samples [0, 63) then [63, 130) (sample0 > 0 shifts the stream's sample index) against one
    render of 130, the ring's and the legacy loop's"""
    cs, flat, seed = scene("16x9", 130)
    want = legacy(knobs, ("16x9", 130, precision), lambda: render("16x9", 130, precision))
    with R.Film(flat, cs.replace(cs_samplesPerPixel=1), seed, precision=precision) as f:
        img = f.add(63).add(67).image()
    assert same(img, want)
    assert same(render("16x9", 130, precision), want)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_frames_on_two_streams(knobs, gpu, precision):
    """the overlapped plan (rt_render_async: 512-id pools): one frame on a stream of its own, the
    next on another stream, each equal to the legacy loop's"""
    torch = gpu
    cs, flat, seed = scene("16x9", 130)
    dtype = torch.float64 if precision == "f64" else torch.float32

    def frames():
        sc = DeviceScene(flat)
        try:
            outs = [torch.zeros((9, 16, 3), dtype=dtype, device="cuda") for _ in range(2)]
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            for k in range(2):
                sc.render_async(cs, 234 + k, outs[k].data_ptr(), stream_ptr=streams[k].cuda_stream, precision=precision)
            torch.cuda.synchronize()
            return np.stack([o.cpu().numpy() for o in outs])
        finally:
            sc.close()

    want = legacy(knobs, ("streams", precision), frames)
    got = frames()
    assert same(got, want)
    assert not same(got[0], got[1]) and got.mean() > 0  # (two seeds: two frames)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_renders_of_one_frame_are_equal(gpu, precision):
    a, b = render("16x9", 65, precision), render("16x9", 65, precision)
    assert same(a, b)
