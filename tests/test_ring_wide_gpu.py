"""The ring loop's deferred commit (rt_trace.h lane_loop_flat_ring, flush_ring) against the legacy
loop (RT_AMD_FLAT_RING=0) on the GPU.

A lane whose path ends keeps its sample; the ring entry it pops next holds the sample until the
wave converts and commits the ring's samples 64 wide before its next refill, and once more after
the loop.  Only the moment of the integer additions moves, so every comparison is of bytes.

The scene is the Cornell box cut to 7x5 and 16x9 pixels.  At these sizes the launch has one wave
per 64 ids (rt_render_kernel.h rt_launch_render), so each wave refills its ring once, every entry
is popped by a lane that holds nothing, and all samples are committed after the loop: the deposit
at a pop and flush_ring would see only -1 tags.  The `one_wave` fixture therefore renders with a
grid of ONE one-wave workgroup (RT_AMD_GRID_RESERVE far above the resident workgroups: rt_api.hip
clamps the grid to 1), whose wave claims every id of the frame: 16x9 at 65 spp is 9360 ids, 146
full refills and one of 16.  From the second refill on, the lanes that pop hold finished samples,
leave them in the entries, and the flush before the next refill commits them.  The legacy render
of each shape is made once, under the same knobs, and shared.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raytrace_amd as R  # noqa: E402
from raytrace_amd import _lib, scenes  # noqa: E402
from raytrace_amd.camera import image_height  # noqa: E402
from raytrace_amd.material import constantTexture, lightSource  # noqa: E402
from raytrace_amd.scene import flatten  # noqa: E402

SIZES = {"7x5": (7, 5), "16x9": (16, 9)}
PRECISIONS = ["f64", "f32"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    return torch


@pytest.fixture
def one_wave(knobs):
    """the render grid cut to one workgroup (the ring kernel's is one wave): one wave claims every
    id, so it refills its ring ceil(ids / 64) times"""
    knobs.setenv("RT_AMD_GRID_RESERVE", "1000000")
    return knobs


def cut(cs, size):
    w, h = SIZES[size]
    cs = cs.replace(cs_imageWidth=w, cs_aspectRatio=w / h)
    assert image_height(cs) == h
    return cs


@functools.lru_cache(maxsize=None)
def scene(size, spp):
    cs, world, seed = scenes.cornell_box(spp=spp, width=SIZES[size][0])
    return cut(cs, size), flatten(world), seed


@functools.lru_cache(maxsize=None)
def scene_with_infinite_light(size, spp):
    """the Cornell world with a light whose red component is 1e300.  The scene builder refuses a
    colour that is not finite (RtInvalid), so this is the largest a light can emit: infinite once
    the FP32 scene converts it, and in binary64 far past the 1e9 beyond which acc_sample takes a
    sample for non-finite and flags its pixel"""
    from raytrace_amd.core import V3, degrees, fromCorners
    from raytrace_amd.geometry import cuboid, group, parallelogram, rotateY, transform, translate
    walls, white = scenes.cornell_walls()
    light = lightSource(constantTexture(V3(1e300, 15.0, 15.0)))
    walls[2] = light << parallelogram(V3(343, 554, 332), V3(-130, 0, 0), V3(0, 0, -105))
    world = group(walls + [
        transform(translate(V3(265, 0, 295)) @ rotateY(degrees(15)),
                  white << cuboid(fromCorners(V3(0, 0, 0), V3(165, 330, 165)))),
        transform(translate(V3(130, 0, 65)) @ rotateY(degrees(-18)),
                  white << cuboid(fromCorners(V3(0, 0, 0), V3(165, 165, 165)))),
    ])
    cs, _, seed = scenes.cornell_box(spp=spp, width=SIZES[size][0])
    return cut(cs, size), flatten(world), seed


def render(size, spp, precision, make=scene):
    cs, flat, seed = make(size, spp)
    return R.raytrace(cs, flat, seed, precision=precision)


_legacy = {}


def legacy(knobs, key, fn):
    """fn() under RT_AMD_FLAT_RING=0 (and the knobs already set), once per key (read-only afterwards)"""
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
@pytest.mark.parametrize("spp", [3, 65])
@pytest.mark.parametrize("size", list(SIZES))
def test_small_pools_on_one_wave(one_wave, gpu, size, spp, precision):
    """One wave, pools of 64 ids, the smallest the queue serves to a wave that asks for 64 at once
    (WaveWork::grab takes a pool that leaves the wave's demand unmet for the queue's last: with 16
    ids per pool and one wave, the queues count as spent after five pools and the rest of the
    frame is never claimed, in the parent as here; rt_host_plan_ring itself stops at 64).  Every
    refill opens a pool and, at 65 spp, a slot; the 6 (binary64) / 5 (FP32) slots are reclaimed
    lazily, and only those whose count the flush has brought to zero, while samples of other pools
    still wait in lanes and in the ring; a pool that finds every slot busy commits directly.  At 3
    spp a pool spans 22 pixels, more than a slot's 8: no aggregation, every commit is direct.  At
    65 spp the last refill is short (7x5: 35 of 64, 16x9: 16) and lies under entries that hold the
    previous generation's committed samples."""
    one_wave.setenv("RT_AMD_POOL_SHIFT", "6")
    want = legacy(one_wave, ("pool1", size, spp, precision), lambda: render(size, spp, precision))
    img = render(size, spp, precision)
    assert same(img, want)
    assert np.isfinite(img).all() and img.mean() > 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("spp", [3, 65])
@pytest.mark.parametrize("shift", [4, 6])
@pytest.mark.parametrize("size", list(SIZES))
def test_small_pools(knobs, gpu, size, shift, spp, precision):
    """Pools of 16 and 64 ids on the launch's own grid, one wave per 64 ids.  With 16, a wave's first
    refill of 64 ids spans its static pool and three from the queues, four slots at once; the wave
    refills once, seldom twice, and commits its samples after the loop (64 is what the plan
    chooses by itself at these sizes)."""
    knobs.setenv("RT_AMD_POOL_SHIFT", str(shift))
    want = legacy(knobs, ("pool", size, shift, spp, precision), lambda: render(size, spp, precision))
    img = render(size, spp, precision)
    assert same(img, want)
    assert np.isfinite(img).all() and img.mean() > 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("size", list(SIZES))
def test_direct_commits(one_wave, gpu, size, precision):
    """no aggregation: the tag is the plain tile pixel (tile pixel 0 and the last one among them,
    none of them the -1 of "no sample held") and every word goes to the global sums"""
    one_wave.setenv("RT_AMD_AGG", "0")
    want = legacy(one_wave, ("direct", size, precision), lambda: render(size, 65, precision))
    img = render(size, 65, precision)
    assert same(img, want)
    assert np.isfinite(img).all() and img.mean() > 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_last_refill_far_below_64(one_wave, gpu, precision):
    """7x5 on one wave.  1 spp: 35 ids, one short refill, nothing deferred.  2 spp: 70 ids, a full
    refill and one of 6 whose entries take real samples; the 58 entries above hold the first
    generation's -1.  5 spp: 175 ids = 64 + 64 + 47: the second generation's 64 entries all take
    real samples, the flush before the third refill commits them, and the 17 entries above the
    third refill's 47 still hold those tags when the wave flushes after the loop: an entry above
    the last refill's count must not be added again."""
    imgs = []
    for spp in (1, 2, 5):
        want = legacy(one_wave, ("7x5", spp, precision), lambda: render("7x5", spp, precision))
        img = render("7x5", spp, precision)
        assert same(img, want)
        assert np.isfinite(img).all()
        imgs.append(img)
    assert imgs[0].sum() != imgs[1].sum()  # (samples are not all dropped)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_non_finite_sample_flags_its_pixel(one_wave, gpu, precision):
    """a light with a component past every finite sample: a lane that ends such a path pops a ray
    of another pixel before the sample is converted, and the flush must flag the pixel the sample
    belongs to, not the one the lane traces by then"""
    fn = lambda: render("16x9", 65, precision, scene_with_infinite_light)  # noqa: E731
    want = legacy(one_wave, ("inf", precision), fn)
    img = fn()
    assert same(img, want)
    nan = np.isnan(img).any(-1)
    assert nan.any() and np.isfinite(img[~nan]).all() and (~nan).any()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_renders_with_small_pools_are_equal(one_wave, gpu, precision):
    one_wave.setenv("RT_AMD_POOL_SHIFT", "6")
    a, b = render("16x9", 65, precision), render("16x9", 65, precision)
    assert same(a, b)
    assert np.isfinite(a).all() and a.mean() > 0
