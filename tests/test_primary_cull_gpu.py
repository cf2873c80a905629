"""The ring loop's camera segments (rt_trace.h lane_loop_flat_ring with RT_RING_PRIMARY,
closest_flat_primary; rt_build.cpp rt_host_cull_rects) on the GPU.

The refill traces the first segment of its 64 samples itself, with the box groups and static
parallelograms that no ray through the lanes' pixels can meet left out, commits the paths that end
there and stores the others as paths past their first segment.  A skipped test is one that would
have reported a miss and the stored state is rebuilt from the same products, so in every case the
frame equals, byte for byte, the frame with every rectangle "every pixel" (RT_AMD_PRIMARY_CULL=0)
and the legacy loop's (RT_AMD_FLAT_RING=0), in binary64 (the form that traces at the refill) and in
FP32 (which keeps the loop that stores camera rays: the same comparisons hold).

`one_wave` cuts the grid to ONE one-wave workgroup (RT_AMD_GRID_RESERVE far above the resident
workgroups: rt_api.hip clamps the grid to 1), which then refills its ring once per 64 ids of the
frame: the cases whose refills store nothing run on it too, so that one wave meets many empty
refills in a row.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raytrace_amd as R  # noqa: E402
from raytrace_amd import _lib, scenes  # noqa: E402
from raytrace_amd.camera import image_height  # noqa: E402
from raytrace_amd.core import V3  # noqa: E402
from raytrace_amd.ray import render_shard  # noqa: E402
from raytrace_amd.scene import flatten  # noqa: E402

PRECISIONS = ["f64", "f32"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    return torch


def cornell(width, height, spp, depth=50, **camera):
    cs, world, seed = scenes.cornell_box(spp=spp, depth=depth, width=width)
    cs = cs.replace(cs_aspectRatio=width / height, **camera)
    assert image_height(cs) == height
    return cs, flatten(world), seed


def gallery(width, height, spp):
    cs, world, seed = scenes.box_gallery(width=width, spp=spp)
    cs = cs.replace(cs_aspectRatio=width / height)
    assert image_height(cs) == height
    return cs, flatten(world), seed


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def three_ways(knobs, fn):
    """fn() with culling, with every rectangle "every pixel", and by the legacy loop"""
    img = fn()
    knobs.setenv("RT_AMD_PRIMARY_CULL", "0")
    plain = fn()
    knobs.delenv("RT_AMD_PRIMARY_CULL")
    knobs.setenv("RT_AMD_FLAT_RING", "0")
    legacy = fn()
    knobs.delenv("RT_AMD_FLAT_RING")
    assert same(img, plain), "culled and unculled camera segments differ"
    assert same(img, legacy), "the ring loop and the legacy loop differ"
    return img


def grid(knobs, which):
    if which == "one_wave":
        knobs.setenv("RT_AMD_GRID_RESERVE", "1000000")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("spp", [1, 3, 70, 200])
def test_cornell_48x48(knobs, gpu, spp, precision):
    """refills that span many pixels (1, 3 spp: 64 and 22 of them, across a row's end), one or two (70,
    which does not divide 64, and 200), and pixels on both sides of every rectangle's edges"""
    cs, flat, seed = cornell(48, 48, spp)
    img = three_ways(knobs, lambda: R.raytrace(cs, flat, seed, precision=precision))
    assert np.isfinite(img).all() and img.mean() > 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("which", ["own_grid", "one_wave"])
@pytest.mark.parametrize("depth", [1, 2])
def test_paths_that_end_in_the_refill(knobs, gpu, depth, which, precision):
    """max_depth 1: every path ends on its first segment, no refill stores an entry and the ring stays
    empty to the end of the queues; max_depth 2: the stored paths end on the segment they are
    popped for.  Only the light's direct view is not black at depth 1."""
    grid(knobs, which)
    cs, flat, seed = cornell(16, 9, 5, depth=depth)
    img = three_ways(knobs, lambda: R.raytrace(cs, flat, seed, precision=precision))
    assert np.isfinite(img).all() and img.max() > 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("which", ["own_grid", "one_wave"])
def test_camera_turned_away(knobs, gpu, which, precision):
    """every camera ray misses the scene (the background is black): refills that store nothing, one
    after the other, until the queues are drained.  The room lies behind the camera: its rectangle is
    "every pixel"."""
    grid(knobs, which)
    cs, flat, seed = cornell(16, 9, 5, cs_lookAt=V3(278, 278, -2000))
    img = three_ways(knobs, lambda: R.raytrace(cs, flat, seed, precision=precision))
    assert (img == 0).all()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("camera", ["inside", "corner_behind", "defocus"])
def test_cameras_without_rectangles(knobs, gpu, camera, precision):
    """a camera inside the room, one beside the tall box with some of its corners behind the image
    plane, and a defocus camera (rays from a disk, not a point)"""
    extra = {"inside": dict(cs_center=V3(278, 278, 20), cs_lookAt=V3(278, 278, 555)),
             "corner_behind": dict(cs_center=V3(255, 200, 350), cs_lookAt=V3(455, 200, 450)),
             "defocus": dict(cs_defocusAngle=0.02, cs_focusDist=1000.0)}[camera]
    cs, flat, seed = cornell(24, 16, 7, **extra)
    img = three_ways(knobs, lambda: R.raytrace(cs, flat, seed, precision=precision))
    assert np.isfinite(img).all() and img.mean() > 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_box_gallery(knobs, gpu, precision):
    """a second set of box groups, under transforms (one of them a reflection)"""
    cs, flat, seed = gallery(16, 9, 3)
    img = three_ways(knobs, lambda: R.raytrace(cs, flat, seed, precision=precision))
    assert np.isfinite(img).all() and img.mean() > 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("height", [30, 31])
def test_shard_rows_interleaved(knobs, gpu, height, precision):
    """shard 1 of 3 with one-row blocks: the tile's rows are the frame's rows 1, 4, 7, ... (the
    rectangles are in the frame's rows, as the lanes' pixels).  With 31 rows the shard's last row,
    31, is a padding row: ids without a sample in the middle of a refill."""
    cs, flat, seed = cornell(30, height, 9)
    img = three_ways(knobs, lambda: render_shard(cs, flat, seed, 3, 1, row_block=1, precision=precision))
    assert img.shape == ((height + 2) // 3, 30, 3) and np.isfinite(img[:10]).all() and img.mean() > 0
