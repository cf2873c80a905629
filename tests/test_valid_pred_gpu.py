"""The closest hit's validity rules as compares (rt_trace.h RT_VALID_MARGINS) on the MI355X.

The product takes the compares in the binary64 flat sets' loops (test_box<true>, isect_plane<1>)
and keeps the margins elsewhere (FP32; the BVH kernels' surface prefix, test_box<false>).

1. The `isect` probe (kind 1: isect_plane<1>, compares in binary64) and the `box` probe
   (test_box<false>, margins) on a grid of constructed edge cases, device against host emulator: the
   same decisions, and the same bits of t wherever both accept.  The device build contracts
   a * b + c into FMAs and makes its reciprocals from the hardware's, so its t has the emulator's
   bits only where every intermediate is exact; the grid is therefore dyadic throughout: the unit
   square and boxes whose axes are coordinate axes with power-of-two extents, direction components
   +-1, +-1/2, +-1/4, +-0.  (Records under a rotation are compared with exact references in
   tests/test_shading_probe.py, and the two forms of the rules with each other, test_box<true>
   included, on the host in tests/test_valid_pred_host.py.)  FP32 flushes denormals on the device and
   not in the emulator, so "one ulp from zero" is the smallest normal number there.  Measured: no
   decision and no bit of an accepted t differs (154 plane cases, 156 + 96 + 96 box cases, each
   precision).
2. Frames of small cuts of the Cornell box and of box_gallery (rays that leave a cuboid from inside,
   a reflected box, the room with its missing face; flat classes: test_box<true> in the kernel),
   both precisions, ring form and legacy loop: byte for byte the frames the library of the commit
   before the rewrite renders on the MI355X (tests/golden/valid_pred_frames.json "gpu", recorded
   once from that commit's build of the library loaded through RT_AMD_LIB into this tree, by
   valid_pred_gpu_digests below).
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "device_probe"))
sys.path.insert(0, os.path.join(ROOT, "tests", "kernel_emu"))
import emu  # noqa: E402
import probe  # noqa: E402

pytestmark = pytest.mark.gpu

PRECISIONS = ["f64", "f32"]
KTMIN = 1e-4  # rt_trace.h kTmin


def real_of(precision):
    return np.float64 if precision == "f64" else np.float32


def bits(x):
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def up(x):
    return np.nextafter(x, x.dtype.type(np.inf))


def dn(x):
    return np.nextafter(x, x.dtype.type(-np.inf))


def float_up(x):
    """rt_trace.h float_up: the next real above x > 0"""
    return (bits(np.asarray(x)) + 1).view(np.asarray(x).dtype)


def least(real):
    """one ulp from zero as the device sees it: FP32 denormals are flushed"""
    return np.finfo(real).tiny if real == np.float32 else np.nextafter(real(0), real(1))


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


# ------------------------------------------------------------------ 1a. isect_plane<1>
def plane_rec(real, q, edge):
    """the square (q, edge x, edge y) in the plane z = q.z: n = +z, wa = x / edge, wb = y / edge"""
    r = np.zeros(16, real)
    r[0:3], r[4:7] = (0, 0, 1), q
    r[8], r[13] = 1.0 / edge, 1.0 / edge
    return r


def plane_grid(precision):
    real = real_of(precision)
    tiny = least(real)
    one = real(1)
    rec, o, d, tmin, self_ = [], [], [], [], []
    def case(r, oo, dd, tm, sf=0):
        rec.append(r), o.append(oo), d.append(dd), tmin.append(tm), self_.append(sf)
    unit = plane_rec(real, (0, 0, 0), 1.0)
    # a, b at 0 and 1 and one ulp to each side (a = x, b = y of the hit point, exactly), all pairs
    edge = [real(0), -real(0), tiny, -tiny, one, up(one), dn(one), real(0.5)]
    for a in edge:
        for b in edge:
            for sf in (0, 1):
                case(unit, (a, b, 1), (0, 0, -1), real(KTMIN), sf)
    # t at tmin_up and one ulp to each side (t is exact)
    for tm in (real(KTMIN), real(0.5), real(3)):
        tu = float_up(tm)
        for T in (tm, tu, up(tu), dn(tm), real(0), -tu):
            case(plane_rec(real, (0, 0, T), 4.0), (0.25, 0.25, 0), (0, 0, 1), tm)
    # |n . d| at 1e-8 and one ulp to each side, both signs, and zero (n . d = delta and n . (q - o) = delta exactly)
    e = real(1e-8)
    wide = plane_rec(real, (0, 0, 0), 4.0)
    for dl in (e, up(e), dn(e), -e, -up(e), -dn(e), real(0), -real(0)):
        case(wide, (0.25, 0.25, -dl), (1, 0, dl), real(KTMIN))
    cr = lambda x, w: np.ascontiguousarray(np.array(x, real).reshape(-1, w))  # noqa: E731
    return cr(rec, 16), cr(o, 3), cr(d, 3), np.array(tmin, real), np.array(self_, np.int32)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_plane_edges_device_decides_as_emulator(gpu, precision):
    args = plane_grid(precision)
    n = len(args[0])
    t_e, q_e, take_e = probe.call("emu", precision, "isect", 1, *args)
    t_g, q_g, take_g = probe.call("gpu", precision, "isect", 1, *args)
    acc_e, acc_g = q_e >= 0, q_g >= 0
    print(f"{precision}: {n} cases, emulator accepts {int(acc_e.sum())}, device {int(acc_g.sum())}, decisions differ "
          f"{int((acc_e != acc_g).sum())}, t bits differ on {int((bits(t_e) != bits(t_g))[acc_e & acc_g].sum())} accepted")
    assert 0 < acc_e.sum() < n
    assert (acc_e == acc_g).all(), np.flatnonzero(acc_e != acc_g)[:8]
    assert (take_e == take_g).all()
    both = acc_e & acc_g
    assert (bits(t_e)[both] == bits(t_g)[both]).all(), np.flatnonzero(both & (bits(t_e) != bits(t_g)))[:8]
    assert not np.isnan(t_g[acc_g]).any()


# ------------------------------------------------------------------ 1b. test_box
def box_rec(precision, corner, extent, missing=-1):
    """DevBox of the box [corner, corner + extent] with coordinate axes: face f = 2 axis + side has key order
    10 + f, gid 20 + f and primitive 40 + f; `missing`: a face the box does not have"""
    b = np.zeros(1, emu.record_dtypes(precision)["boxes"])
    for k in range(3):
        a = np.zeros(3)
        a[k] = 1.0 / extent[k]
        b[0][f"a{k}"] = a
        b[0]["sc"][k] = corner[k] / extent[k]
    code = 0
    for f in range(6):
        code |= (31 if f == missing else f) << (5 * f)
    b[0]["ord_base"], b[0]["gid_base"], b[0]["prim_base"] = 10, 20, 40
    b[0]["ord_code"] = b[0]["gid_code"] = b[0]["prim_code"] = code
    return b


BOXES = {"unit": ((0, 0, 0), (1, 1, 1), -1), "aligned": ((8, 0, -4), (2, 4, 2), -1), "room": ((0, 0, 0), (512, 512, 512), 4)}


def box_grid(precision, name):
    real = real_of(precision)
    corner, extent, missing = BOXES[name]
    corner, extent = np.array(corner, np.float64), np.array(extent, np.float64)
    o, d, tmin, gid = [], [], [], []
    def case(s, ds, tm=real(KTMIN), g=-1):  # box-frame coordinates (s_k in [0, 1] inside) and direction
        o.append(corner + np.array(s, np.float64) * extent), d.append(np.array(ds, np.float64) * extent)
        tmin.append(tm), gid.append(g)
    if name == "unit":
        two = real(2)
        # tf == tn (a ray through the edge x = 1, y = 0) and one ulp to each side; z parallel to the ray
        for oy in (-two, up(-two), dn(-two)):
            for dz in (0.0, -0.0):
                for oz in (0.5, 0.0, 1.0, 1.5):
                    case((-1, oy, oz), (1, 1, dz))
        # the entry and the exit at tmin_up and one ulp to each side
        for tm in (real(KTMIN), real(0.5)):
            tu = float_up(tm)
            for T in (tm, tu, up(tu), dn(tm)):
                case((-T, 0.5, 0.5), (1, 0, 0), tm)
                case((real(1) - T, 0.5, 0.5), (1, 0, 0), tm)
                case((T, 0.5, 0.5), (-1, -0.0, 0.0), tm)
        # slabs whose ends overflow to infinities of one sign: a parallel axis, far outside
        for far in (1e30, -1e30):
            for z in (0.0, -0.0):
                case((-1, far, 0.5), (1, z, z))
                case((0.5, far, far), (1, z, -z))
                case((far, far, far), (z, z, 1))
    # rays parallel to one and to two axes (+0 and -0 components), from inside, outside and a face (self)
    zs = (0.0, -0.0)
    for ax in range(3):
        for par2 in (0, 1):
            for sg in range(4):
                for where in range(4):
                    s = [zs[sg & 1], zs[sg >> 1], zs[(sg ^ (sg >> 1)) & 1]]
                    s[ax] = -1.0 if sg & 1 else 1.0
                    if not par2:
                        s[(ax + 1) % 3] = -0.25 if sg & 2 else 0.5
                    p = [0.25, 0.625, 0.375]
                    g = -1
                    if where == 1:
                        p[ax] = -1.5
                    if where == 2:
                        p[ax] = 2.5
                    if where == 3:
                        p[ax] = 0.0 if s[ax] > 0 else 1.0
                        g = 20 + 2 * ax + (0 if s[ax] > 0 else 1)
                    case(p, s, real(KTMIN), g)
    cr = lambda x: np.ascontiguousarray(np.array(x, real).reshape(-1, 3))  # noqa: E731
    return box_rec(precision, corner, extent, missing), cr(o), cr(d), np.array(tmin, real), np.array(gid, np.int32)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(BOXES))
def test_box_edges_device_decides_as_emulator(gpu, name, precision):
    rec, o, d, tmin, gid = box_grid(precision, name)
    n = len(o)
    t_e, prim_e, ord_e = probe.call("emu", precision, "box", 0, rec, o, d, tmin, gid)
    t_g, prim_g, ord_g = probe.call("gpu", precision, "box", 0, rec, o, d, tmin, gid)
    hit_e, hit_g = prim_e >= 0, prim_g >= 0
    print(f"{name} {precision}: {n} cases, emulator hits {int(hit_e.sum())}, device {int(hit_g.sum())}, decisions differ "
          f"{int(((prim_e != prim_g) | (ord_e != ord_g)).sum())}, t bits differ on "
          f"{int((bits(t_e) != bits(t_g))[hit_e & hit_g].sum())} hits")
    assert 0 < hit_e.sum() < n
    assert (prim_e == prim_g).all() and (ord_e == ord_g).all(), np.flatnonzero((prim_e != prim_g) | (ord_e != ord_g))[:8]
    both = hit_e & hit_g
    assert (bits(t_e)[both] == bits(t_g)[both]).all(), np.flatnonzero(both & (bits(t_e) != bits(t_g)))[:8]
    assert np.isinf(t_g[~hit_g]).all()
    if missing_face(name) >= 0:
        assert not (prim_g == 40 + missing_face(name)).any()
    if name == "unit":
        # oy = -2 (tf == tn) and one ulp inside meet the box, one ulp outside misses it (oz = 0.5: between the
        # z faces; oz = 1.5: beside the box, a miss whatever oy)
        edge = hit_g[:24].reshape(3, 2, 4)
        assert edge[:2, :, 0].all() and not edge[2].any() and not edge[:, :, 3].any(), edge


def missing_face(name):
    return BOXES[name][2]


# ------------------------------------------------------------------ 2. frames
SIZES = {"7x5": (7, 5), "16x9": (16, 9)}
FRAME_CASES = [("cornell", "16x9", 5), ("cornell", "7x5", 5), ("box_gallery", "16x9", 3)]


@functools.lru_cache(maxsize=None)
def frame_scene(name, size, spp):
    from raytrace_amd import scenes
    from raytrace_amd.camera import image_height
    from raytrace_amd.scene import flatten
    w, h = SIZES[size]
    cs, world, seed = scenes.cornell_box(spp=spp, width=w) if name == "cornell" else scenes.box_gallery(width=w, spp=spp)
    cs = cs.replace(cs_imageWidth=w, cs_aspectRatio=w / h)
    assert image_height(cs) == h
    return cs, flatten(world), seed


def frame_digest(name, size, spp, precision):
    import raytrace_amd as R
    cs, flat, seed = frame_scene(name, size, spp)
    img = R.raytrace(cs, flat, seed, precision=precision)
    assert img.shape == (SIZES[size][1], SIZES[size][0], 3)
    assert np.isfinite(img).all() and img.mean() > 0
    return hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest()[:16]


def valid_pred_gpu_digests(setenv, delenv):
    """{case: digest} of every frame below, with the library the process has loaded (the recording run
    loads the parent commit's build through RT_AMD_LIB; RT_AMD_EXPERIMENTS is set by the caller)"""
    out = {}
    for name, size, spp in FRAME_CASES:
        for precision in PRECISIONS:
            for loop in ("ring", "legacy"):
                if loop == "legacy":
                    setenv("RT_AMD_FLAT_RING", "0")
                out[f"{name}/{size}/{spp}spp/{precision}/{loop}"] = frame_digest(name, size, spp, precision)
                if loop == "legacy":
                    delenv("RT_AMD_FLAT_RING")
    return out


with open(os.path.join(GOLDEN, "valid_pred_frames.json")) as _f:
    GPU_FRAMES = json.load(_f)["gpu"]


@pytest.mark.parametrize("loop", ["ring", "legacy"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,size,spp", FRAME_CASES)
def test_frames_are_the_parents(knobs, gpu, name, size, spp, precision, loop):
    from raytrace_amd import _lib
    _lib.load()
    if loop == "legacy":
        knobs.setenv("RT_AMD_FLAT_RING", "0")
    got = frame_digest(name, size, spp, precision)
    assert got == GPU_FRAMES[f"{name}/{size}/{spp}spp/{precision}/{loop}"], got
