"""ctypes front-end of the host emulator of the kernel logic (TEST TOOLING)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.environ.get("RT_EMU_LIB") or os.path.join(HERE, "_build", "librt_emu.so")  # env: sanitizer builds (tests/test_sanitizers.py)
_lib = None


def build():
    subprocess.run(["make", "-C", HERE, "-s"], check=True)


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        _lib.rt_emu_last_error.restype = ctypes.c_char_p
    return _lib


def render(settings, world, seed, n_shards=1, shard=0, row_block=4, nthreads=None, chunk=0, counters=False,
           precision="f64"):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from raytrace_amd import _lib as R
    from raytrace_amd.camera import image_height
    from raytrace_amd.ray import _seed64, shard_rows
    from raytrace_amd.scene import FlatScene, flatten
    flat = world if isinstance(world, FlatScene) else flatten(world)
    cs = R.camera_struct(settings)
    sc = R.scene_struct(flat)
    ex = R.exec_struct(0, n_shards, shard, row_block)
    h = image_height(settings)
    rows = shard_rows(h, n_shards, row_block)
    out = np.zeros((rows, int(settings.cs_imageWidth), 3), np.float64 if precision == "f64" else np.float32)
    L = lib()
    cnt = np.zeros(4, np.int64)
    rc = L.rt_emu_render(ctypes.byref(cs), ctypes.byref(sc), ctypes.c_uint64(_seed64(seed)), ctypes.byref(ex),
                         out.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(nthreads or min(16, os.cpu_count() or 1)),
                         ctypes.c_int(chunk), cnt.ctypes.data_as(ctypes.c_void_p),
                         ctypes.c_int(1 if precision == "f64" else 0))
    if rc != 0:
        raise RuntimeError(f"rt_emu_render failed {rc}: {L.rt_emu_last_error().decode()}")
    if counters:
        return out, dict(zip(["bvh_nodes", "prims_tested", "segments", "samples"], cnt.tolist()))
    return out


def render_params(settings, world, seed, n_shards=1, shard=0, row_block=4, chunk=0, precision="f64"):
    """{member: [values]} of the KernelParams render() builds for these arguments (rt_emu_render_params:
    every number exactly, as a double; a pointer as 0.0 for null or 1.0)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from raytrace_amd import _lib as R
    from raytrace_amd.ray import _seed64
    from raytrace_amd.scene import FlatScene, flatten
    flat = world if isinstance(world, FlatScene) else flatten(world)
    cs, sc, ex = R.camera_struct(settings), R.scene_struct(flat), R.exec_struct(0, n_shards, shard, row_block)
    names, counts, values, n = (ctypes.c_char_p * 128)(), (ctypes.c_int * 128)(), np.zeros(1024), (ctypes.c_int * 2)()
    rc = lib().rt_emu_render_params(ctypes.byref(cs), ctypes.byref(sc), ctypes.c_uint64(_seed64(seed)), ctypes.byref(ex),
                                    ctypes.c_int(precision == "f64"), ctypes.c_int(chunk), names, counts, 128,
                                    values.ctypes.data_as(ctypes.c_void_p), len(values), n)
    if rc != 0:
        raise RuntimeError(f"rt_emu_render_params failed {rc}: {lib().rt_emu_last_error().decode()}")
    assert n[0] <= 128 and n[1] <= len(values), (n[0], n[1])
    ends = np.cumsum(counts[:n[0]])
    return {names[i].decode(): values[ends[i] - counts[i]:ends[i]].tolist() for i in range(n[0])}


def scene_info(world):
    """n_nodes, surface_nodes, max_depth, n_prims, flat, box groups, surface-prefix primitives and
    the one-class leaf kind (1 static triangles, 2 static spheres, 0 mixed) of the host build of
    `world`."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from raytrace_amd import _lib as R
    from raytrace_amd.scene import FlatScene, flatten
    flat = world if isinstance(world, FlatScene) else flatten(world)
    sc = R.scene_struct(flat)
    info = np.zeros(8, np.int32)
    rc = lib().rt_emu_scene_info(ctypes.byref(sc), info.ctypes.data_as(ctypes.c_void_p))
    if rc != 0:
        raise RuntimeError(f"rt_emu_scene_info failed {rc}: {lib().rt_emu_last_error().decode()}")
    return dict(zip(["n_nodes", "surface_nodes", "max_depth", "n_prims", "flat", "boxes", "prefix", "leaf_kind"], info.tolist()))


def scene_variant(world):
    """The variant code (rt_internal.h RT_VAR_*) the host build gives `world`: rt_host_variant(H)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from raytrace_amd import _lib as R
    from raytrace_amd.scene import FlatScene, flatten
    flat = world if isinstance(world, FlatScene) else flatten(world)
    sc = R.scene_struct(flat)
    v = ctypes.c_int(-1)
    rc = lib().rt_emu_scene_variant(ctypes.byref(sc), ctypes.byref(v))
    if rc != 0:
        raise RuntimeError(f"rt_emu_scene_variant failed {rc}: {lib().rt_emu_last_error().decode()}")
    return v.value


def variant_of(flat, n_media, noise, mats, tex, inst, leaf_kind, media_late, stack_depth):
    """The scalar rt_host_variant(...) of rt_build.cpp, passed through."""
    return int(lib().rt_emu_variant_of(*(ctypes.c_int(int(x)) for x in (flat, n_media, noise, mats, tex, inst, leaf_kind,
                                                                         media_late, stack_depth))))


def class_of(precision, variant):
    """rt_class_of(f64, variant) of rt_kernel_class.h: ((var, tex, media, mats, inst, leaf, narrow),
    rt_class_block, rt_class_compiled)."""
    out = (ctypes.c_int * 9)()
    lib().rt_emu_class_of(ctypes.c_int(precision == "f64"), ctypes.c_int(variant), out)
    return tuple(out[:7]), out[7], bool(out[8])


_ARRAYS = ["prims", "prim_uv", "flat_recs", "motions", "uvframes", "texels", "perlin_grad", "prim_shade", "mats",
           "texs", "boxes", "instances", "media"]
# the items of rt_emu_scene_digest, in its order (rt_emu.cpp)
DIGEST_ITEMS = (["nodes", "perlin_perm", "prim_mat", "flat_sets", "scalars"] + ["f32." + a for a in _ARRAYS]
                + ["f64." + a for a in _ARRAYS])


def record_dtypes(precision):
    """numpy layouts (C alignment, padding included) of the Dev* records of rt_internal.h in one
    precision, and of the plain arrays scene_arrays returns."""
    R = "<f8" if precision == "f64" else "<f4"
    i = "<i4"
    return {
        "mats": np.dtype([("kind", i), ("tex", i), ("param", R), ("tex_const", i), ("c0", R, (3,)), ("pad", R)], align=True),
        "texs": np.dtype([("kind", i), ("nu", i), ("nv", i), ("off", i), ("c0", R, (3,)), ("c1", R, (3,)),
                          ("prm", R, (8,)), ("pad", R, (2,))], align=True),
        "boxes": np.dtype([("sc", R, (3,)), ("ord_base", i), ("a0", R, (3,)), ("ord_code", i), ("a1", R, (3,)),
                           ("gid_base", i), ("a2", R, (3,)), ("gid_code", i), ("prim_base", i), ("prim_code", i),
                           ("pad", i, (2,))], align=True),
        "flat_sets": np.dtype([("first", i), ("end_quad", i), ("end_tri", i), ("end_sphere", i), ("end", i),
                               ("box_first", i), ("box_end", i), ("pad", i)], align=True),
        "targets": np.dtype([(k, R, (3,)) for k in ("q", "u", "v", "n", "wa", "wb", "cr")]
                            + [("prob", R), ("thresh", R), ("prob_icr", R)], align=True),
    }


SCENE_ARRAYS = ["prims", "prim_uv", "prim_shade", "mats", "texs", "texels", "uvframes", "boxes", "perlin_perm",
                "perlin_grad", "flat_sets", "flat_recs"]


def scene_arrays(world, precision="f64"):
    """{name: array} of the host build of `world` in one precision (rt_emu_scene_arrays, read-only):
    prims (n, 16), prim_uv (n, 6), flat_recs (n, 16), uvframes (n, 12), texels (n, 4), perlin_grad (256, 4),
    perlin_perm (int32), and the record arrays prim_shade, mats, texs, boxes, flat_sets as structured
    arrays of record_dtypes (their bytes as the builder wrote them)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from raytrace_amd import _lib as R
    from raytrace_amd.scene import FlatScene, flatten
    flat = world if isinstance(world, FlatScene) else flatten(world)
    sc = R.scene_struct(flat)
    real = np.float64 if precision == "f64" else np.float32
    dts = record_dtypes(precision)
    dts["prim_shade"] = dts["mats"]
    width = {"prims": 16, "prim_uv": 6, "flat_recs": 16, "uvframes": 12, "texels": 4, "perlin_grad": 4}
    out = {}
    f = lib().rt_emu_scene_arrays
    for name in SCENE_ARRAYS:
        info = (ctypes.c_longlong * 2)()
        rc = f(ctypes.byref(sc), ctypes.c_int(precision == "f64"), name.encode(), None, ctypes.c_longlong(0), info)
        if rc != 0:
            raise RuntimeError(f"rt_emu_scene_arrays failed {rc}: {lib().rt_emu_last_error().decode()}")
        buf = np.zeros(max(int(info[0]), 1), np.uint8)
        rc = f(ctypes.byref(sc), ctypes.c_int(precision == "f64"), name.encode(), buf.ctypes.data_as(ctypes.c_void_p),
               ctypes.c_longlong(buf.size), info)
        assert rc == 0, (name, rc)
        buf = buf[:int(info[0])]
        if name in dts:
            assert dts[name].itemsize == info[1], (name, dts[name].itemsize, info[1])
            out[name] = buf.view(dts[name]).copy()
        elif name == "perlin_perm":
            out[name] = buf.view(np.int32).copy()
        else:
            out[name] = buf.view(real).reshape(-1, width[name]).copy()
    return out


def scene_digest(world):
    """(rc, error text, {item: [length, "fnv-1a hex"]}) of the host build of `world` (a Geometry or a
    FlatScene): every array and scalar of HostScene in both precisions, so that two builders can be
    compared byte for byte and a mismatch names the array.  rc != 0: the build's error, no items."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from raytrace_amd import _lib as R
    from raytrace_amd.scene import FlatScene, flatten
    flat = world if isinstance(world, FlatScene) else flatten(world)
    sc = R.scene_struct(flat)
    out = np.zeros(2 * len(DIGEST_ITEMS), np.uint64)
    rc = lib().rt_emu_scene_digest(ctypes.byref(sc), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(len(out)))
    if rc != 0:
        return rc, lib().rt_emu_last_error().decode(), {}
    return 0, "", {k: [int(out[2 * i]), f"{int(out[2 * i + 1]):016x}"] for i, k in enumerate(DIGEST_ITEMS)}
