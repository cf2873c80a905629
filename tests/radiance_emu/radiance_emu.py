"""ctypes front-end of the host build of the radiance-query body (TEST TOOLING)."""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "_build", "librt_radiance_emu.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", HERE, "-s"], check=True)
        _lib = ctypes.CDLL(LIB)
        _lib.rt_radiance_emu_last_error.restype = ctypes.c_char_p
    return _lib


def _structs(settings, world):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from raytrace_amd import _lib as R
    from raytrace_amd.scene import FlatScene, flatten
    flat = world if isinstance(world, FlatScene) else flatten(world)
    return R.camera_struct(settings), R.scene_struct(flat)


def words(precision):
    """64-bit workspace words per ray: the sums and the {flag, count} word."""
    return 7 if precision == "f64" else 4


def radiance(settings, world, seed, rays, samples=1, precision="f64", unit_dir=False, work=None):
    """rt_scene_radiance on the host: (out (n,) RADIANCE_DTYPE, work (n, words) uint64).  `work`: a
    workspace to accumulate onto (not modified; RT_RADIANCE_ACCUMULATE)."""
    from raytrace_amd.radiance import PATH_RAY_DTYPE, RADIANCE_DTYPE, radiance_flags
    from raytrace_amd.ray import _seed64
    cs, sc = _structs(settings, world)
    rays = np.ascontiguousarray(rays, PATH_RAY_DTYPE)
    n = len(rays)
    w = np.zeros((n, words(precision)), np.uint64) if work is None else np.array(work, np.uint64, copy=True, order="C")
    assert w.shape == (n, words(precision))
    out = np.zeros(n, RADIANCE_DTYPE)
    rc = lib().rt_radiance_emu(ctypes.byref(cs), ctypes.byref(sc), ctypes.c_uint64(_seed64(seed)),
                               rays.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(n), ctypes.c_int32(samples),
                               ctypes.c_int32(radiance_flags(unit_dir, work is not None)), w.ctypes.data_as(ctypes.c_void_p),
                               out.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(1 if precision == "f64" else 0))
    if rc != 0:
        raise RuntimeError(f"rt_radiance_emu failed {rc}: {lib().rt_radiance_emu_last_error().decode()}")
    return out, w


def camera_rays(settings, world, seed, sample=0, precision="f64"):
    """rt_scene_camera_rays on the host: (height x width,) PATH_RAY_DTYPE, row-major."""
    from raytrace_amd.camera import image_height
    from raytrace_amd.radiance import PATH_RAY_DTYPE
    from raytrace_amd.ray import _seed64
    cs, sc = _structs(settings, world)
    rays = np.zeros(image_height(settings) * int(settings.cs_imageWidth), PATH_RAY_DTYPE)
    rc = lib().rt_radiance_emu_camera_rays(ctypes.byref(cs), ctypes.byref(sc), ctypes.c_uint64(_seed64(seed)),
                                           ctypes.c_int32(sample), rays.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.c_int(1 if precision == "f64" else 0))
    if rc != 0:
        raise RuntimeError(f"rt_radiance_emu_camera_rays failed {rc}: {lib().rt_radiance_emu_last_error().decode()}")
    return rays
