"""ctypes front-end of the host build of the ray-query body (TEST TOOLING)."""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "_build", "librt_query_emu.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", HERE, "-s"], check=True)
        _lib = ctypes.CDLL(LIB)
        _lib.rt_query_emu_last_error.restype = ctypes.c_char_p
    return _lib


def cast(world, rays, precision="f64", any_hit=False, uv=True, want_rc=False):
    """rt_hit records (raytrace_amd.query.HIT_DTYPE) of the rt_ray records `rays` against `world` (a
    scene tree or a FlatScene), as rt_scene_cast returns them from the device, and the scene's kernel
    variant code (rt_internal.h RT_VAR_*)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from raytrace_amd import _lib as R
    from raytrace_amd.query import HIT_DTYPE, RAY_DTYPE, query_flags
    from raytrace_amd.scene import FlatScene, flatten
    flat = world if isinstance(world, FlatScene) else flatten(world)
    sc = R.scene_struct(flat)
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    hits = np.zeros(len(rays), HIT_DTYPE)
    variant = ctypes.c_int(0)
    rc = lib().rt_query_emu(ctypes.byref(sc), rays.ctypes.data_as(ctypes.c_void_p), hits.ctypes.data_as(ctypes.c_void_p),
                            ctypes.c_longlong(len(rays)), ctypes.c_int(query_flags(any_hit, uv)),
                            ctypes.c_int(1 if precision == "f64" else 0), ctypes.byref(variant))
    if want_rc:
        return hits, variant.value, rc
    if rc != 0:
        raise RuntimeError(f"rt_query_emu failed {rc}: {lib().rt_query_emu_last_error().decode()}")
    return hits, variant.value
