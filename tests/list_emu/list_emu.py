"""ctypes front-end of the host build of the per-pixel path body (TEST TOOLING)."""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "_build", "librt_list_emu.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", HERE, "-s"], check=True)
        _lib = ctypes.CDLL(LIB)
        _lib.rt_list_emu_last_error.restype = ctypes.c_char_p
    return _lib


def render(settings, world, seed, counts, precision="f64", n_shards=1, shard=0, row_block=4):
    """The mean image of samples [0, counts[p]) of every tile pixel p: (rows, width, 3) in the
    precision's dtype.  counts: an int (every pixel) or a (rows, width) array."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from raytrace_amd import _lib as R
    from raytrace_amd.camera import image_height
    from raytrace_amd.ray import _seed64, shard_rows
    from raytrace_amd.scene import FlatScene, flatten
    flat = world if isinstance(world, FlatScene) else flatten(world)
    cs, sc, ex = R.camera_struct(settings), R.scene_struct(flat), R.exec_struct(0, n_shards, shard, row_block)
    rows, width = shard_rows(image_height(settings), n_shards, row_block), int(settings.cs_imageWidth)
    cnt = np.ascontiguousarray(np.broadcast_to(np.asarray(counts, np.uint32), (rows, width)))
    out = np.zeros((rows, width, 3), np.float64 if precision == "f64" else np.float32)
    rc = lib().rt_list_emu(ctypes.byref(cs), ctypes.byref(sc), ctypes.c_uint64(_seed64(seed)), ctypes.byref(ex),
                           cnt.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p),
                           ctypes.c_int(1 if precision == "f64" else 0))
    if rc != 0:
        raise RuntimeError(f"rt_list_emu failed {rc}: {lib().rt_list_emu_last_error().decode()}")
    return out
