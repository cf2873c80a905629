"""ctypes front-end of the host build of the first-hit feature body (TEST TOOLING)."""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "_build", "librt_feature_emu.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", HERE, "-s"], check=True)
        _lib = ctypes.CDLL(LIB)
        _lib.rt_feature_emu_last_error.restype = ctypes.c_char_p
    return _lib


def features(settings, world, seed, n_feat, precision="f64", n_shards=1, shard=0, row_block=4):
    """The feature words of samples [0, n_feat): (rows, width, 8) int64 for "f32", (rows, width, 16)
    for "f64", as Film.feature_words returns them from the device."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from raytrace_amd import _lib as R
    from raytrace_amd.camera import image_height
    from raytrace_amd.ray import _seed64, shard_rows
    from raytrace_amd.scene import FlatScene, flatten
    flat = world if isinstance(world, FlatScene) else flatten(world)
    cs, sc, ex = R.camera_struct(settings), R.scene_struct(flat), R.exec_struct(0, n_shards, shard, row_block)
    rows = shard_rows(image_height(settings), n_shards, row_block)
    out = np.zeros((rows, int(settings.cs_imageWidth), 16 if precision == "f64" else 8), np.int64)
    rc = lib().rt_feature_emu(ctypes.byref(cs), ctypes.byref(sc), ctypes.c_uint64(_seed64(seed)), ctypes.byref(ex),
                              ctypes.c_int(int(n_feat)), out.ctypes.data_as(ctypes.c_void_p),
                              ctypes.c_int(1 if precision == "f64" else 0))
    if rc != 0:
        raise RuntimeError(f"rt_feature_emu failed {rc}: {lib().rt_feature_emu_last_error().decode()}")
    return out
