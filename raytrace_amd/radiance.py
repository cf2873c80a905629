"""Batched radiance queries on a resident scene (include/rt.h rt_scene_radiance): the path tracer on
the caller's rays.

The reference's `rayColor` (Ray.hs:174-224) is private to `raytrace`; `DeviceScene.radiance` evaluates
it for n rays at once — an orthographic or panoramic camera, irradiance probes, a lightmap — with the
scene's media, materials, background and redirect targets.  Ray i receives samples `sample0 + [0,
samples)` of Philox stream `stream` (where a render puts the pixel id), so equal records give equal
results, and `DeviceScene.camera_rays` returns the rays whose radiance is a render's sample word for
word.  Rays are traced in the order given, 64 consecutive (ray, sample chunk) items per wave;
`reorder=True` / `order=` trace them in a coherence order instead (raytrace_amd.query), with the
same results and workspace words.

    scene = DeviceScene(world)
    rgb, info = scene.radiance(origins, directions, settings, seed, samples=64)
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

PATH_RAY_DTYPE = np.dtype([("origin", "<f8", (3,)), ("dir", "<f8", (3,)), ("time", "<f8"), ("stream", "<u4"),
                           ("sample0", "<u4")], align=True)
RADIANCE_DTYPE = np.dtype([("rgb", "<f8", (3,)), ("status", "<i4"), ("samples", "<u4")], align=True)


def radiance_flags(unit_dir: bool = False, accumulate: bool = False) -> int:
    return (_lib.RT_RADIANCE_UNIT_DIR if unit_dir else 0) | (_lib.RT_RADIANCE_ACCUMULATE if accumulate else 0)


def workspace_words(precision: str = "f64") -> int:
    """64-bit workspace words per ray: the fixed-point sums in the film state's order (6 in binary64,
    3 in FP32), then the word {NaN flag (low 32 bits), sample count (high 32 bits)}."""
    _lib.dtype_of(precision)
    return 7 if precision == "f64" else 4


def workspace_bytes(n: int, precision: str = "f64") -> int:
    """rt_scene_radiance_workspace_bytes: n rays' words and the kernel's 16-byte tail."""
    return int(n) * workspace_words(precision) * 8 + 16


def make_path_rays(origins, directions, time=0.0, stream=None, sample0=0) -> np.ndarray:
    """rt_path_ray records of the arguments broadcast to (n, 3) / (n,).  stream defaults to the ray's
    index mod 2^32 (every ray its own random stream), sample0 to 0."""
    o = np.asarray(origins, np.float64)
    d = np.asarray(directions, np.float64)
    if o.shape[-1:] != (3,) or d.shape[-1:] != (3,):
        raise ValueError("origins and directions must end in a dimension of 3")
    extra = [np.shape(time), np.shape(sample0)] + ([np.shape(stream)] if stream is not None else [])
    shape = np.broadcast_shapes(o.shape[:-1], d.shape[:-1], *extra)
    if len(shape) > 1:
        raise ValueError("rays are a flat list: origins / directions of shape (n, 3) or (3,)")
    n = shape[0] if shape else 1
    rays = np.zeros(n, PATH_RAY_DTYPE)
    rays["origin"] = np.broadcast_to(o, (n, 3))
    rays["dir"] = np.broadcast_to(d, (n, 3))
    rays["time"] = np.broadcast_to(np.asarray(time, np.float64), (n,))
    rays["stream"] = (np.arange(n, dtype=np.uint64) if stream is None
                      else np.broadcast_to(np.asarray(stream, np.uint64), (n,))) % np.uint64(1 << 32)
    rays["sample0"] = np.broadcast_to(np.asarray(sample0, np.uint64), (n,)) % np.uint64(1 << 32)
    return rays


def radiance_records(scene, rays: np.ndarray, settings, seed, samples: int = 1, precision: str = "f64",
                     unit_dir: bool = False, work: np.ndarray | None = None, reorder: bool = False, order=None):
    """rt_scene_radiance on host records: (n,) PATH_RAY_DTYPE -> ((n,) RADIANCE_DTYPE, (n, words) uint64
    workspace words).  `work`: the words of an earlier call to add onto (RT_RADIANCE_ACCUMULATE; not
    modified).  reorder / order: as query.cast_records (rt_scene_radiance_ordered).  Raises RtError on a
    traversal-stack overflow (RT_E_STACK)."""
    from .ray import _seed64
    rays = np.ascontiguousarray(rays, PATH_RAY_DTYPE)
    n = len(rays)
    w = (np.zeros((n, workspace_words(precision)), np.uint64) if work is None
         else np.array(work, np.uint64, copy=True, order="C"))
    if w.shape != (n, workspace_words(precision)):
        raise ValueError(f"work must have shape {(n, workspace_words(precision))}, not {w.shape}")
    out = np.zeros(n, RADIANCE_DTYPE)
    cs = _lib.camera_struct(settings)
    ex = _lib.exec_struct(device=scene.device, precision=precision)
    args = (scene.handle, ctypes.byref(ex), ctypes.byref(cs), _seed64(seed), rays.ctypes.data_as(ctypes.c_void_p),
            out.ctypes.data_as(ctypes.c_void_p), w.ctypes.data_as(ctypes.c_void_p), n, int(samples),
            radiance_flags(unit_dir, work is not None))
    if reorder or order is not None:
        from .query import order_arg
        o = None if order is None else order_arg(order, n)
        _lib.check(scene._lib.rt_scene_radiance_ordered(*args, None if o is None else o.ctypes.data_as(ctypes.c_void_p)))
    else:
        _lib.check(scene._lib.rt_scene_radiance(*args))
    return out, w


def radiance(world, origins, directions, settings, seed, samples: int = 1, time=0.0, stream=None, sample0=0,
             precision: str = "f64", unit_dir: bool = False, device: int = 0, reorder: bool = False):
    """One-shot form: upload `world`, query, release.  Returns DeviceScene.radiance's (rgb, info)."""
    from .ray import DeviceScene
    scene = DeviceScene(world, device)
    try:
        return scene.radiance(origins, directions, settings, seed, samples, time, stream, sample0, precision, unit_dir,
                              reorder=reorder)
    finally:
        scene.close()
