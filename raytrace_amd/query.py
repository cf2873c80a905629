"""Batched ray queries on a resident scene (include/rt.h rt_scene_cast): closest hit and any hit.

The reference's `Geometry` is a hit function time -> Ray -> (tmin, tmax) -> Maybe (HitRecord, a)
(Geometry.hs:42); `DeviceScene.cast` evaluates it for n rays at once against the scene's surfaces
(`constantMedium` volumes are not hit: their events are random draws keyed by pixel and sample).
Directions may have any non-zero length; `t` is the distance along the normalised direction.  Rays are
traced in the order given, 64 consecutive rays per wave: coherent neighbours run faster.  For
incoherent batches (hemisphere probes, secondary rays) `reorder=True` sorts the batch on the device by
a coherence key first, and `DeviceScene.ray_order` returns that order for reuse (`order=`): the
results are the unordered call's, bit for bit.

    scene = DeviceScene(world)
    h = scene.cast(origins, directions)            # dict of numpy arrays
    depth = np.where(h["hit"], h["t"], np.inf)
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

RAY_DTYPE = np.dtype([("origin", "<f8", (3,)), ("dir", "<f8", (3,)), ("tmin", "<f8"), ("tmax", "<f8"),
                      ("time", "<f8"), ("reserved", "<f8")], align=True)
HIT_DTYPE = np.dtype([("t", "<f8"), ("point", "<f8", (3,)), ("normal", "<f8", (3,)), ("uv", "<f8", (2,)),
                      ("hit", "<i4"), ("front", "<i4"), ("leaf", "<i4"), ("instance", "<i4"), ("material", "<i4"),
                      ("reserved", "<i4")], align=True)


def query_flags(any_hit: bool = False, uv: bool = True) -> int:
    return (_lib.RT_QUERY_ANY_HIT if any_hit else 0) | (_lib.RT_QUERY_UV if uv else 0)


def make_rays(origins, directions, tmin=1e-4, tmax=np.inf, time=0.0) -> np.ndarray:
    """rt_ray records of the arguments broadcast to (n, 3) / (n,)."""
    o = np.asarray(origins, np.float64)
    d = np.asarray(directions, np.float64)
    if o.shape[-1:] != (3,) or d.shape[-1:] != (3,):
        raise ValueError("origins and directions must end in a dimension of 3")
    shape = np.broadcast_shapes(o.shape[:-1], d.shape[:-1], np.shape(tmin), np.shape(tmax), np.shape(time))
    if len(shape) > 1:
        raise ValueError("rays are a flat list: origins / directions of shape (n, 3) or (3,)")
    n = shape[0] if shape else 1
    rays = np.zeros(n, RAY_DTYPE)
    rays["origin"] = np.broadcast_to(o, (n, 3))
    rays["dir"] = np.broadcast_to(d, (n, 3))
    rays["tmin"] = np.broadcast_to(np.asarray(tmin, np.float64), (n,))
    rays["tmax"] = np.broadcast_to(np.asarray(tmax, np.float64), (n,))
    rays["time"] = np.broadcast_to(np.asarray(time, np.float64), (n,))
    return rays


def hits_dict(hits: np.ndarray) -> dict:
    """rt_hit records as a dict of arrays: hit (bool), valid (the ray was well formed), t (inf on a
    miss), point, normal, front (bool), uv, leaf, instance, material."""
    hit = hits["hit"] == 1
    return dict(hit=hit, valid=hits["hit"] >= 0, t=np.where(hit, hits["t"], np.inf), point=hits["point"].copy(),
                normal=hits["normal"].copy(), front=hits["front"] != 0, uv=hits["uv"].copy(), leaf=hits["leaf"].copy(),
                instance=hits["instance"].copy(), material=hits["material"].copy())


def order_arg(order, n: int):
    """A caller's order as the contiguous uint32 array the ordered calls read (kept alive by the caller)."""
    a = np.ascontiguousarray(order, np.uint32)
    if a.shape != (n,):
        raise ValueError(f"order must have shape {(n,)}, not {a.shape}")
    return a


def ray_order_records(scene, rays: np.ndarray) -> np.ndarray:
    """rt_scene_ray_order on host records (RAY_DTYPE or radiance.PATH_RAY_DTYPE): the batch's coherence
    order, (n,) uint32 — position i holds the index of the ray to trace i-th."""
    from .radiance import PATH_RAY_DTYPE
    if rays.dtype not in (RAY_DTYPE, PATH_RAY_DTYPE):
        raise ValueError("rays must be RAY_DTYPE or PATH_RAY_DTYPE records")
    kind = _lib.RT_ORDER_RAYS if rays.dtype == RAY_DTYPE else _lib.RT_ORDER_PATH_RAYS
    rays = np.ascontiguousarray(rays)
    order = np.zeros(len(rays), np.uint32)
    _lib.check(scene._lib.rt_scene_ray_order(scene.handle, rays.ctypes.data_as(ctypes.c_void_p), len(rays), kind,
                                             order.ctypes.data_as(ctypes.c_void_p)))
    return order


def cast_records(scene, rays: np.ndarray, precision: str = "f64", any_hit: bool = False, uv: bool = True,
                 reorder: bool = False, order=None) -> np.ndarray:
    """rt_scene_cast on host records: (n,) RAY_DTYPE -> (n,) HIT_DTYPE.  Raises RtError on a
    traversal-stack overflow (RT_E_STACK).  reorder: trace in the batch's coherence order, computed on
    the device (rt_scene_cast_ordered); order: in this order (a permutation, e.g. ray_order's)."""
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    hits = np.zeros(len(rays), HIT_DTYPE)
    ex = _lib.exec_struct(device=scene.device, precision=precision)
    if reorder or order is not None:
        o = None if order is None else order_arg(order, len(rays))
        _lib.check(scene._lib.rt_scene_cast_ordered(scene.handle, ctypes.byref(ex), rays.ctypes.data_as(ctypes.c_void_p),
                                                    hits.ctypes.data_as(ctypes.c_void_p), len(rays), query_flags(any_hit, uv),
                                                    None if o is None else o.ctypes.data_as(ctypes.c_void_p)))
        return hits
    _lib.check(scene._lib.rt_scene_cast(scene.handle, ctypes.byref(ex), rays.ctypes.data_as(ctypes.c_void_p),
                                        hits.ctypes.data_as(ctypes.c_void_p), len(rays), query_flags(any_hit, uv)))
    return hits


def cast(world, origins, directions, tmin=1e-4, tmax=np.inf, time=0.0, precision: str = "f64", any_hit: bool = False,
         uv: bool = True, device: int = 0, reorder: bool = False) -> dict:
    """One-shot form: upload `world`, cast, release.  Returns DeviceScene.cast's dict."""
    from .ray import DeviceScene
    scene = DeviceScene(world, device)
    try:
        return scene.cast(origins, directions, tmin, tmax, time, precision, any_hit, uv, reorder=reorder)
    finally:
        scene.close()
