"""TEST TOOLING shared by tests/test_ray_order_host.py and tests/test_ray_order_gpu.py: the ray batches
of the order tests and the numpy twin of the coherence key, written from DESIGN §4g's formula (not
from rt_order.h's text).

    valid   the six values finite, dir != 0; an invalid ray's key is 0xFFFFFFFF
    box     lo_a / hi_a = min / max of origin_a over the valid rays
    scale   s_a = 64 / (hi_a - lo_a) if hi_a > lo_a else 0
    cell(x) 63 if x >= 63; floor(x) if x >= 0; else 0
    origin  c_a = cell((origin_a - lo_a) * s_a)
    dir     L = (|dx| + |dy|) + |dz|; px = dx / L; py = dy / L; if dz < 0:
            (px, py) <- (copysign(1 - |py|, px), copysign(1 - |px|, py))
            u = cell((px + 1) * 32); v = cell((py + 1) * 32)
    key     morton3(c_x, c_y, c_z) << 12 | morton2(u, v), x / u in the lowest bit of each interleave
"""
import functools

import numpy as np

import query_cases as QC
from raytrace_amd.query import RAY_DTYPE, make_rays
from raytrace_amd.radiance import PATH_RAY_DTYPE

KEY_LAST = 0xFFFFFFFF
SCENE_BATCHES = ["cornell_box", "bunny_cornell", "pawn_instances", "demo1"]
N_BATCH = 4099


def cell(x):
    with np.errstate(invalid="ignore"):
        return np.where(x >= 63, 63, np.where(x >= 0, np.floor(x), 0)).astype(np.uint32)


def interleave(parts, bits=6):
    key = np.zeros(parts[0].shape, np.uint32)
    for b in range(bits):
        for k, p in enumerate(parts):
            key |= ((p >> np.uint32(b)) & np.uint32(1)) << np.uint32(b * len(parts) + k)
    return key


def twin_keys(origins, dirs):
    o, d = np.asarray(origins, np.float64), np.asarray(dirs, np.float64)
    n = len(o)
    if n == 0:
        return np.zeros(0, np.uint32)
    valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
    lo = o[valid].min(0) if valid.any() else np.zeros(3)
    hi = o[valid].max(0) if valid.any() else np.zeros(3)
    with np.errstate(all="ignore"):
        s = np.where(hi > lo, 64.0 / (hi - lo), 0.0)
        c = cell((o - lo) * s)
        L = (np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2])
        px, py = d[:, 0] / L, d[:, 1] / L
        neg = d[:, 2] < 0
        qx = np.copysign(1.0 - np.abs(py), px)
        qy = np.copysign(1.0 - np.abs(px), py)
        px, py = np.where(neg, qx, px), np.where(neg, qy, py)
        u, v = cell((px + 1.0) * 32.0), cell((py + 1.0) * 32.0)
    key = (interleave([c[:, 0], c[:, 1], c[:, 2]]) << np.uint32(12)) | interleave([u, v])
    return np.where(valid, key, np.uint32(KEY_LAST)).astype(np.uint32)


def seam_directions():
    d = []
    for a in range(3):
        for sgn in (1.0, -1.0):
            e = np.zeros(3)
            e[a] = sgn
            d.append(e)
    for z in (0.0, -0.0):
        for x, y in ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1), (0.3, -0.7), (-2.0, 0.5)):
            d.append(np.array([x, y, z], np.float64))
    for z in (0.25, -0.25, 3.0, -3.0, 1e-300, -1e-300):
        for x, y in ((1, 1), (-1, 1), (1, -1), (-1, -1), (0.5, -0.5), (0, 0), (0.0, -0.0), (-0.0, 2.0)):
            d.append(np.array([x, y, z], np.float64))
    d.append(np.array([1e-150, 0, 0]))
    d.append(np.array([0, -1e150, 1e150]))
    return np.array(d)


def bad_records():
    """(origins, dirs) of records the key calls invalid."""
    o = np.tile([0.5, 1.0, 2.0], (8, 1))
    d = np.tile([0.0, 0.0, 1.0], (8, 1))
    o[0, 1] = np.nan
    o[1, 0] = np.inf
    o[2, 2] = -np.inf
    d[3, 0] = np.nan
    d[4, 2] = np.inf
    d[5] = 0.0
    d[6] = (-0.0, 0.0, -0.0)
    d[7, 1] = -np.inf
    return o, d


def edge_batch(lo, hi, seed):
    """Origins at lo, at hi and at lo + k (hi - lo) / 64 (per axis and mixed), seam directions, with the
    invalid records spread between them."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    rng = np.random.default_rng(seed)
    k = np.arange(65)
    grid = lo + k[:, None] * (hi - lo) / 64
    mixed = lo + rng.integers(0, 65, (200, 3)) * (hi - lo) / 64
    below = np.where(hi > lo, np.nextafter(grid[1:], -np.inf), lo)  # (a degenerate axis stays one)
    o = np.concatenate([lo[None], hi[None], grid, mixed, below])
    seams = seam_directions()
    d = seams[np.arange(len(o)) % len(seams)]
    d2 = seams[rng.integers(0, len(seams), len(o))]
    o, d = np.concatenate([o, o]), np.concatenate([d, d2])
    bo, bd = bad_records()
    at = np.sort(rng.integers(0, len(o), len(bo)))
    return np.insert(o, at, bo, axis=0), np.insert(d, at, bd, axis=0)


@functools.lru_cache(None)
def batch(name):
    """(origins, dirs) of a named batch."""
    if name in SCENE_BATCHES:
        o, d = QC.rays_of(name, N_BATCH)[:2]
        return o, d
    if name == "one_origin":
        rng = np.random.default_rng(21)
        d = rng.normal(size=(N_BATCH, 3))
        return np.tile([0.25, -3.0, 7.5], (N_BATCH, 1)), d
    if name == "edges":
        return edge_batch((-1.0, 2.0, 0.5), (3.0, 2.75, 8.5), 31)
    if name == "degenerate_axis":
        return edge_batch((-1.0, 2.0, 0.5), (3.0, 2.0, 8.5), 32)
    if name == "none_valid":
        return bad_records()
    if name in ("n0", "n1", "n2"):
        n = int(name[1])
        o, d = batch("edges")
        return o[3:3 + n], d[3:3 + n]
    raise KeyError(name)


BATCHES = SCENE_BATCHES + ["one_origin", "edges", "degenerate_axis", "none_valid", "n0", "n1", "n2"]
EDGE_BATCHES = ["edges", "degenerate_axis", "none_valid", "n0", "n1", "n2"]


def records(name, kind):
    """The batch as rt_ray (kind 0) or rt_path_ray (kind 1) records."""
    o, d = batch(name)
    if kind == 0:
        return make_rays(o, d) if len(o) else np.zeros(0, RAY_DTYPE)
    r = np.zeros(len(o), PATH_RAY_DTYPE)
    r["origin"], r["dir"] = o, d
    r["time"] = 0.5
    r["stream"] = np.arange(len(o))
    return r
