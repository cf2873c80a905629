"""Unit-level probes of the shading half of rt_trace.h: eval_texture (checker, image, noise, marble),
perlin_noise / fractal_noise, surface_info, test_box, medium_draw and shade_event / mixture_scatter
called element-wise (tests/device_probe) on the host emulator (backend "emu") and on the device
(backend "gpu").  The records the functions read are the product's own: scenes go through the host
builder and the arrays come back through emu.scene_arrays, so a mismatch between what rt_build.cpp
writes and what the kernel reads fails here too.

Every reference is a restatement of the cited lines of the reference project in numpy long double
(decisions in exact Python integers / Fractions) on the very floats the probe receives; none calls
the emulator, the oracle or the code under test.  The rules are those of test_device_probe.py:

* a decision must equal the exact decision unless an exact margin lies within 64 eps scale of zero,
  scale being the magnitude of the terms subtracted to form it; such cases are at most 0.5 % of a
  family (asserted);
* a continuous output must be within K eps S of the long-double value, S stated per family, K = 8x the
  worst error of the reference's plain formula evaluated in numpy at the working precision on the
  same cases, rounded up to a power of two (k_from_baseline) -- computed at run time, recorded, and
  never taken from the kernel's result.

The worst errors are written with record_measure("shading_probe", ...) and kept in
profiles/probe/shading_probe.jsonl."""
import functools
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT, record_measure

sys.path.insert(0, os.path.join(ROOT, "tests", "device_probe"))
sys.path.insert(0, os.path.join(ROOT, "tests", "kernel_emu"))
import emu  # noqa: E402
from test_device_probe import (LD, KTMIN, backends, both_precisions, dot_i, k_from_baseline, philox_ref,  # noqa: E402
                               plane_exact, random_units, ratio, real_of, run, same_bits, scale_of, to_int,
                               ulp_distance, undecided)

from raytrace_amd import geometry as G  # noqa: E402
from raytrace_amd import material as M  # noqa: E402
from raytrace_amd.core import V3, fromCorners  # noqa: E402

PI_LD = LD("3.14159265358979323846264338327950288419716939937510")
N_FAMILY = 1 << 14
N_EXACT = 1 << 12  # families whose reference needs Python integers


def measure(backend, what, **figures):
    record_measure("shading_probe", dict(backend=backend, probe=what, **figures))


def eps_of(precision):
    return float(np.finfo(real_of(precision)).eps)


def white(g):
    return M.lambertian(M.constantTexture(V3(0.5, 0.5, 0.5))) << g


@functools.lru_cache(None)
def arrays(scene, precision):
    return emu.scene_arrays(SCENES[scene](), precision)


# ------------------------------------------------------------------ the export
def fnv1a(data):
    h = 0xcbf29ce484222325
    for c in data:
        h = ((h ^ c) * 0x100000001b3) & 0xffffffffffffffff
    return h


def field_bytes(a):
    """The bytes of an array field by field, struct padding left out (scene_digest's rule)."""
    if a.dtype.names is None:
        return np.ascontiguousarray(a).tobytes()
    n = len(a)
    cols = [np.ascontiguousarray(a[f]).reshape(n, -1).view(np.uint8).reshape(n, -1) for f in a.dtype.names]
    return np.concatenate(cols, 1).tobytes() if n else b""


def test_scene_arrays_hash_to_scene_digest():
    """emu.scene_arrays returns the very arrays scene_digest hashes: for one scene with box groups, a
    rotated textured sphere, an image, a noise texture and triangle uvs, every exported array's
    length and field-by-field FNV-1a equal the digest's in both precisions (so the export cannot
    drift from the digest), and every record layout in emu.record_dtypes has the C struct's size."""
    world = SCENES["mixed"]()
    rc, err, dig = emu.scene_digest(world)
    assert rc == 0, err
    for precision in ("f32", "f64"):
        A = emu.scene_arrays(world, precision)
        assert sorted(A) == sorted(emu.SCENE_ARRAYS)
        for name, a in A.items():
            key = name if name in ("perlin_perm", "flat_sets") else f"{precision}.{name}"
            length, h = dig[key]
            assert a.size == length if a.dtype.names is None else len(a) == length, (key, a.shape, length)
            assert f"{fnv1a(field_bytes(a)):016x}" == h, key
        assert len(A["boxes"]) >= 1 and len(A["uvframes"]) >= 1 and len(A["texels"]) == 6 and len(A["texs"]) >= 4


# ------------------------------------------------------------------ a. textures: checker and image
CHECKER_DIMS = [1, 2, 3, 7, 64]
# (width, height): the two smallest sizes come after another image, at a non-zero `off`
IMAGE_SIZES = [(7, 3), (1, 1), (2, 1), (1, 2), (2, 2), (3, 7), (64, 2), (3, 64), (7, 7), (64, 64)]
C0, C1 = (0.25, 0.5, 0.75), (1.0, 2.0, 3.0)


def image_of(k, w, h):
    """Texel (row j, column i) of image k is (i, j, k): a wrong index is visible."""
    img = np.zeros((h, w, 3), np.float32)
    img[:, :, 0] = np.arange(w)[None, :]
    img[:, :, 1] = np.arange(h)[:, None]
    img[:, :, 2] = k
    return img


def uv_texture_scene():
    obs, x = [], 0.0
    for nu in CHECKER_DIMS:
        for nv in CHECKER_DIMS:
            obs.append(M.lambertian(M.checkerTexture(nu, nv, V3(*C0), V3(*C1))) << G.sphere(V3(x, 0, 0), 0.25))
            x += 1.0
    for k, (w, h) in enumerate(IMAGE_SIZES):
        obs.append(M.lambertian(M.imageTexture(image_of(k, w, h))) << G.sphere(V3(x, 0, 0), 0.25))
        x += 1.0
    return G.group(obs)


def floor_exact(x, n):
    """floor(x n) of floats x and ints n exactly, and the distance of x n to the nearest integer."""
    fl = np.empty(len(x), object)
    dist = np.empty(len(x), np.float64)
    for k, (a, b) in enumerate(zip(x, n)):
        p = a * int(b)
        f = math.floor(p)
        fl[k] = f
        dist[k] = float(min(p - f, f + 1 - p))
    return fl, dist


def texture_lookup(T, texels, tid, i, j):
    """The colour of cell (i, j) (already wrapped for images) of texture records T[tid]."""
    out = np.zeros((len(tid), 3), np.float64)
    kind = T["kind"][tid]
    chk = kind == M.TEX_CHECKER
    odd = np.array([(int(a) + int(b)) % 2 for a, b in zip(i, j)], bool)
    out[chk] = np.where(odd[chk, None], T["c1"][tid][chk], T["c0"][tid][chk])
    img = kind == M.TEX_IMAGE
    idx = np.array([int(T["off"][t]) + int(b) * int(T["nu"][t]) + int(a) if m else 0
                    for t, a, b, m in zip(tid, i, j, img)], np.int64)
    out[img] = texels[idx[img], :3]
    return out


def uv_reference(T, texels, tid, u, v):
    """Texture.hs:31-53 with the exact floor and the mathematical mod on the floats (u, v): colours, the
    skip mask of the cases where u nu, v nv or (1 - v) h lies within 64 eps scale of an integer (scale: the
    magnitude of the product, at least 1: the one rounding of the product the formula has)."""
    fu = [Fraction(float(x)) for x in u]
    fv = [Fraction(float(x)) for x in v]
    img = T["kind"][tid] == M.TEX_IMAGE
    nu, nv = T["nu"][tid], T["nv"][tid]
    i, di = floor_exact(fu, nu)
    vv = [1 - x if m else x for x, m in zip(fv, img)]
    j, dj = floor_exact(vv, nv)
    i = np.array([a % int(n) if m else a for a, n, m in zip(i, nu, img)], object)
    j = np.array([a % int(n) if m else a for a, n, m in zip(j, nv, img)], object)
    su = np.maximum(1.0, np.abs(u.astype(np.float64)) * nu)
    sv = np.maximum(1.0, (np.abs(v.astype(np.float64)) + img) * nv)
    return texture_lookup(T, texels, tid, i, j), di, dj, su, sv


def run_texture(backend, precision, A, tid, u, v, p=None):
    real = real_of(precision)
    n = len(tid)
    uv = np.stack([u, v], 1).astype(real)
    p = np.zeros((n, 3), real) if p is None else p
    rgb, = run(backend, precision, "texture", A["texs"][tid], A["texels"], A["perlin_perm"], A["perlin_grad"], uv, p)
    return rgb


@backends
@both_precisions
def test_texture_checker_and_image_random(backend, precision):
    """eval_texture on 2^14 random (u, v) in [-3, 4]^2 over every checker (nu, nv) and every image size
    of {1, 2, 3, 7, 64} (non-square images included; texel (i, j) of image k holds (i, j, k)), with the
    builder's DevTexture records and texels, against Texture.hs:31-53 with the exact floor and the
    mathematical mod.  The colour equals the reference's exactly unless u nu, v nv or (1 - v) h is within
    64 eps max(1, |product|) of an integer; at most 0.5 % of the family.  Skipped by the reference
    alone: 0.06 % (FP32), none (binary64); emulator and MI355X: no mismatch."""
    A = arrays("uv_textures", precision)
    real, eps = real_of(precision), eps_of(precision)
    rng = np.random.default_rng(101)
    n = N_FAMILY
    tid = rng.integers(0, len(A["texs"]), n)
    tid = tid[np.isin(A["texs"]["kind"][tid], (M.TEX_CHECKER, M.TEX_IMAGE))]
    n = len(tid)
    assert n > N_FAMILY * 0.9
    u, v = rng.uniform(-3, 4, n).astype(real), rng.uniform(-3, 4, n).astype(real)
    want, di, dj, su, sv = uv_reference(A["texs"], A["texels"], tid, u, v)
    skip = (di <= 64 * eps * su) | (dj <= 64 * eps * sv)
    got = run_texture(backend, precision, A, tid, u, v)
    bad = (got.astype(np.float64) != want).any(1) & ~skip
    measure(backend, f"texture_uv_random_{precision}", n=n, skipped=float(skip.mean()), mismatches=int(bad.sum()))
    assert skip.mean() <= 0.005, skip.mean()
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:8])


@backends
@both_precisions
def test_texture_checker_and_image_edges(backend, precision):
    """Constructed (u, v): every pair of {0, 1, -0.0, 1 - eps, -eps, 2, -1} on every texture, and k / n for
    every cell edge of the 7 x 3 image (and one float either side of it), with no skips.  Here the
    reference's product u w' (one correctly rounded multiplication, and 1 - v before it: Texture.hs:38-39,
    51-52) is taken at the working precision, as the formula states it; the floor, the mod and the parity
    are exact.  u = 1 and v = 0 wrap to column 0 and row 0; negative cells wrap upward."""
    A = arrays("uv_textures", precision)
    real, eps = real_of(precision), eps_of(precision)
    T = A["texs"]
    e = real(eps)
    vals = np.array([0.0, 1.0, -0.0, real(1) - e / 2, -e, 2.0, -1.0], real)
    uu, vv = [x.reshape(-1) for x in np.meshgrid(vals, vals, indexing="ij")]
    tids = np.flatnonzero(np.isin(T["kind"], (M.TEX_CHECKER, M.TEX_IMAGE)))
    tid = np.repeat(tids, len(uu))
    u, v = np.tile(uu, len(tids)), np.tile(vv, len(tids))
    t73 = int(np.flatnonzero((T["kind"] == M.TEX_IMAGE) & (T["nu"] == 7) & (T["nv"] == 3))[0])
    edge_u = np.array([real(k) / real(7) for k in range(-7, 15)], real)
    edge_v = np.array([real(k) / real(3) for k in range(-3, 7)], real)
    tiny = np.finfo(real).tiny  # (no denormals: the device flushes FP32 ones to zero, the build's flag)
    def around(x):
        up, dn = np.nextafter(x, real(np.inf)), np.nextafter(x, real(-np.inf))
        return np.concatenate([x, np.where(x == 0, tiny, up), np.where(x == 0, -tiny, dn)]).astype(real)
    eu, ev = [x.reshape(-1) for x in np.meshgrid(around(edge_u), around(edge_v), indexing="ij")]
    tid = np.concatenate([tid, np.full(len(eu), t73)])
    u, v = np.concatenate([u, eu]).astype(real), np.concatenate([v, ev]).astype(real)
    img = T["kind"][tid] == M.TEX_IMAGE
    pu = u * T["nu"][tid].astype(real)
    pv = np.where(img, real(1) - v, v).astype(real) * T["nv"][tid].astype(real)
    assert pu.dtype == real and pv.dtype == real
    i = [int(math.floor(float(x))) for x in pu]
    j = [int(math.floor(float(x))) for x in pv]
    i = np.array([a % int(w) if m else a for a, w, m in zip(i, T["nu"][tid], img)], object)
    j = np.array([a % int(h) if m else a for a, h, m in zip(j, T["nv"][tid], img)], object)
    want = texture_lookup(T, A["texels"], tid, i, j)
    got = run_texture(backend, precision, A, tid, u, v)
    bad = (got.astype(np.float64) != want).any(1)
    assert not bad.any(), (int(bad.sum()), [(int(tid[k]), float(u[k]), float(v[k])) for k in np.flatnonzero(bad)[:6]])
    # spelled out on the 7 x 3 image: (u, v) = (1, 0) is column 0 of the bottom row ... wrapped to row 0
    k = np.flatnonzero((tid == t73) & (u == 1) & (v == 0))[0]
    assert tuple(got[k]) == (0.0, 0.0, 0.0)
    k = np.flatnonzero((tid == t73) & (u == -e) & (v == 1))[0]
    assert tuple(got[k]) == (6.0, 0.0, 0.0)
    assert (T["off"][tids[T["kind"][tids] == M.TEX_IMAGE]][1:] > 0).all()


# ------------------------------------------------------------------ a. textures: noise and marble
LIPSCHITZ = 19.0  # of perlinNoise per unit |dp|inf: 3 axes x (sum |s'| sqrt 3 <= 3 sqrt 3, plus sum w |g| <= 1)
NOISE_TEXTURES = [(1, 1.0, (0.0, 0.0, 0.0)), (2, 2.0, (10.0, 0.0, 0.0)), (7, 0.5, (-3.25, 7.5, 100.0)),
                  (7, 4.0, (0.0, 0.0, 0.0))]
MARBLE_TEXTURES = [((0.0, 0.0, 1.0), 4.0, (0.0, 0.0, 0.0)), ((0.6, -0.8, 0.0), 1.0, (5.5, -2.25, 300.0))]
NOISE_C0, NOISE_C1 = (0.125, 0.25, 0.0), (1.0, 0.5, 2.0)


def noise_texture_scene():
    obs, x = [], 0.0
    for k, f, s in NOISE_TEXTURES:
        obs.append(M.lambertian(M.noiseTexture(k, f, V3(*s), V3(*NOISE_C0), V3(*NOISE_C1))) << G.sphere(V3(x, 0, 0), 0.25))
        x += 1.0
    for d, f, s in MARBLE_TEXTURES:
        obs.append(M.lambertian(M.marbleTexture(V3(*d), f, V3(*s))) << G.sphere(V3(x, 0, 0), 0.25))
        x += 1.0
    return G.group(obs)


def perlin_np(perm, grad, q, dt):
    """perlinNoise (Noise.hs:15-39) on the rows of q in dtype dt; lattice cells as Python ints (the
    reference floors to a 64-bit Int and keeps the low 8 bits).  Returns the noise and the sum of the
    absolute terms."""
    q = q.astype(dt)
    fl = np.floor(q)
    cell = np.array([[int(x) & 255 for x in row] for row in fl.astype(LD)], np.int64).reshape(-1, 3)
    f = q - fl
    total, mag = np.zeros(len(q), dt), np.zeros(len(q), dt)
    one = dt(1)
    def smooth(x):
        return x * x * (dt(3) - dt(2) * x)
    for i in (0, 1):
        for j in (0, 1):
            for k in (0, 1):
                g = grad[perm[0, (cell[:, 0] + i) & 255] ^ perm[1, (cell[:, 1] + j) & 255] ^ perm[2, (cell[:, 2] + k) & 255]]
                g = g[:, :3].astype(dt)
                rel = np.stack([f[:, 0] - dt(i), f[:, 1] - dt(j), f[:, 2] - dt(k)], 1)
                coef = smooth(f[:, 0] if i else one - f[:, 0]) * smooth(f[:, 1] if j else one - f[:, 1]) * \
                    smooth(f[:, 2] if k else one - f[:, 2])
                total = total + coef * (g * rel).sum(1)
                mag = mag + np.abs(coef) * np.abs(g * rel).sum(1)
    return total, mag


def fractal_np(perm, grad, depth, q, dt):
    """fractalNoise (Noise.hs:42-46): the sum, the sum of the absolute terms and depth x the Lipschitz bound."""
    q = q.astype(dt)
    total, mag, w = np.zeros(len(q), dt), np.zeros(len(q), dt), dt(1)
    for _ in range(depth):
        t, m = perlin_np(perm, grad, q, dt)
        total, mag = total + w * t, mag + w * m
        w, q = w / dt(2), q * dt(2)
    return total, mag


def noise_points(precision, rng, n):
    """q: uniform in [-300, 300]^3 (crossing zero and the period of 256), then lattice points, half-integers
    and the floats either side of an integer in each axis, at positive and negative cells."""
    real = real_of(precision)
    q = rng.uniform(-300, 300, (n, 3)).astype(real)
    ints = np.array([-257.0, -256.0, -255.0, -3.0, -1.0, 0.0, 1.0, 2.0, 127.0, 255.0, 256.0, 257.0, 299.0], real)
    m = n // 8
    q[:m] = rng.choice(ints, (m, 3))
    q[m:2 * m] = rng.choice(ints, (m, 3)) + real(0.5)
    side = rng.choice([-np.inf, np.inf], (m, 3)).astype(real)
    q[2 * m:3 * m] = np.nextafter(rng.choice(ints, (m, 3)).astype(real), side)
    axis = rng.integers(0, 3, m)
    mixed = q[3 * m:4 * m].copy()
    mixed[np.arange(m), axis] = np.nextafter(rng.choice(ints, m).astype(real), side[:, 0])
    q[3 * m:4 * m] = mixed
    return q, m


@backends
@both_precisions
@pytest.mark.parametrize("depth", [0, 1, 2, 7])
def test_perlin_and_fractal_noise(backend, precision, depth):
    """perlin_noise (depth 0) and fractal_noise (depth 1, 2, 7) with the builder's Perlin tables on 2^14
    points: uniform in [-300, 300]^3, lattice points, half-integers and the floats either side of an
    integer, at positive and negative cells, against Noise.hs:15-46 in long double (cells as exact
    integers, low 8 bits).  Within K eps S, S = the sum of the absolute terms + eps-sized input term
    (|q|inf <= 300 enters exactly, so S has no Lipschitz term here).  The noise at a lattice point is
    exactly 0 for one layer.  Measured (units of eps S): plain formula 1.31 - 2.02 (K = 16; 32 for one FP32
    layer); emulator the same figures (it runs the same sequence), MI355X 1.21 - 1.96."""
    A = arrays("noise_textures", precision)
    real, eps = real_of(precision), eps_of(precision)
    perm, grad = A["perlin_perm"].reshape(3, 256), A["perlin_grad"]
    q, m = noise_points(precision, np.random.default_rng(200 + depth), N_FAMILY)
    assert np.abs(q).max() * 2.0 ** max(depth - 1, 0) < 2.0 ** 30
    layers = max(depth, 1)
    ref, mag = fractal_np(perm, grad, layers, q, LD)
    base_v, _ = fractal_np(perm, grad, layers, q, real)
    assert base_v.dtype == real
    S = mag.astype(np.float64) + 2.0 ** -10
    base = float((np.abs(base_v.astype(LD) - ref) / (eps * S)).max())
    K = k_from_baseline(base)
    got, = run(backend, precision, "noise", depth, A["perlin_perm"], grad, q)
    err = float((np.abs(got.astype(LD) - ref) / (eps * S)).max())
    measure(backend, f"noise_depth{depth}_{precision}", n=len(q), baseline_err=base, K=K, worst_err=err)
    assert err <= K, (err, K, base)
    if depth <= 1:
        assert (got[:m] == 0).all() and (ref[:m] == 0).all()
    assert np.abs(got).max() <= 2 * math.sqrt(3) / 2 + 1e-5  # Noise.hs:20, summed over the halving weights


def noise_texture_reference(T, perm, grad, tid, p, dt):
    """Texture.hs:56-79 in dtype dt on the rows of p for texture records T[tid]: colours and their S."""
    out = np.zeros((len(tid), 3), dt)
    S = np.zeros(len(tid), np.float64)
    for t in np.unique(tid):
        sel = tid == t
        prm = T["prm"][t].astype(dt)
        pp = p[sel].astype(dt)
        absp = np.abs(p[sel].astype(np.float64))
        if T["kind"][t] == M.TEX_NOISE:
            depth = int(T["nu"][t])
            q = pp * prm[0] + prm[1:4]
            f, mag = fractal_np(perm, grad, depth, q, dt)
            n = f * (dt(0.5) / dt(0.8)) + dt(0.5)
            c0, c1 = T["c0"][t].astype(dt), T["c1"][t].astype(dt)
            out[sel] = c0 + (c1 - c0) * n[:, None]
            qmag = (absp * abs(float(prm[0])) + np.abs(prm[1:4].astype(np.float64))).max(1)
            Sn = 0.625 * (mag.astype(np.float64) + depth * LIPSCHITZ * qmag) + 1.0
            dc = float(np.abs((c1 - c0).astype(np.float64)).max())
            S[sel] = float(np.abs(c0.astype(np.float64)).max()) + dc * (np.abs(n.astype(np.float64)) + Sn)
        else:
            freq = prm[3]
            dots = pp * prm[0:3]
            arg = freq * (dots[:, 0] + dots[:, 1] + dots[:, 2])
            q = pp * (dt(0.25) * freq) + prm[4:7]
            f, mag = fractal_np(perm, grad, 7, q, dt)
            m = dt(0.5) + dt(0.5) * np.sin(arg + dt(10) * np.abs(f))
            out[sel] = m[:, None]
            qmag = (absp * abs(0.25 * float(freq)) + np.abs(prm[4:7].astype(np.float64))).max(1)
            sarg = abs(float(freq)) * (absp * np.abs(prm[0:3].astype(np.float64))).sum(1)
            # sin's argument: its own terms, the sum's rounding (|sinArg|) and 10 x the turbulence's S
            S[sel] = 0.5 * (2 * sarg + 10.0 * (mag.astype(np.float64) + 7 * LIPSCHITZ * qmag)) + 1.0
    return out, S


@backends
@both_precisions
def test_texture_noise_and_marble(backend, precision):
    """eval_texture<true> on the builder's noise (1, 2 and 7 layers) and marble records: 2^14 hit points p,
    uniform in [-300 / freq, 300 / freq]^3 plus the lattice, half-integer and next-to-integer points of
    the noise family, against Texture.hs:56-79 / Noise.hs:15-50 in long double on the exactly formed
    freq p + shift (FP32 inputs: exact in long double).  Within K eps S; S: the sum of the absolute terms
    plus the noise's Lipschitz bound (19 per layer) times |q|inf, for marble the sine argument's terms and
    |sinArg| as well.  The noise colour stays within [c0, c1] up to K eps S.  Measured (units of eps S): plain
    formula 0.023 in both precisions (the Lipschitz term makes S generous), so K = 1/4; emulator and MI355X 0.023."""
    A = arrays("noise_textures", precision)
    real, eps = real_of(precision), eps_of(precision)
    T = A["texs"]
    perm, grad = A["perlin_perm"].reshape(3, 256), A["perlin_grad"]
    rng = np.random.default_rng(300)
    tids = np.flatnonzero(np.isin(T["kind"], (M.TEX_NOISE, M.TEX_MARBLE)))
    assert len(tids) == len(NOISE_TEXTURES) + len(MARBLE_TEXTURES)
    q, _ = noise_points(precision, rng, N_FAMILY)
    tid = tids[rng.integers(0, len(tids), N_FAMILY)]
    freq = np.where(T["kind"][tid] == M.TEX_NOISE, T["prm"][tid][:, 0], 0.25 * T["prm"][tid][:, 3])
    p = (q.astype(np.float64) / freq[:, None]).astype(real)  # powers of two: q = freq p exactly, shift added after
    ref, S = noise_texture_reference(T, perm, grad, tid, p, LD)
    base_v, _ = noise_texture_reference(T, perm, grad, tid, p, real)
    assert base_v.dtype == real
    base = float((np.abs(base_v.astype(LD) - ref).max(1) / (eps * S)).max())
    K = k_from_baseline(base)
    got = run_texture(backend, precision, A, tid, np.zeros(N_FAMILY), np.zeros(N_FAMILY), p)
    err = float((np.abs(got.astype(LD) - ref).max(1) / (eps * S)).max())
    measure(backend, f"texture_noise_marble_{precision}", n=N_FAMILY, baseline_err=base, K=K, worst_err=err)
    assert err <= K, (err, K, base)
    noise = T["kind"][tid] == M.TEX_NOISE
    lo, hi = np.minimum(NOISE_C0, NOISE_C1), np.maximum(NOISE_C0, NOISE_C1)
    slack = (K * eps * S[noise])[:, None]
    g = got[noise].astype(np.float64)
    assert (g >= lo - slack).all() and (g <= hi + slack).all()
    assert (got[~noise] >= 0).all() and (got[~noise] <= 1).all()


def mixed_scene():
    img = image_of(0, 3, 2)
    rot = G.translate(V3(1, 2, 3)) @ G.rotateY(0.4) @ G.rotateX(-0.3)
    return G.group([
        white(G.cuboid(fromCorners(V3(0, 0, 0), V3(1, 2, 3)))),
        G.transform(rot, M.lambertian(M.imageTexture(img)) << G.sphere(V3(5, 0, 0), 0.5)),
        M.lambertian(M.noiseTexture(2, 2.0, V3(10, 0, 0), V3(0, 0, 0), V3(1, 1, 1))) << G.sphere(V3(-5, 0, 0), 0.5),
        M.lambertian(M.checkerTexture(3, 7, V3(*C0), V3(*C1))) << G.triangle(
            (V3(0, 5, 0), (-0.5, 0.25)), (V3(1, 5, 0), (1.5, 0.0)), (V3(0, 5, 1), (0.25, 2.0))),
    ])


SCENES = {"mixed": mixed_scene, "uv_textures": uv_texture_scene, "noise_textures": noise_texture_scene}


# ------------------------------------------------------------------ b. surface_info
def rec_int(col):
    """The int a record keeps in a real's low 32 bits (rt_trace.h RT_R2I)."""
    col = np.ascontiguousarray(col)
    return col.view(np.int32).copy() if col.dtype == np.float32 else (col.view(np.int64) & 0xffffffff).astype(np.uint32).view(np.int32)


SPHERE_RADII = [0.01, 0.07, 0.4, 1.0, 3.0, 25.0, 100.0, -0.5, -20.0]  # (negative radius: Geometry.hs:83 divides by it)


def sphere_scene():
    """Textured spheres, each once as it is (centre x = z = 0, so that the seam and the poles can be hit
    exactly) and once under a rotation of its own (a `uvframe` from the builder)."""
    tex = M.lambertian(M.imageTexture(image_of(0, 4, 2)))
    obs = []
    for k, r in enumerate(SPHERE_RADII):
        obs.append(tex << G.sphere(V3(0.0, 0.05 * abs(r), 0.0), r))
        rot = G.rotateY(0.3 + 0.7 * k) @ G.rotateX(-1.1 + 0.4 * k) @ G.rotateZ(0.2 * k)
        obs.append(G.transform(rot, tex << G.sphere(V3(0.03 * abs(r), -0.04 * abs(r), 0.02 * abs(r)), 1.5 * r)))
    return G.group(obs)


SCENES["spheres"] = sphere_scene


@functools.lru_cache(None)
def sphere_surface_cases(precision):
    """2^12 hits on the builder's sphere records: half uniform on the sphere, the rest on the seam of
    sphereUV (on.x = +-0, on.z < 0; spheres without a frame), within 1e-6 of it on both sides, on the poles
    and within 1e-6 of them; a quarter of the rays come from inside (back face)."""
    real = real_of(precision)
    A = arrays("spheres", precision)
    rows = np.flatnonzero((rec_int(A["prims"][:, 3]) & 3) == 0)
    assert len(rows) == 2 * len(SPHERE_RADII)
    uvf = rec_int(A["prims"][rows, 6])
    assert (uvf >= 0).sum() == len(SPHERE_RADII) and (uvf < 0).sum() == len(SPHERE_RADII)
    assert (A["prims"][rows, 4] < 0).sum() == 4  # the builder keeps a negative radius
    rng = np.random.default_rng(400)
    n = N_EXACT
    cat = np.where(np.arange(n) % 2 == 0, 0, 1 + (np.arange(n) // 2) % 4)  # 0 uniform, 1 seam, 2 near seam, 3 pole, 4 near pole
    plain = rows[uvf < 0]
    pick = rows[rng.integers(0, len(rows), n)]
    exact = (cat == 1) | (cat == 3)
    pick[exact] = plain[rng.integers(0, len(plain), int(exact.sum()))]
    rec = A["prims"][pick].astype(np.float64)
    c, r = rec[:, 0:3], rec[:, 4]
    fidx = rec_int(A["prims"][pick, 6])
    F = np.tile(np.eye(3), (n, 1, 1))
    framed = fidx >= 0
    F[framed] = A["uvframes"][fidx[framed]].astype(np.float64).reshape(-1, 3, 4)[:, :, :3]
    on = random_units(rng, n)
    sgn = rng.choice([-1.0, 1.0], n)
    y = rng.uniform(-0.95, 0.95, n)
    small = 1e-6 * rng.uniform(0.1, 1.0, n)
    seam = np.stack([np.copysign(0.0, sgn), y, -np.sqrt(1 - y * y)], 1)
    near = np.stack([sgn * small, y, -np.sqrt(1 - y * y - small ** 2)], 1)
    pole = np.stack([np.zeros(n), sgn, np.zeros(n)], 1)
    b = 1e-6 * rng.uniform(-1, 1, n)
    npole = np.stack([small * sgn, rng.choice([-1.0, 1.0], n) * np.sqrt(1 - small ** 2 - b ** 2), b], 1)
    for k, v in ((1, seam), (2, near), (3, pole), (4, npole)):
        on = np.where((cat == k)[:, None], v, on)
    outward = np.einsum("nij,ni->nj", F, on)  # F^T on
    p = c + r[:, None] * outward
    back = rng.random(n) < 0.25
    d = random_units(rng, n)
    for _ in range(64):
        bad = np.abs((d * outward).sum(1)) < 0.05
        if not bad.any():
            break
        d[bad] = random_units(rng, int(bad.sum()))
    flipd = ((d * outward).sum(1) > 0) != back
    d = np.where(flipd[:, None], -d, d)
    # exact seam: the ray lies in the plane x = +-0; exact poles: along the y axis
    ang = rng.uniform(0, 2 * np.pi, n)
    dyz = np.stack([np.copysign(0.0, sgn), np.cos(ang), np.sin(ang)], 1)
    for _ in range(64):
        bad = np.abs((dyz * outward).sum(1)) < 0.05
        if not bad.any():
            break
        ang[bad] = rng.uniform(0, 2 * np.pi, int(bad.sum()))
        dyz = np.stack([np.copysign(0.0, sgn), np.cos(ang), np.sin(ang)], 1)
    flipd = ((dyz * outward).sum(1) > 0) != back
    dyz = np.where(flipd[:, None], -dyz, dyz)
    dyz[:, 0] = np.copysign(0.0, sgn)
    d = np.where((cat == 1)[:, None], dyz, d)
    dy = np.stack([np.zeros(n), np.where(back, 1.0, -1.0) * np.sign(outward[:, 1]), np.zeros(n)], 1)
    d = np.where((cat == 3)[:, None], dy, d)
    t = np.abs(r) * rng.uniform(0.5, 2.0, n)
    o = p - t[:, None] * d
    o[cat == 1, 0] = np.copysign(0.0, sgn[cat == 1])
    o[cat == 3, 0] = 0.0
    o[cat == 3, 2] = 0.0
    cr = lambda x: np.ascontiguousarray(x, dtype=real)  # noqa: E731
    return dict(pick=pick, rec=A["prims"][pick], F=F, framed=framed, cat=cat, back=back, o=cr(o), d=cr(d), t=cr(t))


def sphere_surface_formula(C, dt):
    """Geometry.hs:82-88, 100-104 in dtype dt (the frame applied as the rows of R^T, scene.py uvframe_of):
    n (outward), on, u, v; acos's argument clamped to [-1, 1] (the rounded hit point is not exactly on
    the sphere; the reference's acos is NaN beyond)."""
    pi = PI_LD if dt is LD else dt(np.pi)
    o, d, t = C["o"].astype(dt), C["d"].astype(dt), C["t"].astype(dt)
    c, r = C["rec"][:, 0:3].astype(dt), C["rec"][:, 4].astype(dt)
    outward = ((o + t[:, None] * d) - c) / r[:, None]
    Fm = C["F"].astype(dt)
    on = np.where(C["framed"][:, None], np.stack([(Fm[:, k, :] * outward).sum(1) for k in range(3)], 1), outward)
    u = np.arctan2(on[:, 0], on[:, 2]) / (dt(2) * pi) + dt(0.5)
    v = np.arccos(np.clip(-on[:, 1], dt(-1), dt(1))) / pi
    return outward, on, u, v


@backends
@both_precisions
def test_surface_info_spheres(backend, precision):
    """surface_info on 2^12 hits of the builder's sphere records (radius 1e-2 .. 1e2 and two negative radii;
    with and without a rotated uvframe): uniform hit points, the seam of sphereUV exactly and within 1e-6,
    the poles exactly and within 1e-6, a quarter of the rays from inside.  `front` equals the exact sign of
    d . outward (Python integers) unless the margin is within 64 eps scale (at most 0.5 %); n = +-outward
    and p within K eps Sy, Sy = (|o|inf + |t| + |c|inf) / |r| + 1; u within K eps Su modulo 1 (the seam), Su = Sy / (2 pi
    rho) + 1 with rho = |(on.x, on.z)| (atan2's condition number: u is arbitrary at a pole, where only its range is
    asserted); v within K eps Sv, Sv = Sy / (pi sqrt(max(1 - y^2, eps Sy))) + 1 (acos is ill-conditioned at the
    poles, capped); 0 <= u, v <= 1 always; need_uv = false gives the same p, n, front bit for bit.  K from the
    plain formula of Geometry.hs:82-104 in numpy at the working precision.  Measured (n, u, v in units of
    eps S): plain formula 0.42, 0.42, 0.73 (FP32) and 0.33, 0.40, 0.57 (binary64), so K = 4, 4, 8; emulator 0.46,
    0.50, 0.72 / 0.39, 0.40, 0.57; MI355X 0.43, 0.31, 0.78 / 0.38, 0.30, 0.57; nothing skipped.  (On the MI355X the
    fused -pi (0.5 / pi) + 0.5 gave u = -1.1e-17 at the seam in binary64 before surface_info clamped it.)"""
    C = sphere_surface_cases(precision)
    real, eps = real_of(precision), eps_of(precision)
    A = arrays("spheres", precision)
    n = N_EXACT
    zeros6 = np.zeros((n, 6), real)
    hp, hn, front, uv, gid = run(backend, precision, "surface", 1, C["rec"], zeros6, A["uvframes"], C["o"], C["d"], C["t"])
    hp0, hn0, front0, uv0, gid0 = run(backend, precision, "surface", 0, C["rec"], zeros6, A["uvframes"], C["o"], C["d"], C["t"])
    assert same_bits(hp, hp0).all() and same_bits(hn, hn0).all() and (front == front0).all() and (gid == gid0).all()
    assert (uv0 == 0).all()
    assert (gid == rec_int(C["rec"][:, 7])).all()
    # front: the exact sign of d . (o + t d - c) r
    f = {k: C[k].astype(np.float64) for k in ("o", "d")}
    c64, r64, t64 = C["rec"][:, 0:3].astype(np.float64), C["rec"][:, 4].astype(np.float64), C["t"].astype(np.float64)
    s = scale_of(f["o"], f["d"], c64, t64)
    I = {k: np.stack([to_int(x[:, j], s) for j in range(3)], 1) for k, x in dict(o=f["o"], d=f["d"], c=c64).items()}
    margin = dot_i(I["d"], I["o"] - I["c"]) * (1 << s) + dot_i(I["d"], I["d"]) * to_int(t64, s)
    margin = np.where(r64 < 0, -margin, margin)
    want_front = np.array([m <= 0 for m in margin])
    mscale = (np.abs(f["d"]) * (np.abs(f["o"]) + np.abs(c64))).sum(1) + np.abs(t64) * (f["d"] ** 2).sum(1)
    mfloat = ratio(margin, np.full(n, 1 << (3 * s), object))
    skip = undecided([(mfloat, mscale)], eps)
    assert skip.mean() <= 0.005, skip.mean()
    wrong = ((front != 0) != want_front) & ~skip
    assert not wrong.any(), (int(wrong.sum()), np.flatnonzero(wrong)[:8])
    assert (want_front != C["back"]).all()  # the family holds both faces as constructed
    ok = ~skip
    outward, on, u, v = sphere_surface_formula(C, LD)
    b_out, b_on, b_u, b_v = sphere_surface_formula(C, real)
    assert b_u.dtype == real and b_v.dtype == real
    Sy = (np.abs(f["o"]).max(1) + np.abs(t64) + np.abs(c64).max(1)) / np.abs(r64) + 1.0
    rho = np.sqrt((on[:, 0] ** 2 + on[:, 2] ** 2).astype(np.float64))
    at_pole = C["cat"] == 3
    Su = Sy / (2 * np.pi * np.maximum(rho, 1e-300)) + 1.0
    y2 = (on[:, 1].astype(np.float64)) ** 2
    Sv = Sy / (np.pi * np.sqrt(np.maximum(1 - y2, eps * Sy))) + 1.0
    def mod1(x):
        x = np.abs(x)
        return np.minimum(x, np.abs(1 - x))
    n_ref = np.where(want_front[:, None], outward, -outward)
    def errors(nn, uu, vv):
        en = float((np.abs(nn.astype(LD) - n_ref).max(1)[ok] / (eps * Sy[ok])).max())
        eu = float((mod1(uu.astype(LD) - u)[ok & ~at_pole] / (eps * Su[ok & ~at_pole])).max())
        ev = float((np.abs(vv.astype(LD) - v)[ok] / (eps * Sv[ok])).max())
        return en, eu, ev
    base = errors(np.where(want_front[:, None], b_out, -b_out), b_u, b_v)
    K = [k_from_baseline(x) for x in base]
    got = errors(hn, uv[:, 0], uv[:, 1])
    pl = C["o"].astype(LD) + C["t"].astype(LD)[:, None] * C["d"].astype(LD)
    ep = float((np.abs(hp.astype(LD) - pl).max(1) / (eps * (np.abs(f["o"]).max(1) + np.abs(t64)))).max())
    norm_dev = float((np.abs(np.sqrt((hn.astype(LD) ** 2).sum(1)) - np.sqrt((n_ref ** 2).sum(1)))[ok] / (eps * Sy[ok])).max())
    measure(backend, f"surface_sphere_{precision}", n=n, skipped=float(skip.mean()), baseline_n_u_v=base, K_n_u_v=K,
            worst_n_u_v=got, worst_p=ep, worst_norm_dev=norm_dev)
    assert ep <= 2.0  # p = o + t d: two roundings at most (one with FMA)
    for g, k in zip(got, K):
        assert g <= k, (got, K, base)
    assert norm_dev <= K[0]
    assert (uv >= 0).all() and (uv <= 1).all()
    seam = C["cat"] == 1  # exactly on the seam: the reference's u is 0 or 1, by the sign of the zero
    assert np.isin(u[seam].astype(np.float64), (0.0, 1.0)).all() and 0.3 < (u[seam] == 0).mean() < 0.7
    assert (np.minimum(uv[seam, 0], 1 - uv[seam, 0]) <= K[1] * eps * Su[seam]).all()


TRI_UV = [((-0.5, 0.25), (1.5, 0.0), (0.25, 2.0)), ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0)),
          ((3.0, -2.0), (-1.0, -1.0), (0.5, 0.5)), ((1.0, 1.0), (1.0, 1.0), (-4.0, 2.5))]


def plane_scene():
    rng = np.random.default_rng(500)
    tex = M.lambertian(M.checkerTexture(3, 7, V3(*C0), V3(*C1)))
    obs = []
    for k in range(6):
        size = 10.0 ** (k - 2.5)
        q = size * rng.uniform(-0.1, 0.1, 3)
        while True:
            u, v = random_units(rng, 2) * size * rng.uniform(0.5, 1.0, (2, 1))
            if np.linalg.norm(np.cross(u, v)) > 0.5 * np.linalg.norm(u) * np.linalg.norm(v):
                break
        if k < 4:
            uv = TRI_UV[k]
            obs.append(tex << G.triangle((V3(*q), uv[0]), (V3(*(q + u)), uv[1]), (V3(*(q + v)), uv[2])))
        else:
            obs.append(tex << G.parallelogram(V3(*q), V3(*u), V3(*v)))
    return G.group(obs)


SCENES["planes"] = plane_scene


@functools.lru_cache(None)
def plane_surface_cases(precision):
    real = real_of(precision)
    A = arrays("planes", precision)
    kind = rec_int(A["prims"][:, 3]) & 3
    rows = np.flatnonzero(kind != 0)
    assert (kind == 2).sum() == 4 and (kind == 1).sum() == 2
    rng = np.random.default_rng(501)
    n = N_EXACT
    pick = rows[rng.integers(0, len(rows), n)]
    rec = A["prims"][pick].astype(np.float64)
    nrm, q, wa, wb = rec[:, 0:3], rec[:, 4:7], rec[:, 8:11], rec[:, 12:15]
    # the edges from the record's dual basis: u = wb x n / (wa x wb . n) ... simpler: solve per case
    a = rng.uniform(0.01, 0.99, n)
    b = rng.uniform(0.01, 0.99, n)
    over = (a + b > 0.99) & (kind[pick] == 2)
    a, b = np.where(over, 1 - a, a), np.where(over, 1 - b, b)
    p = np.empty((n, 3))
    for k in range(n):  # p with (p - q) . wa = a, (p - q) . wb = b, (p - q) . n = 0
        p[k] = q[k] + np.linalg.solve(np.stack([wa[k], wb[k], nrm[k]]), [a[k], b[k], 0.0])
    d = random_units(rng, n)
    for _ in range(64):
        bad = np.abs((nrm * d).sum(1)) < 0.1
        if not bad.any():
            break
        d[bad] = random_units(rng, int(bad.sum()))
    size = np.linalg.norm(p - q, axis=1) + np.abs(q).max(1)
    t = size * rng.uniform(0.5, 2.0, n)
    o = p - t[:, None] * d
    cr = lambda x: np.ascontiguousarray(x, dtype=real)  # noqa: E731
    return dict(pick=pick, rec=A["prims"][pick], uv=A["prim_uv"][pick], o=cr(o), d=cr(d), t=cr(t))


def plane_surface_formula(C, dt):
    """Geometry.hs:128-131, 175 in the record's terms (a = p_rel . wa, b = p_rel . wb) in dtype dt."""
    o, d, t = C["o"].astype(dt), C["d"].astype(dt), C["t"].astype(dt)
    rec, uv = C["rec"].astype(dt), C["uv"].astype(dt)
    prel = (o + t[:, None] * d) - rec[:, 4:7]
    a, b = (prel * rec[:, 8:11]).sum(1), (prel * rec[:, 12:15]).sum(1)
    w0 = dt(1) - a - b
    return w0 * uv[:, 0] + a * uv[:, 2] + b * uv[:, 4], w0 * uv[:, 1] + a * uv[:, 3] + b * uv[:, 5]


@backends
@both_precisions
def test_surface_info_triangles_and_parallelograms(backend, precision):
    """surface_info on 2^12 interior hits of the builder's triangle and parallelogram records, with the
    builder's prim_uv (triangle corners with negative and > 1 uvs; a parallelogram's are (0,0), (1,0),
    (0,1), i.e. (u, v) = (a, b)): u, v against the barycentric lerp of Geometry.hs:175 in long double within
    K eps S, S = (1 + Sa + Sb) max|uv| + 1 with Sa = sum (|t d| + |o| + |q|) |wa|; front equals the exact sign
    of n . d (|n . d| >= 0.1: nothing skipped); n = +-the record's normal bit for bit; need_uv = false gives
    the same p, n, front bit for bit.  Measured (units of eps S): plain formula 0.41 / 0.40 (FP32 / binary64),
    K = 4; emulator the same, MI355X 0.46 / 0.40."""
    C = plane_surface_cases(precision)
    real, eps = real_of(precision), eps_of(precision)
    A = arrays("planes", precision)
    n = N_EXACT
    hp, hn, front, uv, gid = run(backend, precision, "surface", 1, C["rec"], C["uv"], A["uvframes"], C["o"], C["d"], C["t"])
    hp0, hn0, front0, uv0, gid0 = run(backend, precision, "surface", 0, C["rec"], C["uv"], A["uvframes"], C["o"], C["d"], C["t"])
    assert same_bits(hp, hp0).all() and same_bits(hn, hn0).all() and (front == front0).all() and (gid == gid0).all()
    assert (uv0 == 0).all() and (gid == rec_int(C["rec"][:, 7])).all()
    f = {k: C[k].astype(np.float64) for k in ("o", "d", "t")}
    rec = C["rec"].astype(np.float64)
    s = scale_of(rec[:, 0:3], f["d"])
    D = dot_i(np.stack([to_int(rec[:, j], s) for j in range(3)], 1), np.stack([to_int(f["d"][:, j], s) for j in range(3)], 1))
    want_front = np.array([x < 0 for x in D])
    assert 0.3 < want_front.mean() < 0.7
    assert ((front != 0) == want_front).all()
    assert same_bits(hn, np.where(want_front[:, None], C["rec"][:, 0:3], -C["rec"][:, 0:3])).all()
    u, v = plane_surface_formula(C, LD)
    bu, bv = plane_surface_formula(C, real)
    assert bu.dtype == real
    reach = np.abs(f["t"])[:, None] * np.abs(f["d"]) + np.abs(f["o"]) + np.abs(rec[:, 4:7])
    Sa, Sb = (reach * np.abs(rec[:, 8:11])).sum(1), (reach * np.abs(rec[:, 12:15])).sum(1)
    S = (1 + Sa + Sb) * np.abs(C["uv"].astype(np.float64)).max(1) + 1.0
    def err(uu, vv):
        return float((np.maximum(np.abs(uu.astype(LD) - u), np.abs(vv.astype(LD) - v)) / (eps * S)).max())
    base = err(bu, bv)
    K = k_from_baseline(base)
    got = err(uv[:, 0], uv[:, 1])
    measure(backend, f"surface_plane_{precision}", n=n, skipped=0.0, baseline_err=base, K=K, worst_err=got)
    assert got <= K, (got, K, base)


# ------------------------------------------------------------------ c. test_box
# a box in its own frame [0, L], placed by a rigid m34 (None: axis-aligned at `corner`); faces: the
# parallelograms the scene has (cuboid: all six; the Cornell room: five walls, the front one missing)
def rigid(angles, shift):
    return G.translate(V3(*shift)) @ G.rotateY(angles[0]) @ G.rotateX(angles[1]) @ G.rotateZ(angles[2])


BOXES = {
    "cuboid": dict(L=(1.0, 2.0, 3.0), m=None),
    "rotated": dict(L=(1.5, 0.5, 4.0), m=rigid((0.7, -0.4, 1.1), (3.0, -2.0, 5.0))),
    "cornell": dict(L=(555.0, 555.0, 555.0), m=None),
}


def box_scene(name):
    B = BOXES[name]
    if name == "cornell":  # the five walls of scenes.cornell_walls (no light): the face z = 0 is missing
        return G.group([white(g) for g in (
            G.parallelogram(V3(555, 0, 0), V3(0, 555, 0), V3(0, 0, 555)),
            G.parallelogram(V3(0, 0, 0), V3(0, 555, 0), V3(0, 0, 555)),
            G.parallelogram(V3(0, 0, 0), V3(555, 0, 0), V3(0, 0, 555)),
            G.parallelogram(V3(555, 555, 555), V3(-555, 0, 0), V3(0, 0, -555)),
            G.parallelogram(V3(0, 0, 555), V3(555, 0, 0), V3(0, 555, 0)))])
    g = white(G.cuboid(fromCorners(V3(0, 0, 0), V3(*B["L"]))))
    return g if B["m"] is None else G.transform(B["m"], g)


for _name in BOXES:
    SCENES["box_" + _name] = functools.partial(box_scene, _name)


def box_faces(A):
    """[(face code f, prim, ord, gid)] of the one box group of a scene's arrays (DevBox's 5-bit codes)."""
    assert len(A["boxes"]) == 1
    b = A["boxes"][0]
    out = []
    for f in range(6):
        off = [(int(b[c]) >> (5 * f)) & 31 for c in ("prim_code", "ord_code", "gid_code")]
        if off[0] != 31:
            assert 31 not in off
            out.append((f, int(b["prim_base"]) + off[0], int(b["ord_base"]) + off[1], int(b["gid_base"]) + off[2]))
        else:
            assert off == [31, 31, 31]
    return out


def box_frame(A64):
    """The box frame of a DevBox (binary64 export): corner c, unit axes e_k (rows) and extents L_k, from
    a_k = e_k / L_k and sc_k = a_k . c; face f = 2 k + side is the plane s_k = side."""
    b = A64["boxes"][0]
    a = np.stack([b["a0"], b["a1"], b["a2"]]).astype(np.float64)
    L = 1.0 / np.linalg.norm(a, axis=1)
    e = a * L[:, None]
    assert np.allclose(e @ e.T, np.eye(3), atol=1e-12)
    c = (b["sc"].astype(np.float64) * L) @ e
    return c, e, L


def inward_dirs(rng, n, axis, sign):
    """Unit directions with every component at least 0.05 in magnitude and the `axis` one of sign `sign`."""
    d = random_units(rng, n)
    for _ in range(64):
        bad = (np.abs(d) < 0.05).any(1)
        if not bad.any():
            break
        d[bad] = random_units(rng, int(bad.sum()))
    d[np.arange(n), axis] = np.abs(d[np.arange(n), axis]) * sign
    return d


@functools.lru_cache(None)
def box_cases(name, precision):
    """2^12 rays against the box in seven families (in the box frame, then placed): 0 from outside onto a
    face (the six faces in turn), 1 missing by 1 % .. 50 % of an edge, 2 from inside, 3 as 0 but tmin between
    entry and exit, 4 / 5 starting on a face with self_gid set, heading inward / outward, 6 as 0 towards the
    box's missing face (the Cornell room's open side: through it; face 0 of a whole cuboid)."""
    real = real_of(precision)
    A = arrays("box_" + name, precision)
    faces = box_faces(A)
    corner, e, L = box_frame(arrays("box_" + name, "f64"))
    absent = sorted(set(range(6)) - {f for f, _, _, _ in faces})
    target = absent[0] if absent else 0
    rng = np.random.default_rng(600 + len(name))
    n = N_EXACT
    fam = np.arange(n) % 7
    axis = (np.arange(n) // 7) % 3
    side = (np.arange(n) // 21) % 2
    axis = np.where(fam == 6, target // 2, axis)
    side = np.where(fam == 6, target % 2, side)
    ab = rng.uniform(0.05, 0.95, (n, 3))
    p = ab * L
    p[np.arange(n), axis] = side * L[axis]  # on the face (axis, side)
    sign_in = np.where(side == 1, -1.0, 1.0)
    d = inward_dirs(rng, n, axis, sign_in)
    miss = fam == 1
    off_axis = (axis + 1 + rng.integers(0, 2, n)) % 3
    off_sign = rng.choice([-1.0, 1.0], n)
    delta = rng.uniform(0.01, 0.5, n)
    pm = p.copy()
    pm[np.arange(n), off_axis] = np.where(off_sign > 0, 1 + delta, -delta) * L[off_axis]
    dm = d.copy()
    dm[np.arange(n), off_axis] = np.abs(dm[np.arange(n), off_axis]) * off_sign  # moving further out
    p, d = np.where(miss[:, None], pm, p), np.where(miss[:, None], dm, d)
    size = L.max()
    t = size * rng.uniform(0.5, 2.0, n)
    o = p - t[:, None] * d
    inside = fam == 2
    o = np.where(inside[:, None], rng.uniform(0.05, 0.95, (n, 3)) * L, o)
    d = np.where(inside[:, None], inward_dirs(rng, n, axis, sign_in), d)
    onface = (fam == 4) | (fam == 5)
    o = np.where(onface[:, None], p, o)
    d = np.where((fam == 5)[:, None], -d, d)
    # exit distance of the line in the box frame (for family 3's tmin)
    with np.errstate(divide="ignore"):
        t0, t1 = (0 - o) / d, (L - o) / d
    t_in, t_out = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
    tmin = np.where(fam == 3, 0.5 * (t_in + t_out), KTMIN)
    gid_of = {f: g for f, _, _, g in faces}
    self_gid = np.array([gid_of.get(2 * a + s, -1) if m else -1 for a, s, m in zip(axis, side, onface)], np.int32)
    cr = lambda x: np.ascontiguousarray(x, dtype=real)  # noqa: E731
    return dict(o=cr(corner + o @ e), d=cr(d @ e), tmin=cr(tmin), self_gid=self_gid, fam=fam, face=2 * axis + side,
                absent=absent)


@functools.lru_cache(None)
def box_family_reference(name, precision):
    A = arrays("box_" + name, precision)
    C = box_cases(name, precision)
    # family 3 has a tmin per case: exact per-case evaluation would need one plane_exact per value; its
    # tmin lies mid-way between entry and exit, so the decision "t > tmin" is taken in long double there
    C3 = dict(C)
    fixed = np.where(C["fam"] == 3, real_of(precision)(KTMIN), C["tmin"]).astype(C["tmin"].dtype)
    C3["tmin"] = fixed
    return A, C, box_reference_with_tmin(A, C, C3, precision)


def box_reference_with_tmin(A, C, C3, precision):
    """box_reference at tmin = 1e-4, then family 3's own tmin applied to each face's exact t (the margin
    t - tmin joins the undecided rule)."""
    real, eps = real_of(precision), eps_of(precision)
    faces = box_faces(A)
    n = len(C["o"])
    tmin = C["tmin"].astype(LD)
    best_t = np.full(n, np.inf, LD)
    hit = np.zeros(n, bool)
    prim, order = np.full(n, -1), np.full(n, -1)
    S_w, tb_w = np.ones(n), np.zeros(n, real)
    per_face = []
    tile = lambda v: np.ascontiguousarray(np.tile(v, (n, 1)))  # noqa: E731
    dotr = lambda a, b: a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]  # noqa: E731
    for f, pi, od, gid in faces:
        r = A["prims"][pi]
        Cf = dict(n=tile(r[0:3]), q=tile(r[4:7]), wa=tile(r[8:11]), wb=tile(r[12:15]), o=C["o"], d=C["d"])
        ok, t, margins, S = plane_exact(Cf, False, float(real(KTMIN)))
        und = undecided(margins, eps)
        late = t > tmin
        und |= np.abs((t - tmin).astype(np.float64)) <= 64 * eps * (S + np.abs(C["tmin"].astype(np.float64)))
        live = C["self_gid"] != gid
        ok = ok & late & live
        und = und & live
        with np.errstate(all="ignore"):
            tb = dotr(Cf["n"], Cf["q"] - Cf["o"]) / dotr(Cf["n"], Cf["d"])
        per_face.append((ok, t, und, S, od))
        better = ok & ((t < best_t) | ((t == best_t) & (od < order)))
        best_t = np.where(better, t, best_t)
        prim, order = np.where(better, pi, prim), np.where(better, od, order)
        S_w, tb_w = np.where(better, S, S_w), np.where(better, tb, tb_w).astype(real)
        hit |= better
    skip = np.zeros(n, bool)
    for ok, t, und, S, od in per_face:
        skip |= und & (~hit | (t <= best_t + 64 * eps * S))
        skip |= ok & hit & (od != order) & (np.abs((t - best_t).astype(np.float64)) <= 64 * eps * np.maximum(S, S_w))
    return hit, prim, order, best_t, S_w, tb_w, skip


def run_box(backend, precision, A, C, count=None):
    sl = slice(0, count)
    return run(backend, precision, "box", 0, A["boxes"], C["o"][sl], C["d"][sl], C["tmin"][sl], C["self_gid"][sl])


@backends
@both_precisions
@pytest.mark.parametrize("name", list(BOXES))
def test_box_group_random_families(backend, precision, name):
    """test_box<false> on the builder's DevBox of an axis-aligned cuboid, a cuboid under a rigid rotation and
    translation, and the five-wall Cornell room (a missing face code): 2^12 rays in seven families (box_cases),
    against the closest hit over the box's face parallelograms, each by plane_exact on the exported face
    records, ties by key order.  Hit / miss, the winning primitive and its key order equal the exact result
    unless the case is undecided (a candidate face's edge or tmin margin within 64 eps scale of zero, or two
    faces' t within 64 eps S): at most 0.5 %.  t within K eps S (S, K as in the plane tests).  Every face the
    box has is reached as entry and as exit, and the result of an element does not depend on its neighbours:
    the first 1, 63, 64 and 65 elements alone give the same bits (the exit face is decoded under a wave-wide
    RT_ANY).  Measured (units of eps S): plain formula 0.36 - 0.44, K = 4; emulator and MI355X 0.51 - 0.60 (FP32)
    and 0.72 - 0.87 (binary64, the reciprocal from the product); skipped 0.05 % (rotated, FP32), else none."""
    A, C, (hit, prim, order, t, S, tb, skip) = box_family_reference(name, precision)
    real, eps = real_of(precision), eps_of(precision)
    n = N_EXACT
    got_t, got_prim, got_ord = run_box(backend, precision, A, C)
    assert skip.mean() <= 0.005, skip.mean()
    got_hit = got_prim >= 0
    assert (np.isinf(got_t) == ~got_hit).all()
    use = ~skip
    wrong = use & ((got_hit != hit) | (got_prim != prim) | (got_ord != order))
    assert not wrong.any(), (int(wrong.sum()), [(int(k), int(C["fam"][k]), int(prim[k]), int(got_prim[k])) for k in np.flatnonzero(wrong)[:8]])
    h = use & hit
    base = float((np.abs(tb[h].astype(LD) - t[h]) / (eps * S[h])).max())
    K = k_from_baseline(base)
    err = float((np.abs(got_t[h].astype(LD) - t[h]) / (eps * S[h])).max())
    fam = C["fam"]
    prim_of = {f: p for f, p, _, _ in box_faces(A)}
    entered = {f for f in prim_of if ((fam == 0) & h & (C["face"] == f) & (prim == prim_of[f])).any()}
    left = {f for f in prim_of if ((fam == 2) & h & (prim == prim_of[f])).any()}
    assert entered == set(prim_of) and left == set(prim_of), (entered, left)
    assert not hit[fam == 1].any() and not hit[fam == 5].any()  # missing; leaving the box from its surface
    if name == "cornell":
        assert len(prim_of) == 5 and len(C["absent"]) == 1
        # through the open side: the exit face from outside; from inside some rays leave through it
        assert hit[fam == 6].all() and 0.05 < 1 - hit[fam == 2].mean() < 0.5 and not hit[fam == 2].all()
    else:
        assert len(prim_of) == 6 and hit[(fam != 1) & (fam != 5)].all()
    measure(backend, f"box_{name}_{precision}", n=n, skipped=float(skip.mean()), baseline_err=base, K=K, worst_err=err,
            hits=int(h.sum()))
    assert err <= K, (err, K, base)
    for count in (1, 63, 64, 65):
        for k in range(7):  # every family at the front of the wave in turn
            Ck = {key: np.roll(C[key], -k, axis=0) for key in ("o", "d", "tmin", "self_gid")}
            for x, y in zip(run_box(backend, precision, A, Ck, count), (got_t, got_prim, got_ord)):
                want = np.roll(y, -k, axis=0)[:count]
                assert (same_bits(x, want) if x.dtype.kind == "f" else x == want).all(), (count, k)


def box_exact_case(faces, prims, o, d, tmin, self_gid):
    """One ray against the box's face records in Fractions (Geometry.hs:117-151, 335-347): (prim, ord, t) of
    the closest accepted face, ties to the lower key order, or None."""
    F = lambda v: [Fraction(float(x)) for x in v]  # noqa: E731
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]  # noqa: E731
    o, d, tmin = F(o), F(d), Fraction(float(tmin))
    best = None
    for f, pi, od, gid in faces:
        if gid == self_gid:
            continue
        r = prims[pi]
        n, q, wa, wb = F(r[0:3]), F(r[4:7]), F(r[8:11]), F(r[12:15])
        denom = dot(n, d)
        if not abs(denom) > Fraction(1e-8):
            continue
        t = dot(n, [a - b for a, b in zip(q, o)]) / denom
        if not t > tmin:
            continue
        prel = [a + t * b - c for a, b, c in zip(o, d, q)]
        a, b = dot(prel, wa), dot(prel, wb)
        if 0 <= a <= 1 and 0 <= b <= 1 and (best is None or (t, od) < (best[2], best[1])):
            best = (pi, od, t)
    return best


def box_constructed(backend, precision, label, x, dl, tmin, K_floor=1.0):
    """Rays given in the frame of the axis-aligned cuboid (exact: its axes are signed coordinate axes and
    its corner is dyadic), against box_exact_case; no skips.  t within K eps |t| (K from the plain formula
    n . (q - o) / n . d of the winning face at the working precision, at least K_floor)."""
    real, eps = real_of(precision), eps_of(precision)
    A = arrays("box_cuboid", precision)
    corner, e, L = box_frame(arrays("box_cuboid", "f64"))
    assert set(np.abs(e).reshape(-1)) == {0.0, 1.0}
    o = np.ascontiguousarray(corner + np.asarray(x) @ e, real)
    d = np.ascontiguousarray(np.asarray(dl) @ e, real)
    n = len(o)
    tm = np.full(n, tmin, real)
    C = dict(o=o, d=d, tmin=tm, self_gid=np.full(n, -1, np.int32))
    got_t, got_prim, got_ord = run_box(backend, precision, A, C)
    faces = box_faces(A)
    want = [box_exact_case(faces, A["prims"], o[k], d[k], tm[k], -1) for k in range(n)]
    w_prim = np.array([-1 if w is None else w[0] for w in want])
    w_ord = np.array([-1 if w is None else w[1] for w in want])
    bad = (got_prim != w_prim) | (got_ord != w_ord)
    assert not bad.any(), (label, int(bad.sum()), [(list(map(float, x[k])), list(map(float, dl[k])), int(w_prim[k]), int(got_prim[k]))
                                                   for k in np.flatnonzero(bad)[:6]])
    hit = w_prim >= 0
    assert np.isinf(got_t[~hit]).all()
    err = base = 0.0
    for k in np.flatnonzero(hit):
        r = A["prims"][w_prim[k]]
        with np.errstate(all="ignore"):
            num = r[0] * (r[4] - o[k, 0]) + r[1] * (r[5] - o[k, 1]) + r[2] * (r[6] - o[k, 2])
            den = r[0] * d[k, 0] + r[1] * d[k, 1] + r[2] * d[k, 2]
            plain = num / den
        t = want[k][2]
        unit = eps * float(abs(t))
        base = max(base, float(abs(Fraction(float(plain)) - t)) / unit)
        err = max(err, float(abs(Fraction(float(got_t[k])) - t)) / unit)
    K = max(k_from_baseline(base), K_floor)
    measure(backend, f"box_{label}_{precision}", n=n, hits=int(hit.sum()), baseline_err=base, K=K, worst_err=err)
    assert err <= K, (label, err, K, base)
    return hit


def axis_parallel_rays(rng):
    """Directions exactly parallel to one and to two axes of the cuboid (zero components of both signs),
    from origins inside and outside the slabs of the parallel axes, inside and outside the box."""
    L = np.array([1.0, 2.0, 3.0])  # extents in the DevBox frame's order are read from the frame; any order works
    xs, ds = [], []
    for zero_axes in ([0], [1], [2], [0, 1], [0, 2], [1, 2]):
        for rep in range(24):
            d = rng.choice([-1.0, 1.0], 3) * rng.uniform(0.3, 1.0, 3)
            for k in zero_axes:
                d[k] = rng.choice([-0.0, 0.0])
            d = d / np.linalg.norm(d)
            s = rng.uniform(0.05, 0.95, 3)  # inside
            where = rep % 4
            if where == 1:  # outside the slab of a parallel axis: a miss
                s[zero_axes[0]] = rng.choice([-0.5, 1.5])
            if where >= 2:  # outside the box along a moving axis, ahead of or behind it
                moving = [k for k in range(3) if k not in zero_axes]
                k = moving[rep % len(moving)]
                s[k] = -0.7 if (d[k] > 0) == (where == 2) else 1.7
            xs.append(s)
            ds.append(d)
    return np.array(xs), np.array(ds)


@backends
@both_precisions
def test_box_group_axis_parallel_rays(backend, precision):
    """Directions exactly parallel to one and to two box axes (+0 and -0 components) on the axis-aligned
    cuboid: binary64 takes the guarded-reciprocal branch (the product of the three a_k . d is zero), FP32
    divides by zero.  Origins inside the parallel axes' slabs (the ray meets the box: from inside the exit
    face, from outside the entry face, behind it nothing) and outside them (a miss), against the exact
    closest hit over the face parallelograms (a parallel face is never hit: |n . d| > 1e-8 fails).  No skips.
    This test found the rays inside a parallel axis's slab missing the box (t1 = fma(-s, inf, inf) = NaN); see
    box_rcp in rt_trace.h.  Measured (units of eps |t|): plain formula 0.73 / 0.63, K = 8; both backends 1.53 / 1.03."""
    corner, e, L = box_frame(arrays("box_cuboid", "f64"))
    s, d = axis_parallel_rays(np.random.default_rng(700))
    hit = box_constructed(backend, precision, "axis_parallel", s * L, d, KTMIN)
    assert 0.4 < hit.mean() < 0.8, hit.mean()


@backends
def test_box_group_extreme_direction_components(backend):
    """Binary64 direction components of 1e-200 and 1e200 (the product of the three a_k . d underflows or
    overflows: the guarded-reciprocal branch; with one such component the product is in range), origins
    inside and outside the box, tmin = 1e-300 so that the hits at t ~ 1e-200 count.  Against the exact
    closest hit; a face whose |n . d| <= 1e-8 is never hit (Geometry.hs:125).  No skips."""
    corner, e, L = box_frame(arrays("box_cuboid", "f64"))
    rng = np.random.default_rng(701)
    xs, ds = [], []
    for big in (1e-200, 1e200):
        for pattern in ((0, 1), (0, 2), (1, 2), (0,), (1,), (2,)):
            for rep in range(16):
                d = rng.choice([-1.0, 1.0], 3) * rng.uniform(0.3, 1.0, 3)
                for k in pattern:
                    d[k] = np.sign(d[k]) * big
                s = rng.uniform(0.05, 0.95, 3)
                if rep % 4 == 1:
                    s[pattern[0]] = rng.choice([-0.5, 1.5])
                if rep % 4 >= 2:
                    k = rng.integers(0, 3)
                    s[k] = -0.7 if (d[k] > 0) == (rep % 4 == 2) else 1.7
                xs.append(s * L)
                ds.append(d)
    hit = box_constructed(backend, "f64", "extreme_components", np.array(xs), np.array(ds), 1e-300, K_floor=8.0)
    assert 0.3 < hit.mean() < 0.9, hit.mean()


# ------------------------------------------------------------------ e. medium_draw
def kernel_log_1mu(backend, precision, words):
    """RT_LOG(1 - u01(w)) of the backend itself (probe "uniform", bounded in test_device_probe.py): the
    draw's one inexact function, so that the roundings around it can be checked bit for bit."""
    out, = run(backend, precision, "uniform", 2, np.ascontiguousarray(words, np.uint32))
    return out


@backends
@both_precisions
def test_medium_draw(backend, precision):
    """medium_draw (Geometry.hs:312-328) on 2^14 random draws: the word is w[m & 3] for every m; hit_dist =
    neg_inv_density log(1 - u) and t = lo + hit_dist are two roundings with no FMA: with the backend's own
    log (probe "uniform") the expected t is fl(lo + fl(nid log)), and tbest equals it bit for bit in
    binary64 and within 1 ulp in FP32 (__logf is re-evaluated inline); both comparisons are strict:
    hit_dist == hi - lo and t == tbest are no hit; u01 = 0 gives hit_dist = 0 and t = lo exactly.  At least
    one random draw in twenty would differ under FMA contraction (checked with exact arithmetic; 9 % do)."""
    real, eps = real_of(precision), eps_of(precision)
    rng = np.random.default_rng(800)
    n = N_FAMILY
    m = rng.integers(0, 4, n).astype(np.int32)
    w = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    nid = (-1.0 / 10.0 ** rng.uniform(-2, 1, n)).astype(real)
    lo = rng.uniform(0.0, 5.0, n).astype(real)
    seg = (10.0 ** rng.uniform(-2, 1.5, n)).astype(real)
    hi = (lo + seg).astype(real)
    tb = np.where(rng.random(n) < 0.5, np.inf, lo + rng.uniform(0, 1, n) * seg).astype(real)
    wsel = w[np.arange(n), m]
    lg = kernel_log_1mu(backend, precision, wsel)
    dist = (nid * lg).astype(real)
    t = (lo + dist).astype(real)
    assert dist.dtype == real and t.dtype == real
    want_hit = (dist < (hi - lo).astype(real)) & (t < tb)
    tbest, hm = run(backend, precision, "medium", m, w, nid, np.stack([lo, hi], 1), tb)
    assert 0.2 < want_hit.mean() < 0.8
    if precision == "f64":
        assert ((hm == m) == want_hit).all() and (hm[~want_hit] == -1).all()
        assert same_bits(tbest, np.where(want_hit, t, tb).astype(real)).all()
        worst = 0
    else:
        # FP32: the inline __logf may differ from the probe's by an ulp, so a decision within an ulp is open
        close = (np.abs(dist - (hi - lo)) <= 4 * eps * np.abs(dist)) | (np.abs(t - tb) <= 4 * eps * np.abs(t))
        assert close.mean() <= 0.005
        assert (((hm == m) == want_hit) | close).all() and ((hm == -1) | (hm == m)).all()
        both = want_hit & (hm == m)
        worst = int(ulp_distance(tbest[both], t[both]).max())
        assert worst <= 1 and same_bits(tbest[hm == -1], tb[hm == -1]).all()
    sample = np.flatnonzero(want_hit)[:512]
    fused = np.array([float(Fraction(float(lo[k])) + Fraction(float(nid[k])) * Fraction(float(lg[k]))) for k in sample])
    differ = float((fused.astype(real) != t[sample]).mean())
    measure(backend, f"medium_draw_{precision}", n=n, hits=int(want_hit.sum()), worst_ulp=worst, fma_would_differ=differ)
    assert differ >= 0.05, differ
    # constructed: strictness and the zero draw (lo = 0 keeps hi - lo exact)
    k = 64
    w0 = rng.integers(256, 1 << 32, k, dtype=np.uint64).astype(np.uint32)
    words = np.stack([w0, w0 ^ 0xffffffff, w0 + 1, w0 + 2], 1).astype(np.uint32)
    mm = (np.arange(k) % 4).astype(np.int32)
    sel = words[np.arange(k), mm]
    nid0 = np.full(k, -0.75, real)
    d0 = (nid0 * kernel_log_1mu(backend, precision, sel)).astype(real)
    assert (d0 > 0).all()
    zero, inf = np.zeros(k, real), np.full(k, np.inf, real)
    up = np.nextafter(d0, real(np.inf))
    if precision == "f64":
        tb_, hm_ = run(backend, precision, "medium", mm, words, nid0, np.stack([zero, d0], 1), inf)
        assert (hm_ == -1).all() and np.isinf(tb_).all()  # hit_dist == hi - lo: no hit
        tb_, hm_ = run(backend, precision, "medium", mm, words, nid0, np.stack([zero, up], 1), inf)
        assert (hm_ == mm).all() and same_bits(tb_, d0).all()
        tb_, hm_ = run(backend, precision, "medium", mm, words, nid0, np.stack([zero, inf], 1), d0)
        assert (hm_ == -1).all() and same_bits(tb_, d0).all()  # t == tbest: no hit
        tb_, hm_ = run(backend, precision, "medium", mm, words, nid0, np.stack([zero, inf], 1), up)
        assert (hm_ == mm).all() and same_bits(tb_, d0).all()
    # u01 = 0 (the word below 256): hit_dist = 0 exactly, t = lo; a hit iff 0 < hi - lo and lo < tbest
    wz = np.stack([np.arange(k, dtype=np.uint32) * 4 % 256] * 4, 1).astype(np.uint32)
    lo1 = rng.uniform(0.5, 2.0, k).astype(real)
    tb_, hm_ = run(backend, precision, "medium", mm, wz, nid0, np.stack([lo1, lo1 + real(1)], 1), inf)
    assert (hm_ == mm).all() and same_bits(tb_, lo1).all()
    tb_, hm_ = run(backend, precision, "medium", mm, wz, nid0, np.stack([lo1, lo1], 1), inf)
    assert (hm_ == -1).all()  # 0 < 0 is false
    tb_, hm_ = run(backend, precision, "medium", mm, wz, nid0, np.stack([lo1, lo1 + real(1)], 1), lo1)
    assert (hm_ == -1).all() and same_bits(tb_, lo1).all()  # t == tbest


# ------------------------------------------------------------------ d. shade_event / mixture_scatter
KEY = (0x1234abcd, 0x9e3779b9)
EV_SCATTER = 2  # rt_internal.h RT_EV_SCATTER
IORS, FUZZ, HG_G = [1.0, 1.3, 1.5, 2.4], [0.0, 0.3, 1.0], [-0.9, 0.0, 0.9]
TEX = (0.8, 0.5, 0.25)
BG0, BG1 = (1.0, 1.0, 1.0), (0.5, 0.7, 1.0)


def dot3(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def absdot3(a, b):
    return (np.abs(a.astype(np.float64)) * np.abs(b.astype(np.float64))).sum(1)


def u01_of(w, dt):
    return (w >> np.uint32(8)).astype(dt) * dt(2.0 ** -24)


def unit_vector_ref(a, b, dt):
    """rt_trace.h unit_vector: z = 1 - 2 u(a), phi = 2 pi u(b) (the project's map of two uniforms to the
    distribution of randomUnitVector, Core.hs:54-60)."""
    z = dt(1) - dt(2) * u01_of(a, dt)
    r = np.sqrt(np.maximum(dt(0), dt(1) - z * z))
    ang = (dt(2) * (PI_LD if dt is LD else dt(np.pi))) * u01_of(b, dt)
    return np.stack([r * np.cos(ang), r * np.sin(ang), z], 1)


def normalize_ref(v):
    return v / np.sqrt(dot3(v, v))[:, None]


def make_targets(precision, specs):
    """DevTarget records (rt_internal.h; Ray.hs:138-151) of [(prob, q, u, v)]."""
    T = np.zeros(len(specs), emu.record_dtypes(precision)["targets"])
    acc = 0.0
    for k, (prob, q, u, v) in enumerate(specs):
        q, u, v = (np.asarray(x, np.float64) for x in (q, u, v))
        cr = np.cross(u, v)
        ncr = np.linalg.norm(cr)
        n = cr / ncr
        ns = n / ncr
        acc += prob
        T[k]["q"], T[k]["u"], T[k]["v"], T[k]["n"], T[k]["cr"] = q, u, v, n, cr
        T[k]["wa"], T[k]["wb"] = np.cross(v, ns), np.cross(ns, u)
        T[k]["prob"], T[k]["thresh"], T[k]["prob_icr"] = prob, acc, prob / ncr
    return T


TARGET_SETS = {
    0: [],
    1: [(0.25, (-1.0, 6.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0))],
    2: [(0.25, (-1.0, 6.0, -1.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0)), (0.5, (5.0, -2.0, -2.0), (0.0, 3.0, 1.0), (0.0, -1.0, 3.0))],
}


def shade_inputs(precision, kind, seed, n=N_FAMILY):
    """n hits on plane records: unit d, the record's unit normal on either side of it (front and back
    faces), incidence from normal (exactly, 1 / 64 of the cases) to grazing (cos log-uniform down to 1e-3
    for an eighth of the cases and down to 1e-6 for 1 / 64), the material's parameter cycling through its
    values, random Philox counters, radiance L and throughput T."""
    real = real_of(precision)
    rng = np.random.default_rng(seed)
    nrm = random_units(rng, n)
    tang = np.cross(nrm, random_units(rng, n))
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    cos = rng.uniform(0.02, 1.0, n)
    idx = np.arange(n)
    cos = np.where(idx % 8 == 1, 10.0 ** rng.uniform(-3, 0, n), cos)
    cos = np.where(idx % 64 == 2, 10.0 ** rng.uniform(-6, -2, n), cos)
    params = {M.METAL: FUZZ, M.DIELECTRIC: IORS, M.ANISOTROPIC: HG_G}.get(kind, [0.0])
    param = np.array(params)[(idx // 64) % len(params)]  # (every incidence class meets every value)
    if kind == M.DIELECTRIC:  # ior = 1: sin_t > 1 / ratio = 1 is open at grazing incidence, keep away from it
        cos = np.where((param == 1.0) & (cos < 0.05), rng.uniform(0.05, 1.0, n), cos)
    sin = np.sqrt(np.maximum(0.0, 1 - cos * cos))
    d = -cos[:, None] * nrm + sin[:, None] * tang
    d = np.where((idx % 64 == 3)[:, None], -nrm, d)
    back = rng.random(n) < (0.5 if kind == M.DIELECTRIC else 0.25)
    nrm = np.where(back[:, None], -nrm, nrm)
    o = rng.uniform(-2, 2, (n, 3))
    t = rng.uniform(0.5, 4.0, n)
    prims = np.zeros((n, 16), real)
    prims[:, 0:3] = nrm
    gid = rng.integers(0, 1 << 20, n).astype(np.int32)
    ints = np.zeros((n, 16), np.int64 if real is np.float64 else np.int32)
    ints[:, 3], ints[:, 7] = 1, gid  # kind 1 (parallelogram), gid
    prims = np.where(ints != 0, ints.view(real), prims)
    mats = np.zeros(n, emu.record_dtypes(precision)["mats"])
    mats["kind"], mats["param"], mats["tex_const"], mats["c0"] = kind, param, 1, TEX
    ctr = np.stack([rng.integers(0, 1 << 24, n), rng.integers(0, 1 << 10, n), rng.integers(0, 50, n)], 1).astype(np.uint32)
    LT = np.concatenate([rng.uniform(0, 2, (n, 3)), rng.uniform(0.05, 1, (n, 3))], 1).astype(real)
    ray = np.concatenate([o, d, t[:, None]], 1).astype(real)
    return dict(prims=prims, mats=mats, how=np.zeros(n, np.int32), ray=ray, ctr=ctr, LT=LT, gid=gid)


def philox_words(ctr):
    c = np.concatenate([ctr, np.full((len(ctr), 1), EV_SCATTER, np.uint32)], 1)
    return philox_ref(c, *KEY)


def run_shade(backend, precision, form, I, targets, rem_prob=None, bg_kind=0, med_mat=0):
    rem = 1.0 - sum(float(p) for p in targets["prob"]) if rem_prob is None else rem_prob
    kp = dict(mats=I["mats"], med_mat=med_mat, key0=KEY[0], key1=KEY[1], targets=targets,
              cfg=[rem, bg_kind] + list(BG0) + list(BG1))
    return run(backend, precision, "shade", form, kp, I["prims"], I["how"], I["ray"], I["ctr"], I["LT"])


def target_terms(T, p, dirn, dt):
    """Ray.hs:199-204: sum_k p_k t_k^2 / |cross_k . dir| over the targets the ray (p, dir) hits (rt_hit: the
    parallelogram on (0, inf), Geometry.hs:117-151, in the record's terms); the decisions' margins; the
    conditioning of the sum's terms."""
    mix = np.zeros(len(p), dt)
    cond = np.zeros(len(p))
    margins = []
    for k in range(len(T)):
        n, q, wa, wb = (np.tile(T[k][f].astype(dt), (len(p), 1)) for f in ("n", "q", "wa", "wb"))
        denom = dot3(n, dirn)
        qo = q - p
        num = dot3(n, qo)
        with np.errstate(all="ignore"):
            t = num / denom
            prel = t[:, None] * dirn - qo
            a, b = dot3(prel, wa), dot3(prel, wb)
            ok = (np.abs(denom) > dt(1e-8)) & (t > 0) & (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)
            term = dt(T[k]["prob_icr"]) * (t * t / np.abs(denom))
        mix = mix + np.where(ok, term, dt(0))
        if dt is LD:
            f64 = lambda x: np.nan_to_num(x.astype(np.float64), posinf=1e300, neginf=-1e300)  # noqa: E731
            sd = absdot3(n, dirn)
            st = (absdot3(n, q) + absdot3(n, p)) / np.maximum(np.abs(f64(denom)), 1e-300) + np.abs(f64(t)) * sd / np.maximum(np.abs(f64(denom)), 1e-300)
            reach = np.abs(f64(t))[:, None] * np.abs(f64(dirn)) + np.abs(f64(q)) + np.abs(f64(p))
            sa = (reach * np.abs(f64(wa))).sum(1) + st * absdot3(dirn, wa)
            sb = (reach * np.abs(f64(wb))).sum(1) + st * absdot3(dirn, wb)
            front_of = f64(t) > 0  # edges matter only for a plane in front of the ray
            big = np.full(len(p), 1e300)
            margins += [(f64(t), st), (np.where(front_of, f64(a), big), sa), (np.where(front_of, f64(1 - a), big), 1 + sa),
                        (np.where(front_of, f64(b), big), sb), (np.where(front_of, f64(1 - b), big), 1 + sb)]
            cond += np.where(ok, 2 * st / np.maximum(np.abs(f64(t)), 1e-300) + sd / np.maximum(np.abs(f64(denom)), 1e-300), 0.0)
    return mix, margins, cond


def shade_reference(I, T, rem_prob, dt):
    """Material.hs:41-129 and Ray.hs:180-224 in dtype dt on the probe's floats.  Returns terminate, L, nd, Tf
    (rows of terminating paths: NaN), the decisions' (margin, scale) list and the scales S_nd, S_Tf."""
    n = len(I["how"])
    pi = PI_LD if dt is LD else dt(np.pi)
    kind = I["mats"]["kind"]
    param = I["mats"]["param"].astype(dt)
    tex = I["mats"]["c0"].astype(dt)
    o, d, t = I["ray"][:, 0:3].astype(dt), I["ray"][:, 3:6].astype(dt), I["ray"][:, 6].astype(dt)
    L, Tp = I["LT"][:, 0:3].astype(dt), I["LT"][:, 3:6].astype(dt)
    w = philox_words(I["ctr"])
    medium = I["how"] == 1
    nrec = I["prims"][:, 0:3].astype(dt)
    nd_ = dot3(nrec, d)
    front = np.where(medium, True, nd_ < 0)
    hn = np.where(medium[:, None], -d, np.where(front[:, None], nrec, -nrec))
    p = o + t[:, None] * d
    margins = [(np.where(medium, 1.0, nd_.astype(np.float64)), absdot3(nrec, d))]
    term = np.zeros(n, bool)
    nd = np.full((n, 3), np.nan, dt)
    Tf = np.full((n, 3), np.nan, dt)
    S_nd, S_tf = np.ones(n), np.ones(n)
    Lout = L.copy()
    k0 = kind == M.LIGHT
    Lout[k0] = (L + Tp * tex)[k0]
    term |= k0 | (kind == M.BLACK)
    refl = d - (dt(2) * dot3(hn, d))[:, None] * hn
    sel = kind == M.MIRROR
    nd[sel], Tf[sel] = normalize_ref(refl)[sel], tex[sel]
    sel = kind == M.TRANSPARENT
    nd[sel], Tf[sel] = d[sel], tex[sel]
    uu = unit_vector_ref(w[:, 1], w[:, 2], dt)
    sel = kind == M.METAL
    if sel.any():
        d2 = refl + param[:, None] * uu
        m = dot3(d2, hn)
        margins.append((np.where(sel, m.astype(np.float64), 1.0), np.where(sel, 3 * absdot3(d, hn) + absdot3(hn, hn) * 0 + 1 + np.abs(param.astype(np.float64)), 1.0)))
        go = sel & (m > 0)
        term |= sel & ~(m > 0)
        nd[go], Tf[go] = normalize_ref(d2)[go], tex[go]
        S_nd = np.where(sel, 1 + (3 + np.abs(param.astype(np.float64))) / np.maximum(np.sqrt(dot3(d2, d2).astype(np.float64)), 1e-300), S_nd)
    sel = kind == M.DIELECTRIC
    if sel.any():
        ratio = np.where(front, dt(1) / param, param)
        cos_t = np.minimum(dt(1), -dot3(hn, d))
        sin_t = np.sqrt(np.maximum(dt(0), dt(1) - cos_t * cos_t))
        r0 = ((dt(1) - ratio) / (dt(1) + ratio)) ** 2
        refl_ce = r0 + (dt(1) - r0) * (dt(1) - cos_t) ** 5
        u = u01_of(w[:, 0], dt)
        tir = ratio * sin_t > 1
        s64, r64 = sin_t.astype(np.float64), ratio.astype(np.float64)
        margins.append((np.where(sel, (ratio * sin_t - 1).astype(np.float64), 1.0), np.where(sel, 1 + r64 * (s64 + np.minimum(1 / np.maximum(s64, 1e-300), 1 / np.sqrt(float(np.finfo(I["ray"].dtype).eps)))), 1.0)))
        margins.append((np.where(sel & ~tir, (refl_ce - u).astype(np.float64), 1.0), np.where(sel, 1 + 8 * absdot3(hn, d), 1.0)))
        perp = ratio[:, None] * (d + cos_t[:, None] * hn)
        para = np.sqrt(np.abs(dt(1) - dot3(perp, perp)))
        refr = normalize_ref(perp - para[:, None] * hn)
        branch = tir | (u < refl_ce)
        nd[sel] = np.where(branch[:, None], normalize_ref(refl), refr)[sel]
        Tf[sel] = dt(1)
        # the refracted direction: para = sqrt|1 - perp^2| loses accuracy as it goes to zero (the critical angle)
        S_nd = np.where(sel & ~branch, 1 + 4 * (1 + r64 ** 2) / np.maximum(para.astype(np.float64), np.sqrt(np.finfo(np.float64).tiny)), S_nd)
    sel = np.isin(kind, (M.LAMBERT, M.LOMMEL, M.ISOTROPIC, M.ANISOTROPIC))
    if sel.any():
        hemi = np.isin(kind, (M.LAMBERT, M.LOMMEL))
        cr = u01_of(w[:, 0], dt)
        choice = np.full(n, -1)
        for k in range(len(T) - 1, -1, -1):
            choice = np.where(cr < dt(T[k]["thresh"]), k, choice)
        hu = hn + uu
        dirn = np.where(hemi[:, None], normalize_ref(hu), uu)
        cond_dir = np.where(hemi, 2 / np.maximum(np.sqrt(dot3(hu, hu).astype(np.float64)), 1e-300), 1.0)
        for k in range(len(T)):
            lp = T[k]["q"].astype(dt) + u01_of(w[:, 1], dt)[:, None] * T[k]["u"].astype(dt) + u01_of(w[:, 2], dt)[:, None] * T[k]["v"].astype(dt)
            to = lp - p
            pick = choice == k
            dirn = np.where(pick[:, None], normalize_ref(to), dirn)
            reach = np.abs(T[k]["q"]).max() + np.abs(T[k]["u"]).max() + np.abs(T[k]["v"]).max() + np.abs(p.astype(np.float64)).max(1)
            cond_dir = np.where(pick, 1 + reach / np.maximum(np.sqrt(dot3(to, to).astype(np.float64)), 1e-300), cond_dir)
        mu1 = dot3(dirn, hn)
        pdf1 = np.where(hemi, mu1 / pi, dt(0.25) / pi)
        below = hemi & ~(pdf1 > 0)
        margins.append((np.where(sel & hemi, mu1.astype(np.float64), 1.0), np.where(sel, cond_dir, 1.0)))
        mix, tmargins, tcond = target_terms(T, p, dirn, dt)
        margins += [(np.where(sel & ~below, m, 1e300), s) for m, s in tmargins]
        pdf = dt(rem_prob) * pdf1 + mix
        mu0 = -dot3(d, hn)
        f = tex.copy()
        ls, hg = kind == M.LOMMEL, kind == M.ANISOTROPIC
        with np.errstate(all="ignore"):
            f = np.where(ls[:, None], (dt(0.25) / (mu0 + mu1))[:, None] * tex, f)
            mu = dot3(d, dirn)
            base = dt(1) + param * param - dt(2) * param * mu
            f = np.where(hg[:, None], ((dt(1) - param * param) / (base * np.sqrt(base)))[:, None] * tex, f)
            tf = (pdf1 / pdf)[:, None] * f
        go = sel & ~below
        term |= sel & below
        nd[go], Tf[go] = dirn[go], tf[go]
        S_nd = np.where(sel, cond_dir, S_nd)
        c = np.ones(n)
        if len(T):
            c += np.where(hemi, cond_dir / np.maximum(np.abs(mu1.astype(np.float64)), 1e-300), 0.0) + tcond
        c += np.where(ls, 2 * (1 + cond_dir) / np.maximum(np.abs((mu0 + mu1).astype(np.float64)), 1e-300), 0.0)
        c += np.where(hg, 6 * (1 + cond_dir) / np.maximum(np.abs(base.astype(np.float64)), 1e-300), 0.0)
        S_tf = np.where(sel, c, S_tf)
    return dict(term=term, L=Lout, nd=nd, Tf=Tf, p=p, margins=margins, S_nd=S_nd, S_tf=S_tf)


def check_shade(backend, precision, label, I, T, outs, rem_prob=None, cap=0.005):
    """The assertions of every shade family; returns the reference, the mask of decided cases."""
    real, eps = real_of(precision), eps_of(precision)
    rem = 1.0 - sum(float(x) for x in T["prob"]) if rem_prob is None else rem_prob
    term, Lo, np_, nd, Tf, ngid = outs
    R = shade_reference(I, T, rem, LD)
    B = shade_reference(I, T, rem, real)
    skip = undecided(R["margins"], eps)
    assert skip.mean() <= cap, (label, skip.mean())
    use = ~skip
    wrong = use & ((term != 0) != R["term"])
    assert not wrong.any(), (label, int(wrong.sum()), np.flatnonzero(wrong)[:8])
    light = I["mats"]["kind"] == M.LIGHT
    L, Tp, tex = I["LT"][:, 0:3], I["LT"][:, 3:6], I["mats"]["c0"]
    assert same_bits(Lo[~light], L[~light]).all()  # only a light adds radiance
    if light.any():
        room = eps * (np.abs(L.astype(np.float64)) + np.abs(Tp.astype(np.float64) * tex.astype(np.float64)))
        assert (np.abs(Lo.astype(LD) - R["L"])[light] <= room[light]).all()  # L + T tex, one or two roundings
    go = use & ~R["term"]
    pscale = np.abs(I["ray"][:, 0:3].astype(np.float64)).max(1) + np.abs(I["ray"][:, 6].astype(np.float64))
    hitp = I["how"] != 2
    assert (np.abs(np_.astype(LD) - R["p"]).max(1)[go] <= 2 * eps * pscale[go]).all()
    assert (ngid[go] == np.where(I["how"] == 1, -1, I["gid"])[go]).all()
    fig = dict(n=int(len(term)), skipped=float(skip.mean()), continuing=int(go.sum()))
    if go.any():
        def errs(x_nd, x_tf):
            e_nd = float((np.abs(x_nd.astype(LD) - R["nd"]).max(1)[go] / (eps * R["S_nd"][go])).max())
            tfscale = np.abs(R["Tf"].astype(np.float64)).max(1) * R["S_tf"] + 1e-300
            e_tf = float((np.abs(x_tf.astype(LD) - R["Tf"]).max(1)[go] / (eps * tfscale[go])).max())
            return e_nd, e_tf
        same_branch = go & ~B["term"] & np.isfinite(B["nd"].astype(np.float64)).all(1)
        keep = go
        go = same_branch
        base = errs(B["nd"], B["Tf"])
        go = keep
        # no less than 8 single roundings (8 x eps / 2): where the plain formula is exact by cancellation
        # (pdf1 / pdf = 1 without targets) the kernel's pdf1 * rcp(pdf) * f still rounds three times
        K = [max(k_from_baseline(b), 4.0) for b in base]
        got = errs(nd, Tf)
        norm_dev = float((np.abs(np.sqrt((nd.astype(LD) ** 2).sum(1)) - 1)[go] / eps).max())
        fig.update(baseline_nd_tf=base, K_nd_tf=K, worst_nd_tf=got, worst_norm_dev_in_eps=norm_dev)
        measure(backend, f"shade_{label}_{precision}", **fig)
        assert got[0] <= K[0] and got[1] <= K[1], (label, got, K, base)
        assert norm_dev <= 8.0, (label, norm_dev)
    else:
        measure(backend, f"shade_{label}_{precision}", **fig)
    return R, use


@backends
@both_precisions
@pytest.mark.parametrize("kind", range(10))
def test_shade_event_each_material(backend, precision, kind):
    """shade_event<2, true, false> on 2^14 random hits per material (kinds 0-9; shade_inputs) without
    redirect targets, against Material.hs and Ray.hs:180-224 in long double from philox_ref of the same
    counter.  The branch taken (emit / absorb, reflect or refract, metal absorbed, front or back face)
    equals the reference's unless a decision's margin is within 64 eps scale (at most 0.5 %; the share of
    grazing rays whose face is open in FP32 is what the inputs are sized for); nd within K eps S_nd and unit
    within 8 eps; Tf within K eps |Tf| S_tf (S_tf: 1 / (mu0 + mu1) for Lommel-Seeliger, 1 / base for
    Henyey-Greenstein, 1 / pdf's terms with targets); L is L + T tex for a light and the same bits
    otherwise; np = o + t d and ngid = the record's gid.  Measured (profiles/probe/shading_probe.jsonl): skipped
    0.20 - 0.29 % in FP32 (the grazing rays' face), none in binary64; nd: plain formula 0.7 - 4.8 eps S (K = 8 .. 64),
    emulator the same, MI355X 0.3 - 1.5; Tf: plain formula 0 - 0.77 (K = 4 or 8), emulator 0 - 0.77, MI355X 0 - 1.25;
    | |nd| - 1 | at most 4.8 eps (transparent: the input's own) on both."""
    I = shade_inputs(precision, kind, 900 + kind)
    T = make_targets(precision, TARGET_SETS[0])
    outs = run_shade(backend, precision, 1, I, T)
    R, use = check_shade(backend, precision, f"kind{kind}", I, T, outs)
    if kind in (M.LIGHT, M.BLACK):
        assert R["term"].all()
    if kind == M.TRANSPARENT:
        assert same_bits(outs[3], I["ray"][:, 3:6]).all()
    if kind in (M.MIRROR, M.METAL, M.TRANSPARENT):
        go = use & ~R["term"]
        assert same_bits(outs[4][go], I["mats"]["c0"][go]).all()
    if kind == M.DIELECTRIC:
        assert (outs[4] == 1).all()
    if kind == M.METAL:
        assert 0.02 < R["term"].mean() < 0.5  # fuzz sends some directions below the surface


@backends
@both_precisions
@pytest.mark.parametrize("n_targets", [1, 2])
@pytest.mark.parametrize("kind", [M.LAMBERT, M.LOMMEL, M.ISOTROPIC, M.ANISOTROPIC])
def test_mixture_scatter_with_targets(backend, precision, kind, n_targets):
    """mixture_scatter (through shade_event<2, true, false>) with one and with two redirect targets
    (probabilities 0.25 and 0.5, built as Ray.hs:138-151 states them) on 2^14 hits per HemisphereF / SphereF
    material: the target follows cr < thresh, the direction is the target point's or the default
    sampler's, a HemisphereF direction below the surface ends the path, and the pdf is rem_prob pdf1 + sum
    p t^2 / |cross . dir| over every target the new ray actually hits (Ray.hs:199-204), each hit decided as
    target_hit does (undecided within 64 eps scale of an edge, of t = 0: at most 0.5 %)."""
    I = shade_inputs(precision, kind, 950 + 10 * kind + n_targets)
    T = make_targets(precision, TARGET_SETS[n_targets])
    outs = run_shade(backend, precision, 1, I, T)
    R, use = check_shade(backend, precision, f"kind{kind}_targets{n_targets}", I, T, outs)
    cr = u01_of(philox_words(I["ctr"])[:, 0], np.float64)
    chosen = cr < float(T["thresh"][-1])
    assert 0.1 < chosen.mean() < 0.9
    if kind in (M.LAMBERT, M.LOMMEL):
        assert 0.05 < R["term"][chosen].mean() < 0.95  # some targets lie below the surface
    else:
        assert not R["term"].any()
    # the mixture pdf matters: where a target is hit, Tf is not the no-target value
    R0 = shade_reference(I, make_targets(precision, []), 1.0, LD)
    go = use & ~R["term"] & ~R0["term"] & chosen
    moved = np.abs((R["Tf"] - R0["Tf"]).astype(np.float64)).max(1)[go] > 1e-3
    assert moved.mean() > 0.5


def constructed_hits(precision, kind, param, n_rec, d, ctr, n=None):
    """Hits at the origin (o = -t d, t = 1) on records with normal n_rec for one material."""
    real = real_of(precision)
    d = np.atleast_2d(np.asarray(d, np.float64))
    n = len(d)
    I = shade_inputs(precision, kind, 1, n=max(n, 1))
    I["prims"][:, 0:3] = np.broadcast_to(np.asarray(n_rec, np.float64), (n, 3)).astype(real)
    I["ray"] = np.concatenate([-d, d, np.ones((n, 1))], 1).astype(real)
    I["mats"]["param"] = param
    I["ctr"] = np.broadcast_to(np.asarray(ctr, np.uint32), (n, 3)).copy()
    return I


# Philox counters (pix, sample, seg = 0) under KEY whose first scatter word w.x has u01(w.x) = k 2^-24 on a
# constructed threshold (found by a search of 2^25 counters; the test checks each with philox_ref)
COUNTERS = {"u=1/4": ((7134146, 0, 0), 1 << 22), "u=1/4-": ((9824534, 0, 0), (1 << 22) - 1),
            "u=3/4": ((14767549, 0, 0), 3 << 22), "u=3/4-": ((14054896, 0, 0), (3 << 22) - 1),
            "r1.5-": ((3816093, 0, 0), None), "r1.5+": ((1531227, 0, 0), None)}


def counter_u(name):
    ctr = np.array([COUNTERS[name][0]], np.uint32)
    k = int(philox_words(ctr)[0, 0]) >> 8
    assert COUNTERS[name][1] in (None, k), (name, k)
    return ctr[0], k


@backends
@both_precisions
def test_dielectric_constructed_cases(backend, precision):
    """ior = 1: the refracted direction is the incoming one within K eps (K = 16: refract's five roundings per
    component and the renormalisation, times 8 / 2).  The critical angle: on a back face, with cos_t = c a
    float whose 1 - c c rounds the same with and without FMA and ior the float with fl(ior sin_t) = 1
    exactly, `> 1` is false and the ray refracts (along the surface); a few floats of c towards grazing,
    where fl(ior sin_t) > 1, it reflects (asserted in binary64, whose square root is IEEE on both backends;
    in FP32 the direction must be one of the two).  Binary64: u01(w.x) one step (2^-24) below and at-or-above the reflectance r0 at normal
    incidence for ior = 1.5 reflects and refracts (counters found by search; in FP32 a step of u is inside
    the 64 eps band)."""
    real, eps = real_of(precision), eps_of(precision)
    T = make_targets(precision, [])
    rng = np.random.default_rng(990)
    # ior = 1
    nrm = random_units(rng, 256)
    tang = np.cross(nrm, random_units(rng, 256))
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    cos = rng.uniform(0.3, 1.0, 256)
    d = -cos[:, None] * nrm + np.sqrt(1 - cos * cos)[:, None] * tang
    I = constructed_hits(precision, M.DIELECTRIC, 1.0, nrm, d, (5, 6, 7))
    I["ctr"][:, 0] = np.arange(256)
    term, Lo, np_, nd, Tf, ngid = run_shade(backend, precision, 1, I, T)
    u = u01_of(philox_words(I["ctr"])[:, 0], np.float64)
    refract = u >= (1 - cos) ** 5 + 1e-3
    assert refract.sum() > 100 and not term.any()
    dev = float((np.abs(nd.astype(LD) - I["ray"][:, 3:6].astype(LD)).max(1)[refract] / eps).max())
    measure(backend, f"dielectric_ior1_{precision}", n=int(refract.sum()), worst_dev_in_eps=dev)
    assert dev <= 16.0
    # the critical angle from inside (ratio = ior): a float c = cos_t whose 1 - c c is the same float with and
    # without FMA contraction, sin_t = its correctly rounded square root, and ior the float with
    # fl(ior sin_t) = 1 exactly; a second c a few floats towards grazing with fl(ior sin_t) > 1 both ways
    def sin_of(cand):
        two_step = real(1) - real(cand * cand)
        fused = real(float(1 - Fraction(float(cand)) ** 2))
        return np.sqrt(two_step) if two_step == fused else None
    def product(ior, s_):
        return real(float(Fraction(float(ior)) * Fraction(float(s_))))
    found = None
    cand = real(0.8)
    for _ in range(4096):
        cand = np.nextafter(cand, real(0))
        s_ = sin_of(cand)
        if s_ is None:
            continue
        for ior in (real(1) / s_, np.nextafter(real(1) / s_, real(0)), np.nextafter(real(1) / s_, real(4))):
            if product(ior, s_) == 1:
                beyond = cand
                for _ in range(16):
                    beyond = np.nextafter(beyond, real(0))
                    s2 = sin_of(beyond)
                    if s2 is not None and product(ior, s2) > 1:
                        found = (cand, beyond, ior)
                        break
            if found:
                break
        if found:
            break
    assert found is not None
    cs = np.array(found[:2], real)
    ior_c = float(found[2])
    sx = np.sqrt(1 - cs.astype(np.float64) ** 2)
    d = np.stack([sx, np.zeros(2), cs.astype(np.float64)], 1)  # back face: n . d = c > 0, h.n = -n, cos_t = c exactly
    ctr, k = counter_u("u=3/4")  # u = 0.75: far above the reflectance there
    I = constructed_hits(precision, M.DIELECTRIC, ior_c, (0.0, 0.0, 1.0), d, ctr)
    I["ray"][:, 3:6] = d.astype(real)
    I["ray"][:, 5] = cs
    term, Lo, np_, nd, Tf, ngid = run_shade(backend, precision, 1, I, T)
    assert not term.any()
    refracted = (np.abs(nd[:, 2]) <= 64 * math.sqrt(eps)) & (nd[:, 0] > 0.99)  # along the surface
    reflected = nd[:, 2] < -0.5 * cs
    assert (refracted != reflected).all(), nd
    if precision == "f64":  # sqrt is the IEEE one on both backends (test_device_probe.py): every step is pinned
        assert refracted[0] and reflected[1], nd
    if precision == "f64":
        for name, want_reflect in (("r1.5-", True), ("r1.5+", False)):
            ctr, k = counter_u(name)
            ratio = 1.0 / 1.5
            r0 = ((1 - ratio) / (1 + ratio)) ** 2
            assert (k * 2.0 ** -24 < r0) == want_reflect and abs(k * 2.0 ** -24 - r0) <= 2.0 ** -24
            I = constructed_hits(precision, M.DIELECTRIC, 1.5, (0.0, 0.0, 1.0), [(0.0, 0.0, -1.0)], ctr)
            term, Lo, np_, nd, Tf, ngid = run_shade(backend, precision, 1, I, T)
            assert not term.any() and (nd[0, 2] > 0.99) == want_reflect, (name, nd[0])


@backends
@both_precisions
def test_metal_without_fuzz_is_the_mirror(backend, precision):
    """metal 0 (Material.hs:72-78) scatters where the mirror does, in the mirror's direction within 4 eps (the
    two normalise differently: linear's normalize leaves a vector within 1e-12 of unit alone), with the same Tf."""
    eps = eps_of(precision)
    T = make_targets(precision, [])
    Im = shade_inputs(precision, M.MIRROR, 991, n=4096)
    Ime = dict(Im)
    Ime["mats"] = Im["mats"].copy()
    Ime["mats"]["kind"], Ime["mats"]["param"] = M.METAL, 0.0
    a = run_shade(backend, precision, 1, Im, T)
    b = run_shade(backend, precision, 1, Ime, T)
    assert not a[0].any() and not b[0].any()
    assert float(np.abs(a[3].astype(LD) - b[3].astype(LD)).max() / eps) <= 4.0
    assert same_bits(a[4], b[4]).all()


@backends
@both_precisions
def test_target_choice_on_the_thresholds(backend, precision):
    """The choice of target follows cr < thresh strictly (Ray.hs:151 drops thresholds with r >= them): with
    thresholds 1/4 and 3/4, cr = 1/4 - 2^-24 picks target 0, cr = 1/4 and 3/4 - 2^-24 target 1, cr = 3/4 the default
    sampler (isotropic: the direction tells which)."""
    T = make_targets(precision, TARGET_SETS[2])
    assert float(T["thresh"][0]) == 0.25 and float(T["thresh"][1]) == 0.75
    for name, want in (("u=1/4-", 0), ("u=1/4", 1), ("u=3/4-", 1), ("u=3/4", -1)):
        ctr, k = counter_u(name)
        I = constructed_hits(precision, M.ISOTROPIC, 0.0, (0.0, 0.0, 1.0), [(0.0, 0.0, -1.0)], ctr)
        R = shade_reference(I, T, 0.25, LD)
        term, Lo, np_, nd, Tf, ngid = run_shade(backend, precision, 1, I, T)
        w = philox_words(I["ctr"])
        for j in range(2):  # the direction towards target j's sampled point
            lp = T[j]["q"].astype(LD) + u01_of(w[:, 1], LD)[:, None] * T[j]["u"].astype(LD) + u01_of(w[:, 2], LD)[:, None] * T[j]["v"].astype(LD)
            to_j = normalize_ref(lp - R["p"])
            near = float(np.abs(nd.astype(LD) - to_j).max()) < 1e-5
            assert near == (want == j), (name, j, nd, to_j)
        assert float(np.abs(nd.astype(LD) - R["nd"]).max()) < 1e-5 and not term.any()


@backends
@both_precisions
def test_medium_hits_misses_and_the_two_forms(backend, precision):
    """A medium hit (n = -d, gid = -1) with the isotropic and the anisotropic material (g = -0.9, 0.9) of
    KernelParams::media[0]; a miss adds T times the background, constant or the sky lerp of Ray.hs:179 (camera's
    `sky`: a = (d.y + 1) / 2); and shade_event<0, false, false>, the form compiled for scenes with only lights,
    black and lambertian surfaces, returns the same terminate, L, np and ngid for kinds 0, 1, 2 as
    shade_event<2, true, false>, with and without a target (nd and Tf: the next test)."""
    real, eps = real_of(precision), eps_of(precision)
    T0 = make_targets(precision, [])
    for kind, g in ((M.ISOTROPIC, 0.0), (M.ANISOTROPIC, -0.9), (M.ANISOTROPIC, 0.9)):
        I = shade_inputs(precision, kind, 992, n=4096)
        I["mats"]["param"] = g
        I["how"][:] = 1
        outs = run_shade(backend, precision, 1, I, T0, med_mat=7)
        I["mats"][:] = I["mats"][7]  # (every element reads material record media[0].material = 7)
        R, use = check_shade(backend, precision, f"medium_kind{kind}_g{g}", I, T0, outs)
        assert (outs[5] == -1).all() and not R["term"].any()
    # misses
    I = shade_inputs(precision, M.LAMBERT, 993, n=4096)
    I["how"][:] = 2
    L, Tp, d = I["LT"][:, 0:3].astype(LD), I["LT"][:, 3:6].astype(LD), I["ray"][:, 3:6].astype(LD)
    for bg_kind in (0, 1):
        term, Lo, np_, nd, Tf, ngid = run_shade(backend, precision, 1, I, T0, bg_kind=bg_kind)
        a = LD(0.5) * (d[:, 1] + 1)
        bg = np.tile(np.array(BG0, LD), (4096, 1))
        if bg_kind:
            bg = (1 - a)[:, None] * bg + a[:, None] * np.array(BG1, real).astype(LD)
        want = L + Tp * bg
        room = 4 * eps * (np.abs(L) + np.abs(Tp * bg)).astype(np.float64)
        assert term.all() and (np.abs(Lo.astype(LD) - want) <= room).all()
    # the two compiled forms: the decisions and the radiance
    for n_targets in (0, 1):
        T = make_targets(precision, TARGET_SETS[n_targets])
        for kind in (M.LIGHT, M.BLACK, M.LAMBERT):
            I = shade_inputs(precision, kind, 994 + kind, n=4096)
            full = run_shade(backend, precision, 1, I, T)
            lean = run_shade(backend, precision, 0, I, T)
            assert (full[0] == lean[0]).all() and same_bits(full[1], lean[1]).all()
            go = full[0] == 0
            assert go.any() == (kind == M.LAMBERT)
            assert same_bits(full[2][go], lean[2][go]).all() and (full[5][go] == lean[5][go]).all()


@backends
@both_precisions
def test_lambertian_forms_agree_bit_for_bit(backend, precision):
    """For lambertian hits shade_event<0, false, false> returns the same nd and Tf, bit for bit, as
    shade_event<2, true, false>, with and without a target.  This test found the two forms apart on the
    MI355X (23 % of the components, by up to 1478 units in the last place of a near-zero component in FP32
    and 752 in binary64), for two reasons, both the compiler's choice per instantiation: unit_vector's
    products were fused into the sum h.n + uu in one form and not in the other, and of x x + y y + z z in
    normalize another product stayed unfused (FP32: 7 % of the components, up to 2 ulp).  rt_trace.h now
    states both as fixed fused chains (normal_plus_unit_vector, normalize_fused) in every form of the
    scatter.  Measured since (profiles/probe/shading_probe.jsonl, probe lambertian_forms_*): 0 ulp on the
    emulator and on the MI355X."""
    worst, share = 0, 0.0
    for n_targets in (0, 1):
        T = make_targets(precision, TARGET_SETS[n_targets])
        I = shade_inputs(precision, M.LAMBERT, 996, n=4096)
        full = run_shade(backend, precision, 1, I, T)
        lean = run_shade(backend, precision, 0, I, T)
        go = (full[0] == 0) & (lean[0] == 0)
        for k in (3, 4):
            d = ulp_distance(full[k][go].reshape(-1), lean[k][go].reshape(-1))
            worst, share = max(worst, int(d.max())), max(share, float((d != 0).mean()))
    measure(backend, f"lambertian_forms_{precision}", worst_ulp=worst, share_differing=share)
    assert worst == 0, (worst, share)
