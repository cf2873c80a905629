"""A film's first-hit feature buffers and its variance-guided denoiser (include/rt.h rt_denoise_*).

    film = Film(world, settings, seed)
    film.add(4); film.add(4)
    preview = film.denoised()          # the 8-spp image, filtered; film.image() is still the raw one
    guides = film.features()           # albedo, normal, depth, coverage of the primary rays

The filter (raytrace_amd/csrc/rt_denoise.h, DESIGN.md "Denoiser") divides the mean colour by the
first-hit albedo, runs `levels` passes of a 5 x 5 a-trous kernel whose taps are weighted by normal,
depth, albedo and — in units of the film's own variance estimate — luminance similarity, and multiplies by
the albedo again.  It is written in binary64 with + - x / sqrt, min / max and comparisons only, in
one fixed order, so `denoise_reference` below gives the device's result bit for bit.

`emitter_twin(world)` is the scene whose render IS the albedo buffer: the same geometry with every
material replaced by a light source of its albedo texture.
"""
from __future__ import annotations

import copy
import ctypes

import numpy as np

from . import _lib
from . import geometry as G
from . import material as M

# the shipped parameters (rt_denoise.h rt_dn_defaults; profiles/denoise/README.md was measured with them)
DEFAULT_PARAMS = dict(levels=5, k=5, sigma_z=0.1, sigma_l=4.0, sigma_a=0.1, eps_n=1e-6, eps_z=1e-6, eps_l=1e-10)
ALBEDO_FLOOR = 1.0 / 256.0
FEATURE_WORDS = 8  # per pixel: albedo RGB, normal xyz, depth sum (units of 2^-32), hit count; binary64: low words follow
_KERNEL = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


def resolve_params(params=None, **kw) -> dict:
    """DEFAULT_PARAMS overridden by `params` and keywords; unknown names raise."""
    p = dict(DEFAULT_PARAMS)
    for k, v in {**(params or {}), **kw}.items():
        if k not in p:
            raise TypeError(f"unknown denoise parameter {k!r} (known: {sorted(p)})")
        p[k] = type(p[k])(v)
    return p


def params_struct(params=None, **kw) -> "_lib.RtDenoiseParams":
    p = resolve_params(params, **kw)
    return _lib.RtDenoiseParams(**p)


def features_from_words(words: np.ndarray, n_feat: int) -> dict:
    """The feature buffers from the device's integer words, (rows, width, 8) of an FP32 film or
    (rows, width, 16) of a binary64 one (8 high words, then their low words), by the arithmetic of
    rt_denoise.h rt_dn_prepare: a sum = (high + low 2^-32) 2^-32; albedo and normal = sum / n_feat,
    depth = depth sum / hits (0 without hits), coverage = hits / n_feat."""
    w = np.asarray(words, np.int64)
    n = float(n_feat)
    lo = w[..., 8:15].astype(np.uint64).astype(np.float64) if w.shape[-1] == 2 * FEATURE_WORDS else 0.0
    sums = (w[..., :7].astype(np.float64) + lo * 2.0 ** -32) * 2.0 ** -32
    hits = w[..., 7].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(hits > 0, sums[..., 6] / hits, 0.0)
    return dict(albedo=sums[..., 0:3] / n, normal=sums[..., 3:6] / n, depth=depth, coverage=hits / n)


def film_inputs(state: np.ndarray) -> tuple:
    """(mean, variance, flags) of a saved film state as the denoiser reads them: the mean colour
    c = (high word + low word 2^-32) 2^-32 / N (the image's own mean; an FP32 film has no low words)
    and the variance of the mean of R + G + B from the high words, rt_film_variance(q, T, N, K) / N
    2^-64 (radiance units squared).  Needs two passes."""
    from .film import unpack_state
    u = unpack_state(state)
    N, K = float(u["header"]["samples"]), int(u["header"]["passes"])
    if K < 2:
        raise ValueError("the denoiser's variance needs two passes")
    hi = u["sums"][..., :3]
    lo = u["sums"][..., 3:6].astype(np.uint64).astype(np.float64) if u["sums"].shape[-1] == 6 else 0.0
    mean = (hi.astype(np.float64) + lo * 2.0 ** -32) * 2.0 ** -32 / N
    T = hi.sum(-1, dtype=np.int64).astype(np.float64)
    d = u["q"] - (T * T) / N
    var = np.where(d > 0.0, d, 0.0) / float(K - 1)
    return mean, var / N * 2.0 ** -64, u["flags"]


def _max(a, b):
    return np.where(a > b, a, b)  # (rt_denoise.h rt_dn_max)


def _shift(arr, dy, dx, fill):
    """out[y, x] = arr[y + dy, x + dx], `fill` outside the frame."""
    H, W = arr.shape[:2]
    out = np.full_like(arr, fill)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = arr[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def _level(e, v, ok, nrm, nn, z, cov, ap, step, P):
    """One a-trous level: rt_denoise.h rt_dn_filter on every pixel at once, tap by tap in its order."""
    gs, gw = np.zeros_like(v), np.zeros_like(v)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            k = float((2 - abs(dx)) * (2 - abs(dy)))
            okq = _shift(ok, dy, dx, False)
            gs = gs + np.where(okq, k * _shift(v, dy, dx, 0.0), 0.0)
            gw = gw + np.where(okq, k, 0.0)
    lden = (P["sigma_l"] * P["sigma_l"]) * (gs / gw) + P["eps_l"]
    lp = (e[..., 0] + e[..., 1]) + e[..., 2]
    fp, cp = nn < P["eps_n"], cov > 0.0
    sw, sv, se = np.zeros_like(v), np.zeros_like(v), np.zeros_like(e)
    for dy in (-2, -1, 0, 1, 2):
        for dx in (-2, -1, 0, 1, 2):
            sy, sx = dy * step, dx * step
            okq = _shift(ok, sy, sx, False)
            eq, vq = _shift(e, sy, sx, 0.0), _shift(v, sy, sx, 0.0)
            nq, nnq = _shift(nrm, sy, sx, 0.0), _shift(nn, sy, sx, 0.0)
            zq, covq = _shift(z, sy, sx, 0.0), _shift(cov, sy, sx, 0.0)
            aq = _shift(ap, sy, sx, 1.0)
            fq, cq = nnq < P["eps_n"], covq > 0.0
            d = (nrm[..., 0] * nq[..., 0] + nrm[..., 1] * nq[..., 1]) + nrm[..., 2] * nq[..., 2]
            wn = _max(0.0, d) / _max(np.sqrt(nn * nnq), P["eps_n"])
            for _ in range(P["k"]):
                wn = wn * wn
            wn = np.where(fp & fq, 1.0, np.where(fp | fq, 0.0, wn))
            dz = np.where(z > zq, z - zq, zq - z)
            r = dz / (P["sigma_z"] * _max(_max(z, zq), P["eps_z"]))
            wz = np.where(~cp & ~cq, 1.0, np.where(~cp | ~cq, 0.0, 1.0 / (1.0 + r * r)))
            ra = (ap - aq) / _max(ap, aq)
            wa = 1.0 / (1.0 + ((ra[..., 0] * ra[..., 0] + ra[..., 1] * ra[..., 1]) + ra[..., 2] * ra[..., 2])
                        / (P["sigma_a"] * P["sigma_a"]))
            dl = lp - ((eq[..., 0] + eq[..., 1]) + eq[..., 2])
            wl = 1.0 / (1.0 + dl * dl / lden)
            w = (((_KERNEL[dx + 2] * _KERNEL[dy + 2] * wn) * wz) * wa) * wl
            sw = sw + np.where(okq, w, 0.0)
            se = se + np.where(okq[..., None], w[..., None] * eq, 0.0)
            sv = sv + np.where(okq, (w * w) * vq, 0.0)
    return se / sw[..., None], sv / (sw * sw)


def denoise_reference(mean, variance, flags, features, params=None) -> np.ndarray:
    """The denoiser in numpy, operation for operation as the device runs it (rt_denoise.h).

    mean (H, W, 3), variance (H, W), flags (H, W): `film_inputs(film.state())`; features:
    `film.features(n)`, with the remodulation albedo `film.albedo(m)` under "albedo_out" if the film
    has one; params: a dict over DEFAULT_PARAMS.  Returns (H, W, 3) float64 — the bits
    of `film.denoised()` for a binary64 film, and of it before its one rounding for an FP32 film;
    NaN where a pixel is flagged."""
    P = resolve_params(params)
    if not 1 <= P["levels"] <= 8 or not 0 <= P["k"] <= 16:
        raise ValueError("levels must be 1..8 and k 0..16")
    mean = np.asarray(mean, np.float64)
    a = np.asarray(features["albedo"], np.float64)
    nrm = np.asarray(features["normal"], np.float64)
    z = np.asarray(features["depth"], np.float64)
    cov = np.asarray(features["coverage"], np.float64)
    bad = np.asarray(flags) != 0
    ok = ~bad
    with np.errstate(all="ignore"):
        ap = _max(a, ALBEDO_FLOOR)
        e = mean / ap
        m = _max(((a[..., 0] + a[..., 1]) + a[..., 2]) / 3.0, ALBEDO_FLOOR)
        v = np.asarray(variance, np.float64) / (m * m)
        nn = (nrm[..., 0] * nrm[..., 0] + nrm[..., 1] * nrm[..., 1]) + nrm[..., 2] * nrm[..., 2]
        for i in range(P["levels"]):
            e2, v2 = _level(e, v, ok, nrm, nn, z, cov, ap, 1 << i, P)
            e, v = np.where(bad[..., None], e, e2), np.where(bad, v, v2)
        b = features.get("albedo_out")  # the remodulation albedo (Film.albedo), if any
        out = e * (ap if b is None else _max(np.asarray(b, np.float64), ALBEDO_FLOOR))
    out[bad] = np.nan
    return out


def emitter_twin(world: G.Geometry) -> G.Geometry:
    """The same geometry with every material replaced by lightSource(<its albedo texture>): the
    material's own texture, constant 1 for dielectric, constant 0 for pitchBlack.  One sample of the
    twin returns what the feature pass calls the albedo of that sample's first hit (a medium's phase
    material included; a miss returns the background in both)."""
    memo: dict = {}

    def albedo(mat: M.Material) -> M.Material:
        if mat.kind == M.DIELECTRIC:
            return M.lightSource(M.constantTexture(1.0))
        if mat.kind == M.BLACK:
            return M.lightSource(M.constantTexture(0.0))
        return M.lightSource(mat.texture)

    def twin(node):
        key = id(node)
        if key in memo:
            return memo[key]
        if isinstance(node, (G.Sphere, G.PlaneShape)):
            out = node  # (leaves carry no material; the same objects keep the scene's leaf identities)
        else:
            out = copy.copy(node)
            if isinstance(node, G.WithMaterial):
                out.material = albedo(node.material)
                out.child = twin(node.child)
            elif isinstance(node, G.Group):
                out.children = [twin(c) for c in node.children]
            elif isinstance(node, G.BvhNode):
                out.left, out.right = twin(node.left), twin(node.right)
            elif isinstance(node, (G.Transform, G.Moving, G.ConstantMedium)):
                out.child = twin(node.child)
            else:
                raise TypeError(f"emitter_twin: geometry node {type(node).__name__}")
        memo[key] = out
        return out

    return twin(world)
