"""The film's first-hit features and denoiser on the GPU (include/rt.h rt_denoise_*, raytrace_amd.denoise).

Features: the device's albedo against the FP64 oracle's render of the emitter twin and its normals,
depth and coverage against the host build of the same body (tests/feature_emu), under
tests/test_gpu.py's per-precision bars for small renders; analytic scenes; determinism.  Filter: the
device's output against the numpy twin bit for bit, an exact-identity case, the error against a
4096-spp render, and the error returns.
"""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, record_measure

pytestmark = pytest.mark.gpu

import raytrace_amd as R  # noqa: E402
from raytrace_amd import _lib, denoise, film, scenes  # noqa: E402
from raytrace_amd.camera import camera_basis  # noqa: E402
from raytrace_amd.errors import RtInvalid, RtUnsupported  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests", "feature_emu"))

N_FEAT = 4
FEATURE_SCENES = {"cornell_box": 48, "box_gallery": 40, "noise_test": 40, "instance_gallery": 40, "bunny_cornell": 40,
                  "pawn_fog": 40}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    return torch


@functools.lru_cache(maxsize=None)
def scene(name):
    cs, world, seed = getattr(scenes, name)(width=FEATURE_SCENES[name], spp=N_FEAT)
    return cs, world, seed


@functools.lru_cache(maxsize=None)
def oracle_albedo(name):
    """The reference of the albedo tests: the oracle's Philox render of the emitter twin (once)."""
    import oracle
    oracle.build()
    cs, world, seed = scene(name)
    ref = oracle.render(cs, denoise.emitter_twin(world), seed, mode=oracle.RNG_PHILOX)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def host_features(name):
    """The binary64 host build's features of a scene (once)."""
    import feature_emu
    cs, world, seed = scene(name)
    return denoise.features_from_words(feature_emu.features(cs, world, seed, N_FEAT, precision="f64"), N_FEAT)


@functools.lru_cache(maxsize=None)
def device_features(name, precision):
    cs, world, seed = scene(name)
    with R.Film(world, cs, seed, precision=precision) as f:
        return f.features(N_FEAT)


def assert_bars(x, ref, precision, what, spp, lmax, need32=0.99, mean=True):
    """tests/test_gpu.py assert_parity's per-pixel, worst-pixel and mean bars (its numbers; x and ref
    are (H, W, C) binary64): f64 >= 99.9 % of pixels within 1e-9 relative on the max(|ref|, 1e-3)
    scale and the worst within 2 L / spp; f32 >= need32 within 1e-3 (relative above 1) and the worst
    within 4 L / spp + 1e-3; the channel means within 5e-3."""
    assert x.shape == ref.shape and np.isfinite(x).all(), what
    d = np.abs(x - ref)
    if precision == "f64":
        frac = float(((d / np.maximum(np.abs(ref), 1e-3)).max(-1) <= 1e-9).mean())
        print(what, precision, "fraction within 1e-9:", frac, "worst:", float(d.max()))
        assert frac >= 0.999, (what, frac)
        assert d.max() <= 2 * lmax / spp, (what, float(d.max()))
    else:
        frac = float(((d / np.maximum(np.abs(ref), 1.0)).max(-1) < 1e-3).mean())
        print(what, precision, "fraction within 1e-3:", frac, "worst:", float(d.max()))
        assert frac >= need32, (what, frac)
        assert d.max() <= 4 * lmax / spp + 1e-3, (what, float(d.max()))
    if mean:
        np.testing.assert_allclose(x.reshape(-1, x.shape[-1]).mean(0), ref.reshape(-1, x.shape[-1]).mean(0), rtol=5e-3,
                                   atol=1e-6)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", list(FEATURE_SCENES))
def test_device_albedo_matches_oracle_emitter_twin(gpu, name, precision):
    """Flat, box-group, noise-texture, instanced, triangle-BVH and media classes at 40-48 px, n_feat 4:
    the device's albedo is the oracle's 4-spp render of the emitter twin (for pawn_fog the oracle
    renders the fog's phase material as a light source like any other).  L: the largest value one
    sample can take, the largest albedo in the reference."""
    ref = oracle_albedo(name)
    got = device_features(name, precision)["albedo"]
    assert_bars(got, ref, precision, name, N_FEAT, max(1.0, float(ref.max())))


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", list(FEATURE_SCENES))
def test_device_guides_match_host_build(gpu, name, precision):
    """Normals, depth and coverage of the device against the binary64 host build of the same body
    under the same bars (L: 1 for a unit normal and for the coverage, the largest depth for the
    depth).  The channel-mean bar is the albedo test's: a normal's mean is a difference of large
    terms, which a relative bar does not fit."""
    ref, got = host_features(name), device_features(name, precision)
    assert_bars(got["normal"], ref["normal"], precision, name + " normal", N_FEAT, 1.0, mean=False)
    zmax = float(ref["depth"].max())
    scale = max(zmax, 1.0)  # (the bars' floors are absolute: depths in units of the largest one)
    assert_bars(got["depth"][..., None] / scale, ref["depth"][..., None] / scale, precision, name + " depth", N_FEAT, 1.0,
                mean=False)
    assert_bars(got["coverage"][..., None], ref["coverage"][..., None], precision, name + " coverage", N_FEAT, 1.0,
                mean=False)
    if precision == "f64":  # the same arithmetic: identical but for the device's own division and square root
        for k in ("albedo", "normal", "depth", "coverage"):
            assert (np.abs(got[k] - ref[k]) <= 1e-9 * np.maximum(np.abs(ref[k]), 1e-3)).mean() >= 0.999, k


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_analytic_quad_sphere_and_empty_scene(gpu, precision):
    white = R.lambertian(R.constantTexture(0.5))
    # a view-filling quad facing the camera: normal exactly +-(0, 0, 1), coverage 1, depth >= 1
    cs = R.defaultCameraSettings(cs_imageWidth=19, cs_aspectRatio=19 / 11, cs_samplesPerPixel=1, cs_vfov=np.pi / 3)
    quad = white << R.parallelogram((-8.0, -8.0, -1.0), (16.0, 0.0, 0.0), (0.0, 16.0, 0.0))
    with R.Film(quad, cs, 3, precision=precision) as f:
        g = f.features(N_FEAT)
    assert g["normal"].shape == (11, 19, 3) and (g["coverage"] == 1.0).all()
    assert (g["normal"][..., :2] == 0.0).all() and (np.abs(g["normal"][..., 2]) == 1.0).all()
    assert (g["albedo"] == 0.5).all() and (g["depth"] >= 1.0 - 1e-6).all()
    # the camera at the centre of a sphere, no defocus: depth = r, normal = -(ray direction)
    r = 2.5
    cs = R.defaultCameraSettings(cs_imageWidth=21, cs_aspectRatio=21 / 13, cs_samplesPerPixel=1, cs_vfov=np.pi / 2,
                                 cs_center=(0.25, -0.5, 1.0), cs_lookAt=(0.25, -0.5, 0.0))
    with R.Film(white << R.sphere((0.25, -0.5, 1.0), r), cs, 5, precision=precision) as f:
        g = f.features(N_FEAT)
    # binary64: 1e-9 relative.  FP32: t = h + sqrt(r^2 - |l|^2) with h ~ 0, |l| ~ 0 in a few FP32
    # roundings (2^-24 each), summed over 4 samples in units of 2^-32: 8 x 2^-24 relative
    tol = 1e-9 if precision == "f64" else 8 * 2.0 ** -24
    assert (g["coverage"] == 1.0).all() and (np.abs(g["depth"] - r) <= tol * r).all(), float(np.abs(g["depth"] - r).max())
    b = camera_basis(cs)
    yy, xx = np.mgrid[0:b.height, 0:b.width]
    d = (np.array(b.top_left) + (xx[..., None] + 0.5) * np.array(b.pixel_u) + (yy[..., None] + 0.5) * np.array(b.pixel_v)
         - np.array(b.center))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    n = g["normal"] / np.linalg.norm(g["normal"], axis=-1, keepdims=True)
    angle = np.arccos(np.clip((n * -d).sum(-1), -1.0, 1.0))
    pixel_width = float(np.linalg.norm(b.pixel_u) / cs.cs_focusDist)  # the widest pixel's angle (image centre)
    assert (angle <= pixel_width).all(), (float(angle.max()), pixel_width)
    # nothing to hit: coverage 0, normal 0, depth 0, albedo = the background of each ray
    cs = R.defaultCameraSettings(cs_imageWidth=12, cs_aspectRatio=1.5, cs_samplesPerPixel=1, cs_background=R.sky)
    far = white << R.sphere((0.0, 0.0, 50.0), 1.0)  # behind the camera
    with R.Film(far, cs, 7, precision=precision) as f:
        g = f.features(N_FEAT)
        img = f.add(N_FEAT).image()
    assert (g["coverage"] == 0).all() and (g["normal"] == 0).all() and (g["depth"] == 0).all()
    # the same rays' background: equal to the fixed point (2^-32 per word), and to the float32 image's
    # own rounding (values <= 1: 2^-24) for an FP32 film
    np.testing.assert_allclose(g["albedo"], img, rtol=0, atol=2.0 ** -31 + (2.0 ** -24 if precision == "f32" else 0.0))


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", ["cornell_box", "pawn_fog"])
def test_features_are_deterministic_and_leave_the_film_alone(gpu, name, precision):
    cs, world, seed = scene(name)
    flat = R.flatten(world)
    with R.Film(flat, cs, seed, precision=precision) as a, R.Film(flat, cs, seed, precision=precision) as b:
        a.add(3), b.add(3)
        w1 = a.feature_words(8).copy()
        a._feature_samples = 0  # (run the pass again)
        assert np.array_equal(a.feature_words(8), w1)
        a.add(5), b.add(5)
        a.denoised()
        a._feature_samples = 0
        assert np.array_equal(a.feature_words(8), w1)  # features do not depend on the passes added
        assert np.array_equal(a.state(), b.state())  # byte-identical to a film that never denoised
        a.add(4), b.add(4)
        one = R.raytrace(cs.replace(cs_samplesPerPixel=12), flat, seed, precision=precision)
        assert np.array_equal(a.image(), one, equal_nan=True) and np.array_equal(b.image(), one, equal_nan=True)


def twin_of(f, n_feat, n_albedo, **params):
    mean, var, flags = denoise.film_inputs(f.state())
    feats = f.features(n_feat)
    if n_albedo:
        feats["albedo_out"] = f.albedo(n_albedo)
    return denoise.denoise_reference(mean, var, flags, feats, params)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("width,aspect,levels,n_albedo", [(48, 1.0, 5, 64), (37, 37 / 23, 5, 64), (9, 1.0, 5, 64),
                                                          (48, 1.0, 2, 0)],
                         ids=["48x48", "37x23", "9x9", "48x48-2levels-no-albedo"])
def test_device_filter_equals_numpy_twin_bitwise(gpu, precision, width, aspect, levels, n_albedo):
    """A real film (Cornell, passes 1 + 7 + 3): denoised() equals denoise_reference fed from
    unpack_state and features() bit for bit, rounded once to float32 for an FP32 film.  48 x 48 is
    one workgroup column short of a tile and several rows of tiles; 37 x 23 and 9 x 9 are smaller
    than a tile and (9 x 9) than the largest step; levels = 2 ends on the other ping-pong buffer,
    runs only the LDS kernels and multiplies by the features' own albedo (no remodulation albedo)."""
    cs, world, seed = scenes.cornell_box(width=width, spp=1)
    cs = cs.replace(cs_aspectRatio=aspect)
    with R.Film(world, cs, seed, precision=precision) as f:
        for n in (1, 7, 3):
            f.add(n)
        got = f.denoised(levels=levels, albedo_samples=n_albedo)
        want = twin_of(f, 8, n_albedo, levels=levels)
    assert got.dtype == f.dtype and got.shape == want.shape
    want = want.astype(got.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint64 if precision == "f64" else np.uint32),
                          want[ok].view(np.uint64 if precision == "f64" else np.uint32))


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_all_emitter_scene_is_left_unchanged(gpu, precision):
    """Every surface a light source, feature samples = the film's samples: the variance is zero and
    the colour IS the albedo (e = 1 exactly, every weight multiplies 1), so the output is the albedo
    it is multiplied by, within 4 ulp of the output type: image() itself when that is the features'
    albedo (albedo_samples = 0), and the 64-sample albedo by default — the same image with the edge
    pixels' coverage estimated from 64 primary rays instead of 8."""
    cs, world, seed = scenes.cornell_box(width=40, spp=1)
    with R.Film(denoise.emitter_twin(world), cs, seed, precision=precision) as f:
        f.add(4), f.add(4)
        img, dn = f.image(), f.denoised(feature_samples=8, albedo_samples=0)
        dn64, a64, a8 = f.denoised(feature_samples=8), f.albedo(64), f.features(8)["albedo"]
    assert np.isfinite(img).all()
    assert (np.abs(dn.astype(np.float64) - img.astype(np.float64)) <= 4 * np.spacing(np.abs(img))).all()
    lit = (a8 >= denoise.ALBEDO_FLOOR).all(-1)  # (below the floor e = c / floor is not 1)
    a64 = np.maximum(a64, denoise.ALBEDO_FLOOR).astype(img.dtype)
    assert lit.mean() > 0.9
    assert (np.abs(dn64.astype(np.float64) - a64.astype(np.float64)) <= 4 * np.spacing(np.abs(a64)))[lit].all()
    inner = np.abs(a64.astype(np.float64) - img) <= 4 * np.spacing(np.abs(img))  # pixels no edge crosses
    assert inner.all(-1).mean() > 0.8


def rmse(a, b):
    ok = np.isfinite(a).all(-1) & np.isfinite(b).all(-1)
    return float(np.sqrt(((a[ok].astype(np.float64) - b[ok]) ** 2).mean()))


QUALITY_BAR = 0.441  # the first run's rho, 0.3528, x 1.25 (below the cap 0.7 of the condition)


def test_denoised_error_against_a_converged_render(gpu):
    """Cornell at 96 px, film passes 4 + 4, against R.raytrace at 4096 spp: rho = RMSE(denoised) /
    RMSE(raw 8 spp) over finite pixels must be below 1 and at most 0.7; the asserted bar is the rho of
    the first MI355X run, 0.3528 (RMSE raw 0.1767, denoised 0.0623), x 1.25 for compiler-version
    jitter in the renders.  bunny_cornell at 80 px, recorded: 0.449 (profiles/denoise/README.md)."""
    cs, world, seed = scenes.cornell_box(width=96, spp=1)
    ref = R.raytrace(cs.replace(cs_samplesPerPixel=4096), world, seed, precision="f32").astype(np.float64)
    with R.Film(world, cs, seed, precision="f64") as f:
        f.add(4), f.add(4)
        raw, dn = f.image(), f.denoised()
    rho = rmse(dn, ref) / rmse(raw, ref)
    print("rho cornell 96 px:", rho, "rmse raw", rmse(raw, ref), "rmse denoised", rmse(dn, ref))
    record_measure("denoise_quality", dict(scene="cornell_box", width=96, rho=rho, rmse_raw=rmse(raw, ref),
                                           rmse_denoised=rmse(dn, ref)))
    assert rho < 1.0 and rho <= QUALITY_BAR, rho


def test_denoise_error_returns(gpu):
    cs, world, seed = scenes.cornell_box(width=16, spp=1)
    flat = R.flatten(world)
    with R.Film(flat, cs, seed) as f:
        f.add(8)
        with pytest.raises(RtInvalid):  # one pass only
            f.denoised()
        f.add(1)
        for levels in (0, 9):
            with pytest.raises(RtInvalid):
                f.denoised(levels=levels)
        with pytest.raises(RtInvalid):
            f.denoised(sigma_z=0.0)
        assert np.isfinite(f.denoised(levels=1)).all() and np.isfinite(f.denoised(levels=8)).all()
    with R.Film(flat, cs, seed) as f:  # features not computed: the C entry point refuses
        f.add(1), f.add(1)
        out = np.zeros(f.shape)
        rc = f._lib.rt_denoise_film_read(f.handle, None, out.ctypes.data)
        assert rc == _lib.RT_E_INVALID and b"features" in f._lib.rt_last_error()
    with R.Film(flat, cs, seed, n_shards=2, shard=1, row_block=2) as f:
        f.add(2), f.add(2)
        assert f.features(4)["albedo"].shape == f.shape  # a shard has features ...
        with pytest.raises(RtUnsupported):  # ... but no filter: its rows are interleaved
            f.denoised()
    img, info = R.raytrace_until(cs, flat, seed, noise=0.0, batch=4, max_spp=8, denoise=True)
    assert info["passes"] == 2 and info["raw"].shape == img.shape and not np.array_equal(img, info["raw"])
