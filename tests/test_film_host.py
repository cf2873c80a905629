"""The progressive film without a GPU: the kernel's item decode with a first-sample index, the
film's per-pixel arithmetic against its numpy restatement, the estimator's statistics, and the new
C-ABI entry points' argument checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raytrace_amd import _lib, film, scenes

CSRC = os.path.join(ROOT, "raytrace_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "film")
CXXFLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]


def compile_program(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    cmd = ["g++", *CXXFLAGS, "-o", exe, os.path.join(SRC, name + ".cpp"), *extra, "-lm", "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def within_ulps(a, b, ulps):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(np.abs(a - b) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b)))))


def test_items_cover_the_sample_range_once(tmp_path):
    """rt_trace.h open_item over every item id of rt_host_plan_work's plans, sample0 in {0, 1, 37} x
    spp in {1, 3, 17, 64}, one and two item sizes, whole images and shards with padding rows: each
    pixel's items cover [sample0, sample0 + spp) exactly once, padding rows get nothing."""
    exe = compile_program(tmp_path, "item_cover", [os.path.join(CSRC, "rt_build.cpp"), os.path.join(CSRC, "rt_bvh.cpp")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("RT_AMD_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-4000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) > 1000


def synthetic_passes(rng, sizes, n_pixels):
    """Integer pass sums as a render leaves them: per sample a non-negative radiance per channel,
    in the fixed-point unit 2^-32; dark, mid and bright pixels (some below the 3/256 floor)."""
    level = rng.choice([0.0, 1e-3, 0.05, 0.7, 15.0], size=(n_pixels, 1))
    sums = np.zeros((len(sizes), n_pixels, 3), np.int64)
    for k, n in enumerate(sizes):
        x = level[None] * rng.gamma(2.0, 0.5, size=(n, n_pixels, 3))
        sums[k] = np.floor(x * 2.0 ** 32).astype(np.int64).sum(0)
    return sums


@pytest.mark.parametrize("sizes", [[1, 7, 3, 16, 5], [4, 4], [1, 2, 3, 4, 5, 6, 7, 8], [300, 1, 25]])
def test_pixel_functions_match_noise_from_sums(tmp_path, sizes):
    """rt_film.h's q and r (the kernels' text, compiled for the host) against film.noise_from_sums
    on synthetic integer pass sums, K <= 8 passes of unequal sizes: the same operation sequence, so
    4 ulp (the slack covers contraction choices only)."""
    exe = compile_program(tmp_path, "pixel_math")
    rng = np.random.default_rng(len(sizes) * 1000 + sizes[0])
    n = 257
    sums = synthetic_passes(rng, sizes, n)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(sizes), n] + sizes, np.int64).tobytes())
        f.write(sums.tobytes())
    subprocess.run([exe, src, dst], check=True)
    q, v, r = np.fromfile(dst, np.float64).reshape(3, n)
    want = film.noise_from_sums(sums, sizes)
    assert np.isfinite(r).all() and (r >= 0).all() and (r > 0).any()
    assert within_ulps(q, want["q"], 4)
    assert within_ulps(r, want["r"], 4)
    assert within_ulps(v, want["v"], 4)


def test_batch_means_estimate_the_sample_variance():
    """noise_from_sums on normal samples, 4096 pixels, K = 8 batches of 1..8 samples: the mean of v
    lies within 5 standard errors of sigma^2; the estimator's own standard error is sigma^2
    sqrt(2 / ((K - 1) 4096)) (v (K - 1) / sigma^2 is chi-squared with K - 1 degrees of freedom)."""
    rng = np.random.default_rng(20240607)
    n_pix, sizes, mu, sigma = 4096, list(range(1, 9)), 2.0, 0.25
    sums = np.zeros((len(sizes), n_pix, 3), np.int64)
    for k, n in enumerate(sizes):
        x = rng.normal(mu, sigma, size=(n, n_pix))
        sums[k, :, 1] = np.rint(x * 2.0 ** 32).astype(np.int64).sum(0)  # (the luminance word adds R, G and B)
    est = film.noise_from_sums(sums, sizes)
    v = est["v"] * 2.0 ** -64
    K = len(sizes)
    bound = 5 * sigma ** 2 * np.sqrt(2.0 / ((K - 1) * n_pix))
    assert abs(v.mean() - sigma ** 2) <= bound, (v.mean(), sigma ** 2, bound)
    # and the mean and its standard error are what they say
    N = sum(sizes)
    assert abs(est["mean"].mean() - mu) < 5 * sigma / np.sqrt(N * n_pix)
    assert np.allclose(est["se"], np.sqrt(v / N), rtol=1e-12)
    assert np.allclose(est["r"], est["se"] / est["mean"], rtol=1e-12)
    with pytest.raises(ValueError):
        film.noise_from_sums(sums[:1], sizes[:1])


def test_film_symbols_are_exported():
    L = _lib.load()
    names = [n for n in _lib.EXPORTED if n.startswith("rt_film_")]
    assert sorted(names) == sorted(["rt_film_create", "rt_film_destroy", "rt_film_reset", "rt_film_add", "rt_film_resolve",
                                    "rt_film_read", "rt_film_noise", "rt_film_get_info", "rt_film_state_bytes",
                                    "rt_film_save", "rt_film_load"])
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    for n in names:
        assert hasattr(L, n) and f" T {n}\n" in out.stdout, n
    hdr = open(os.path.join(ROOT, "include", "rt.h")).read()
    assert "#define RT_ABI_VERSION 6" in hdr and "typedef struct rt_film_info" in hdr
    import raytrace_amd as R
    assert R.Film is film.Film and R.raytrace_until is film.raytrace_until and R.noise_from_sums is film.noise_from_sums


def test_film_arguments_are_checked_before_the_device():
    """Null and invalid arguments are RT_E_INVALID with a message, before any device is touched (the
    scene handle of these calls is never read: a placeholder)."""
    L = _lib.load()
    cs = _lib.camera_struct(scenes.cornell_box(spp=1, width=4)[0])
    ex = _lib.exec_struct()
    h = ctypes.c_void_p()
    scene = ctypes.create_string_buffer(4096)

    def create(c, e, s=scene, out=h):
        return L.rt_film_create(s, ctypes.byref(c) if c is not None else None, 1,
                                ctypes.byref(e) if e is not None else None, ctypes.byref(out) if out is not None else None)

    for args in ((cs, ex, None), (None, ex), (cs, None)):
        assert create(*args) == _lib.RT_E_INVALID and b"null" in L.rt_last_error()
    assert L.rt_film_create(scene, ctypes.byref(cs), 1, ctypes.byref(ex), None) == _lib.RT_E_INVALID
    assert create(cs, _lib.exec_struct(devices=[0])) == _lib.RT_E_INVALID and b"n_devices" in L.rt_last_error()
    for enc in ("srgb", "sqrt"):
        assert create(cs, _lib.exec_struct(encode=enc)) == _lib.RT_E_INVALID and b"linear" in L.rt_last_error()
    bad = _lib.exec_struct()
    bad.flags = 0x100
    assert create(cs, bad) == _lib.RT_E_INVALID and b"unknown" in L.rt_last_error()
    assert create(cs, _lib.exec_struct(n_shards=2, shard=2)) == _lib.RT_E_INVALID
    cs0 = _lib.camera_struct(scenes.cornell_box(spp=1, width=4)[0].replace(cs_samplesPerPixel=0))
    assert create(cs0, ex) == _lib.RT_E_INVALID and L.rt_last_error()
    assert h.value is None
    # every entry point refuses a null film
    d = ctypes.c_double()
    n = ctypes.c_int64()
    info = _lib.RtFilmInfo()
    buf = ctypes.create_string_buffer(64)
    for rc in (L.rt_film_add(None, 1, None), L.rt_film_reset(None), L.rt_film_resolve(None, buf, None),
               L.rt_film_read(None, buf), L.rt_film_noise(None, None, ctypes.byref(d)),
               L.rt_film_get_info(None, ctypes.byref(info)), L.rt_film_state_bytes(None, ctypes.byref(n)),
               L.rt_film_save(None, buf, 64), L.rt_film_load(None, buf, 64)):
        assert rc == _lib.RT_E_INVALID
        assert b"null" in L.rt_last_error()
    assert L.rt_film_destroy(None) == _lib.RT_OK


def test_film_info_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rt_film_info), offsetof(rt_film_info, samples),\n'
                   '         offsetof(rt_film_info, passes), offsetof(rt_film_info, width), offsetof(rt_film_info, rows),\n'
                   '         offsetof(rt_film_info, nan_pixels), offsetof(rt_film_info, f32));\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    F = _lib.RtFilmInfo
    assert got == [ctypes.sizeof(F), F.samples.offset, F.passes.offset, F.width.offset, F.rows.offset,
                   F.nan_pixels.offset, F.f32.offset]
    assert film.HEADER_DTYPE.itemsize == 64
