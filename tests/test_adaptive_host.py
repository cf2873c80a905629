"""Adaptive film passes without a GPU: the per-pixel functions of rt_adaptive.h (select, list merge,
resolve and noise with counts) in a stand-alone host program against their numpy twin
film.noise_from_counts, the same program under AddressSanitizer and UBSan, the new entry points'
argument checks before any device call, and the new names in the header, the library and the
binding."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raytrace_amd import _lib, film

SRC = os.path.join(ROOT, "tests", "adaptive", "list_math.cpp")
CXXFLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
NAMES = ["rt_adaptive_add", "rt_adaptive_get_info", "rt_adaptive_counts_read", "rt_adaptive_selection_read"]


def compile_program(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", *CXXFLAGS, *extra, "-o", exe, SRC, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def synthetic_state(rng, n_pixels, words, n):
    """A non-uniform film's words as passes leave them: per pixel K_p >= 2 batches of unequal sizes of
    a non-negative radiance in the fixed-point unit 2^-32 — dark, mid and bright pixels, some below
    the 3/256 floor —, a few NaN-flagged pixels and padding pixels (0, 0), and one more pass of n."""
    level = rng.choice([0.0, 1e-3, 0.05, 0.7, 15.0], size=n_pixels)
    K = rng.integers(2, 6, n_pixels)
    total = np.zeros((n_pixels, words), np.int64)
    q = np.zeros(n_pixels)
    counts = np.zeros((n_pixels, 2), np.uint32)
    for p in range(n_pixels):
        for _ in range(K[p]):
            size = int(rng.integers(1, 9))
            s = np.floor(level[p] * rng.gamma(2.0, 0.5, size=(size, 3)) * 2.0 ** 32).astype(np.int64).sum(0)
            total[p, :3] += s
            L = float(s.sum())
            q[p] = q[p] + (L * L) / float(size)
            counts[p] += np.array((size, 1), np.uint32)
    if words == 6:
        total[:, 3:] = rng.integers(0, 2 ** 36, (n_pixels, 3))
    flags = (rng.random(n_pixels) < 0.05).astype(np.uint32)
    pad = rng.random(n_pixels) < 0.05
    counts[pad] = 0
    total[pad] = 0
    q[pad] = 0.0
    pas = np.zeros((n_pixels, words), np.int64)
    pas[:, :3] = np.floor(level[:, None] * rng.gamma(2.0, 0.5, size=(n_pixels, 3)) * n * 2.0 ** 32).astype(np.int64)
    if words == 6:
        pas[:, 3:] = rng.integers(0, 2 ** 36, (n_pixels, 3))
    pass_flags = (rng.random(n_pixels) < 0.02).astype(np.uint32)
    listed = (rng.random(n_pixels) < 0.4).astype(np.uint8)
    return total, flags, q, counts, pas, pass_flags, listed


def run_list_math(exe, tmp_path, words, n, threshold, max_samples, seed):
    rng = np.random.default_rng(seed)
    n_pixels = 777
    total, flags, q, counts, pas, pass_flags, listed = synthetic_state(rng, n_pixels, words, n)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([n_pixels, words, n, max_samples], np.int64).tobytes())
        f.write(np.array([threshold], np.float64).tobytes())
        for a in (total, flags, q, counts, pas, pass_flags, listed):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-4000:]
    assert int(r.stdout.split()[1]) == int(listed.sum()) > 100
    raw = np.fromfile(dst, np.uint8)
    got_r = raw[:8 * n_pixels].view(np.float64)
    got_sel = raw[8 * n_pixels:].astype(bool)
    return total, flags, q, counts, got_r, got_sel


@pytest.mark.parametrize("words", [3, 6])
def test_pixel_functions_match_noise_from_counts(tmp_path, words):
    """The select predicate and the noise with counts (rt_adaptive.h, compiled for the host without
    contraction) against film.noise_from_counts on the same words: the same binary64 operation
    sequence, so the same bits; the program itself checks the list merge against the whole-frame
    merge and the resolve with counts against the uniform resolve."""
    exe = compile_program(tmp_path, "list_math")
    n, max_samples = 8, 30
    for threshold in (0.05, -1.0, 1e9):
        total, flags, q, counts, got_r, got_sel = run_list_math(exe, tmp_path, words, n, threshold, max_samples, 11 + words)
        want_r = film.noise_from_counts(total, q, counts)
        counted = counts[:, 0] > 0
        assert np.isfinite(want_r[counted]).all() and (want_r[counted] > 0).any()
        assert np.array_equal(got_r[counted].view(np.uint64), want_r[counted].view(np.uint64))
        below_cap = counts[:, 0].astype(np.int64) + n <= max_samples
        want_sel = counted & (flags == 0) & below_cap & ((want_r > threshold) if threshold >= 0 else True)
        assert np.array_equal(got_sel, want_sel)
        if threshold == 0.05:
            assert 0 < want_sel.sum() < counted.sum() and (counted & (flags == 0) & ~below_cap).any()
        if threshold == 1e9:
            assert not want_sel.any()


def test_pixel_functions_under_sanitizers(tmp_path):
    """The same stand-alone program built with AddressSanitizer and UBSan, run once per word count."""
    exe = compile_program(tmp_path, "list_math_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for words in (3, 6):
        run_list_math(exe, tmp_path, words, 8, 0.05, 30, 5 + words)


def test_noise_from_counts_on_uniform_counts_is_noise_from_sums():
    rng = np.random.default_rng(3)
    sizes = [4, 4, 8]
    sums = np.floor(rng.gamma(2.0, 0.5, size=(3, 50, 3)) * 2.0 ** 32 * np.array(sizes)[:, None, None]).astype(np.int64)
    est = film.noise_from_sums(sums, sizes)
    r = film.noise_from_counts(sums.sum(0), est["q"], np.broadcast_to((16, 3), (50, 2)))
    assert np.array_equal(r, est["r"])
    assert np.isnan(film.noise_from_counts(sums.sum(0), est["q"], np.zeros((50, 2), np.uint32))).all()


def test_unpack_state_reads_both_layout_versions():
    rows, width = 3, 5
    n = rows * width
    for version, words in ((1, 3), (2, 6)):
        hd = np.zeros(1, film.HEADER_DTYPE)
        hd["version"], hd["f32"], hd["rows"], hd["width"] = version, words == 3, rows, width
        body = [np.arange(n * words, dtype="<i8"), np.arange(n, dtype="<u4"), np.arange(n, dtype="<f8")]
        if version == 2:
            body.append(np.arange(2 * n, dtype="<u4"))
        st = film.unpack_state(np.concatenate([hd.view(np.uint8)] + [b.view(np.uint8) for b in body]))
        assert st["sums"].shape == (rows, width, words) and st["q"][2, 4] == n - 1
        assert ("counts" in st) == (version == 2)
        if version == 2:
            assert st["counts"].shape == (rows, width, 2) and st["counts"][2, 4, 1] == 2 * n - 1


def test_adaptive_symbols_are_declared_and_exported():
    L = _lib.load()
    assert sorted(n for n in _lib.EXPORTED if n.startswith("rt_adaptive_")) == sorted(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    hdr = open(os.path.join(ROOT, "include", "rt.h")).read()
    for n in NAMES:
        assert hasattr(L, n) and f" T {n}\n" in out.stdout and f"int {n}(" in hdr, n
    assert "#define RT_ABI_VERSION 6" in hdr and "typedef struct rt_adaptive_info" in hdr
    assert ctypes.sizeof(_lib.RtAdaptiveInfo) == 32
    import raytrace_amd as R
    assert R.noise_from_counts is film.noise_from_counts
    assert all(hasattr(film.Film, m) for m in ("add_where", "sample_map", "adaptive_info"))


def test_adaptive_arguments_are_checked_before_the_device():
    """Null and invalid arguments are RT_E_INVALID with a message before any device is touched (the
    film handle of the n_samples and threshold checks is never read: a placeholder)."""
    L = _lib.load()
    info = _lib.RtAdaptiveInfo()
    buf = ctypes.create_string_buffer(64)
    n = ctypes.c_int64()
    for rc in (L.rt_adaptive_add(None, 8, 0.1, 0, None), L.rt_adaptive_get_info(None, ctypes.byref(info)),
               L.rt_adaptive_counts_read(None, buf), L.rt_adaptive_selection_read(None, buf, 1, ctypes.byref(n))):
        assert rc == _lib.RT_E_INVALID and b"null" in L.rt_last_error()
    placeholder = ctypes.create_string_buffer(4096)
    assert L.rt_adaptive_get_info(placeholder, None) == _lib.RT_E_INVALID
    assert L.rt_adaptive_counts_read(placeholder, None) == _lib.RT_E_INVALID
    assert L.rt_adaptive_selection_read(placeholder, buf, 1, None) == _lib.RT_E_INVALID
    for bad_n in (0, -3):
        assert L.rt_adaptive_add(placeholder, bad_n, 0.1, 0, None) == _lib.RT_E_INVALID and b"at least one" in L.rt_last_error()
    assert L.rt_adaptive_add(placeholder, 8, float("nan"), 0, None) == _lib.RT_E_INVALID and b"NaN" in L.rt_last_error()
    for bad_cap in (-1, (1 << 24) + 1):
        assert L.rt_adaptive_add(placeholder, 8, 0.1, bad_cap, None) == _lib.RT_E_INVALID and b"max_samples" in L.rt_last_error()


def test_raytrace_until_adaptive_refuses_denoise_and_devices():
    from raytrace_amd import scenes
    from raytrace_amd.errors import RtInvalid
    cs, world, seed = scenes.cornell_box(spp=64, width=8)
    for kw in (dict(denoise=True), dict(devices=[0]), dict(max_spp=16)):
        with pytest.raises(RtInvalid):
            film.raytrace_until(cs, world, seed, 0.05, batch=16, adaptive=True, **kw)
