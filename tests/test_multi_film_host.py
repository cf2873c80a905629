"""The multi-device film without a GPU: the row map its merge kernel runs (rt_film.h
rt_film_block_span) against a plain loop over rt_shard_row, the merge restated for the host against
numpy, and the new C-ABI entry points' symbols and argument checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raytrace_amd import _lib, film
from raytrace_amd.ray import shard_row_index, shard_rows

SRC = os.path.join(ROOT, "tests", "film")
CXXFLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
NAMES = ["rt_multi_film_create", "rt_multi_film_destroy", "rt_multi_film_reset", "rt_multi_film_add",
         "rt_multi_film_load", "rt_multi_film_frame", "rt_multi_film_copies"]


@pytest.fixture(scope="module")
def merge_rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merge_rows") / "merge_rows")
    r = subprocess.run(["g++", *CXXFLAGS, "-o", exe, os.path.join(SRC, "merge_rows.cpp"), "-ldl", "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_block_spans_are_the_shard_row_map(merge_rows):
    """rt_film_block_span against a plain loop over the library's rt_shard_row: height {1, 7, 8, 50} x
    width {1, 9, 50} x row_block {1, 3, 4} x n_shards {1, 2, 3, 5}, every shard.  Every frame pixel is
    the target of exactly one (shard, tile pixel); padding rows target nothing."""
    _lib.load()
    r = subprocess.run([merge_rows, "map", _lib.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-2000:]
    # each of the 144 cases covers its frame once
    assert int(r.stdout.split()[1]) == sum(h * w for h in (1, 7, 8, 50) for w in (1, 9, 50)) * 3 * 4


def synthetic_passes(rng, sizes, n_pixels, words):
    """Integer pass sums as a render leaves them (tests/test_film_host.py): the RGB sums in units of
    2^-32, in binary64 layouts the next 32 bits of each as three more words; a few NaN flags."""
    level = rng.choice([0.0, 1e-3, 0.05, 0.7, 15.0], size=(n_pixels, 1))
    sums = np.zeros((len(sizes), n_pixels, words), np.int64)
    for k, n in enumerate(sizes):
        x = level[None] * rng.gamma(2.0, 0.5, size=(n, n_pixels, 3))
        sums[k, :, :3] = np.floor(x * 2.0 ** 32).astype(np.int64).sum(0)
        if words == 6:
            sums[k, :, 3:] = rng.integers(0, n << 32, size=(n_pixels, 3))
    flags = (rng.random((len(sizes), n_pixels)) < 0.02).astype(np.uint32) << rng.integers(0, 3, size=(len(sizes), n_pixels)).astype(np.uint32)
    flags[0, 0] |= 1   # (whatever the draw: the first and the last pixel carry one)
    flags[-1, -1] |= 2
    return sums, flags


def run_merge(exe, tmp_path, sums, flags, sizes, width, height, row_block, n_shards):
    """The host merge over the passes cut into n_shards tiles (numpy, by ray.shard_row_index: the
    test's own statement of the interleave, zeros in padding rows)."""
    K, n, words = sums.shape
    rows = shard_rows(height, n_shards, row_block)
    src, dst = str(tmp_path / f"in{n_shards}.bin"), str(tmp_path / f"out{n_shards}.bin")
    with open(src, "wb") as f:
        f.write(np.array([words, width, height, row_block, n_shards, K] + list(sizes), np.int64).tobytes())
        for k in range(K):
            fs, ff = sums[k].reshape(height, width, words), flags[k].reshape(height, width)
            for r in range(n_shards):
                g = shard_row_index(height, n_shards, r, row_block)
                ts, tf = np.zeros((rows, width, words), np.int64), np.zeros((rows, width), np.uint32)
                ts[g < height], tf[g < height] = fs[g[g < height]], ff[g[g < height]]
                f.write(ts.tobytes())
                f.write(tf.tobytes())
    subprocess.run([exe, "merge", src, dst], check=True)
    raw = np.fromfile(dst, np.uint8)
    a, b = 8 * n * words, 8 * n * words + 4 * n
    return raw[:a].view(np.int64).reshape(n, words), raw[a:b].view(np.uint32), raw[b:].view(np.float64)


@pytest.mark.parametrize("words", [3, 6])
@pytest.mark.parametrize("width,height,row_block", [(9, 7, 3), (50, 50, 4), (1, 8, 1)])
def test_host_merge_equals_the_unsharded_merge(merge_rows, tmp_path, words, width, height, row_block):
    """Two and three shards against one unsharded merge and against numpy: totals, flags and q byte
    for byte (the same integer adds; q by the same three roundings per pass, film.noise_from_sums)."""
    sizes = [1, 7, 3, 16, 5]
    rng = np.random.default_rng(1000 * words + width)
    sums, flags = synthetic_passes(rng, sizes, width * height, words)
    one = run_merge(merge_rows, tmp_path, sums, flags, sizes, width, height, row_block, 1)
    assert np.array_equal(one[0], sums.sum(0, dtype=np.int64))
    assert np.array_equal(one[1], np.bitwise_or.reduce(flags, 0)) and one[1].any()
    want_q = film.noise_from_sums(sums[..., :3], sizes)["q"]
    assert one[2].tobytes() == want_q.tobytes() and (want_q > 0).any()
    for n_shards in (2, 3):
        got = run_merge(merge_rows, tmp_path, sums, flags, sizes, width, height, row_block, n_shards)
        for g, w in zip(got, one):
            assert g.tobytes() == w.tobytes(), n_shards


def test_multi_film_symbols_are_exported():
    L = _lib.load()
    assert sorted(n for n in _lib.EXPORTED if n.startswith("rt_multi_film_")) == sorted(NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    hdr = open(os.path.join(ROOT, "include", "rt.h")).read()
    for n in NAMES:
        assert hasattr(L, n) and f" T {n}\n" in out.stdout, n
        assert f"int {n}(" in hdr, n
    assert "#define RT_ABI_VERSION 6" in hdr and "typedef struct rt_multi_film rt_multi_film;" in hdr
    assert L.rt_abi_version() == 6
    import raytrace_amd as R
    assert R.MultiFilm is film.MultiFilm and issubclass(R.MultiFilm, R.Film)


def test_multi_film_arguments_are_checked_before_the_device():
    """Null arguments are RT_E_INVALID with a message, before any device is touched (the scene
    handle of the create calls is never read: a placeholder)."""
    from raytrace_amd import scenes
    L = _lib.load()
    cs = _lib.camera_struct(scenes.cornell_box(spp=1, width=4)[0])
    ex = _lib.exec_struct()
    h = ctypes.c_void_p()
    scene = ctypes.create_string_buffer(4096)
    for args in ((None, ctypes.byref(cs), 1, ctypes.byref(ex), ctypes.byref(h)),
                 (scene, None, 1, ctypes.byref(ex), ctypes.byref(h)),
                 (scene, ctypes.byref(cs), 1, None, ctypes.byref(h)),
                 (scene, ctypes.byref(cs), 1, ctypes.byref(ex), None)):
        assert L.rt_multi_film_create(*args) == _lib.RT_E_INVALID and b"null" in L.rt_last_error()
    # a device list or a shard in rt_exec: the film's devices are the scene's, its frame the whole image
    two = _lib.exec_struct()
    two.n_shards = 2
    assert L.rt_multi_film_create(scene, ctypes.byref(cs), 1, ctypes.byref(two), ctypes.byref(h)) == _lib.RT_E_INVALID
    assert b"n_shards" in L.rt_last_error()
    lst = _lib.exec_struct(devices=[0])
    assert L.rt_multi_film_create(scene, ctypes.byref(cs), 1, ctypes.byref(lst), ctypes.byref(h)) == _lib.RT_E_INVALID
    assert b"n_devices" in L.rt_last_error() and h.value is None
    buf = ctypes.create_string_buffer(64)
    for rc in (L.rt_multi_film_add(None, 1), L.rt_multi_film_reset(None), L.rt_multi_film_load(None, buf, 64),
               L.rt_multi_film_load(scene, None, 64), L.rt_multi_film_frame(None, ctypes.byref(h)),
               L.rt_multi_film_frame(scene, None), L.rt_multi_film_copies(None, ctypes.byref(ctypes.c_int64())),
               L.rt_multi_film_copies(scene, None)):
        assert rc == _lib.RT_E_INVALID and b"null" in L.rt_last_error()
    assert L.rt_multi_film_destroy(None) == _lib.RT_OK
