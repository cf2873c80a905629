"""Adaptive film passes on the GPU (include/rt.h rt_adaptive_*, raytrace_amd.film add_where).

Sums are integers keyed by (pixel, sample index), so every comparison of a pixel that holds N_p
samples against a uniform film at N_p is bit for bit: sums, flags and image.  The selection is
compared with the numpy twin film.noise_from_counts on the film's own words (the same binary64
operation sequence as rt_film.h: exact), and the estimator word q with the twin's q + L^2 / n.
Every test in both precisions on 24 x 14 pixels unless it says otherwise."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raytrace_amd as R  # noqa: E402
from raytrace_amd import _lib, film, scenes  # noqa: E402
from raytrace_amd.errors import RtInvalid, RtUnsupported  # noqa: E402
from raytrace_amd.scene import FlatScene, flatten  # noqa: E402
from test_render_params import _instanced  # noqa: E402

# the kernel classes: flat with the deferred redirect pdf, flat with textures, a BVH with the full
# material set, media, two-level instancing, noise textures
SCENES = {
    "cornell": lambda: scenes.cornell_box(width=24, spp=1),
    "readme": lambda: scenes.readme_scene(width=24, spp=1),
    "demo1": lambda: scenes.demo1(width=24, spp=1),
    "pawn_fog": lambda: scenes.pawn_fog(width=24, spp=1),
    "instanced": _instanced,
    "noise": lambda: scenes.noise_test(width=24, spp=1),
}
PRECISIONS = ["f64", "f32"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.load()
    return torch


@functools.lru_cache(maxsize=None)
def scene(name, width=24, height=14):
    cs, world, seed = SCENES[name]()
    cs = cs.replace(cs_imageWidth=width, cs_aspectRatio=width / height, cs_samplesPerPixel=1)
    return cs, world if isinstance(world, FlatScene) else flatten(world), seed


def new_film(name, precision, width=24, height=14, **kw):
    cs, flat, seed = scene(name, width, height)
    return R.Film(flat, cs, seed, precision=precision, **kw)


def snapshot(f):
    """The film's state, unpacked, with its image; read-only copies"""
    st = film.unpack_state(f.state().copy())
    st["image"] = f.image()
    return st


@functools.lru_cache(maxsize=None)
def uniform(name, precision, passes, width=24, height=14, shard=None):
    """The reference of every comparison: a uniform film after `passes` (computed once, read-only)."""
    kw = dict(n_shards=3, shard=shard, row_block=4) if shard is not None else {}
    with new_film(name, precision, width, height, **kw) as f:
        for n in passes:
            f.add(n)
        st = snapshot(f)
    for a in st.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return st


def counts_of(st):
    return st["counts"] if "counts" in st else np.broadcast_to(
        np.array((st["header"]["samples"], st["header"]["passes"]), np.uint32), st["q"].shape + (2,))


def rel_error(st):
    """r per pixel in binary64 from a state's words, and the pixels that count (whole frames)"""
    return film.noise_from_counts(st["sums"], st["q"], counts_of(st)), st["flags"] == 0


def threshold_by_rank(r, counting, k):
    """A threshold that selects exactly the k counting pixels of largest r: the midpoint of the gap
    below the k-th largest (which must be a gap); every counting pixel: negative"""
    v = np.sort(r[counting])[::-1]
    if k == len(v):
        return -1.0
    assert v[k - 1] > v[k], "the ranks around the cut hold equal errors: choose another scene"
    t = 0.5 * (v[k - 1] + v[k])
    assert v[k - 1] > t >= v[k]
    return t


def median_threshold(r, counting):
    """The midpoint of a gap between two adjacent distinct r values nearest the median"""
    v = np.unique(r[counting])
    assert len(v) >= 2
    m = max(1, len(v) // 2)
    t = 0.5 * (v[m - 1] + v[m])
    assert v[m - 1] <= t < v[m]
    return t


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_pixels_equal(got, want, mask, what):
    """sums, flags and image of the masked pixels, bit for bit"""
    for k in ("sums", "flags", "image"):
        g, w = got[k][mask], want[k][mask]
        assert bits_equal(np.ascontiguousarray(g), np.ascontiguousarray(w)), \
            f"{what}: {k} differ on {int(np.any((g != w).reshape(len(g), -1), axis=1).sum())} of {len(g)} pixels"


def twin_q(before, after, mask, n):
    """q of the masked pixels after a pass of n samples: rt_film_q_add on the pass's luminance word"""
    L = (after["sums"][..., :3] - before["sums"][..., :3]).sum(-1, dtype=np.int64).astype(np.float64)
    return np.where(mask, before["q"] + (L * L) / float(n), before["q"])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(SCENES))
def test_selected_pixels_are_a_uniform_film_at_their_count(gpu, name, precision):
    """add(4), add(4), add_where(8, t) with t in a gap of the film's own errors near their median: the
    selection is the twin's, its pixels are a uniform film's after add(16) and the others one's after
    add(8), bit for bit; q is the twin's."""
    with new_film(name, precision) as f:
        f.add(4).add(4)
        before = snapshot(f)
        assert before["header"]["version"] == 1
        r, counting = rel_error(before)
        t = median_threshold(r, counting)
        f.add_where(8, t)
        want_sel = np.flatnonzero(((r > t) & counting).ravel())
        info = f.adaptive_info()
        assert 0 < info["selected"] < int(counting.sum())
        assert np.array_equal(f.selection(), want_sel)
        assert info["selected"] == len(want_sel) and info["nonuniform"] and info["adaptive_passes"] == 1
        sel = np.zeros(r.size, bool)
        sel[want_sel] = True
        sel = sel.reshape(r.shape)
        assert np.array_equal(f.sample_map(), np.where(sel, 16, 8))
        assert np.array_equal(f.counts()[..., 1], np.where(sel, 3, 2))
        assert (f.spp, f.passes) == (16, 3)
        assert info["total_samples"] == int(np.where(sel, 16, 8)[counting].sum())
        assert (info["min_samples"], info["max_samples"]) == (8, 16)
        after = snapshot(f)
    assert_pixels_equal(after, uniform(name, precision, (16,)), sel, "selected")
    assert_pixels_equal(after, uniform(name, precision, (8,)), ~sel, "not selected")
    assert_pixels_equal(after, before, ~sel, "not selected, before")
    assert bits_equal(after["q"], twin_q(before, after, sel, 8))
    assert np.isfinite(after["image"]).all() and after["image"].mean() > 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_empty_selection_changes_nothing(gpu, precision):
    with new_film("cornell", precision) as f:
        f.add(4).add(4)
        before = f.state().copy()
        f.add_where(8, 1e30)
        assert f.adaptive_info()["selected"] == 0 and len(f.selection()) == 0
        after = f.state()
        st = film.unpack_state(after)
    assert bits_equal(after[64:len(before)], before[64:])  # sums, flags, q
    assert st["header"]["version"] == 2 and (st["header"]["samples"], st["header"]["passes"]) == (8, 2)
    assert np.array_equal(st["counts"], np.broadcast_to(np.array((8, 2), np.uint32), st["counts"].shape))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["cornell", "demo1"])
def test_selecting_every_pixel_is_a_uniform_pass(gpu, name, precision):
    want = uniform(name, precision, (4, 4, 8))
    with new_film(name, precision) as f:
        f.add(4).add(4).add_where(8, -1.0)
        assert f.adaptive_info()["selected"] == 24 * 14
        got = snapshot(f)
        noise, noise_map = f.noise(), f.noise_map()
    with new_film(name, precision) as u:
        u.add(4).add(4).add(8)
        want_noise, want_map = u.noise(), u.noise_map()
    every = np.ones(got["q"].shape, bool)
    assert_pixels_equal(got, want, every, "every pixel")
    assert bits_equal(got["q"], want["q"])
    assert np.array_equal(got["counts"], np.broadcast_to(np.array((16, 3), np.uint32), got["counts"].shape))
    assert noise == want_noise and bits_equal(noise_map, want_map)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("k", [1, 63, 64, 65])
def test_list_lengths_around_a_wave(gpu, k, precision):
    """13 x 5 pixels of the pawn in fog (every pixel's error is positive and no two are equal), the
    threshold cut below the k-th largest error: lists of 1, 63, 64 and 65 entries"""
    with new_film("pawn_fog", precision, 13, 5) as f:
        f.add(4).add(4)
        before = snapshot(f)
        r, counting = rel_error(before)
        assert counting.all()
        t = threshold_by_rank(r, counting, k)
        f.add_where(8, t)
        picked = f.selection()
        after = snapshot(f)
    assert len(picked) == k and np.array_equal(picked, np.flatnonzero(((r > t) if t >= 0 else counting).ravel()))
    sel = np.zeros(r.size, bool)
    sel[picked] = True
    sel = sel.reshape(r.shape)
    assert_pixels_equal(after, uniform("pawn_fog", precision, (16,), 13, 5), sel, "selected")
    assert_pixels_equal(after, before, ~sel, "not selected")
    assert np.array_equal(after["counts"][..., 0], np.where(sel, 16, 8))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_max_spp_stops_pixels_at_the_cap(gpu, precision):
    with new_film("cornell", precision) as f:
        f.add(4).add(4)
        r, counting = rel_error(snapshot(f))
        f.add_where(8, median_threshold(r, counting))   # some pixels at 16, the others at 8
        some = f.adaptive_info()["selected"]
        f.add_where(8, -1.0, max_spp=16)                # only the pixels at 8 fit under the cap
        assert f.adaptive_info()["selected"] == 24 * 14 - some
        assert (f.sample_map() == 16).all()
        got, raw = snapshot(f), f.state().copy()
        f.add_where(8, -1.0, max_spp=23)                # nobody fits
        assert f.adaptive_info()["selected"] == 0 and (f.sample_map() == 16).all()
        assert bits_equal(f.state(), raw)
    assert_pixels_equal(got, uniform("cornell", precision, (16,)), np.ones(r.shape, bool), "at the cap")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_shards_padding_rows_are_never_selected(gpu, precision):
    """shard 1 of 3 in blocks of 4 rows: tile rows 0-3 are the frame's rows 4-7, tile rows 4-7 padding"""
    kw = dict(n_shards=3, shard=1, row_block=4)
    with new_film("cornell", precision, **kw) as f:
        assert f.shape[:2] == (8, 24)
        f.add(4).add(4)
        assert np.array_equal(f.counts()[4:], np.zeros((4, 24, 2), np.uint32)) and (f.counts()[:4] == (8, 2)).all()
        f.add_where(8, -1.0)
        picked = f.selection()
        got = snapshot(f)
        info = f.adaptive_info()
        noise_map = f.noise_map()
    assert np.array_equal(picked, np.arange(4 * 24))
    assert (got["counts"][:4] == (16, 3)).all() and (got["counts"][4:] == 0).all()
    assert info["total_samples"] == 16 * 4 * 24 and (info["min_samples"], info["max_samples"]) == (16, 16)
    want = uniform("cornell", precision, (16,), shard=1)
    assert_pixels_equal(got, want, np.ones((8, 24), bool), "shard")
    assert (got["image"][4:] == 0).all() and np.isnan(noise_map[4:]).all() and np.isfinite(noise_map[:4]).all()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["cornell", "pawn_fog"])
def test_chunking_and_reruns_do_not_change_the_state(knobs, gpu, name, precision):
    """RT_AMD_LIST_CHUNK = 1 and 3 at n = 8 against the default, and the default twice: identical bytes"""
    def run(chunk):
        if chunk:
            knobs.setenv("RT_AMD_LIST_CHUNK", str(chunk))
        else:
            knobs.delenv("RT_AMD_LIST_CHUNK", raising=False)
        with new_film(name, precision) as f:
            f.add(4).add(4)
            r, counting = rel_error(snapshot(f))
            return f.add_where(8, median_threshold(r, counting)).state().copy()
    base = run(0)
    assert film.unpack_state(base)["header"]["version"] == 2
    for chunk in (0, 1, 3):
        assert bits_equal(run(chunk), base), chunk


@pytest.mark.parametrize("precision", PRECISIONS)
def test_state_round_trip_and_layout_versions(gpu, precision):
    words = 3 if precision == "f32" else 6
    with new_film("cornell", precision) as f:
        f.add(4).add(4)
        v1 = f.state().copy()
        hd = film.unpack_state(v1)["header"]
        # a uniform film's state: layout version 1, the header and the three planes, nothing more
        assert hd["version"] == 1 and len(v1) == 64 + 24 * 14 * (8 * words + 4 + 8)
        assert (hd["samples"], hd["passes"], hd["reserved"]) == (8, 2, 0)
        r, counting = rel_error(film.unpack_state(v1))
        t = median_threshold(r, counting)
        f.add_where(8, t)
        v2 = f.state().copy()
        st2 = film.unpack_state(v2)
        assert st2["header"]["version"] == 2 and len(v2) == len(v1) + 24 * 14 * 8
        assert (st2["header"]["samples"], st2["header"]["passes"]) == (16, 3)
        r2, counting2 = rel_error(st2)
        t2 = median_threshold(r2, counting2)
        unbroken = f.add_where(8, t2).state().copy()
        picked = f.selection()
    with new_film("cornell", precision) as g:
        g.restore(v2)
        assert g.adaptive_info()["nonuniform"] and (g.spp, g.passes) == (16, 3)
        assert bits_equal(g.state(), v2)
        assert len(g.selection()) == 0
        resumed = g.add_where(8, t2).state().copy()
        assert np.array_equal(g.selection(), picked)
        assert bits_equal(resumed, unbroken)
        g.restore(v1)  # a version-1 state makes the film uniform again
        assert not g.adaptive_info()["nonuniform"] and bits_equal(g.state(), v1)
        g.add(8)
    assert 0 < len(picked) < 24 * 14


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals_on_a_non_uniform_film(gpu, precision):
    with new_film("cornell", precision) as f:
        with pytest.raises(RtInvalid, match="two passes"):
            f.add(4).add_where(8, 0.1)
        f.add(4).add_where(8, 0.05)
        state = f.state().copy()
        with pytest.raises(RtInvalid, match="negative threshold"):
            f.add(8)
        with pytest.raises(RtUnsupported, match="non-uniform"):
            f.denoised()
        cs, flat, seed = scene("cornell")
        with R.MultiFilm(flat, cs, seed, devices=[0], precision=precision) as m:
            with pytest.raises(RtInvalid, match="non-uniform"):
                m.restore(state)
            with pytest.raises(RtInvalid):
                m.add(4).add(4).add_where(8, 0.05)
        f.reset()
        info = f.adaptive_info()
        assert not info["nonuniform"] and info["adaptive_passes"] == 0 and (f.spp, f.passes) == (0, 0)
        got = snapshot(f.add(16))
    assert got["header"]["version"] == 1
    assert_pixels_equal(got, uniform("cornell", precision, (16,)), np.ones((14, 24), bool), "after reset")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_raytrace_until_adaptive_converges_per_pixel(gpu, precision):
    """The Cornell box at 48 pixels: every pixel that counts ends at r <= noise or within `batch` of
    max_spp, from the returned sample map and the twin's errors; the samples are spent unevenly."""
    cs, world, seed = scenes.cornell_box(width=48, spp=1)
    noise, batch, max_spp = 0.08, 8, 96
    img, info = film.raytrace_until(cs, world, seed, noise, batch=batch, max_spp=max_spp, adaptive=True, precision=precision)
    n, r = info["sample_map"], info["rel_error"]
    counting = np.isfinite(r)
    assert counting.all() and img.shape == (48, 48, 3) and np.isfinite(img).all()
    assert np.all((r <= noise) | (n.astype(np.int64) + batch > max_spp))
    assert n.min() >= 2 * batch and n.max() == info["spp_max"] == info["spp"] <= max_spp
    assert info["spp_mean"] == n.mean() and info["spp_mean"] < info["spp_max"]
    assert len(info["selected"]) >= 1 and all(0 < s <= 48 * 48 for s in info["selected"])
    assert 3 <= info["passes"] <= 2 + len(info["selected"])
    assert info["converged"] == bool(np.all(r <= noise))
