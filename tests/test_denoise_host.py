"""The film's denoiser and feature pass without a GPU: the filter's per-pixel functions (the kernels'
text, compiled for the host under AddressSanitizer / UBSan) against the numpy twin bit for bit, the
feature body's host build against the FP64 oracle's render of the emitter twin, the emitter twin
itself, and the new C-ABI entry points' symbols and argument checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from raytrace_amd import _lib, denoise, film, scenes

SRC = os.path.join(ROOT, "tests", "denoise")
CXXFLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function",
            "-Wno-unknown-pragmas"]


@pytest.fixture(scope="module")
def dn_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dn") / "dn_host")
    r = subprocess.run(["g++", *CXXFLAGS, "-o", exe, os.path.join(SRC, "dn_host.cpp"), "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def synthetic_frame(rng, W, H, sizes=(1, 7, 3), n_feat=8):
    """A film's words as renders leave them (integer sums in units of 2^-32, q by the film's own
    formula) and feature words: smooth albedo regions with an edge, dark pixels below the albedo
    floor, unit-ish normals of two orientations, a block of zero-coverage pixels (misses) and a few
    NaN-flagged pixels."""
    n = W * H
    level = rng.choice([0.0, 1e-3, 0.05, 0.7, 15.0], size=(n, 1))
    sums = np.zeros((len(sizes), n, 3), np.int64)
    for k, m in enumerate(sizes):
        x = level[None] * rng.gamma(2.0, 0.5, size=(m, n, 3))
        sums[k] = np.floor(x * 2.0 ** 32).astype(np.int64).sum(0)
    q = film.noise_from_sums(sums, sizes)["q"]
    S = sums.sum(0)
    yy, xx = np.divmod(np.arange(n), W)
    F = np.zeros((n, 8), np.int64)
    hits = rng.integers(1, n_feat + 1, size=n)
    miss = (xx >= W // 2) & (yy < max(1, H // 3))
    hits[miss] = 0
    alb = np.where((xx < W // 3)[:, None], [0.73, 0.2, 0.05], rng.uniform(0.0, 1.0, size=(n, 3)))
    alb[rng.random(n) < 0.1] = 1e-3  # below the floor
    F[:, 0:3] = np.floor(alb * 2.0 ** 32).astype(np.int64) * n_feat
    nrm = np.where((yy < H // 2)[:, None], [0.0, 0.6, -0.8], [-1.0, 0.0, 0.0]) + rng.normal(0, 0.05, size=(n, 3))
    F[:, 3:6] = np.floor(nrm * 2.0 ** 32).astype(np.int64) * hits[:, None]
    F[:, 6] = np.floor((3.0 + 0.1 * xx + rng.uniform(0, 0.05, n)) * 2.0 ** 32).astype(np.int64) * hits
    F[:, 7] = hits
    flags = (rng.random(n) < 0.05).astype(np.uint32)
    if n > 4:
        flags[n // 2] = 1
    return S, q, F, flags, sum(sizes), len(sizes)


def pack_state(S, q, flags, W, H, N, K):
    hd = np.zeros(1, film.HEADER_DTYPE)
    hd["magic"], hd["version"], hd["f32"], hd["width"], hd["height"], hd["rows"] = 0x4d4c4652, 1, S.shape[-1] == 3, W, H, H
    hd["n_shards"], hd["row_block"], hd["passes"], hd["samples"] = 1, 4, K, N
    return np.concatenate([hd.view(np.uint8), S.astype("<i8").view(np.uint8).ravel(),
                           flags.astype("<u4").view(np.uint8), q.astype("<f8").view(np.uint8)])


@pytest.mark.parametrize("W,H,fw,n_albedo,params", [(9, 7, 8, 0, {}), (37, 23, 16, 64, {}), (1, 1, 8, 0, {}),
                                                    (37, 23, 8, 32, dict(levels=3, k=2, sigma_l=1.5, sigma_a=0.3)),
                                                    (9, 7, 16, 64, {})],
                         ids=["9x7", "37x23-f64words-albedo64", "1x1", "37x23-k2-albedo32", "9x7-f64words-albedo64"])
def test_filter_functions_equal_numpy_twin_bitwise(dn_host, tmp_path, W, H, fw, n_albedo, params):
    """rt_denoise.h's rt_dn_prepare and rt_dn_filter, built with -fsanitize=address,undefined
    -ffp-contract=off as a stand-alone program, on synthetic frames at levels = 5 (the largest step,
    16, exceeds the 9 x 7 frame; no size is a multiple of anything; 1 x 1 has the centre tap only;
    feature words as FP32 and as binary64 films hold them, with and without a remodulation albedo):
    the output equals denoise_reference BIT FOR BIT, NaN-flagged pixels included."""
    rng = np.random.default_rng(1000 * W + H)
    n_feat = 8
    S, q, F, flags, N, K = synthetic_frame(rng, W, H, n_feat=n_feat)
    if fw == 16:  # a binary64 film's feature words: low words (sums of 32-bit fractions) behind the high ones
        F = np.concatenate([F, rng.integers(0, n_feat << 32, size=(W * H, 7)), np.zeros((W * H, 1), np.int64)], axis=1)
        S = np.concatenate([S, rng.integers(0, N << 32, size=(W * H, 3))], axis=1)  # ... and so do its colour sums
    F2 = None
    if n_albedo:  # the remodulation albedo's words: the same albedo, estimated from other samples
        F2 = F.copy()
        F2[:, 0:3] = (F[:, 0:3] // n_feat + rng.integers(-(1 << 24), 1 << 24, size=(W * H, 3))).clip(0) * n_albedo
        if fw == 16:
            F2[:, 8:15] = rng.integers(0, n_albedo << 32, size=(W * H, 7))
    P = denoise.resolve_params(params)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array([W, H, P["levels"], P["k"], n_feat, K, fw, n_albedo], "<i4").tofile(f)
        np.array([N], "<i8").tofile(f)
        np.array([P["sigma_z"], P["sigma_l"], P["sigma_a"], P["eps_n"], P["eps_z"], P["eps_l"]], "<f8").tofile(f)
        S.astype("<i8").tofile(f), q.astype("<f8").tofile(f), F.astype("<i8").tofile(f)
        if F2 is not None:
            F2.astype("<i8").tofile(f)
        flags.astype("<u4").tofile(f)
    r = subprocess.run([dn_host, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    got = np.fromfile(fout, "<f8").reshape(H, W, 3)
    mean, var, fl = denoise.film_inputs(pack_state(S, q, flags, W, H, N, K))
    feats = denoise.features_from_words(F.reshape(H, W, fw), n_feat)
    if F2 is not None:
        feats["albedo_out"] = denoise.features_from_words(F2.reshape(H, W, fw), n_albedo)["albedo"]
    want = denoise.denoise_reference(mean, var, fl, feats, P)
    bad = flags.reshape(H, W) != 0
    assert np.isnan(got[bad]).all() and np.isnan(want[bad]).all() and np.isfinite(got[~bad]).all()
    assert np.array_equal(got.view(np.uint64)[~bad], want.view(np.uint64)[~bad])
    if W > 4:  # the filter does something: it moves pixels, and it lowers the variance-driven spread
        raw = mean.copy()
        assert not np.array_equal(got[~bad], raw[~bad])


def test_twin_is_the_identity_without_variance():
    """With zero variance and a constant demodulated colour (e = 1 everywhere: the colour is the
    albedo) every level returns e = 1 exactly, so the output is the albedo above its floor."""
    H, W = 11, 13
    rng = np.random.default_rng(5)
    a = rng.uniform(0.01, 1.0, size=(H, W, 3))
    feats = dict(albedo=a, normal=rng.normal(size=(H, W, 3)), depth=rng.uniform(1, 2, (H, W)), coverage=np.ones((H, W)))
    out = denoise.denoise_reference(a, np.zeros((H, W)), np.zeros((H, W), np.uint32), feats)
    assert np.array_equal(out, a)


def test_emitter_twin_replaces_every_material():
    import raytrace_amd as R
    from raytrace_amd import material as M
    for fn, kw in [(scenes.cornell_box, dict(spp=1, width=8)), (scenes.pawn_fog, dict(spp=1, width=8)),
                   (scenes.instance_gallery, dict(spp=1, width=8))]:
        cs, world, seed = fn(**kw)
        a, b = R.flatten(world), R.flatten(denoise.emitter_twin(world))
        assert len(a.prims) == len(b.prims) and len(a.media) == len(b.media) and len(a.instances) == len(b.instances)
        assert np.array_equal(a.prims, b.prims)  # the same leaves, orders and gids
        assert (np.asarray(b.materials)["kind"] == M.LIGHT).all()
    tw = denoise.emitter_twin(M.dielectric(1.5) << R.sphere((0, 0, 0), 1.0))
    assert tw.material.kind == M.LIGHT and tuple(tw.material.texture.c0) == (1.0, 1.0, 1.0)
    tw = denoise.emitter_twin(M.pitchBlack << R.sphere((0, 0, 0), 1.0))
    assert tw.material.kind == M.LIGHT and tuple(tw.material.texture.c0) == (0.0, 0.0, 0.0)


# ---- the feature body's host build against the FP64 oracle (tests/feature_emu)

def assert_parity64(img, ref, what, spp, lmax=1.0):
    """tests/test_gpu.py's binary64 bar for small renders: >= 99.9 % of pixels within 1e-9 relative
    (max(|ref|, 1e-3) scale), the worst pixel within 2 L / spp, the mean colour within 5e-3."""
    assert img.shape == ref.shape and np.isfinite(img).all(), what
    d = np.abs(img - ref)
    rel = (d / np.maximum(np.abs(ref), 1e-3)).max(-1)
    frac = float((rel <= 1e-9).mean())
    assert frac >= 0.999, (what, frac)
    assert d.max() <= 2 * lmax / spp, (what, float(d.max()))
    np.testing.assert_allclose(img.reshape(-1, 3).mean(0), ref.reshape(-1, 3).mean(0), rtol=5e-3, atol=1e-6)


FEATURE_SCENES = [("cornell_box", dict(width=24)), ("box_gallery", dict(width=24)), ("noise_test", dict(width=24)),
                  ("instance_gallery", dict(width=24)), ("bunny_cornell", dict(width=24))]


@pytest.mark.parametrize("name,kw", FEATURE_SCENES, ids=[c[0] for c in FEATURE_SCENES])
def test_host_feature_albedo_matches_oracle_emitter_twin(oracle_mod, name, kw):
    """The feature body (rt_features.h over rt_trace.h, RT_HOST_EMU, binary64) at n_feat = 4: its
    albedo is the oracle's 4-spp Philox render of emitter_twin(world) — the same primary rays, first
    hits, uvs, textures and instances, with every first hit emitting its albedo."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "feature_emu"))
    import feature_emu
    cs, world, seed = getattr(scenes, name)(spp=4, **kw)
    words = feature_emu.features(cs, world, seed, 4, precision="f64")
    f = denoise.features_from_words(words, 4)
    ref = oracle_mod.render(cs, denoise.emitter_twin(world), seed, mode=oracle_mod.RNG_PHILOX)
    assert_parity64(f["albedo"], ref, name, 4)
    hit = f["coverage"] > 0
    assert hit.any() and (f["depth"][hit] > 0).all() and (f["depth"][~hit] == 0).all()
    nlen = np.linalg.norm(f["normal"], axis=-1)
    assert (nlen <= f["coverage"] + 1e-6).all()  # a mean of unit vectors over the samples that hit


# ---- symbols and argument checks

NEW = ["rt_denoise_default_params", "rt_denoise_features", "rt_denoise_features_read", "rt_denoise_albedo",
       "rt_denoise_albedo_read", "rt_denoise_film",
       "rt_denoise_film_read"]


def test_denoise_symbols_are_exported():
    L = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    for n in NEW:
        assert n in _lib.EXPORTED and hasattr(L, n) and f" T {n}\n" in out.stdout, n
    hdr = open(os.path.join(ROOT, "include", "rt.h")).read()
    assert "#define RT_ABI_VERSION 6" in hdr and "typedef struct rt_denoise_params" in hdr
    assert L.rt_abi_version() == _lib.ABI_VERSION == 6
    import raytrace_amd as R
    assert R.denoise_reference is denoise.denoise_reference and R.emitter_twin is denoise.emitter_twin
    assert hasattr(R.Film, "features") and hasattr(R.Film, "denoised")


def test_denoise_argument_checks_need_no_device(tmp_path):
    """Null arguments return RT_E_INVALID before any device call, and the default parameters are
    the documented ones (the C struct's layout is the ctypes one)."""
    L = _lib.load()
    p = _lib.RtDenoiseParams()
    assert L.rt_denoise_default_params(None) == _lib.RT_E_INVALID
    assert L.rt_denoise_default_params(ctypes.byref(p)) == _lib.RT_OK
    assert {k: getattr(p, k) for k in denoise.DEFAULT_PARAMS} == denoise.DEFAULT_PARAMS
    buf = (ctypes.c_char * 64)()
    n = ctypes.c_int32()
    for rc in (L.rt_denoise_features(None, 8, None), L.rt_denoise_features_read(None, buf, ctypes.byref(n)),
               L.rt_denoise_albedo(None, 64, None), L.rt_denoise_albedo_read(None, buf, ctypes.byref(n)),
               L.rt_denoise_film(None, ctypes.byref(p), buf, None), L.rt_denoise_film_read(None, ctypes.byref(p), buf)):
        assert rc == _lib.RT_E_INVALID
        assert b"null" in L.rt_last_error()
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(rt_denoise_params), offsetof(rt_denoise_params, k),\n'
                   '         offsetof(rt_denoise_params, sigma_z), offsetof(rt_denoise_params, sigma_a),\n'
                   '         offsetof(rt_denoise_params, eps_l));\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    D = _lib.RtDenoiseParams
    assert got == [ctypes.sizeof(D), D.k.offset, D.sigma_z.offset, D.sigma_a.offset, D.eps_l.offset] == [56, 4, 8, 24, 48]
    with pytest.raises(TypeError):
        denoise.resolve_params(dict(sigma=1.0))
