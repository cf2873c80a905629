"""Progressive rendering: a `Film` keeps a frame's accumulation state on the GPU (include/rt.h
rt_film_*), so samples can be added to it in passes, the image read at any time, the noise
estimated and the state saved and restored.

The sample index is a word of the Philox counter and the per-pixel sums are integers, so passes
of a, b, c samples give exactly the image of `raytrace` at a + b + c samples per pixel.

    film = Film(world, settings, seed)
    film.add(8); preview = film.image()
    while film.passes < 2 or film.noise() > 0.02:
        film.add(16)
    state = film.state()            # a numpy uint8 array: np.save it, film.restore it later

`raytrace_until` is that loop as one call.  `noise_from_sums` restates the estimator in numpy.
`film.denoised()` is the image filtered for a preview and `film.features()` its guide buffers
(raytrace_amd.denoise).  `film.add_where(n, threshold)` adds samples only to the pixels whose own
noise estimate is above a threshold (an adaptive pass; `film.sample_map()` is the per-pixel count,
`raytrace_until(..., adaptive=True)` the loop, `noise_from_counts` the estimator with per-pixel
counts in numpy).  `MultiFilm(world, settings, seed, devices=[0, 1, ...])` is the same film
rendered by several GPUs into one frame; `raytrace_until(..., devices=[...])` runs on it.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib
from .camera import CameraSettings
from .ray import DeviceScene, _seed64

MAX_SAMPLES = 1 << 24  # per pixel and film (rt_film.h RT_FILM_MAX_SAMPLES)
FLOOR = 3.0 / 256.0    # one 8-bit code per channel: below it a relative error cannot be shown


class Film:
    """The resident accumulation state of one (scene, camera, seed, precision, shard) on one GPU.

    `world`: a scene description (uploaded here, freed by close()) or a DeviceScene (the caller's:
    it must outlive the film).  `settings.cs_samplesPerPixel` is validated and otherwise ignored:
    the film's sample count `.spp` is what has been added in `.passes` passes.  With n_shards > 1
    the film holds that shard's tile (rt_exec row interleave; `render_shard`'s rows)."""

    def __init__(self, world, settings: CameraSettings, seed, precision: str = "f64", device: int = 0,
                 n_shards: int = 1, shard: int = 0, row_block: int = 4):
        self._lib = _lib.load()
        self.handle = None
        self._own_scene = not isinstance(world, DeviceScene)
        self.scene = DeviceScene(world, device) if self._own_scene else world
        self._create(settings, seed, precision, self.scene.device, dict(n_shards=n_shards, shard=shard, row_block=row_block))

    def _create(self, settings, seed, precision, device, exec_kw):
        """The part of construction every kind of film shares: the camera and rt_exec records, the
        library handle(s) from `_new_film(seed64)` (the film's own scene is closed again if that
        fails) and the attributes the reading methods use."""
        self.device = device  # where the state lives (torch buffers of noise_map)
        self.settings = settings
        self.precision = precision
        try:
            self.dtype = _lib.dtype_of(precision)
            self._cs = _lib.camera_struct(settings)
            self._ex = _lib.exec_struct(device=device, precision=precision, **exec_kw)
            self._new_film(_seed64(seed))
        except Exception:
            if self._own_scene:
                self.scene.close()
            raise
        info = self.info()
        self.shape = (info["rows"], info["width"], 3)
        self._feature_samples = 0  # n of the feature words on the device (0: not computed)
        self._albedo_samples = 0   # ... of the remodulation albedo (0: none)

    def _new_film(self, seed64):
        h = ctypes.c_void_p()
        _lib.check(self._lib.rt_film_create(self.scene.handle, ctypes.byref(self._cs), seed64, ctypes.byref(self._ex),
                                            ctypes.byref(h)))
        self.handle = h

    def _ready(self):
        """Before a read.  A plain film's reads follow its last add by stream order: nothing to do."""

    def info(self) -> dict:
        st = _lib.RtFilmInfo()
        _lib.check(self._lib.rt_film_get_info(self.handle, ctypes.byref(st)))
        return dict(samples=st.samples, passes=st.passes, width=st.width, rows=st.rows, nan_pixels=st.nan_pixels,
                    f32=bool(st.f32))

    @property
    def spp(self) -> int:
        return self.info()["samples"]

    @property
    def passes(self) -> int:
        return self.info()["passes"]

    def add(self, n: int, stream_ptr: int = 0):
        """Enqueue samples [spp, spp + n) of every pixel (asynchronous; returns self)."""
        _lib.check(self._lib.rt_film_add(self.handle, int(n), ctypes.c_void_p(stream_ptr or None)))
        return self

    def add_where(self, n: int, threshold: float, max_spp: int | None = None, stream_ptr: int = 0):
        """Enqueue an adaptive pass (rt_adaptive_add; asynchronous; returns self): samples [N_p, N_p + n)
        of every pixel that counts (inside the frame, not NaN-flagged), whose relative error
        (noise_from_counts: noise_map's value in binary64) is > threshold and whose count N_p + n stays
        within max_spp (None: the film's limit, 2^24).  A negative threshold selects every such pixel.
        The film needs two passes.  From the first call on the film is non-uniform: .spp and .passes
        are the per-pixel maxima, sample_map() the counts, state() layout version 2, add() and
        denoised() raise (RtInvalid / RtUnsupported) until reset().  A selected pixel's colour is bit
        for bit a uniform film's at its count; selection reads the pixel's own earlier samples, so
        the adaptive mean carries the usual small adaptive-sampling bias, which nothing corrects."""
        _lib.check(self._lib.rt_adaptive_add(self.handle, int(n), float(threshold), int(max_spp or 0),
                                             ctypes.c_void_p(stream_ptr or None)))
        return self

    def counts(self) -> np.ndarray:
        """(rows, width, 2) uint32: each pixel's samples N_p and passes K_p ((spp, passes) on a uniform
        film; (0, 0) on a shard's padding rows)."""
        self._ready()
        c = np.zeros(self.shape[:2] + (2,), np.uint32)
        _lib.check(self._lib.rt_adaptive_counts_read(self.handle, c.ctypes.data_as(ctypes.c_void_p)))
        return c

    def sample_map(self) -> np.ndarray:
        """(rows, width) uint32: the samples each pixel holds."""
        return np.ascontiguousarray(self.counts()[..., 0])

    def selection(self) -> np.ndarray:
        """The tile pixels (row * width + column, ascending) the last add_where selected: int32."""
        self._ready()
        n = ctypes.c_int64()
        _lib.check(self._lib.rt_adaptive_selection_read(self.handle, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, np.int32)
        if n.value:
            _lib.check(self._lib.rt_adaptive_selection_read(self.handle, out.ctypes.data_as(ctypes.c_void_p), n.value,
                                                            ctypes.byref(n)))
        return out

    def adaptive_info(self) -> dict:
        """total_samples (over the pixels that count), min_samples, max_samples, selected (by the last
        add_where), adaptive_passes and nonuniform (rt_adaptive_get_info)."""
        self._ready()
        st = _lib.RtAdaptiveInfo()
        _lib.check(self._lib.rt_adaptive_get_info(self.handle, ctypes.byref(st)))
        return dict(total_samples=st.total_samples, min_samples=st.min_samples, max_samples=st.max_samples,
                    selected=st.selected, adaptive_passes=st.adaptive_passes, nonuniform=bool(st.nonuniform))

    def image(self, out: np.ndarray | None = None) -> np.ndarray:
        """The mean of the samples so far: (rows, width, 3) linear RGB, as `raytrace` at .spp (a
        non-uniform film: each pixel as `raytrace` at its own count)."""
        from .ray import _out_buffer
        self._ready()
        out = _out_buffer(out, self.shape, self.dtype)
        _lib.check(self._lib.rt_film_read(self.handle, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def noise(self) -> float:
        """sqrt(mean r^2) of the per-pixel relative standard error r (noise_map); needs two passes."""
        self._ready()
        v = ctypes.c_double()
        _lib.check(self._lib.rt_film_noise(self.handle, None, ctypes.byref(v)))
        return v.value

    def noise_map(self) -> np.ndarray:
        """(rows, width) float32: each pixel's relative standard error of its mean R + G + B against
        max(mean, 3/256); NaN for pixels with a non-finite sample and a shard's padding rows."""
        import torch
        self._ready()
        m = torch.empty(self.shape[0] * self.shape[1], dtype=torch.float32, device=f"cuda:{self.device}")
        v = ctypes.c_double()
        _lib.check(self._lib.rt_film_noise(self.handle, ctypes.c_void_p(m.data_ptr()), ctypes.byref(v)))
        return m.cpu().numpy().reshape(self.shape[:2])

    def feature_words(self, n: int = 8, stream_ptr: int = 0) -> np.ndarray:
        """The first-hit feature pass over samples [0, n) of every pixel (rt_denoise_features; run
        again only when n changes) and its integer words: (rows, width, 8) int64 — albedo RGB, normal
        xyz and the depth sum in units of 2^-32, and the hit count —, in a binary64 film (rows, width,
        16): those, then the next 32 bits of each sum (denoise.features_from_words)."""
        self._ready()
        if self._feature_samples != int(n):
            self._feature_samples = 0
            _lib.check(self._lib.rt_denoise_features(self.handle, int(n), ctypes.c_void_p(stream_ptr or None)))
            self._feature_samples = int(n)
        words = np.zeros(self.shape[:2] + (8 if self.precision == "f32" else 16,), np.int64)
        got = ctypes.c_int32()
        _lib.check(self._lib.rt_denoise_features_read(self.handle, words.ctypes.data_as(ctypes.c_void_p), ctypes.byref(got)))
        assert got.value == self._feature_samples
        return words

    def features(self, n: int = 8) -> dict:
        """The guide buffers of the primary rays of samples [0, n): `albedo` (rows, width, 3) — the
        first hit's texture (1 for dielectric, 0 for pitchBlack, the background on a miss) —,
        `normal` (rows, width, 3) — the mean unit normal facing the ray (0 in a medium or on a miss) —,
        `depth` (rows, width) — the mean hit distance over the samples that hit — and `coverage`
        (rows, width), the fraction that hit.  A function of scene, camera and seed: adding samples
        to the film does not change them, and they are not part of state()."""
        from .denoise import features_from_words
        return features_from_words(self.feature_words(n), n)

    def albedo(self, n: int = 64) -> np.ndarray:
        """The remodulation albedo (rt_denoise_albedo): the first-hit albedo over samples [0, n),
        (rows, width, 3).  The filter divides the colour by features()'s albedo — the film's own first
        samples, whose coverage noise at an emitter's or a texture's edge cancels in the quotient — and
        multiplies the result by this better estimate.  Computed once: it does not change as samples
        are added."""
        from .denoise import features_from_words
        self._ready()
        if self._albedo_samples != int(n):
            self._albedo_samples = 0
            _lib.check(self._lib.rt_denoise_albedo(self.handle, int(n), None))
            self._albedo_samples = int(n)
        words = np.zeros(self.shape[:2] + (8 if self.precision == "f32" else 16,), np.int64)
        got = ctypes.c_int32()
        _lib.check(self._lib.rt_denoise_albedo_read(self.handle, words.ctypes.data_as(ctypes.c_void_p), ctypes.byref(got)))
        assert got.value == self._albedo_samples
        return features_from_words(words, n)["albedo"]

    def denoised(self, out: np.ndarray | None = None, levels: int = 5, feature_samples: int = 8, albedo_samples: int = 64,
                 **params) -> np.ndarray:
        """The image filtered by the variance-guided denoiser (raytrace_amd.denoise; rt_denoise_film):
        (rows, width, 3) in the film's dtype.  Needs two passes (the variance estimate) and a film of
        n_shards = 1 (RtUnsupported otherwise: a shard's rows are interleaved with the others').
        Computes the features (feature_samples: at most the film's samples, so that colour and albedo
        share their first samples) and the remodulation albedo (albedo_samples; see albedo()) if they
        are missing.  params: k, sigma_z, sigma_l, sigma_a, eps_n, eps_z, eps_l
        (denoise.DEFAULT_PARAMS)."""
        from .denoise import params_struct
        from .ray import _out_buffer
        p = params_struct(params, levels=levels)
        self._ready()
        if self._feature_samples != int(feature_samples):
            self._feature_samples = 0
            _lib.check(self._lib.rt_denoise_features(self.handle, int(feature_samples), None))
            self._feature_samples = int(feature_samples)
        if self._albedo_samples != int(albedo_samples):
            self._albedo_samples = 0
            _lib.check(self._lib.rt_denoise_albedo(self.handle, int(albedo_samples), None))
            self._albedo_samples = int(albedo_samples)
        out = _out_buffer(out, self.shape, self.dtype)
        _lib.check(self._lib.rt_denoise_film_read(self.handle, ctypes.byref(p), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def state(self) -> np.ndarray:
        """The film's state as bytes (header, sums, flags, estimator words): see `unpack_state`."""
        self._ready()
        n = ctypes.c_int64()
        _lib.check(self._lib.rt_film_state_bytes(self.handle, ctypes.byref(n)))
        buf = np.zeros(n.value, np.uint8)
        _lib.check(self._lib.rt_film_save(self.handle, buf.ctypes.data_as(ctypes.c_void_p), n.value))
        return buf

    def restore(self, state: np.ndarray):
        """Load a state saved from a film of the same frame, seed, precision and shard (the header is
        checked; that scene and camera are the same is the caller's responsibility)."""
        buf = np.ascontiguousarray(state, np.uint8)
        _lib.check(self._lib.rt_film_load(self.handle, buf.ctypes.data_as(ctypes.c_void_p), buf.size))
        return self

    def reset(self):
        _lib.check(self._lib.rt_film_reset(self.handle))
        return self

    def close(self):
        if self.handle:
            self._lib.rt_film_destroy(self.handle)
            self.handle = None
            if self._own_scene:
                self.scene.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiFilm(Film):
    """A film over a list of GPUs of this process (include/rt.h rt_multi_film_*): `Film`'s interface,
    one frame.  Shard k of every pass renders on devices[k] (rows dealt round-robin in blocks of
    `row_block`, as `raytrace(..., devices=...)`) and is merged straight into ONE accumulation state
    on devices[0], which is bit for bit the state of a plain `Film` after the same passes: images,
    noise figures, feature buffers and denoised images are equal, and `state()` / `restore()`
    interchange with a plain `Film(..., row_block=row_block)` of the same frame, whatever the device
    counts.  The feature and albedo passes (first hits only) run on devices[0].  Every reading method
    first waits for every device (rt_multi_film_frame), so a traversal-stack overflow on any device
    is raised by whichever is called.

    `world`: a scene description (uploaded to `devices`, default every GPU; freed by close()) or a
    MultiDeviceScene (the caller's: it must outlive the film).  A device may repeat."""

    def __init__(self, world, settings: CameraSettings, seed, devices=None, precision: str = "f64", row_block: int = 4):
        from .errors import RtInvalid
        from .ray import MultiDeviceScene
        self._lib = _lib.load()
        self.handle = None   # the frame: an ordinary one-shard film, owned by the multi film
        self._multi = None
        self._own_scene = not isinstance(world, MultiDeviceScene)
        if not self._own_scene and devices is not None and [int(d) for d in devices] != world.devices:
            raise RtInvalid(f"the scene is resident on devices {world.devices}, not {list(devices)}")
        if self._own_scene and devices is None:
            devices = list(range(_lib.check(self._lib.rt_device_count())))
        self.scene = MultiDeviceScene(world, devices) if self._own_scene else world
        self.devices = list(self.scene.devices)
        self._create(settings, seed, precision, self.devices[0], dict(row_block=row_block))

    def _new_film(self, seed64):
        m = ctypes.c_void_p()
        _lib.check(self._lib.rt_multi_film_create(self.scene.handle, ctypes.byref(self._cs), seed64, ctypes.byref(self._ex),
                                                  ctypes.byref(m)))
        self._multi = m
        self._frame()

    def _frame(self):
        """Wait for every device and take the frame handle (rt_multi_film_frame: raises on a
        traversal-stack overflow on any device)."""
        h = ctypes.c_void_p()
        rc = self._lib.rt_multi_film_frame(self._multi, ctypes.byref(h))
        self.handle = h
        _lib.check(rc)

    def add(self, n: int):
        """Enqueue samples [spp, spp + n) of every pixel on every device (asynchronous; returns self)."""
        _lib.check(self._lib.rt_multi_film_add(self._multi, int(n)))
        return self

    def add_where(self, n, threshold, max_spp=None, stream_ptr=0):
        from .errors import RtInvalid
        raise RtInvalid("adaptive passes run on a one-device Film, not on a MultiFilm")

    _ready = _frame  # every read (image, noise, state, features, denoised) reports every device's status

    @property
    def copied_passes(self) -> int:
        """Shard passes so far whose sums reached devices[0] through the staging copy (devices
        without peer access to it; 0 otherwise)."""
        n = ctypes.c_int64()
        _lib.check(self._lib.rt_multi_film_copies(self._multi, ctypes.byref(n)))
        return n.value

    def restore(self, state: np.ndarray):
        """Load a state saved from a MultiFilm (of any device list) or a plain one-shard Film of the
        same frame, seed, precision and row_block."""
        buf = np.ascontiguousarray(state, np.uint8)
        _lib.check(self._lib.rt_multi_film_load(self._multi, buf.ctypes.data_as(ctypes.c_void_p), buf.size))
        return self

    def reset(self):
        _lib.check(self._lib.rt_multi_film_reset(self._multi))
        return self

    def close(self):
        if self._multi:
            self._lib.rt_multi_film_destroy(self._multi)
            self._multi = None
            self.handle = None
            if self._own_scene:
                self.scene.close()


HEADER_DTYPE = np.dtype([("magic", "<u4"), ("version", "<u4"), ("f32", "<i4"), ("width", "<i4"), ("height", "<i4"),
                         ("rows", "<i4"), ("n_shards", "<i4"), ("shard", "<i4"), ("row_block", "<i4"),
                         ("passes", "<i4"), ("key0", "<u4"), ("key1", "<u4"), ("samples", "<i8"), ("reserved", "<i8")])


def unpack_state(state: np.ndarray) -> dict:
    """A saved state's parts: `header` (HEADER_DTYPE record), `sums` (rows, width, words) int64 — 3
    words per pixel in FP32 (the RGB sums in units of 2^-32), 6 in binary64 (those, then the next
    32 bits of each) —, `flags` (rows, width) uint32 and `q` (rows, width) float64.  A non-uniform
    film's state (layout version 2; header samples / passes: the per-pixel maxima) also has `counts`
    (rows, width, 2) uint32, each pixel's samples and passes."""
    state = np.ascontiguousarray(state, np.uint8)
    hd = state[:HEADER_DTYPE.itemsize].view(HEADER_DTYPE)[0]
    rows, width, words = int(hd["rows"]), int(hd["width"]), 3 if hd["f32"] else 6
    n = rows * width
    o = HEADER_DTYPE.itemsize
    sums = state[o:o + 8 * n * words].view("<i8").reshape(rows, width, words)
    o += 8 * n * words
    flags = state[o:o + 4 * n].view("<u4").reshape(rows, width)
    o += 4 * n
    q = state[o:o + 8 * n].view("<f8").reshape(rows, width)
    o += 8 * n
    out = dict(header=hd, sums=sums, flags=flags, q=q)
    if int(hd["version"]) >= 2:
        out["counts"] = state[o:o + 8 * n].view("<u4").reshape(rows, width, 2)
    return out


def noise_from_counts(sums, q, counts) -> np.ndarray:
    """The per-pixel relative error of a film with per-pixel counts, in numpy and binary64: the
    operation sequence of rt_film.h rt_film_rel_error over a state's words (`unpack_state`: `sums`
    (..., words) int64, `q` (...) float64, `counts` (..., 2) — N_p, K_p; for a uniform state
    np.broadcast_to((samples, passes), q.shape + (2,))).  It is the value Film.noise_map shows as
    float32 and the one Film.add_where compares: a pixel that counts is selected iff r > threshold.
    NaN where a pixel holds no samples or fewer than two passes."""
    sums = np.asarray(sums, np.int64)
    q = np.asarray(q, np.float64)
    counts = np.asarray(counts)
    N = counts[..., 0].astype(np.float64)
    K = counts[..., 1].astype(np.float64)
    T = (sums[..., 0] + sums[..., 1] + sums[..., 2]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = q - (T * T) / N
        v = np.where(d > 0.0, d, 0.0) / (K - 1.0)
        se = np.sqrt(v / N) * 2.0 ** -32
        M = T / N * 2.0 ** -32
        r = se / np.where(M > FLOOR, M, FLOOR)
    return np.where((counts[..., 0] > 0) & (counts[..., 1] >= 2), r, np.nan)


def noise_from_sums(pass_sums, pass_sizes) -> dict:
    """The film's noise estimate from per-pass sums, in numpy (the operation sequence of rt_film.h).

    pass_sums: integer array (K, ..., 3): per pass and pixel the RGB sums of that pass's samples in
    the film's fixed-point unit 2^-32 (the first three words of `unpack_state(...)["sums"]`,
    differenced between passes).  pass_sizes: the K sample counts.  Returns q, the per-sample
    variance v (batch means: E[sum_k n_k (m_k - M)^2] = (K - 1) sigma^2 for any sizes) in squared
    fixed-point units, the pixel mean M and its standard error se (both in radiance units), the
    relative error r = se / max(M, 3/256) and the frame figure noise = sqrt(mean r^2)."""
    sums = np.asarray(pass_sums, np.int64)
    sizes = [int(n) for n in pass_sizes]
    K = len(sizes)
    if K < 2 or sums.shape[0] != K or sums.shape[-1] != 3 or min(sizes) <= 0:
        raise ValueError("noise_from_sums needs K >= 2 passes of positive sizes and sums of shape (K, ..., 3)")
    N = float(sum(sizes))
    q = np.zeros(sums.shape[1:-1], np.float64)
    for k in range(K):
        L = sums[k].sum(-1, dtype=np.int64).astype(np.float64)
        q = q + (L * L) / float(sizes[k])
    T = sums.sum(0, dtype=np.int64).sum(-1, dtype=np.int64).astype(np.float64)
    v = np.maximum(0.0, q - (T * T) / N) / float(K - 1)
    se = np.sqrt(v / N) * 2.0 ** -32
    M = T / N * 2.0 ** -32
    r = se / np.maximum(M, FLOOR)
    noise = math.sqrt(math.fsum((r * r).ravel().tolist()) / r.size) if r.size else float("nan")
    return dict(q=q, v=v, se=se, mean=M, r=r, noise=noise)


def raytrace_until(settings: CameraSettings, world, seed, noise: float, batch: int = 16, max_spp: int | None = None,
                   denoise: bool = False, denoise_params: dict | None = None, devices=None, adaptive: bool = False, **kw):
    """Render in passes of `batch` samples until the frame's noise figure (Film.noise) is at most
    `noise` (checked from the second pass on) or `max_spp` samples per pixel are reached (default
    cs_samplesPerPixel; the last pass is cut to fit).  Returns (image, info): the image is
    `raytrace`'s at info["spp"] samples; info has spp, passes, noise (None before two passes) and
    converged.  denoise=True returns the denoised image instead (Film.denoised with denoise_params;
    it needs two passes: max_spp > batch) and keeps the raw one in info["raw"].  kw: Film's
    precision, device, n_shards, shard, row_block.  `devices`: a list of GPUs that render the passes
    together (a MultiFilm; kw: precision, row_block); image and info are the one-device call's.

    adaptive=True: convergence is per pixel.  Two uniform passes of `batch`, then adaptive passes
    (Film.add_where(batch, noise, max_spp)) until one selects nothing: every pixel that counts then
    has a relative error <= noise or is within `batch` of max_spp.  Each pixel is `raytrace`'s at its
    own count; info["spp"] is the largest count and info gains spp_mean, spp_max, selected (the
    pixels each adaptive pass took), sample_map and rel_error (noise_from_counts of the final state; NaN
    where a pixel does not count); converged: no pixel was stopped by max_spp.
    Needs max_spp > batch; with denoise=True or devices= it raises RtInvalid."""
    from .errors import RtInvalid
    if batch <= 0:
        raise RtInvalid("batch must be positive")
    max_spp = int(settings.cs_samplesPerPixel if max_spp is None else max_spp)
    if adaptive:
        if denoise or devices is not None:
            raise RtInvalid("adaptive=True runs on one device and returns the raw image (no denoise=, no devices=)")
        if max_spp <= batch:
            raise RtInvalid("adaptive=True needs two uniform passes first: max_spp > batch")
        with Film(world, settings, seed, **kw) as film:
            film.add(batch).add(min(batch, max_spp - batch))
            selected = []
            while True:
                film.add_where(batch, noise, max_spp)
                took = film.adaptive_info()["selected"]
                if took == 0:
                    break
                selected.append(took)
            st = unpack_state(film.state())
            r = noise_from_counts(st["sums"], st["q"], st["counts"])
            counting = (st["flags"] == 0) & (st["counts"][..., 0] > 0)
            ai = film.adaptive_info()
            info = dict(spp=ai["max_samples"], passes=film.passes, noise=film.noise(),
                        converged=not bool(np.any(r[counting] > noise)), spp_max=ai["max_samples"],
                        spp_mean=ai["total_samples"] / max(1, int(counting.sum())), selected=selected,
                        sample_map=st["counts"][..., 0].copy(), rel_error=np.where(counting, r, np.nan))
            return film.image(), info
    with (Film(world, settings, seed, **kw) if devices is None else
          MultiFilm(world, settings, seed, devices=devices, **kw)) as film:
        spp, passes, figure, converged = 0, 0, None, False
        while spp < max_spp:
            n = min(batch, max_spp - spp)
            film.add(n)
            spp, passes = spp + n, passes + 1
            if passes >= 2:
                figure = film.noise()
                if figure <= noise:
                    converged = True
                    break
        info = dict(spp=spp, passes=passes, noise=figure, converged=converged)
        if denoise:
            info["raw"] = film.image()
            return film.denoised(**(denoise_params or {})), info
        return film.image(), info
