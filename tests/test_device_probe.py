"""Unit-level probes of rt_trace.h: the kernel's own math macros, primitive tests, fixed-point
conversion and Philox called element-wise (tests/device_probe), on the host emulator (backend
"emu", no GPU) and on the device (backend "gpu"), against exact (Python int / Fraction-style
integer arithmetic) or numpy long-double references.  The image tests bound these functions only
statistically; a probe fails on one wrong input.

Where the figures come from: no bar in this module was measured on a GPU.  The binary64 bars are
the project's own record (profiles/r2/f64_math_check.json) and the comments of rt_trace.h; the
binary64 sin / cos bar is from a CPU restatement of the algorithm; the FP32 bars are what the
consumer of each value needs (stated at each test).  The worst errors each backend reached are
written with conftest.record_measure("device_probe", ...) and kept in profiles/probe/."""
import functools
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT, record_measure

sys.path.insert(0, os.path.join(ROOT, "tests", "device_probe"))
import probe  # noqa: E402
from test_node_test import exact_accept, make_cases  # noqa: E402

LD = np.longdouble
BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
backends = pytest.mark.parametrize("backend", BACKENDS)
both_precisions = pytest.mark.parametrize("precision", ["f32", "f64"])
TWO_PI_LD = 2 * LD("3.14159265358979323846264338327950288419716939937510")
P52 = 2.0 ** -52
N24 = 1 << 24


def run(backend, precision, name, *inputs):
    if backend == "gpu":
        import torch
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return probe.call(backend, precision, name, *inputs)


def real_of(precision):
    return np.float64 if precision == "f64" else np.float32


def measure(backend, what, **figures):
    record_measure("device_probe", dict(backend=backend, probe=what, **figures))


def ulp_distance(a, b):
    """|a - b| in units in the last place for finite floats of one dtype (sign-magnitude order)."""
    it = np.int64 if a.dtype == np.float64 else np.int32
    def key(x):
        i = x.view(it).astype(np.int64) if it is np.int32 else x.view(it)
        return np.where(i < 0, np.iinfo(it).min - i, i)
    return np.abs(key(np.ascontiguousarray(a)) - key(np.ascontiguousarray(b)))


def same_bits(a, b):
    it = np.uint64 if a.dtype == np.float64 else np.uint32
    return np.ascontiguousarray(a).view(it) == np.ascontiguousarray(b).view(it)


# ------------------------------------------------------------------ the build
def _hipflags(path):
    text = open(path).read().replace("\\\n", " ")
    m = re.search(r"^HIPFLAGS\s*:=\s*(.*)$", text, re.M)
    return m.group(1).split()


def test_probe_hipflags_match_product():
    """The probes are compiled with the product's HIPFLAGS, word for word: the denormal flush,
    -O3 and the contraction default are part of what they test."""
    product = _hipflags(os.path.join(ROOT, "raytrace_amd", "csrc", "Makefile"))
    mine = _hipflags(os.path.join(ROOT, "tests", "device_probe", "Makefile"))
    assert mine == product
    for flag in ("-O3", "-fno-slp-vectorize", "-munsafe-fp-atomics", "-fgpu-flush-denormals-to-zero"):
        assert flag in mine


# ------------------------------------------------------------------ a. binary64 device math
@functools.lru_cache(None)
def math64_inputs():
    rng = np.random.default_rng(64)
    n = 1 << 20
    x = np.ldexp(1.0 + rng.random(n), rng.integers(-40, 41, n))
    k = rng.integers(1, 1 << 26, 1 << 12).astype(np.float64)
    squares = np.concatenate([k * k, np.ldexp(k * k, rng.integers(-40, 40, k.size) * 2), [1.0, 4.0, 0.25]])
    tiny = np.finfo(np.float64).tiny
    edge_pos = np.array([tiny, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 1.0])
    return x, squares, edge_pos


@backends
def test_f64_rcp_bit_equal_to_ieee_division(backend):
    """rt_math64::rcp: bit-equal to IEEE 1 / x (rt_trace.h: "bit-identical to IEEE division";
    profiles/r2/f64_math_check.json rcp max_ulp 0), +-0 -> +-inf, +-inf -> +-0, NaN -> NaN.
    Measured (profiles/probe/device_probe.jsonl): 0 ulp on the MI355X and on the emulator."""
    x, squares, edge = math64_inputs()
    v = np.concatenate([x, -x[:4096], squares, edge, -edge, [0.0, -0.0, np.inf, -np.inf, np.nan]])
    got, = run(backend, "f64", "math1", 0, v)
    with np.errstate(divide="ignore"):
        want = 1.0 / v
    nan = np.isnan(want)
    measure(backend, "f64_rcp", n=int(v.size), worst_ulp=int(ulp_distance(got[~nan], want[~nan]).max()))
    assert np.isnan(got[nan]).all()
    assert same_bits(got[~nan], want[~nan]).all()


@backends
def test_f64_rcp_nz_within_one_ulp(backend):
    """rt_math64::rcp_nz on finite non-zero x: within 1 ulp of 1 / x (nothing is asserted at 0 and
    inf, where it is documented to give NaN).  Measured: 0 ulp on both backends."""
    x, squares, edge = math64_inputs()
    v = np.concatenate([x, -x[:4096], squares, edge, -edge])
    got, = run(backend, "f64", "math1", 1, v)
    d = ulp_distance(got, 1.0 / v)
    measure(backend, "f64_rcp_nz", n=int(v.size), worst_ulp=int(d.max()))
    assert np.isfinite(got).all() and d.max() <= 1


@backends
def test_f64_sqrt_bit_equal_to_ieee(backend):
    """rt_math64::sqrt_nonneg: bit-equal to the IEEE square root (f64_math_check.json sqrt max_ulp 0),
    including exact squares, +-0 and +inf.  Measured: 0 ulp on both backends."""
    x, squares, edge = math64_inputs()
    v = np.concatenate([x, squares, edge, [0.0, -0.0, np.inf]])
    got, = run(backend, "f64", "math1", 2, v)
    want = np.sqrt(v)
    measure(backend, "f64_sqrt", n=int(v.size), worst_ulp=int(ulp_distance(got, want).max()))
    assert same_bits(got, want).all()
    k = np.arange(1, 4097, dtype=np.float64)
    got, = run(backend, "f64", "math1", 2, k * k)
    assert (got == k).all()


@backends
def test_f64_rsqrt_within_two_ulp(backend):
    """rt_math64::rsqrt: within 2 ulp of the long-double 1 / sqrt(x) (rt_trace.h: "within 2 ulp, as
    two Newton steps were"; f64_math_check.json rsqrt max_ulp 2).  Measured: 0.98 ulp on the MI355X,
    1.48 ulp for the emulator's 1 / sqrt (two roundings)."""
    x, squares, edge = math64_inputs()
    v = np.concatenate([x, squares, edge])
    got, = run(backend, "f64", "math1", 3, v)
    ref = 1 / np.sqrt(v.astype(LD))
    err = np.abs(got.astype(LD) - ref) / np.spacing(ref.astype(np.float64)).astype(LD)
    measure(backend, "f64_rsqrt", n=int(v.size), worst_ulp=float(err.max()))
    assert err.max() <= 2.0


# ------------------------------------------------------------------ b / c. sin, cos of 2 pi u
def uniform_words():
    """Every 24-bit uniform once: u01(w) = k 2^-24 for w = k << 8, in both precisions."""
    return np.arange(N24, dtype=np.uint32) << np.uint32(8)


@functools.lru_cache(None)
def trig_reference(which):
    """sin or cos of 2 pi k 2^-24 in long double (argument and function good to ~4e-19 absolute,
    0.002 of 2^-52), computed once per module."""
    out = np.empty(N24, LD)
    fn = np.sin if which == "sin" else np.cos
    step = 1 << 20
    for a in range(0, N24, step):
        out[a:a + step] = fn(TWO_PI_LD * (np.arange(a, a + step).astype(LD) / LD(N24)))
    return out


@functools.lru_cache(None)
def trig_outputs(backend, precision):
    s, c = run(backend, precision, "sincos", uniform_words())
    return {"sin": s, "cos": c}


@backends
@pytest.mark.parametrize("which", ["sin", "cos"])
def test_f64_sincos_turns_exhaustive(backend, which):
    """rt_math64::sincos_turns over all 2^24 uniforms: absolute error against long double <= 1.5 2^-52.
    Basis: a float64 restatement of the algorithm without FMA reaches 0.92 2^-52 over the same
    inputs; FMA only removes roundings; 1.5 still excludes a wrong coefficient or reduction.
    Measured: 0.689 2^-52 for sin and for cos, the same on the MI355X and on the host build of the
    algorithm (the emulator's own libm macro, sin(fl(2 pi) u), is 3.11 2^-52 off and is not what runs
    here: probe_body.h pb_sincos)."""
    got = trig_outputs(backend, "f64")[which]
    err = np.abs(got.astype(LD) - trig_reference(which))
    worst = float(err.max() / LD(P52))
    measure(backend, "f64_" + which + "_turns", n=N24, worst_abs_in_2m52=worst, at_k=int(err.argmax()))
    assert worst <= 1.5


@backends
def test_f64_sincos_turns_on_the_unit_circle(backend):
    """sin^2 + cos^2 - 1 of the binary64 pair is within 4 2^-52 for every uniform.  Measured: 1.79 2^-52
    on both backends."""
    o = trig_outputs(backend, "f64")
    s, c = o["sin"].astype(LD), o["cos"].astype(LD)
    dev = float(np.abs(s * s + c * c - 1).max() / LD(P52))
    measure(backend, "f64_sincos_norm", worst_in_2m52=dev)
    assert dev <= 4.0


def test_sincos_table_is_correctly_rounded():
    """Every entry of rt_sincos_table.h is the correctly rounded (sin, cos)(2 pi k / 128) (a table
    entry off by one ulp would pass the 1.5 2^-52 bar above) and is what tools/gen_sincos_table.py
    produces."""
    tab = probe.sincos_table()
    assert tab.shape == (128, 2)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_sincos_table as gen
    from decimal import Decimal
    for k in range(128):
        s, c = gen.sin_cos(2 * gen.PI * k / gen.N)
        for got, exact in ((tab[k, 0], s), (tab[k, 1], c)):
            want = 0.0 if abs(exact) < Decimal(10) ** -50 else float(exact)  # the generator's rule
            assert got == want, (k, got, want)
            # correctly rounded: no neighbour is nearer to the 60-digit value
            for nb in (np.nextafter(got, np.inf), np.nextafter(got, -np.inf)):
                assert abs(Decimal(float(got)) - exact) <= abs(Decimal(float(nb)) - exact), (k, got)


@backends
@pytest.mark.parametrize("which", ["sin", "cos"])
def test_f32_sincos_turns_exhaustive(backend, which):
    """RT_SINCOS_TURNS(u01(w)) in FP32 (v_sin_f32 / v_cos_f32 on the device) over all 2^24 uniforms:
    absolute error <= 1e-6, what the consumer needs (test_known_answer_hits' FP32 atol; a sampled
    direction off by 1e-6 is far inside the FP32 per-pixel bar of 1e-3).  Measured
    (profiles/probe/device_probe.jsonl): v_sin_f32 and v_cos_f32 1.25e-7 on the MI355X; sinf / cosf of
    fl(2 pi) u 4.1e-7 / 3.8e-7 on the emulator."""
    got = trig_outputs(backend, "f32")[which]
    err = np.abs(got.astype(LD) - trig_reference(which))
    worst = float(err.max())
    measure(backend, "f32_" + which + "_turns", n=N24, worst_abs=worst, at_k=int(err.argmax()))
    assert worst <= 1e-6


# ------------------------------------------------------------------ c. FP32 device math
@functools.lru_cache(None)
def log_reference():
    """log(1 - k 2^-24) in long double for every k (1 - u is exact in FP32)."""
    out = np.empty(N24, LD)
    step = 1 << 20
    for a in range(0, N24, step):
        out[a:a + step] = np.log((N24 - np.arange(a, a + step)).astype(LD) / LD(N24))
    return out


@backends
def test_f32_free_flight_log_exhaustive(backend):
    """RT_LOG(1 - u01(w)) in FP32 (__logf on the device) for all 2^24 uniforms: the free-flight
    distance neg_inv_density log(1 - u) (medium_draw) must be within 1e-4 relative for every u, a
    tenth of the FP32 per-pixel bar of 1e-3 in test_gpu.py; log(1) = 0 exactly.  The worst
    relative errors for 1 - u >= 0.5 and 1 - u < 0.5 are recorded separately.  Measured: __logf on the
    MI355X 1.83e-7 (1 - u >= 0.5) and 1.88e-7 (1 - u < 0.5), no loss next to 1; logf on the emulator
    7.7e-8 and 6.0e-8."""
    words = uniform_words()
    x, = run(backend, "f32", "uniform", 1, words)
    k = np.arange(N24)
    assert (x.astype(np.float64) == (N24 - k) / N24).all()  # 1 - u is exact, in (0, 1]
    got, = run(backend, "f32", "uniform", 2, words)
    ref = log_reference()
    assert got[0] == 0.0
    rel = np.abs(got[1:].astype(LD) - ref[1:]) / np.abs(ref[1:])
    near = x[1:] >= 0.5
    w_near, w_far = float(rel[near].max()), float(rel[~near].max())
    measure(backend, "f32_log_1mu", n=N24, worst_rel_ge_half=w_near, worst_rel_lt_half=w_far,
            at_k=int(rel.argmax()) + 1)
    assert max(w_near, w_far) <= 1e-4


@backends
def test_f32_sqrt_of_uniform_exhaustive(backend):
    """RT_SQRT(u01(w)) in FP32 over all 2^24 uniforms: within 1 ulp of the correctly rounded square
    root (rt_trace.h: "v_sqrt_f32 (1 ulp)"); sqrt(0) = 0.  Measured: 1 ulp on the MI355X, 0 on the emulator."""
    words = uniform_words()
    u, = run(backend, "f32", "uniform", 0, words)
    assert (u.astype(np.float64) == np.arange(N24) / N24).all()  # u01(w) = (w >> 8) 2^-24
    got, = run(backend, "f32", "uniform", 3, words)
    d = ulp_distance(got, np.sqrt(u))
    measure(backend, "f32_sqrt_u", n=N24, worst_ulp=int(d.max()))
    assert got[0] == 0.0 and d.max() <= 1


def ftz32(x):
    """FP32 denormals as the device sees them under -fgpu-flush-denormals-to-zero: a signed zero."""
    x = np.asarray(x, np.float32)
    den = (np.abs(x) < np.finfo(np.float32).tiny) & (x != 0)
    return np.where(den, np.copysign(np.float32(0), x), x).astype(np.float32)


def expected32(backend, fn, x):
    """The correctly rounded FP32 result under the backend's denormal rule: the device flushes
    denormal inputs and results to zero (the build flag), the host emulator is IEEE."""
    with np.errstate(all="ignore"):
        if backend == "gpu":
            return ftz32(fn(ftz32(x)))
        return fn(np.asarray(x, np.float32)).astype(np.float32)


F32_OPS = {
    "rcp": (0, lambda v: np.float32(1) / v),
    "sqrt": (2, np.sqrt),
    "rsqrt": (3, lambda v: np.float32(1) / np.sqrt(v)),  # (special values only: exact either way)
}


@functools.lru_cache(None)
def f32_log_uniform():
    rng = np.random.default_rng(32)
    n = 1 << 20
    # exponents -125 .. 125: the operand and the result of all three functions are normal
    return np.ldexp(1.0 + rng.random(n), rng.integers(-125, 126, n)).astype(np.float32)


@backends
@pytest.mark.parametrize("op", ["rcp", "sqrt", "rsqrt"])
def test_f32_rcp_sqrt_rsqrt(backend, op):
    """RT_RCP / RT_SQRT / RT_RSQRT in FP32 on 2^20 log-uniform normal floats.  rcp and sqrt: within
    1 ulp of the correctly rounded result (rt_trace.h says "1 ulp" of v_sqrt_f32; test_node_test.py
    rests on 1 ulp for v_rcp_f32).  rsqrt: relative error <= 2^-22 against long double (2 ulp at
    worst: the re-normalised directions of normalize / unit then have |v| = 1 within 4 eps, the
    class of unit_vector's bound below; the emulator's 1 / sqrtf is two correct roundings, at
    most 1.5 ulp).  Special values are exact under the backend's denormal rule: the device flushes
    (denormal inputs count as zero, denormal results become zero), so a change of the build's
    denormal flag fails here.  Measured: v_rcp_f32 and v_sqrt_f32 1 ulp, __frsqrt_rn 1.56 2^-24
    relative on the MI355X; 0 ulp, 0 ulp and 1.50 2^-24 on the emulator."""
    code, fn = F32_OPS[op]
    x = f32_log_uniform()
    v = np.concatenate([x, -x[:4096]]) if op == "rcp" else x
    got, = run(backend, "f32", "math1", code, v)
    if op == "rsqrt":
        ref = 1 / np.sqrt(v.astype(LD))
        rel = float((np.abs(got.astype(LD) - ref) / ref).max())
        measure(backend, "f32_rsqrt", n=int(v.size), worst_rel=rel, worst_rel_in_2m24=rel * 2.0 ** 24)
        assert rel <= 2.0 ** -22
    else:
        d = ulp_distance(got, fn(v))
        measure(backend, "f32_" + op, n=int(v.size), worst_ulp=int(d.max()))
        assert d.max() <= 1
    den = np.array([1e-45, 1e-40, 5.877e-39, 1.1754942e-38], np.float32)  # denormals up to the largest
    if op == "rcp":
        edge = np.concatenate([den, -den, np.array([0.0, -0.0, np.inf, -np.inf, 2.0 ** 127, -2.0 ** 127], np.float32)])
    else:
        edge = np.concatenate([den, np.array([0.0, np.inf], np.float32)])
    got, = run(backend, "f32", "math1", code, edge)
    want = expected32(backend, fn, edge)
    if backend == "gpu":  # spelled out: the flushed results
        z = np.float32(0)
        flushed = {"rcp": [np.inf] * 4 + [-np.inf] * 4 + [np.inf, -np.inf, z, -z, z, -z],
                   "sqrt": [z] * 5 + [np.inf], "rsqrt": [np.inf] * 5 + [z]}[op]
        assert same_bits(want, np.array(flushed, np.float32)).all()
    assert same_bits(got, want).all(), (edge, got, want)


# ------------------------------------------------------------------ d. the FP32 BVH node test
@functools.lru_cache(None)
def node_cases(seed):
    n = 6000
    o, d, box, tr = make_cases(n, seed)
    exact = [exact_accept(o[i], d[i], box[i], tr[i, 0], tr[i, 1]) for i in range(n)]
    return o, d, box, tr, exact


@backends
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fp32_node_test_with_the_devices_reciprocal(backend, seed):
    """tests/test_node_test.py's cases and assertions through rtk64::prep_ray + node_slabs_f32 on
    the backend: on the device the direction reciprocal is v_rcp_f32 itself, not the "1 ulp either
    way" model: every exactly accepted box is entered, every clear miss is rejected."""
    o, d, box, tr, exact = node_cases(seed)
    n = len(exact)
    acc, = run(backend, "f64", "node", o, d, box, tr)
    assert np.all((acc == 0) | (acc == 3)), "the two children (the same box) must agree"
    n_exact = n_clear_miss = n_clear_rejected = 0
    for i in range(n):
        ok, near, far = exact[i]
        if ok:
            n_exact += 1
            assert acc[i] == 3, f"case {i}: the exact slab test enters the box, the FP32 test does not"
        elif (near - far) > Fraction(1, 10 ** 5) * (abs(near) + Fraction(float(np.max(np.abs(o[i] / d[i]))))):
            n_clear_miss += 1
            n_clear_rejected += acc[i] == 0
    assert n_exact > n // 5 and n_clear_miss > n // 20, (n_exact, n_clear_miss)
    assert n_clear_rejected == n_clear_miss, (n_clear_rejected, n_clear_miss)


# ------------------------------------------------------------------ exact arithmetic on arrays
def to_int(x, s):
    """x 2^s as an object array of Python ints (exact; every x 2^s must be an integer)."""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)
    mi = (m * 2.0 ** 53).astype(np.int64)
    sh = np.where(x == 0, 0, e.astype(np.int64) - 53 + s)
    low = sh < 0  # trailing zero bits of the mantissa may cover a negative shift
    if low.any():
        assert (mi[low] % (1 << (-sh[low]).astype(np.int64)) == 0).all(), "scale too small"
        mi = np.where(low, mi >> np.where(low, -sh, 0), mi)
        sh = np.where(low, 0, sh)
    return mi.astype(object) << sh.astype(object)


def scale_of(*arrays):
    """The smallest s for which every finite value of the arrays times 2^s is an integer."""
    s = 0
    for a in arrays:
        a = np.asarray(a, np.float64)
        a = a[(a != 0) & np.isfinite(a)]
        if a.size:
            s = max(s, int((53 - np.frexp(a)[1]).max()))
    return s


def ratio(num, den):
    """num / den of object int arrays, correctly rounded to float64."""
    return np.array([n / d for n, d in zip(num, den)], np.float64)


def ratio_ld(num, den):
    """num / den of object int arrays (den > 0) in long double: the float64 quotient plus its
    exactly computed remainder."""
    hi = ratio(num, den)
    k = 1140  # every float64 times 2^1140 is an integer
    rem = num * (1 << k) - to_int(hi, k) * den
    lo = ratio(rem, den * (1 << k))
    return hi.astype(LD) + lo.astype(LD)


def dot_i(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


# ------------------------------------------------------------------ e. primitive tests
KTMIN = 1e-4  # Ray.hs:178
N_PRIM = 1 << 16


def random_units(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@functools.lru_cache(None)
def plane_cases(precision, tri):
    """2^16 well-conditioned parallelogram / triangle cases in the record's own terms (n, q, wa, wb):
    a third hit with (a, b) at least 1 % inside, a third missed by at least 1 % of the edge (a
    quarter of those with the plane behind the ray), a third grazing an edge within 1e-4 .. 1e-3 of
    its length (either side).  The plane is near the coordinate origin and the ray starts 0.5 .. 2
    edge lengths away, so that the rounding of the kernel's own differences (q - o, t d - qo) stays
    two decades below the grazing offsets and few cases fall inside the skip band."""
    real = real_of(precision)
    rng = np.random.default_rng(7 + tri)
    n = N_PRIM
    size = 10.0 ** rng.uniform(-2, 2, n)
    u = random_units(rng, n)
    v = random_units(rng, n)
    for _ in range(64):  # edges at an angle: |u x v| >= 0.5
        bad = np.linalg.norm(np.cross(u, v), axis=1) < 0.5
        if not bad.any():
            break
        v[bad] = random_units(rng, int(bad.sum()))
    u *= (size * rng.uniform(0.5, 1.0, n))[:, None]
    v *= (size * rng.uniform(0.5, 1.0, n))[:, None]
    q = size[:, None] * rng.uniform(-0.1, 0.1, (n, 3))
    cp = np.cross(u, v)
    ncp = np.linalg.norm(cp, axis=1, keepdims=True)
    nrm = cp / ncp
    ns = nrm / ncp
    wa, wb = np.cross(v, ns), np.cross(ns, u)
    mode = np.arange(n) % 3  # 0 hit, 1 miss, 2 grazing
    a = rng.uniform(0.01, 0.99, n)
    b = rng.uniform(0.01, 0.99, n)
    if tri:  # fold into a + b <= 0.99 (both stay >= 0.01)
        over = a + b > 0.99
        a, b = np.where(over, 1.0 - a, a), np.where(over, 1.0 - b, b)
        over = a + b > 0.99
        a = np.where(over, 0.01, a)
        b = np.where(over, 0.5, b)
    out = rng.uniform(0.01, 0.5, n)
    off = rng.uniform(1e-4, 1e-3, n) * rng.choice([-1.0, 1.0], n)
    edge = rng.integers(0, 3 if tri else 4, n)
    miss, graze = mode == 1, mode == 2
    for sel, delta in ((miss, out), (graze, -off)):  # delta > 0: outside
        if tri:
            a = np.where(sel & (edge == 0), -delta, a)
            b = np.where(sel & (edge == 1), -delta, b)
            # the hypotenuse: a + b = 1 + delta at a point of the edge's inner half
            s = rng.uniform(0.1, 0.9, n)
            a = np.where(sel & (edge == 2), s * (1 + delta), a)
            b = np.where(sel & (edge == 2), (1 - s) * (1 + delta), b)
            b = np.where(sel & (edge == 0), np.minimum(b, 0.9), b)
            a = np.where(sel & (edge == 1), np.minimum(a, 0.9), a)
        else:
            a = np.where(sel & (edge == 0), -delta, a)
            a = np.where(sel & (edge == 1), 1 + delta, a)
            b = np.where(sel & (edge == 2), -delta, b)
            b = np.where(sel & (edge == 3), 1 + delta, b)
    p = q + a[:, None] * u + b[:, None] * v
    d = random_units(rng, n)
    for _ in range(64):  # |n . d| >= 0.1 (0.05 is asked for)
        bad = np.abs((nrm * d).sum(1)) < 0.1
        if not bad.any():
            break
        d[bad] = random_units(rng, int(bad.sum()))
    tstar = size * rng.uniform(0.5, 2.0, n)
    behind = miss & (np.arange(n) % 12 == 1)  # a quarter of the misses: the plane lies behind the ray
    inside_ab = rng.uniform(0.2, 0.4, (n, 2))
    p = np.where(behind[:, None], q + inside_ab[:, :1] * u + inside_ab[:, 1:] * v, p)
    o = p - np.where(behind, -tstar, tstar)[:, None] * d
    c = lambda x: np.ascontiguousarray(x, dtype=real)  # noqa: E731
    return dict(n=c(nrm), q=c(q), wa=c(wa), wb=c(wb), o=c(o), d=c(d), mode=mode)


def plane_exact(C, tri, tmin):
    """Geometry.hs:117-144 in exact integer arithmetic on the case's floats: denom = n . d, t =
    n . (q - o) / denom, p_rel = o + t d - q, a = p_rel . wa, b = p_rel . wb; accepted when
    |denom| > 1e-8, t > tmin and the shape's test holds.  Returns the decision, t (long double), the
    margins and, per margin, the magnitude of the terms the kernel subtracts to form it."""
    f = {k: C[k].astype(np.float64) for k in ("n", "q", "wa", "wb", "o", "d")}
    s = scale_of(*f.values(), [tmin])
    I = {k: np.stack([to_int(x[:, j], s) for j in range(3)], 1) for k, x in f.items()}
    D = dot_i(I["n"], I["d"])  # 2s
    qo = I["q"] - I["o"]
    N = dot_i(I["n"], qo)  # 2s
    neg = np.array([x < 0 for x in D])
    zero = np.array([x == 0 for x in D])
    D = np.where(neg, -D, D) + zero.astype(object)  # (denom = 0: any positive stand-in; rejected below)
    N = np.where(neg, -N, N)
    pr = N[:, None] * I["d"] - D[:, None] * qo  # p_rel D, 3s
    A, B = dot_i(pr, I["wa"]), dot_i(pr, I["wb"])  # a D 2^2s, 4s
    one = D * (1 << (2 * s))
    T = to_int([tmin], s)[0]
    tm_num = N * (1 << s) - T * D  # (t - tmin) D 2^s
    E = to_int([1e-8], 2 * s)[0]
    denom_ok = np.array([x > E for x in D])
    if tri:
        shape = [A, B, one - A - B]
    else:
        shape = [A, B, one - A, one - B]
    ok = denom_ok & ~zero & np.array([x > 0 for x in tm_num])
    for m in shape:
        ok &= np.array([x >= 0 for x in m])
    t = ratio_ld(N, D)
    denom = np.abs((f["n"] * f["d"]).sum(1))
    tf = np.abs(t.astype(np.float64))
    # magnitudes of the subtracted terms: t from n . (q - o) / denom; a from (t d - (q - o)) . wa
    # plus t's own error carried through d . wa
    sc_t = (np.abs(f["n"]) * (np.abs(f["q"]) + np.abs(f["o"]))).sum(1) / denom
    def sc(w):
        return ((tf[:, None] * np.abs(f["d"]) + np.abs(f["q"]) + np.abs(f["o"])) * np.abs(w)).sum(1) + \
            sc_t * np.abs(f["d"] * w).sum(1)
    sa, sb = sc(f["wa"]), sc(f["wb"])
    margins = [(ratio(A, one), sa), (ratio(B, one), sb), (ratio(tm_num, D * (1 << s)), sc_t + tmin)]
    if tri:
        margins.append((ratio(one - A - B, one), 1 + sa + sb))
    else:
        margins += [(ratio(one - A, one), 1 + sa), (ratio(one - B, one), 1 + sb)]
    S = (np.abs(f["o"]).max(1) + np.abs(f["q"]).max(1) + tf) / denom
    return ok, t, margins, S


def undecided(margins, eps):
    skip = np.zeros(len(margins[0][0]), bool)
    for m, scale in margins:
        skip |= np.abs(m) <= 64 * eps * scale
    return skip


def k_from_baseline(worst):
    """8x the plain formula's own worst error, rounded up to a power of two."""
    return 2.0 ** math.ceil(math.log2(8 * max(worst, 2.0 ** -10)))


PLANE_KINDS = {"quad": (1, False), "tri": (2, True), "either_quad": (3, False), "either_tri": (4, True)}


@functools.lru_cache(None)
def plane_reference(precision, tri):
    C = plane_cases(precision, tri)
    real = real_of(precision)
    eps = float(np.finfo(real).eps)
    ok, t, margins, S = plane_exact(C, tri, float(real(KTMIN)))
    skip = undecided(margins, eps)
    # the reference's plain formula (Geometry.hs as written) in numpy at the working precision
    n_, q_, o_, d_ = C["n"], C["q"], C["o"], C["d"]
    dotr = lambda a, b: a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]  # noqa: E731
    tb = dotr(n_, q_ - o_) / dotr(n_, d_)
    assert tb.dtype == real
    use = ok & ~skip
    base = float((np.abs(tb[use].astype(LD) - t[use]) / (eps * S[use])).max())
    return C, ok, t, skip, S, base


@backends
@both_precisions
@pytest.mark.parametrize("kind", list(PLANE_KINDS))
def test_plane_tests_random_cases(backend, precision, kind):
    """isect_plane<1>, <0> and <-1> (both `quad` values) on 2^16 random well-conditioned cases
    against the exact evaluation of Geometry.hs:117-151, 168-176 on the same floats.  Accept /
    reject equals the exact decision unless an exact margin (a, b, 1 - a, 1 - b | 1 - a - b, t - tmin)
    lies within 64 eps scale of zero (scale: the magnitude of the terms subtracted); such cases are
    at most 0.5 % of the family.  An accepted t is within K eps S of the exact t, S = (|o|inf +
    |q|inf + |t|) / |n . d|, K = 8x the worst error (same units) of the reference's plain formula
    evaluated in numpy at the working precision, rounded up to a power of two.  Measured (units of
    eps S): plain formula 0.90 - 0.96, so K = 8; both backends 0.88 - 1.20; skipped 0.14 % (parallelogram)
    and 0.36 % (triangle) in FP32, none in binary64."""
    code, tri = PLANE_KINDS[kind]
    C, ok, t, skip, S, base = plane_reference(precision, tri)
    real = real_of(precision)
    eps = float(np.finfo(real).eps)
    n = N_PRIM
    tmin = np.full(n, KTMIN, real)
    got_t, got_q, take = run(backend, precision, "isect", code, rec_plane(C), C["o"], C["d"], tmin,
                             np.zeros(n, np.int32))
    assert skip.mean() <= 0.005, skip.mean()
    acc = take != 0
    assert (acc == (got_q >= 0)).all()  # finite inputs: the margin alone decides
    wrong = (acc != ok) & ~skip
    assert not wrong.any(), (int(wrong.sum()), np.flatnonzero(wrong)[:8])
    for mode in range(3):  # every third of the family is exercised on both sides it can fall
        assert (C["mode"][~skip] == mode).sum() > n // 4
    assert ok[C["mode"] == 0].all() and not ok[C["mode"] == 1].any()
    hit = ok & ~skip
    K = k_from_baseline(base)
    err = float((np.abs(got_t[hit].astype(LD) - t[hit]) / (eps * S[hit])).max())
    measure(backend, f"isect_plane_{kind}_{precision}", n=n, skipped=float(skip.mean()), baseline_err=base, K=K,
            worst_err=err, hits=int(hit.sum()))
    assert np.isfinite(got_t[acc]).all()
    assert err <= K, (err, K, base)


@backends
@both_precisions
def test_target_hit_random_cases(backend, precision):
    """target_hit (a parallelogram on (0, infinity), Ray.hs:143-145) on the parallelogram cases:
    the same exact decision with tmin = 0, the same bound on t, and rinv = 1 / (n . d) within
    4 eps cond of the exact value, cond = sum |n_k d_k| / |n . d| (three roundings of the dot product,
    each at most eps / 2 of the largest partial sum, and the reciprocal's 1 ulp: 2.5 eps cond at most)."""
    C = plane_cases(precision, False)
    real = real_of(precision)
    eps = float(np.finfo(real).eps)
    ok, t, margins, S = target_reference(precision)
    skip = undecided(margins, eps)
    tg = np.concatenate([C["q"], C["n"], C["wa"], C["wb"]], 1)
    hit, got_t, rinv = run(backend, precision, "target", tg, C["o"], C["d"])
    assert skip.mean() <= 0.005, skip.mean()
    wrong = ((hit != 0) != ok) & ~skip
    assert not wrong.any(), (int(wrong.sum()), np.flatnonzero(wrong)[:8])
    use = ok & ~skip
    base = plane_reference(precision, False)[5]
    K = k_from_baseline(base)
    err = float((np.abs(got_t[use].astype(LD) - t[use]) / (eps * S[use])).max())
    f = {k: C[k].astype(np.float64) for k in ("n", "d")}
    s = scale_of(f["n"], f["d"])
    D = dot_i(np.stack([to_int(f["n"][:, j], s) for j in range(3)], 1),
              np.stack([to_int(f["d"][:, j], s) for j in range(3)], 1))
    neg = np.array([x < 0 for x in D])
    inv = ratio_ld(np.full(len(D), 1 << (2 * s), object), np.where(neg, -D, D)) * np.where(neg, -1, 1)
    cond = (np.abs(f["n"] * f["d"]).sum(1) / np.abs((f["n"] * f["d"]).sum(1)))[use]  # of the 3-term dot product
    rerr = float((np.abs(rinv[use].astype(LD) - inv[use]) / np.abs(inv[use]) / (eps * cond)).max())
    measure(backend, f"target_hit_{precision}", n=N_PRIM, skipped=float(skip.mean()), baseline_err=base, K=K,
            worst_err=err, rinv_rel_in_eps_cond=rerr)
    assert err <= K and rerr <= 4.0


@functools.lru_cache(None)
def target_reference(precision):
    return plane_exact(plane_cases(precision, False), False, 0.0)


def rec_plane(C):
    """The primitive records of plane cases: a = (n, -), b = (q, -), c = (wa, -), e = (wb, -)."""
    n = len(C["n"])
    r = np.zeros((n, 16), C["n"].dtype)
    r[:, 0:3], r[:, 4:7], r[:, 8:11], r[:, 12:15] = C["n"], C["q"], C["wa"], C["wb"]
    return r


def rec_sphere(c, r2, radius=None):
    r = np.zeros((len(c), 16), c.dtype)
    r[:, 0:3] = c
    r[:, 4] = np.sqrt(r2) if radius is None else radius
    r[:, 5] = r2
    return r


@functools.lru_cache(None)
def sphere_cases(precision):
    """2^16 well-conditioned sphere cases: radius 1e-2 .. 1e2, the centre within 0.1 radius of the
    coordinate origin, the ray passing the centre at distance l: a third hit (l <= 0.99 r; an
    eighth of them from inside), a third missed (l >= 1.01 r, or the sphere behind the ray), a
    third grazing (l = r (1 +- 1e-4 .. 1e-3)); the origin 1.2 .. 2.5 r before the closest point."""
    real = real_of(precision)
    rng = np.random.default_rng(11)
    n = N_PRIM
    r = 10.0 ** rng.uniform(-2, 2, n)
    c = r[:, None] * rng.uniform(-0.1, 0.1, (n, 3))
    d = random_units(rng, n)
    e = np.cross(d, random_units(rng, n))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    mode = np.arange(n) % 3
    l = r * rng.uniform(0.0, 0.99, n)
    l = np.where(mode == 1, r * rng.uniform(1.01, 1.5, n), l)
    l = np.where(mode == 2, r * (1 + rng.uniform(1e-4, 1e-3, n) * rng.choice([-1.0, 1.0], n)), l)
    h = r * rng.uniform(1.2, 2.5, n)
    inside = (mode == 0) & (np.arange(n) % 24 == 0)
    h = np.where(inside, r * rng.uniform(-0.5, 0.5, n), h)
    l = np.where(inside, r * rng.uniform(0.0, 0.5, n), l)
    behind = (mode == 1) & (np.arange(n) % 6 == 1)
    h = np.where(behind, -h, h)
    l = np.where(behind, r * rng.uniform(0.0, 0.9, n), l)
    o = c + l[:, None] * e - h[:, None] * d
    cr = lambda x: np.ascontiguousarray(x, dtype=real)  # noqa: E731
    rr = cr(r)
    return dict(c=cr(c), o=cr(o), d=cr(d), r=rr, r2=(rr * rr).astype(real), mode=mode)


@functools.lru_cache(None)
def sphere_reference(precision):
    """Geometry.hs:58-77 on the case's floats: oc = c - o, h = d . oc, c' = |oc|^2 - r^2 (the record's
    r^2), discriminant h^2 - c' in exact integers; its square root and the roots in long double."""
    C = sphere_cases(precision)
    real = real_of(precision)
    eps = float(np.finfo(real).eps)
    tmin = float(real(KTMIN))
    f = {k: C[k].astype(np.float64) for k in ("c", "o", "d")}
    r2 = C["r2"].astype(np.float64)
    s = scale_of(f["c"], f["o"], f["d"])
    assert scale_of(r2) <= 2 * s
    I = {k: np.stack([to_int(x[:, j], s) for j in range(3)], 1) for k, x in f.items()}
    oc = I["c"] - I["o"]
    H = dot_i(I["d"], oc)  # 2s
    Cq = dot_i(oc, oc) - to_int(r2, 2 * s)  # 2s
    disc_i = H * H - Cq * (1 << (2 * s))  # 4s
    nonneg = np.array([x >= 0 for x in disc_i])
    one2, one4 = np.full(len(H), 1 << (2 * s), object), np.full(len(H), 1 << (4 * s), object)
    h = ratio_ld(H, one2)
    disc = ratio_ld(disc_i, one4)
    sq = np.sqrt(np.maximum(disc, 0))
    r1, r2_ = h - sq, h + sq
    first = r1 > tmin
    t = np.where(first, r1, r2_)
    ok = nonneg & (first | (r2_ > tmin))
    absoc = np.abs(f["c"]) + np.abs(f["o"])
    sc_disc = (absoc ** 2).sum(1) + r2
    S = np.abs(f["o"]).max(1) + np.abs(f["c"]).max(1) + np.abs(t.astype(np.float64))
    margins = [(disc.astype(np.float64), sc_disc), ((r1 - tmin).astype(np.float64), S), ((r2_ - tmin).astype(np.float64), S)]
    skip = undecided(margins, eps)
    # the plain formula at the working precision
    c_, o_, d_ = C["c"], C["o"], C["d"]
    dotr = lambda a, b: a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]  # noqa: E731
    ocb = c_ - o_
    hb = dotr(d_, ocb)
    sqb = np.sqrt(np.maximum(hb * hb - (dotr(ocb, ocb) - C["r"] * C["r"]), real(0)))
    tb = np.where(first, hb - sqb, hb + sqb)
    assert tb.dtype == real
    use = ok & ~skip
    base = float((np.abs(tb[use].astype(LD) - t[use]) / (eps * S[use])).max())
    return C, ok, t, skip, S, base


@backends
@both_precisions
def test_sphere_test_random_cases(backend, precision):
    """isect_sphere on 2^16 random well-conditioned cases against Geometry.hs:58-77 evaluated
    exactly (square root in long double).  The rules are those of the plane test: decisions equal
    unless the discriminant or a root's t - tmin is within 64 eps scale of zero (at most 0.5 % of
    the cases), accepted t within K eps S, S = |o|inf + |c|inf + |t|, K from the plain formula.
    Measured (units of eps S): plain formula 88.9 (FP32) and 84.6 (binary64) on the grazing hits,
    where the square root amplifies the discriminant's rounding, so K = 1024; the kernel 31.3 / 33.7
    (FP32, emulator / MI355X) and 65.9 (binary64, both); nothing skipped."""
    C, ok, t, skip, S, base = sphere_reference(precision)
    real = real_of(precision)
    eps = float(np.finfo(real).eps)
    n = N_PRIM
    got_t, got_q, take = run(backend, precision, "isect", 0, rec_sphere(C["c"], C["r2"], C["r"]), C["o"], C["d"],
                             np.full(n, KTMIN, real), np.zeros(n, np.int32))
    assert skip.mean() <= 0.005, skip.mean()
    acc = take != 0
    assert (acc == (got_q >= 0)).all()  # finite inputs: the margin alone decides
    wrong = (acc != ok) & ~skip
    assert not wrong.any(), (int(wrong.sum()), np.flatnonzero(wrong)[:8])
    for mode in range(3):
        assert (C["mode"][~skip] == mode).sum() > n // 4
    assert ok[C["mode"] == 0].all() and not ok[C["mode"] == 1].any()
    hit = ok & ~skip
    K = k_from_baseline(base)
    err = float((np.abs(got_t[hit].astype(LD) - t[hit]) / (eps * S[hit])).max())
    measure(backend, f"isect_sphere_{precision}", n=n, skipped=float(skip.mean()), baseline_err=base, K=K,
            worst_err=err, hits=int(hit.sum()))
    assert err <= K, (err, K, base)


# ---- constructed edges: exact assertions, no skips
def isect(backend, precision, kind, rec, o, d, tmin, self_=None):
    """(t, accepted) of constructed cases; accepted: the kernel's closest-hit update (`consider`)
    takes the candidate for a ray without a hit so far, i.e. its margin q >= 0 and t < +inf."""
    real = real_of(precision)
    rec = np.asarray(rec, real).reshape(-1, 16)
    n = len(rec)
    o = np.broadcast_to(np.asarray(o, real), (n, 3))
    d = np.broadcast_to(np.asarray(d, real), (n, 3))
    tmin = np.broadcast_to(np.asarray(tmin, real), (n,))
    self_ = np.zeros(n, np.int32) if self_ is None else np.broadcast_to(np.asarray(self_, np.int32), (n,))
    t, q, take = run(backend, precision, "isect", kind, rec, o, d, tmin, self_)
    assert not (take[~(q >= 0)]).any()  # a negative (or NaN) margin is never taken
    return t, take != 0


def plane_rec(real, n, q, u, v):
    """The record of the parallelogram / triangle (q, u, v) with axis-aligned dyadic edges (exact)."""
    n, q, u, v = (np.asarray(x, np.float64) for x in (n, q, u, v))
    cp = np.cross(u, v)
    ns = n / np.linalg.norm(cp)
    r = np.zeros(16, real)
    r[0:3], r[4:7], r[8:11], r[12:15] = n, q, np.cross(v, ns), np.cross(ns, u)
    return r


PLANE_CODES = [1, 2, 3, 4]  # isect_plane<1>, <0>, <-1> quad, <-1> triangle


@backends
@both_precisions
def test_plane_denominator_edges(backend, precision):
    """|n . d| against 1e-8: isect_plane accepts iff |denom| - 1e-8 >= 0 (the kernel's margin),
    target_hit iff |denom| > 1e-8 (its own guard, the reference's rule); denom = 0 (t = NaN or inf)
    is never accepted, and an accepted t is finite."""
    real = real_of(precision)
    e = real(1e-8)
    up, dn = np.nextafter(e, real(1)), np.nextafter(e, real(0))
    deltas = np.array([0.0, -0.0, e, -e, up, -up, dn, -dn], real)
    want = np.array([False, False, True, True, True, True, False, False])
    rec = plane_rec(real, [0, 0, 1], [0, 0, 0], [4, 0, 0], [0, 4, 0])
    n = len(deltas)
    d = np.stack([np.ones(n, real), np.zeros(n, real), deltas], 1)  # n . d = delta exactly
    o = np.stack([np.full(n, 0.25, real), np.full(n, 0.25, real), -deltas], 1)  # t ~ 1, (a, b) ~ (0.31, 0.06)
    for code in PLANE_CODES:
        t, acc = isect(backend, precision, code, np.tile(rec, (n, 1)), o, d, KTMIN)
        assert (acc == want).all(), (code, acc)
        assert np.isfinite(t[acc]).all() and np.allclose(t[acc], 1.0, rtol=1e-6)
    tg = np.tile(np.concatenate([rec[4:7], rec[0:3], rec[8:11], rec[12:15]]), (n, 1))
    hit, t, rinv = run(backend, precision, "target", tg, o, d)
    strict = np.array([False, False, False, False, True, True, False, False])
    assert ((hit != 0) == strict).all(), hit
    assert np.isfinite(t[hit != 0]).all()


@backends
@both_precisions
def test_open_interval_at_tmin(backend, precision):
    """t equal to tmin, one ulp above and one ulp below, on an axis-aligned ray (t is exact): the
    interval is open, accepted iff t > tmin — planes and the sphere's far root."""
    real = real_of(precision)
    tm = real(KTMIN)
    ts = np.array([tm, np.nextafter(tm, real(1)), np.nextafter(tm, real(0))], real)
    want = np.array([False, True, False])
    recs = np.stack([plane_rec(real, [0, 0, 1], [0, 0, T], [4, 0, 0], [0, 4, 0]) for T in ts])
    for code in PLANE_CODES:
        t, acc = isect(backend, precision, code, recs, [0.25, 0.25, 0], [0, 0, 1], tm)
        assert (t == ts).all() and (acc == want).all(), (code, t, acc)
    # sphere: centre 0, r = 1, origin (0, 0, 0.5) looking along +z: roots -1.5 and 0.5 exactly
    half = real(0.5)
    tmins = np.array([half, np.nextafter(half, real(0)), np.nextafter(half, real(1))], real)
    rec = rec_sphere(np.zeros((3, 3), real), np.ones(3, real))
    t, acc = isect(backend, precision, 0, rec, [0, 0, 0.5], [0, 0, 1], tmins)
    assert (t == half).all() and (acc == [False, True, False]).all(), (t, acc)
    # the near root equal to tmin (origin (0, 0, -1.5): roots 0.5 and 2.5): the far root is returned
    t, acc = isect(backend, precision, 0, rec, [0, 0, -1.5], [0, 0, 1], tmins)
    assert (t == [2.5, 0.5, 2.5]).all() and acc.all(), (t, acc)


@backends
@both_precisions
def test_plane_closed_bounds(backend, precision):
    """a, b and a + b exactly 0 or 1 (unit axis-aligned edges, dyadic hit points): the shape's
    bounds are closed, so the corner and edge points are accepted; one step outside is not."""
    real = real_of(precision)
    rec = plane_rec(real, [0, 0, 1], [0, 0, 0], [1, 0, 0], [0, 1, 0])
    out = 2.0 ** -10
    pts = [(0, 0), (1, 0), (0, 1), (0.5, 0.5), (0, 0.5), (0.5, 0), (1, 1), (1, 0.5), (0.5, 1), (0.75, 0.5),
           (-out, 0.5), (0.5, -out), (1 + out, 0.5), (0.5, 1 + out), (0.5, 0.5 + out)]
    o = np.array([(a, b, 1.0) for a, b in pts], real)
    in_quad = np.array([0 <= a <= 1 and 0 <= b <= 1 for a, b in pts])
    in_tri = np.array([a >= 0 and b >= 0 and a + b <= 1 for a, b in pts])
    for code, want in ((1, in_quad), (3, in_quad), (2, in_tri), (4, in_tri)):
        t, acc = isect(backend, precision, code, np.tile(rec, (len(pts), 1)), o, [0, 0, -1], KTMIN)
        assert (t == 1.0).all() and (acc == want).all(), (code, acc, want)
    tg = np.tile(np.concatenate([rec[4:7], rec[0:3], rec[8:11], rec[12:15]]), (len(pts), 1))
    hit, t, rinv = run(backend, precision, "target", tg, o, np.tile(np.array([0, 0, -1], real), (len(pts), 1)))
    assert ((hit != 0) == in_quad).all() and (t == 1.0).all() and (rinv == -1.0).all()


@backends
@both_precisions
def test_sphere_constructed_cases(backend, precision):
    """Origin inside: the far root.  Both roots <= tmin: rejected.  Discriminant exactly 0
    (axis-aligned tangent): accepted.  self: t = 2 h, valid iff 2 h > tmin; a plane is never
    valid for the leaf the ray leaves.  A record whose r^2 is an FP32 denormal behaves as r^2 = 0."""
    real = real_of(precision)
    z = [0, 0, 1]
    unit = rec_sphere(np.zeros((1, 3), real), np.ones(1, real))
    t, acc = isect(backend, precision, 0, rec_sphere(np.zeros((1, 3), real), np.full(1, 4, real)), [0, 0, 0.5], z, KTMIN)
    assert t[0] == 1.5 and acc[0]  # roots -2.5, 1.5
    t, acc = isect(backend, precision, 0, unit, [0, 0, 5], z, KTMIN)
    assert not acc[0]  # roots -6, -4
    t, acc = isect(backend, precision, 0, rec_sphere(np.array([[1, 0, 0]], real), np.ones(1, real)), [0, 0, -2], z, KTMIN)
    assert t[0] == 2.0 and acc[0]  # tangent: disc = 0
    t, acc = isect(backend, precision, 0, np.tile(unit, (2, 1)), [[0, 0, -1], [0, 0, 1]], z, KTMIN, 1)
    assert (t == [2.0, -2.0]).all() and (acc == [True, False]).all()  # self: 2 h
    rec = plane_rec(real, [0, 0, 1], [0, 0, 0], [1, 0, 0], [0, 1, 0])
    for code in PLANE_CODES:
        t, acc = isect(backend, precision, code, rec, [0.25, 0.25, 1], [0, 0, -1], KTMIN, 1)
        assert not acc[0]
        t, acc = isect(backend, precision, code, rec, [0.25, 0.25, 1], [0, 0, -1], KTMIN, 0)
        assert acc[0] and t[0] == 1.0
    if precision == "f32":
        tiny = rec_sphere(np.zeros((2, 3), real), np.array([1e-40, 0.0], real), np.array([1e-20, 0.0], real))
        t, acc = isect(backend, precision, 0, tiny, [0, 0, -1], z, KTMIN)
        assert (t == 1.0).all() and acc.all()  # through the centre: disc = r^2 (flushed: 0), t = h
        t, acc = isect(backend, precision, 0, tiny, [2.0 ** -60, 0, -1], z, KTMIN)
        assert not acc.any()  # l^2 = 2^-120 > r^2: missed with r^2 = 1e-40 and with 0 alike


@backends
@both_precisions
def test_non_finite_origin_never_accepted(backend, precision):
    """NaN or inf in the ray origin: no primitive test accepts, whatever the component and sign."""
    real = real_of(precision)
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        for k in range(3):
            o = np.array([0.25, 0.25, 1.0])
            o[k] = v
            bad.append(o)
    bad.append(np.full(3, np.nan))
    bad.append(np.full(3, np.inf))
    bad.append(np.full(3, -np.inf))
    o = np.array(bad, real)
    n = len(o)
    rec = plane_rec(real, [0, 0, 1], [0, 0, 0], [1, 0, 0], [0, 1, 0])
    dirs = ([0, 0, -1], [0, 0, 1], [0.6, 0, -0.8], [-0.6, 0.64, 0.48])
    for d in dirs:
        for code in PLANE_CODES:
            t, acc = isect(backend, precision, code, np.tile(rec, (n, 1)), o, d, KTMIN)
            assert not acc.any(), (code, d, acc)
        sph = rec_sphere(np.zeros((n, 3), real), np.ones(n, real))
        t, acc = isect(backend, precision, 0, sph, o, d, KTMIN)
        assert not acc.any(), ("sphere", d, acc, t)
        tg = np.tile(np.concatenate([rec[4:7], rec[0:3], rec[8:11], rec[12:15]]), (n, 1))
        hit, t, rinv = run(backend, precision, "target", tg, o, np.tile(np.array(d, real), (n, 1)))
        assert not hit.any(), ("target", d, hit)


# ------------------------------------------------------------------ f. fixed-point accumulation
def fixed_reference(x, precision):
    """(hi, lo, bad) of one radiance x in Python integers: x 2^64 floored, split at 32 bits (the
    FP32 accumulator keeps the high word, truncated toward zero); bad when not |x| < 1e9."""
    if not abs(x) < 1.0e9:  # NaN included
        return 0, 0, 1
    w = math.floor(Fraction(x) * (1 << 64))
    if precision == "f64":
        return w >> 32, w & 0xffffffff, 0
    return int(Fraction(x) * (1 << 32)), 0, 0  # int(): toward zero


@backends
@both_precisions
def test_fixed_point_words(backend, precision):
    """rtk::to_fixed / rtk64::acc_add against Python integers: for x >= 0 the FP32 word is exactly
    trunc(x 2^32) and the binary64 pair exactly trunc(x 2^64) split at 32 bits; values that are not
    below 1e9 in magnitude (2^31 - 1 among them), NaN and +-inf set `bad` and add nothing; negative
    binary64 inputs are exact (floor and fraction); negative FP32 inputs are within 2^-25 relative
    (the comment's claim)."""
    real = real_of(precision)
    eps = float(np.finfo(real).eps)
    below = np.nextafter(real(1e9), real(0))
    listed = [0.0, 2.0 ** -33, 2.0 ** -32, 2.0 ** -32 * (1 + eps), 2.0 ** -32 * (1 - eps), 1 - 2.0 ** -24, 1.0, 15.0,
              float(below), 2.0 ** 31 - 1, 1e9, np.nan, np.inf, -np.inf, 0.5, 2.0 ** -64, 3.0 * 2.0 ** -64, 63.999]
    rng = np.random.default_rng(5)
    x = np.concatenate([np.array(listed), rng.uniform(0, 64, 1 << 16), 10.0 ** rng.uniform(-12, 8.9, 4096)]).astype(real)
    assert x[8] < 1e9 and not (x[9] < 1e9)
    hi, lo, bad = run(backend, precision, "acc", x)
    ref = [fixed_reference(float(v), precision) for v in x]
    assert bad.tolist() == [r[2] for r in ref]
    assert bad[9:14].all() and not bad[:9].any()
    assert hi.tolist() == [r[0] for r in ref]
    assert lo.tolist() == [r[1] for r in ref]
    # negative radiances (negative user colours)
    xn = -np.concatenate([rng.uniform(2.0 ** -20, 64, 1 << 12), [1.0, 0.5, 2.0 ** -20, 15.0, 63.999]]).astype(real)
    hi, lo, bad = run(backend, precision, "acc", xn)
    assert not bad.any()
    if precision == "f64":
        ref = [fixed_reference(float(v), precision) for v in xn]
        assert hi.tolist() == [r[0] for r in ref] and lo.tolist() == [r[1] for r in ref]
    else:
        want = np.array([float(Fraction(float(v)) * (1 << 32)) for v in xn])
        rel = np.abs(hi.astype(np.float64) - want) / np.abs(want)
        measure(backend, "f32_to_fixed_negative", worst_rel_in_2m25=float(rel.max() * 2.0 ** 25))
        assert rel.max() <= 2.0 ** -25


# ------------------------------------------------------------------ g. Philox and the samplers
def philox_ref(ctr, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) in numpy uint64: ctr (n, 4) uint32, one key."""
    c = [ctr[:, j].astype(np.uint64) for j in range(4)]
    k0, k1, m32 = np.uint64(k0), np.uint64(k1), np.uint64(0xffffffff)
    for r in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, 1).astype(np.uint32)


def test_philox_restatement_known_answers():
    """The numpy restatement against Random123's published known-answer vectors (philox4x32-10)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox_ref(np.array([ctr], np.uint32), *key)
        assert tuple(int(v) for v in got[0]) == want


@backends
@both_precisions
def test_philox_bit_equal(backend, precision):
    """rtk::philox and rtk64::philox (bitop3 XORs and 64-bit products on the device) bit-equal to
    Philox4x32-10: the published vectors, counter words that make every hi / lo product carry, and
    2^16 random (pixel, sample, segment, event) counters under 16 random keys plus the all-zero and
    all-one keys (one key per call: the kernel keeps it in scalar registers)."""
    rng = np.random.default_rng(9)
    special = np.array([0, 1, 2, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff, 0x243f6a88, 0x13198a2e], np.uint32)
    grid = np.stack(np.meshgrid(special, special, special[[0, 6, 7]], special[[0, 6, 8]], indexing="ij"), -1).reshape(-1, 4)
    keys = [(0, 0), (0xffffffff, 0xffffffff), (0xa4093822, 0x299f31d0)] + \
        [tuple(int(v) for v in rng.integers(0, 1 << 32, 2)) for _ in range(16)]
    for i, (k0, k1) in enumerate(keys):
        ctr = np.concatenate([grid, np.array([[0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]], np.uint32),
                              rng.integers(0, 1 << 32, (4096, 4), dtype=np.uint64).astype(np.uint32)])
        got, = run(backend, precision, "philox", ctr, k0, k1)
        assert (got == philox_ref(ctr, k0, k1)).all(), (k0, k1)


@backends
@both_precisions
def test_u01_and_unit_vector(backend, precision):
    """u01(w) = (w >> 8) 2^-24 exactly and 1 - u01(w) in (0, 1] (w = 0 and 0xffffffff included);
    unit_vector(a, b): z = 1 - 2 u01(a) exactly and | |v|^2 - 1 | <= 8 eps."""
    real = real_of(precision)
    eps = float(np.finfo(real).eps)
    rng = np.random.default_rng(3)
    w = np.concatenate([np.array([0, 0xff, 0x100, 0xffffff00, 0xffffffff, 0x80000000], np.uint32),
                        rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32)])
    u, = run(backend, precision, "uniform", 0, w)
    assert (u.astype(np.float64) == (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).all()
    m, = run(backend, precision, "uniform", 1, w)
    assert (m.astype(np.float64) == 1.0 - u.astype(np.float64)).all() and (m > 0).all() and (m <= 1).all()
    assert m[0] == 1.0 and m[4] == 2.0 ** -24
    b = np.concatenate([w[::-1][:6], rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32)])
    v, = run(backend, precision, "unit_vector", w, b)
    assert (v[:, 2].astype(np.float64) == 1.0 - 2.0 * u.astype(np.float64)).all()
    vl = v.astype(LD)
    dev = float(np.abs((vl * vl).sum(1) - 1).max() / eps)
    measure(backend, f"unit_vector_{precision}", n=int(w.size), worst_norm_dev_in_eps=dev)
    assert dev <= 8.0
