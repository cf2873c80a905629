"""The closest hit's validity rules as compares (rt_trace.h RT_VALID_MARGINS=0, the product's form)
against the same rules as margins (RT_VALID_MARGINS=1), on the host.

tests/valid_pred/pred_equiv.cpp is built twice over rt_trace.h under RT_HOST_EMU (g++
-ffp-contract=off), once per form; each program prints one line per case — the decision and the bits
of t (pred_body.h lists the cases: isect_plane<1> with and without the target term, test_box<true>
and test_box<false> on an axis-aligned record, one rotated about y, a doubly rotated one and the
room with its missing face; both precisions; test_box<false>, the BVH kernels' surface prefix, keeps
the margins in both builds).  The two outputs must be equal line by line on every
case whose operands (t, a, b; the box's entry and exit) hold no NaN; a case with a NaN operand is
rejected by the compare form whatever the margins made of it.

The emulator's frames are those of the commit before the rewrite (tests/golden/valid_pred_frames.json).
"""
import collections
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

SRC = os.path.join(ROOT, "tests", "valid_pred")


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """{form: lines} of the two builds of pred_equiv.cpp"""
    d = tmp_path_factory.mktemp("valid_pred")
    out = {}
    for form in (0, 1):
        exe = str(d / f"pred_equiv_{form}")
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-ffp-contract=off", f"-DRT_VALID_MARGINS={form}", "-o", exe,
                        os.path.join(SRC, "pred_equiv.cpp"), "-lm"], check=True)
        lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
        assert lines[0] == f"form margins={form}", lines[0]
        out[form] = lines[1:]
    return out


def family(line):
    w = line.split()
    return " ".join(w[:4] if w[1].startswith("box_") else w[:3])


def test_compares_decide_as_margins_did(outputs):
    cmp_, mar = outputs[0], outputs[1]
    assert len(cmp_) == len(mar) > 500000
    total, accepted, with_nan, differ = (collections.Counter() for _ in range(4))
    bad = []
    for a, b in zip(cmp_, mar):
        f = family(a)
        total[f] += 1
        nan = a.endswith("nan=1")
        assert nan == b.endswith("nan=1")  # (the operands are the same numbers in both builds)
        if nan:
            with_nan[f] += 1
            if "dec=1" in a or "take=1" in a:  # the NaN rule: the compare form rejects
                bad.append(("nan accepted", a))
            differ[f] += a != b
        else:
            accepted[f] += "dec=1" in a
            if a != b:  # same decision, same bits of t, same face / target term
                bad.append((a, b))
    assert not bad, (len(bad), bad[:6])
    # every family is there in both precisions, and decides both ways
    for prec in ("f32", "f64"):
        for tgt in ("tgt0", "tgt1"):
            assert total[f"{prec} random {tgt}"] == 1 << 16
            assert 0.3 < accepted[f"{prec} random {tgt}"] / (1 << 16) < 0.5
            for fam in ("ab_edge", "t_edge", "denom_edge", "target_t"):
                k = f"{prec} {fam} {tgt}"
                assert 0 < accepted[k] < total[k], k
        for rec in ("aligned", "rot_y", "rot_xy", "room"):
            for key in ("key0", "key1"):
                k = f"{prec} box_random {rec} {key}"
                assert total[k] == 1 << 14 and 0.5 < accepted[k] / total[k] < 0.9, (k, accepted[k])
                k = f"{prec} box_parallel {rec} {key}"
                assert 0 < accepted[k] < total[k], k
        for key in ("key0", "key1"):
            k = f"{prec} box_edge unit {key}"  # tf == tn and one ulp below meet the box, one ulp above misses
            assert accepted[k] * 3 == total[k], (k, accepted[k], total[k])
            assert total[f"{prec} box_overflow unit {key}"] == 12 and accepted[f"{prec} box_overflow unit {key}"] == 0
        # the cases with a NaN operand: listed apart; the margins accepted some of them (fmin drops a NaN)
        n_nan = sum(v for k, v in with_nan.items() if k.startswith(prec))
        n_diff = sum(v for k, v in differ.items() if k.startswith(prec))
        assert n_nan >= 40 and 0 < n_diff < n_nan, (prec, n_nan, n_diff)


def test_constructed_edges_decide_as_stated(outputs):
    """t at tmin_up and |n . d| at 1e-8 in the compare form: the interval is open at tmin (t >= tmin_up), the
    denominator's bound closed for the hit and open for the target term."""
    lines = outputs[0]
    for prec in ("f32", "f64"):
        t_edge = [l for l in lines if l.startswith(f"{prec} t_edge tgt0 ")]
        assert len(t_edge) == 24
        # per tmin: T = tmin, tmin_up, up(tmin_up), dn(tmin), 0, -tmin_up
        assert ["dec=1" in l for l in t_edge] == [False, True, True, False, False, False] * 4
        den = [l for l in lines if l.startswith(f"{prec} denom_edge tgt1 ")]
        # delta = e, up(e), dn(e), -e, -up(e), -dn(e), 0, -0, 1e-30, -1e-30
        assert ["dec=1" in l for l in den] == [True, True, False, True, True, False, False, False, False, False]
        zero = "tg=0"
        assert [not l.split()[7] == zero for l in den] == [False, True, False, False, True, False, False, False, False, False]
        tg = [l for l in lines if l.startswith(f"{prec} target_t tgt1 ")]
        # T = 0, up(0), 1e-6, tmin, tmin_up, -1e-6 (not self, self): a target hit for every t > 0, self or not
        # (the smallest denormal's t^2 underflows: its term is 0 as well)
        assert [not l.split()[7] == zero for l in tg] == [False] * 4 + [True] * 6 + [False] * 2
        assert ["dec=1" in l for l in tg] == [False] * 8 + [True, False] + [False] * 2


with open(os.path.join(GOLDEN, "valid_pred_frames.json")) as _f:
    FRAMES = json.load(_f)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", ["cornell", "box_gallery"])
def test_emulator_frames_are_the_parents(emu_mod, name, precision):
    """The host emulator's frame, byte for byte the one the commit before the rewrite renders (recorded
    from that commit's tree): Cornell 64 px wide at 16 spp, box_gallery 48 px wide at 8 spp, depth 50."""
    from raytrace_amd import scenes
    cs, world, seed = (scenes.cornell_box(spp=16, width=64, depth=50) if name == "cornell"
                       else scenes.box_gallery(width=48, spp=8, depth=50))
    img = emu_mod.render(cs, world, seed, precision=precision)
    assert np.isfinite(img).all() and img.mean() > 0
    got = hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest()[:16]
    assert got == FRAMES["emulator"][f"{name}/{precision}"], (name, precision, got)
