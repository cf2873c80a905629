"""Every dispatchable render-kernel class on the host (no GPU): the table's argument space is walked
through the product's own rt_host_variant and rt_class_of (tests/kernel_emu exports), every class has a
scene that reaches it from the public constructors (tests/class_scenes.py), and the host emulator of the
kernel logic renders each of those scenes against the FP64 oracle under tests/test_gpu.py's bars.

The device sweep (tests/test_class_sweep_gpu.py) renders the same scenes; here the scenes themselves are
held to more than the bars, so that the device's share of a bar is not spent by the scene: the binary64
host render matches the oracle on every pixel, and the FP32 host render clears its bar by a percent
(every pixel where the bar is 0.99)."""
import collections
import functools

import numpy as np
import pytest

import class_scenes as CS
from test_gpu import assert_parity

CASES = CS.all_cases()
IDS = [f"{CS.class_id(c)}-{p}" for c, p in CASES]
# dispatchable classes per precision (rt_kernel_class.h at the time of writing; ISSUE: 72 + 91 = 163)
COUNTS = {"f32": {"flat": 12, "bvh": 34, "inst": 18, "narrow": 8, "all": 72},
          "f64": {"flat": 12, "bvh": 34, "inst": 18, "narrow": 27, "all": 91}}


def test_enumeration_finds_every_dispatchable_class(emu_mod):
    """The scalar rt_host_variant over flat x media x {tex 0, 1, noise} x mats x inst x leaf kind x
    media_late x {shallow, deep}, each code through rt_class_of in both precisions: 72 FP32 and 91
    binary64 classes, every one compiled.  A class added to the table later changes these counts, and
    then needs a scene in class_scenes.scene_of."""
    for precision in ("f32", "f64"):
        found = CS.enumerated_classes(precision)
        groups = collections.Counter("narrow" if c[5] else c[0] for c in found)
        groups["all"] = len(found)
        assert dict(groups) == COUNTS[precision], (precision, dict(groups))
        for cls, (fields, block, compiled) in found.items():
            assert compiled, (precision, cls)
            assert CS.to_fields(cls) == fields
            assert block == 512 if cls[5] else block in (64, 256, 768, 1024), (cls, block)
            assert block == 64 if cls[0] == "flat" else block >= 256, (cls, block)
    # the stack depths of the walk stand on either side of the twin's threshold, and a scene's variant
    # is one of the walk's codes
    shallow = emu_mod.variant_of(0, 0, 0, 0, 0, 0, 2, 0, 22)
    assert emu_mod.variant_of(0, 0, 0, 0, 0, 0, 2, 0, 23) == shallow | 1024
    assert CS.SHALLOW_STACK < 22 and CS.DEEP_STACK >= 23


def test_generated_and_unreachable_classes_are_the_enumerated_ones():
    for precision in ("f32", "f64"):
        want = set(CS.enumerated_classes(precision))
        generated = {c for c, p in CASES if p == precision}
        unreachable = {c for c, p in CS.UNREACHABLE if p == precision}
        assert not (generated & unreachable)
        assert generated | unreachable == want
    assert len(CS.UNREACHABLE) == 0  # reviewed as empty; an entry carries its reason from the builder


@functools.lru_cache(maxsize=None)
def variant(cls):
    import emu
    return emu.scene_variant(CS.scene_of(cls)[1])


@pytest.mark.parametrize("cls,precision", CASES, ids=IDS)
def test_scene_of_reaches_its_class(emu_mod, cls, precision):
    """scene_of(cls) flattens, builds, and the library's own dispatch gives it exactly cls."""
    fields, block, compiled = emu_mod.class_of(precision, variant(cls))
    assert CS.from_fields(fields) == cls, (CS.class_id(cls), CS.class_id(CS.from_fields(fields)))
    assert compiled and block == CS.enumerated_classes(precision)[cls][1]
    info = emu_mod.scene_info(CS.scene_of(cls)[1])
    assert info["n_prims"] <= 200, info  # tiny scenes: tens of primitives, a hundred where the class needs them
    assert bool(info["flat"]) == (cls[0] == "flat")
    if cls[0] != "flat":
        assert info["n_nodes"] > 0, info  # a BVH to traverse, not a prefix alone


@functools.lru_cache(maxsize=None)
def oracle_frame(cls):
    import oracle
    cs, world, seed, _ = CS.scene_of(cls)
    ref = oracle.render(cs, world, seed, mode=oracle.RNG_PHILOX)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("cls,precision", CASES, ids=IDS)
def test_emulator_matches_oracle(emu_mod, oracle_mod, cls, precision):
    """48 x 32 at 4 spp: the host build of the class's lane loop against the oracle on the same Philox
    numbers, under assert_parity's per-pixel, worst-pixel and mean bars (a narrow twin runs its wide
    class's lane loop on the host, on the twin's own deep scene).  And the scene's own margin: every
    binary64 pixel within 1e-9, the FP32 share a percent above its bar."""
    cs, world, seed, lmax = CS.scene_of(cls)
    ref = oracle_frame(cls)
    assert ref.shape == (CS.HEIGHT, CS.WIDTH, 3)
    sky = np.abs(ref - ref[:1, :1]).max(-1) < 0.2  # (the top-left pixel sees the sky)
    assert 0.02 < sky.mean() < 0.5, float(sky.mean())  # hits and misses
    img = emu_mod.render(cs, world, seed, precision=precision)
    need = CS.need32(cls)
    assert_parity(img, ref, precision, need, None, CS.class_id(cls), CS.SPP, lmax)
    d = np.abs(img.astype(np.float64) - ref)
    if precision == "f64":
        assert ((d / np.maximum(np.abs(ref), 1e-3)).max(-1) <= 1e-9).all()
    else:
        frac = float(((d / np.maximum(np.abs(ref), 1.0)).max(-1) < 1e-3).mean())
        assert frac >= min(1.0, need + 0.01), frac
