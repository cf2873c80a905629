#!/usr/bin/env python3
"""How many dispatchable render-kernel classes the GPU suite's scenes launch, without and with the
class sweep: every scene the GPU render tests name (tests/test_gpu.py, test_gpu_full_spp.py,
test_adaptive_gpu.py's SCENES, test_denoise_gpu.py's FEATURE_SCENES, the known-answer and edge-case
scenes), with the experiment knobs some of those tests set, through the host's own dispatch
(tests/kernel_emu scene_variant, class_of).  No GPU.  profiles/class_sweep/README.md quotes the output.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("", "oracle", "tests", os.path.join("tests", "kernel_emu")):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

import class_scenes as CS  # noqa: E402
import emu  # noqa: E402
import raytrace_amd as R  # noqa: E402
import test_gpu as TG  # noqa: E402
from raytrace_amd import scenes  # noqa: E402
from test_oracle_golden import _kat_scene  # noqa: E402
from test_render_params import _instanced  # noqa: E402


def worlds():
    """(label, world, knobs) of every scene a GPU render test launches"""
    out = []
    for name, fn, kw, *_ in TG.CASES + TG.FULL:
        out.append((name, fn(**kw)[1], {}))
    for name, fn in TG.DETERMINISM_SCENES.items():
        out.append((name, fn()[1], {"RT_AMD_MEDIA_LATE": "0"} if name == "demo2_chain" else {}))
    for name in ("cornell_box", "pawn_fog", "bunny_cornell", "demo1"):  # test_kernel_variants_bitwise_identical
        out.append((name + " as BVH", getattr(scenes, name)(width=96, spp=8)[1], {"RT_AMD_VARIANT": "2", "RT_AMD_NO_BOX": "1"}))
    for name in ("bunny_cornell", "demo1", "pawn_fog"):  # test_one_class_leaf_kernels_are_exact
        out.append((name + " generic leaves", getattr(scenes, name)(width=96, spp=8)[1], {"RT_AMD_LEAF_KIND": "0"}))
    for name in ("pawn_fog", "demo2"):  # test_media_events_in_shading_phase_are_exact
        out.append((name + " chain", getattr(scenes, name)(width=80, spp=8)[1], {"RT_AMD_MEDIA_LATE": "0"}))
    out.append(("box_gallery", scenes.box_gallery()[1], {}))
    out.append(("noise_test", scenes.noise_test()[1], {}))
    out.append(("instance_gallery", scenes.instance_gallery()[1], {}))
    out.append(("image", TG._image_scene()[1], {}))
    out.append(("mixed_leaf", TG.mixed_leaf_scene()[1], {}))
    out.append(("instanced", _instanced()[1], {}))
    out.append(("bunny_instances baked", R.flatten(scenes.bunny_instances(n=3)[1], instance_min=0), {}))
    for mats in (False, True):  # test_deep_bvh_against_oracle
        objs = [R.lambertian(R.constantTexture(0.5)) << R.sphere((0, -1000.5, -1), 1000)]
        objs += [R.lambertian(R.constantTexture((0.8, 0.3, 0.2))) << R.sphere((0.3 * (k % 3 - 1), 0.0, -2.0 - 8.0 ** k), 0.2)
                 for k in range(40)]
        if mats:
            objs.append(R.metal(0.2, R.constantTexture(0.8)) << R.sphere((0.6, 0.1, -2.5), 0.3))
        out.append((f"deep_bvh mats={mats}", R.group(objs), {}))
    # test_all_materials_against_oracle's classes: a checker floor, the full material set, two media spheres
    out.append(("all_materials", R.group([
        R.lambertian(R.checkerTexture(10, 10, 0.2, 0.9)) << R.parallelogram((-10, -1, -10), (20, 0, 0), (0, 0, 20)),
        R.metal(0.3, R.constantTexture(0.8)) << R.sphere((0, -0.5, -4), 0.45),
        R.isotropic(R.constantTexture(0.8)) << R.constantMedium(1.5, R.sphere((1, -0.5, -4), 0.45))]), {}))
    for kind in ("sphere", "triangle", "parallelogram", "mirror"):
        out.append(("kat " + kind, _kat_scene(kind)[1], {}))
    return out


def main():
    before = {"f32": set(), "f64": set()}
    for label, world, knobs in worlds():
        for k in [k for k in os.environ if k.startswith("RT_AMD_")]:
            del os.environ[k]
        if knobs:
            os.environ.update(knobs, RT_AMD_EXPERIMENTS="1")
        v = emu.scene_variant(world)
        for p in before:
            fields, _, compiled = emu.class_of(p, v)
            if fields[0] in (0, 2) and compiled:
                before[p].add(CS.from_fields(fields))
        print(f"{label:32s} variant {v:5d}  {CS.class_id(CS.from_fields(emu.class_of('f64', v)[0]))}")
    for k in [k for k in os.environ if k.startswith("RT_AMD_")]:
        del os.environ[k]
    for p in ("f32", "f64"):
        every = set(CS.enumerated_classes(p))
        swept = {c for c, q in CS.all_cases() if q == p}
        print(f"{p}: {len(every)} dispatchable classes; launched before the sweep {len(before[p] & every)}, "
              f"with the sweep {len((before[p] | swept) & every)}")


if __name__ == "__main__":
    main()
