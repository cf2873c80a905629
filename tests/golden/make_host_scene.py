"""Freezes the host scene builder's output into tests/golden/host_scene.json: for every scene of
tests/test_host_build.py the per-array (length, FNV-1a) digests of HostScene in both precisions
(tests/kernel_emu rt_emu_scene_digest), and for every single-defect scene the return code and the
message.

The file pins a restructured builder to the one before it, so it is recorded from the PARENT's
rt_build.cpp, never from the tree under test.  The digest export only reads HostScene, so this
tree's rt_emu.cpp compiles against the older builder:

  git archive <parent commit> raytrace_amd/csrc include | tar -x -C <dir>
  python tests/golden/make_host_scene.py --csrc <dir>/raytrace_amd/csrc

(recorded from commit 0bc6d27, the builder as one 530-line function).
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
EMU = os.path.join(ROOT, "tests", "kernel_emu")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", required=True, help="raytrace_amd/csrc of the builder to record from")
    ap.add_argument("--out", default=os.path.join(HERE, "host_scene.json"))
    args = ap.parse_args()
    lib = os.path.join(EMU, "_build", "librt_emu_recorded.so")
    subprocess.run(["make", "-C", EMU, "-s", "CSRC=" + os.path.abspath(args.csrc), "OUT=" + lib], check=True)
    os.environ["RT_EMU_LIB"] = lib
    for k in [k for k in os.environ if k.startswith("RT_AMD_")]:
        del os.environ[k]
    for p in (ROOT, EMU, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import emu
    import test_host_build as T

    out = {"source": "rt_host_build_scene of commit 0bc6d27 (tests/golden/make_host_scene.py)",
           "items": emu.DIGEST_ITEMS, "digests": {}, "errors": {}}
    for case, scene, knob in T.digest_cases():
        if knob:
            os.environ["RT_AMD_EXPERIMENTS"] = "1"
            name, value = knob.split("=")
            os.environ[name] = value
        rc, err, items = emu.scene_digest(scene())
        if knob:
            del os.environ["RT_AMD_EXPERIMENTS"], os.environ[name]
        assert rc == 0, (case, rc, err)
        out["digests"][case] = items
        print(case, items["scalars"], flush=True)
    for name in T.DEFECTS:
        out["errors"][name] = T.defect_result(emu, name)
        print(name, out["errors"][name], flush=True)
    with open(args.out, "w") as f:  # one line per case
        f.write('{\n "source": %s,\n "items": %s,\n' % (json.dumps(out["source"]), json.dumps(out["items"])))
        for key in ("digests", "errors"):
            rows = [f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in out[key].items()]
            f.write(' "%s": {\n%s\n }%s\n' % (key, ",\n".join(rows), "," if key == "digests" else ""))
        f.write("}\n")


if __name__ == "__main__":
    main()
