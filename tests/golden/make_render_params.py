"""Freezes the kernel arguments of the cases of tests/test_render_params.py into
tests/golden/render_params.json (tests/kernel_emu rt_emu_render_params).

The file pins the one fill function (rt_build.cpp rt_host_render_params) to the hand-written fill it
replaced, so it was recorded BEFORE that function existed: on commit 6e0061e with only the probe entry
added — emu_body.h's render() split into params() + render() without touching a line of the fill, and
the probe calling rt_host_match_target on the result, which is what that commit's lane loop computed
from the same arguments on entry.  Running this script on a later tree rewrites the file from the
code under test, which is not a pin.

  python tests/golden/make_render_params.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    for k in [k for k in os.environ if k.startswith("RT_AMD_")]:
        del os.environ[k]
    for p in (ROOT, os.path.join(ROOT, "tests", "kernel_emu"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import emu
    import test_render_params as T

    rows = []
    for case, (name, precision, layout, knob) in T.cases().items():
        if knob:
            os.environ["RT_AMD_EXPERIMENTS"] = "1"
            key, value = knob.split("=")
            os.environ[key] = value
        got = T.params(emu, name, precision, layout)
        if knob:
            del os.environ["RT_AMD_EXPERIMENTS"], os.environ[key]
        rows.append(f"  {json.dumps(case)}: {json.dumps(got)}")
        print(case, got["target_defer"], got["target_rec"], got["n_big_chunks"], flush=True)
    source = "the emulator's hand-written fill of commit 6e0061e (tests/golden/make_render_params.py)"
    with open(os.path.join(HERE, "render_params.json"), "w") as f:  # one line per case
        f.write('{\n "source": %s,\n "cases": {\n%s\n }\n}\n' % (json.dumps(source), ",\n".join(rows)))


if __name__ == "__main__":
    main()
