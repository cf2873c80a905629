"""The ring form of the flat lane loop without a GPU: its work plan (rt_build.cpp rt_host_plan_ring)
makes an item id one sample of a linear stream over the shard, pixel-major and sample-minor, which
the kernel decodes with open_item (rt_trace.h)."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "raytrace_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "flat_ring")
CXXFLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]


def test_stream_ids_cover_every_sample_once(tmp_path):
    """7x5 and 16x9 pixels, spp 1, 3, 63, 64, 65, 130, depth 8 / 1 / 0, a later film pass, three shards
    of 2-row blocks (padding rows), both pool sizes, and 144 random (width, height, spp, shards,
    row_block, sample0) tuples: every (pixel, sample) of the shard is exactly one id, padding rows
    and a render without depth get none, an aggregated pool fits its slot; the other classes, an
    image of 2.4e9 samples and RT_AMD_FLAT_RING=0 keep the legacy plan."""
    exe = str(tmp_path / "stream_cover")
    cmd = ["g++", *CXXFLAGS, "-o", exe, os.path.join(SRC, "stream_cover.cpp"), os.path.join(CSRC, "rt_build.cpp"),
           os.path.join(CSRC, "rt_bvh.cpp"), "-lm", "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("RT_AMD_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-4000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) > 100000
