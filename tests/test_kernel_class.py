"""raytrace_amd/csrc/rt_kernel_class.h: the table from a variant code to the render kernel's class
and launch shape.  The kernel takes its launch bound, occupancy floor, stack stride and LDS layout
from this header and the host launches with the same functions; here the whole mapping is pinned,
for both precisions and every variant code, to what the hand-written macros and their run-time
mirror gave before the table existed (tests/golden/kernel_class.json, recorded from that commit)."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "raytrace_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_class.json")
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CXX is None, reason="no C++ compiler")

RT_VAR_BASE, RT_VAR_FLAT, RT_VAR_BVH_LOCKSTEP, RT_VAR_INST = 3, 0, 1, 64

# one row per precision and variant code, the golden's columns in order
PROGRAM = r"""
#include <stdio.h>
#include "rt_kernel_class.h"
int main(void) {
  for (int f64 = 0; f64 < 2; ++f64)
    for (int v = 0; v < 2048; ++v) {
      if ((v & RT_VAR_BASE) == RT_VAR_BASE) continue;
      const KernelClass c = rt_class_of(f64, v);
      printf("%d %d %d %d %d %d %d %d %d %d %d", f64, v, c.leaf, rt_class_waves(f64, c), rt_class_block(f64, c),
             (int)rt_class_fixed_lds(f64, c), (int)rt_class_acc_lds(f64, c), (int)!rt_class_nolicm(f64, c), c.media,
             rt_class_agg_slots(f64, c), rt_class_agg_pix(f64, c));
      const int depths[4] = {1, 22, 23, 64}, nodes[2] = {0, 100};
      for (int d : depths)
        for (int n : nodes) printf(" %zu", rt_class_lds_bytes(f64, c, d, n));
      printf(" %d\n", (int)rt_class_compiled(f64, c));
    }
  return 0;
}
"""


def build(tmp_path, *defs):
    src, exe = tmp_path / "kernel_class.cpp", tmp_path / "kernel_class"
    src.write_text(PROGRAM)
    subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, *defs, "-o", str(exe), str(src)], check=True)
    return str(exe)


def test_mapping_equals_the_recorded_one(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, check=True).stdout
    got = {}
    for line in out.splitlines():
        f = [int(x) for x in line.split()]
        assert f[-1] == 1, f"variant {f[1]} (f64 {f[0]}): rt_class_of names a class that is not compiled"
        got[(f[0], f[1])] = f[2:-1]
    golden = json.load(open(GOLDEN))
    ncol = len(golden["columns"])
    codes = [v for v in range(2048) if v & RT_VAR_BASE != RT_VAR_BASE]
    assert len(codes) == 1536 and len(got) == 2 * len(codes)
    tu = golden["columns"].index("in_main_unit")
    for f64, name in ((0, "f32"), (1, "f64")):
        rows, index = golden[name]["rows"], golden[name]["index"]
        assert len(index) == len(codes) and all(len(r) == ncol for r in rows)
        want = {v: rows[i] for v, i in zip(codes, index)}
        for v in codes:
            exp = want[v]
            if v & RT_VAR_BASE == RT_VAR_FLAT and v & RT_VAR_INST:
                # The one set of codes on which the recorded commit contradicted itself (no scene
                # gets them: instances run on a BVH base): its launch-shape functions described the
                # flat kernel, its dispatch returned an instanced decoupled BVH kernel.  The table
                # launches what it dispatches: the instanced kernel with the media mode of a base
                # other than RT_VAR_BVH, which is the recorded row of the same flags on the lockstep
                # base, in the unit the recorded dispatch's kernel was in.
                exp = want[(v & ~RT_VAR_BASE) | RT_VAR_BVH_LOCKSTEP]
                assert exp[tu] == want[v][tu], (name, v)
            assert got[(f64, v)] == exp, (name, v, dict(zip(golden["columns"], zip(got[(f64, v)], exp))))


def test_header_compiles_with_the_lockstep_kernels(tmp_path):
    """the experiment build's and the host emulator's setting: the header's static_asserts hold"""
    build(tmp_path, "-DRT_LOCKSTEP_KERNELS=1")
