// pred_equiv.cpp — TEST TOOLING: the hit tests of raytrace_amd/csrc/rt_trace.h whose validity rules
// are compares (RT_VALID_MARGINS=0, the product's form) or margins (=1), on the host.  A stand-alone
// program: tests/test_valid_pred_host.py builds it once per form (g++ -ffp-contract=off) and compares
// the two outputs line by line.  Cases: pred_body.h.  Never linked into librt_amd.so.
#define RT_HOST_EMU 1
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../include/rt.h"
#include "../../raytrace_amd/csrc/rt_internal.h"

#define RT_F64 0
#include "../../raytrace_amd/csrc/rt_trace.h"
namespace pred32 {
#include "pred_body.h"
}  // namespace pred32
#undef RT_F64
#define RT_F64 1
#include "../../raytrace_amd/csrc/rt_trace.h"
namespace pred64 {
#include "pred_body.h"
}  // namespace pred64

namespace rt_emu {
thread_local long long counters[4];
}

int main() {
  std::printf("form margins=%d\n", RT_VALID_MARGINS);
  pred32::run_all();
  pred64::run_all();
  return 0;
}
