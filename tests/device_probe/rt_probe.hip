// rt_probe.hip — TEST TOOLING: the element-wise probes of probe_body.h as gfx950 kernels, so the
// tests call rt_trace.h's own functions (the device math, the primitive tests, Philox, the
// fixed-point conversion) on the device, built with the product's HIPFLAGS.  One 256-thread
// kernel per probe, thread i handles element i (i < n), no shared state.  The launchers take
// device pointers and a stream; they do not synchronise.  Never linked into librt_amd.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RT_PROBE_CAT2(a, b) a##b
#define RT_PROBE_CAT(a, b) RT_PROBE_CAT2(a, b)
#define RT_PROBE_DEFINE(name, params, args)                                                                          \
  __global__ __launch_bounds__(256) void k_##name(int n, RT_PROBE_UNPACK params) {                                   \
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);                                                            \
    if (i >= n) return;                                                                                              \
    pb_##name(i, RT_PROBE_UNPACK args);                                                                              \
  }                                                                                                                  \
  extern "C" int RT_PROBE_CAT(rt_probe_##name, RT_PROBE_SFX)(int n, RT_PROBE_UNPACK params, void* stream) {          \
    if (n <= 0) return 0;                                                                                            \
    hipLaunchKernelGGL(k_##name, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,            \
                       RT_PROBE_UNPACK args);                                                                        \
    return hipGetLastError() == hipSuccess ? 0 : -1;                                                                 \
  }

#define RT_F64 0
#include "../../raytrace_amd/csrc/rt_trace.h"
#define RT_PROBE_SFX _f32
namespace probe32 {
#include "probe_body.h"
}  // namespace probe32
#undef RT_PROBE_SFX
#undef RT_F64
#define RT_F64 1
#include "../../raytrace_amd/csrc/rt_trace.h"
#define RT_PROBE_SFX _f64
namespace probe64 {
#include "probe_body.h"
}  // namespace probe64
