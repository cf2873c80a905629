// rt_list.hip — the pixel-list kernel in FP32 (rt_list_kernel.h; rt_list64_nl.hip builds the binary64
// one from the same text): whole paths of listed pixels, the render half of an adaptive film pass
// (rt_adaptive.h).
#include <algorithm>
#define RT_F64 0
#include "rt_list_kernel.h"
