// rt_radiance_ord.hip — the ordered radiance-query kernel (include/rt.h rt_scene_radiance_ordered) in
// FP32: rt_radiance.hip's path kernel with RT_RADIANCE_ORDERED (rt_radiance_kernel.h).
#include <algorithm>
#define RT_F64 0
#define RT_RADIANCE_ORDERED 1
#include "rt_radiance_kernel.h"
