// rt_query.hip — the ray-query kernel (include/rt.h rt_scene_cast) in FP32, every class
// (rt_query_kernel.h; rt_query64.hip and rt_query64_bvh.hip build the binary64 ones from the same text).
#include <algorithm>
#define RT_F64 0
#define RT_QUERY_PART 0
#include "rt_query_kernel.h"
