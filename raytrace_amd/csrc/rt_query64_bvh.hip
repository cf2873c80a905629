// rt_query64_bvh.hip — the ray-query kernel in binary64: the BVH classes (generic, triangle and
// sphere leaves, instancing), a unit of their own (rt_query_kernel.h RT_QUERY_PART 2).
#include <algorithm>
#define RT_F64 1
#define RT_QUERY_PART 2
#include "rt_query_kernel.h"
