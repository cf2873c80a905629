// rt_query64.hip — the ray-query kernel in binary64: the flat class and the launcher
// (rt_query_kernel.h, as rt_query.hip); the BVH classes are rt_query64_bvh.hip's.
#include <algorithm>
#define RT_F64 1
#define RT_QUERY_PART 1
#include "rt_query_kernel.h"
