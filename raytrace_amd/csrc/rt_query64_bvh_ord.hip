// rt_query64_bvh_ord.hip — the ordered ray-query kernel in binary64: the BVH classes,
// rt_query64_bvh.hip's text with RT_QUERY_ORDERED (rt_query_kernel.h).
#include <algorithm>
#define RT_F64 1
#define RT_QUERY_PART 2
#define RT_QUERY_ORDERED 1
#include "rt_query_kernel.h"
