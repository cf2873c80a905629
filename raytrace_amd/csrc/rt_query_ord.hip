// rt_query_ord.hip — the ordered ray-query kernel (include/rt.h rt_scene_cast_ordered) in FP32, every
// class: rt_query.hip's text with RT_QUERY_ORDERED (rt_query_kernel.h).
#include <algorithm>
#define RT_F64 0
#define RT_QUERY_PART 0
#define RT_QUERY_ORDERED 1
#include "rt_query_kernel.h"
