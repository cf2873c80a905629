// rt_query64_ord.hip — the ordered ray-query kernel in binary64: the flat class and the launcher,
// rt_query64.hip's text with RT_QUERY_ORDERED (rt_query_kernel.h).
#include <algorithm>
#define RT_F64 1
#define RT_QUERY_PART 1
#define RT_QUERY_ORDERED 1
#include "rt_query_kernel.h"
