// rt_radiance64_ord_nl.hip — the ordered radiance-query kernel in binary64: rt_radiance64_nl.hip's
// path kernel with RT_RADIANCE_ORDERED (rt_radiance_kernel.h), compiled without MachineLICM like it.
#include <algorithm>
#define RT_F64 1
#define RT_RADIANCE_ORDERED 1
#include "rt_radiance_kernel.h"
