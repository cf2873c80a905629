// rt_radiance64_nl.hip — the radiance-query kernels in binary64 (rt_radiance_kernel.h, as
// rt_radiance.hip), compiled without MachineLICM like rt_list64_nl.hip (Makefile NOLICM): the path
// body is rt_list.h's, whose binary64 classes the pass drives into spills.
#include <algorithm>
#define RT_F64 1
#include "rt_radiance_kernel.h"
