// rt_features64_nl.hip — the film's first-hit feature kernel in binary64 (rt_features_kernel.h, as
// rt_features.hip), compiled without MachineLICM like the heavier render classes (Makefile NOLICM;
// rt_kernel_class.h rt_class_nolicm): with the pass the texture and noise classes hoist their
// binary64 constants out of the sample loop into up to 256 VGPRs and spill SGPRs; without it every
// class fits 156 VGPRs with no spills of either kind.
#include <algorithm>
#define RT_F64 1
#include "rt_features_kernel.h"
