// rt_list64_nl.hip — the pixel-list kernel in binary64 (rt_list_kernel.h, as rt_list.hip), compiled
// without MachineLICM like rt_features64_nl.hip (Makefile NOLICM): with the pass every class hoists
// its binary64 constants out of the sample loop (up to 256 VGPRs and 99 spilled SGPRs); without it
// the heaviest class takes 158 VGPRs and no kernel spills a VGPR.
#include <algorithm>
#define RT_F64 1
#include "rt_list_kernel.h"
