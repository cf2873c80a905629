// rt_features.hip — the film's first-hit feature kernel in FP32 (rt_features_kernel.h;
// rt_features64_nl.hip builds the binary64 one from the same text): albedo, normal, depth and hit
// count of the primary rays, the guides of the denoiser (rt_denoise.h).
#include <algorithm>
#define RT_F64 0
#include "rt_features_kernel.h"
