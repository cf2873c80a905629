// rt_radiance.hip — the radiance-query kernels in FP32 (rt_radiance_kernel.h; rt_radiance64_nl.hip
// builds the binary64 ones from the same text): whole paths from the caller's rays (include/rt.h
// rt_scene_radiance) and the render's camera rays as records (rt_scene_camera_rays).
#include <algorithm>
#define RT_F64 0
#include "rt_radiance_kernel.h"
