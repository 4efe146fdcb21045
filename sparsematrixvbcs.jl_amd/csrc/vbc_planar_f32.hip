// Planar-kernel launchers, fp32 (with the split kernels and the occupancy queries; no lane pairs).
#define VBC_PLANAR_T float
#define VBC_PLANAR_SUFFIX f32
#include "vbc_planar_launch.inc"
