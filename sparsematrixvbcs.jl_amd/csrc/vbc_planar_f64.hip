// Planar-kernel launchers, fp64 (with the split kernels, the lane pairs and the occupancy queries).
#define VBC_PLANAR_T double
#define VBC_PLANAR_SUFFIX f64
#include "vbc_planar_launch.inc"
