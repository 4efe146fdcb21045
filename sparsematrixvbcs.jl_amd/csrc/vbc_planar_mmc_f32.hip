// spmm_planar_col launchers, fp32 (the lane-pair layout is fp64 only).
#define VBC_PLANAR_T float
#define VBC_PLANAR_SUFFIX f32
#include "vbc_planar_mmc_launch.inc"
