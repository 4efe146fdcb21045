// spmm_planar_col / spmm_pair_col launchers, fp64.
#define VBC_PLANAR_T double
#define VBC_PLANAR_SUFFIX f64
#include "vbc_planar_mmc_launch.inc"
