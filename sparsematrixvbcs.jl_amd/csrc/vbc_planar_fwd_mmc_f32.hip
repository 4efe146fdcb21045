// spmm_planar_fwd_col launchers, fp32 (the lane pairs have no fp32 form).
#define VBC_PLANAR_T float
#define VBC_PLANAR_SUFFIX f32
#define VBC_PLANAR_FWD
#include "vbc_planar_mmc_launch.inc"
