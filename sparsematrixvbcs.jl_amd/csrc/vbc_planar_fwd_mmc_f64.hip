// spmm_planar_fwd_col / spmm_pair_col<..., DOT> launchers, fp64.
#define VBC_PLANAR_T double
#define VBC_PLANAR_SUFFIX f64
#define VBC_PLANAR_FWD
#include "vbc_planar_mmc_launch.inc"
