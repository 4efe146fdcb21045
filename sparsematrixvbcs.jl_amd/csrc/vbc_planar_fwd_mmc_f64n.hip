// spmm_planar_fwd_col / spmm_pair_col<..., DOT> launchers, fp64 compute on Float32 stored values
// (VBC_CREATE_NARROW_PLANAR, VBC_CREATE_NARROW_PAIRS).
#define VBC_PLANAR_T double
#define VBC_PLANAR_S float
#define VBC_PLANAR_SUFFIX f64n
#define VBC_PLANAR_FWD
#include "vbc_planar_mmc_launch.inc"
