// spmm_slots_col launchers, fp32.
#define VBC_SLOTS_T float
#define VBC_SLOTS_SUFFIX f32
#include "vbc_slots_mmc_launch.inc"
