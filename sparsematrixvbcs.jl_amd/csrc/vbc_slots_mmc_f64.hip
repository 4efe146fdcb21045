// spmm_slots_col launchers, fp64.
#define VBC_SLOTS_T double
#define VBC_SLOTS_SUFFIX f64
#define VBC_SLOTS_COL
#include "vbc_slots_mm_launch.inc"
