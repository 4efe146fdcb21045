// spmm_slots_col launchers, fp32.
#define VBC_SLOTS_T float
#define VBC_SLOTS_SUFFIX f32
#define VBC_SLOTS_COL
#include "vbc_slots_mm_launch.inc"
