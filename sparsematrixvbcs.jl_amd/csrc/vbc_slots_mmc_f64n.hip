// spmm_slots_col launchers, fp64 compute on Float32 stored values (VBC_CREATE_NARROW_VALUES).
#define VBC_SLOTS_T double
#define VBC_SLOTS_S float
#define VBC_SLOTS_SUFFIX f64n
#define VBC_SLOTS_COL
#include "vbc_slots_mm_launch.inc"
