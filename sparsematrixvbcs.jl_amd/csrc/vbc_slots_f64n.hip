// Slotted-kernel launchers, fp64 compute on Float32 stored values (VBC_CREATE_NARROW_VALUES): the kernels of
// vbc_slots_f64.hip with the value stream read as floats and widened in registers.  U = 8 rows per step as
// the wide kernel: 16 rows (the wide kernel's value bytes in flight per wave) measured slower on the FE-2D
// matrix, 116.5 against 109.4 us per B'x (narrow value storage).
#define VBC_SLOTS_T double
#define VBC_SLOTS_S float
#ifndef VBC_SLOTS_NARROW_U
#define VBC_SLOTS_NARROW_U 8
#endif
#define VBC_SLOTS_U VBC_SLOTS_NARROW_U
#define VBC_SLOTS_SUFFIX f64n
#define VBC_SLOTS_NO_OCCUPANCY
#define VBC_SLOTS_NO_NARROW2
#include "vbc_slots_launch.inc"
