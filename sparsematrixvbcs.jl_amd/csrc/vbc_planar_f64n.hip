// Planar-kernel launchers, fp64 compute on Float32 stored values read as floats and widened in registers: row chunks
// and forward row runs (VBC_CREATE_NARROW_PLANAR), lane pairs (VBC_CREATE_NARROW_PAIRS) and lane streams
// (VBC_CREATE_NARROW_STREAMS).  No split form.
#define VBC_PLANAR_T double
#define VBC_PLANAR_S float
#define VBC_PLANAR_SUFFIX f64n
#include "vbc_planar_launch.inc"
