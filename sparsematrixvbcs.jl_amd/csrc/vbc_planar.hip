// Dispatch of the planar-kernel launchers by value type (the kernels live in vbc_planar_f64.hip, vbc_planar_f32.hip
// and vbc_planar_f64n.hip -- fp64 on Float32 stored values -- one translation unit each, all of vbc_planar_launch.inc).
#include <hip/hip_runtime.h>

#include "vbc_kernels.h"

namespace vbc {

typedef int PlanarLaunch(const SlotBin &hb, bool faste, bool staged, const void *x, void *y, double alpha, double beta,
                         bool rd, hipStream_t s);
typedef int SplitMultiLaunch(const SplitMulti &M, int P, const void *x, void *y, double alpha, double beta, bool rd,
                             hipStream_t s);
PlanarLaunch launch_planar_f64, launch_planar_f32, launch_planar_f64n;
SplitMultiLaunch launch_split_multi_f64, launch_split_multi_f32;
int occupancy_planar_f64(), occupancy_planar_f32();
int occupancy_lanes_f64(), occupancy_lanes_f32();
int occupancy_split_multi_f64(int P), occupancy_split_multi_f32(int P);

int launch_planar(int esz, const SlotBin &hb, bool faste, bool staged, const void *x, void *y, double alpha, double beta,
                  bool rd, hipStream_t s)
{
    if (hb.nranges <= 0) return (int)hipSuccess;
    if (hb.vsz) {  // Float32 stored values on an fp64 handle; any other pair has no kernel and is an error
        if (esz != 8) return (int)hipErrorInvalidValue;
        return launch_planar_f64n(hb, faste, staged, x, y, alpha, beta, rd, s);
    }
    return esz == 8 ? launch_planar_f64(hb, faste, staged, x, y, alpha, beta, rd, s)
                    : launch_planar_f32(hb, faste, staged, x, y, alpha, beta, rd, s);
}

int launch_split_multi(int esz, const SplitMulti &M, int P, const void *x, void *y, double alpha, double beta, bool rd,
                       hipStream_t s)
{
    if (M.nchunks <= 0) return (int)hipSuccess;
    return esz == 8 ? launch_split_multi_f64(M, P, x, y, alpha, beta, rd, s)
                    : launch_split_multi_f32(M, P, x, y, alpha, beta, rd, s);
}

int occupancy_planar(int esz) { return esz == 8 ? occupancy_planar_f64() : occupancy_planar_f32(); }
int occupancy_lanes(int esz) { return esz == 8 ? occupancy_lanes_f64() : occupancy_lanes_f32(); }
int occupancy_split_multi(int esz, int P)
{
    return esz == 8 ? occupancy_split_multi_f64(P) : occupancy_split_multi_f32(P);
}

}  // namespace vbc
