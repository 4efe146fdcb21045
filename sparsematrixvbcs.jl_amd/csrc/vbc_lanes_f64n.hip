// Lane-stream kernel launchers, fp64 compute on Float32 stored values (VBC_CREATE_NARROW_STREAMS):
// spmv_planar_lanes of vbc_planar.h with the value stream read as floats in the Float32 column-group arrangement
// and widened in registers.  A translation unit of its own, so vbc_planar.hip compiles as before.  The variants
// are those launch_lanes_w of vbc_planar.hip picks for a wide lane-stream bin (w in 3..8, runs of 1..3; the RD,
// the DEEP and the plain form); a bin that is not a plain lane-stream bin has no kernel here and is an error.
#include <hip/hip_runtime.h>

#include "vbc_planar.h"

namespace vbc {

template <int W_, int RUN>
static void launch_lanes_w_n(const SlotBin &hb, const double *xs, double *ys, double alpha, double beta, bool rd,
                             hipStream_t s)
{
    const dim3 grid((hb.nranges + kWavesPerBlock - 1) / kWavesPerBlock), blk(kBlockThreads);
    if (rd)
        hipLaunchKernelGGL((spmv_planar_lanes<double, W_, RUN, false, true, 0, float>), grid, blk, 0, s, hb, xs, ys,
                           alpha, beta);
    else if (hb.deep)
        hipLaunchKernelGGL((spmv_planar_lanes<double, W_, RUN, true, false, 0, float>), grid, blk, 0, s, hb, xs, ys,
                           alpha, beta);
    else
        hipLaunchKernelGGL((spmv_planar_lanes<double, W_, RUN, false, false, 0, float>), grid, blk, 0, s, hb, xs, ys,
                           alpha, beta);
}

template <int RUN>
static int launch_lanes_r_n(const SlotBin &hb, const double *xs, double *ys, double alpha, double beta, bool rd,
                            hipStream_t s)
{
    switch (hb.wkey) {
    case 3: launch_lanes_w_n<3, RUN>(hb, xs, ys, alpha, beta, rd, s); break;
    case 4: launch_lanes_w_n<4, RUN>(hb, xs, ys, alpha, beta, rd, s); break;
    case 5: launch_lanes_w_n<5, RUN>(hb, xs, ys, alpha, beta, rd, s); break;
    case 6: launch_lanes_w_n<6, RUN>(hb, xs, ys, alpha, beta, rd, s); break;
    case 7: launch_lanes_w_n<7, RUN>(hb, xs, ys, alpha, beta, rd, s); break;
    case 8: launch_lanes_w_n<8, RUN>(hb, xs, ys, alpha, beta, rd, s); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

int launch_lanes_f64n(const SlotBin &hb, const void *x, void *y, double alpha, double beta, bool rd, hipStream_t s)
{
    // only plain lane-stream bins (B'x form, kind 0) come here: a missing kernel is an error, never another
    // kernel on the wrong bytes
    if (hb.vsz != 4 || !hb.planar || !hb.lanes || hb.pair || hb.kind != 0 || hb.split > 1 || hb.fused || hb.holes)
        return (int)hipErrorInvalidValue;
    const double *xs = static_cast<const double *>(x);
    double *ys = static_cast<double *>(y);
    switch (hb.run) {
    case 1: return launch_lanes_r_n<1>(hb, xs, ys, alpha, beta, rd, s);
    case 2: return launch_lanes_r_n<2>(hb, xs, ys, alpha, beta, rd, s);
    case 3: return launch_lanes_r_n<3>(hb, xs, ys, alpha, beta, rd, s);
    default: return (int)hipErrorInvalidValue;
    }
}

}  // namespace vbc
