// Lane-pair kernel launchers, fp64 compute on Float32 stored values (VBC_CREATE_NARROW_PAIRS): spmv_planar_pair
// and spmv_pair_lanes of vbc_planar.h with the run-row read as 288 floats (pair_load) and widened in registers.  A
// translation unit of its own, so vbc_planar.hip compiles as before.  The variants are those launch_pair /
// launch_planar of vbc_planar.hip pick for a wide pair bin; a bin that is not a lane-pair bin has no kernel here
// and is an error.
#include <hip/hip_runtime.h>

#include "vbc_planar.h"

namespace vbc {

template <bool KC, bool DOT>
static int launch_pair_n(const SlotBin &hb, bool faste, bool staged, const double *xs, double *ys, double alpha,
                         double beta, bool rd, hipStream_t s)
{
    const dim3 grid((hb.nranges + kWavesPerBlock - 1) / kWavesPerBlock), blk(kBlockThreads);
    if (hb.mask)
        hipLaunchKernelGGL((spmv_planar_pair<false, 0, KC, true, DOT, float>), grid, blk, 0, s, hb, xs, ys, alpha, beta,
                           (int)rd);
    else if (faste && staged)
        hipLaunchKernelGGL((spmv_planar_pair<true, 8, KC, false, DOT, float>), grid, blk, 0, s, hb, xs, ys, alpha, beta,
                           (int)rd);
    else if (faste)
        hipLaunchKernelGGL((spmv_planar_pair<true, 0, KC, false, DOT, float>), grid, blk, 0, s, hb, xs, ys, alpha, beta,
                           (int)rd);
    else
        hipLaunchKernelGGL((spmv_planar_pair<false, 0, KC, false, DOT, float>), grid, blk, 0, s, hb, xs, ys, alpha, beta,
                           (int)rd);
    return (int)hipGetLastError();
}

int launch_pair_f64n(const SlotBin &hb, bool faste, bool staged, const void *x, void *y, double alpha, double beta,
                     bool rd, hipStream_t s)
{
    // only lane-pair bins (fp64, w = 3, runs of 3) come here: a missing kernel is an error, never another kernel
    // on the wrong bytes
    if (hb.vsz != 4 || !hb.planar || !hb.pair || hb.wkey != 3 || hb.run != 3 || hb.split > 1 || hb.fused || hb.holes)
        return (int)hipErrorInvalidValue;
    const double *xs = static_cast<const double *>(x);
    double *ys = static_cast<double *>(y);
    if (hb.lanes) {  // lane-pair streams (B'x)
        if (hb.kind != 0) return (int)hipErrorInvalidValue;
        const dim3 grid((hb.nranges + kWavesPerBlock - 1) / kWavesPerBlock), blk(kBlockThreads);
        if (rd) hipLaunchKernelGGL((spmv_pair_lanes<true, float>), grid, blk, 0, s, hb, xs, ys, alpha, beta);
        else hipLaunchKernelGGL((spmv_pair_lanes<false, float>), grid, blk, 0, s, hb, xs, ys, alpha, beta);
        return (int)hipGetLastError();
    }
    if (hb.kind != 0) return (int)hipErrorInvalidValue;  // (the forward form is a kind-0 bin with SlotBin::dot)
    if (hb.dot)
        return hb.kc ? launch_pair_n<true, true>(hb, faste, staged, xs, ys, alpha, beta, rd, s)
                     : launch_pair_n<false, true>(hb, faste, staged, xs, ys, alpha, beta, rd, s);
    return hb.kc ? launch_pair_n<true, false>(hb, faste, staged, xs, ys, alpha, beta, rd, s)
                 : launch_pair_n<false, false>(hb, faste, staged, xs, ys, alpha, beta, rd, s);
}

}  // namespace vbc
