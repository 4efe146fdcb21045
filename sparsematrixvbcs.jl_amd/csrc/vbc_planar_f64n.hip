// Planar-kernel launchers, fp64 compute on Float32 stored values (VBC_CREATE_NARROW_PLANAR): spmv_planar and
// spmv_planar_fwd of vbc_planar.h with the value stream read as floats in the Float32 column-group arrangement
// and widened in registers.  A translation unit of its own, so it compiles beside vbc_planar.hip.  The
// variants are those launch_w / launch_fwd_wr of vbc_planar.hip pick for a bin that is neither split, pair
// nor lanes; anything else has no narrow kernel and is an error.
#include <hip/hip_runtime.h>

#include "vbc_planar.h"

namespace vbc {

template <int W_, bool KC, int RUN>
static void launch_w_n(const SlotBin &hb, bool faste, bool staged, const double *xs, double *ys, double alpha,
                       double beta, bool rd, hipStream_t s)
{
    const dim3 grid((hb.nranges + kWavesPerBlock - 1) / kWavesPerBlock), blk(kBlockThreads);
    constexpr int NB = planar_nb<double, W_>();
    if (hb.mask)
        hipLaunchKernelGGL((spmv_planar<double, W_, false, 0, KC, RUN, true, float>), grid, blk, 0, s, hb, xs, ys, alpha,
                           beta, (int)rd);
    else if (faste && staged)
        hipLaunchKernelGGL((spmv_planar<double, W_, true, NB, KC, RUN, false, float>), grid, blk, 0, s, hb, xs, ys, alpha,
                           beta, (int)rd);
    else if (faste)
        hipLaunchKernelGGL((spmv_planar<double, W_, true, 0, KC, RUN, false, float>), grid, blk, 0, s, hb, xs, ys, alpha,
                           beta, (int)rd);
    else
        hipLaunchKernelGGL((spmv_planar<double, W_, false, 0, KC, RUN, false, float>), grid, blk, 0, s, hb, xs, ys, alpha,
                           beta, (int)rd);
}

template <bool KC, int RUN>
static int launch_r_n(const SlotBin &hb, bool faste, bool staged, const double *xs, double *ys, double alpha,
                      double beta, bool rd, hipStream_t s)
{
    switch (hb.wkey) {
    case 3: launch_w_n<3, KC, RUN>(hb, faste, staged, xs, ys, alpha, beta, rd, s); break;
    case 4: launch_w_n<4, KC, RUN>(hb, faste, staged, xs, ys, alpha, beta, rd, s); break;
    case 5: launch_w_n<5, KC, RUN>(hb, faste, staged, xs, ys, alpha, beta, rd, s); break;
    case 6: launch_w_n<6, KC, RUN>(hb, faste, staged, xs, ys, alpha, beta, rd, s); break;
    case 7: launch_w_n<7, KC, RUN>(hb, faste, staged, xs, ys, alpha, beta, rd, s); break;
    case 8: launch_w_n<8, KC, RUN>(hb, faste, staged, xs, ys, alpha, beta, rd, s); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

template <bool KC>
static int launch_t_n(const SlotBin &hb, bool faste, bool staged, const double *xs, double *ys, double alpha,
                      double beta, bool rd, hipStream_t s)
{
    switch (hb.run) {
    case 1: return launch_r_n<KC, 1>(hb, faste, staged, xs, ys, alpha, beta, rd, s);
    case 2: return launch_r_n<KC, 2>(hb, faste, staged, xs, ys, alpha, beta, rd, s);
    case 3: return launch_r_n<KC, 3>(hb, faste, staged, xs, ys, alpha, beta, rd, s);
    default: return (int)hipErrorInvalidValue;
    }
}

template <int W_, int R, bool KC>
static void launch_fwd_wr_n(const SlotBin &hb, bool faste, bool staged, const double *xs, double *ys, double alpha,
                            double beta, bool rd, hipStream_t s)
{
    const dim3 grid((hb.nranges + kWavesPerBlock - 1) / kWavesPerBlock), blk(kBlockThreads);
    constexpr int NB = (8192 / (64 * R * (int)sizeof(double))) > 8 ? 8 : (8192 / (64 * R * (int)sizeof(double)));
    if (hb.mask)
        hipLaunchKernelGGL((spmv_planar_fwd<double, W_, R, false, 0, KC, true, float>), grid, blk, 0, s, hb, xs, ys, alpha,
                           beta, (int)rd);
    else if (faste && staged)
        hipLaunchKernelGGL((spmv_planar_fwd<double, W_, R, true, NB, KC, false, float>), grid, blk, 0, s, hb, xs, ys, alpha,
                           beta, (int)rd);
    else if (faste)
        hipLaunchKernelGGL((spmv_planar_fwd<double, W_, R, true, 0, KC, false, float>), grid, blk, 0, s, hb, xs, ys, alpha,
                           beta, (int)rd);
    else
        hipLaunchKernelGGL((spmv_planar_fwd<double, W_, R, false, 0, KC, false, float>), grid, blk, 0, s, hb, xs, ys, alpha,
                           beta, (int)rd);
}

// forward row runs: w in {2, 3, 4}, R in {2, 3}
template <bool KC>
static int launch_fwd_n(const SlotBin &hb, bool faste, bool staged, const double *xs, double *ys, double alpha,
                        double beta, bool rd, hipStream_t s)
{
#define VBC_FWD_N(W, RR)                                                                   \
    if (hb.wkey == W && hb.run == RR) {                                                    \
        launch_fwd_wr_n<W, RR, KC>(hb, faste, staged, xs, ys, alpha, beta, rd, s);         \
        return (int)hipGetLastError();                                                     \
    }
    VBC_FWD_N(2, 2) VBC_FWD_N(2, 3) VBC_FWD_N(3, 2) VBC_FWD_N(3, 3) VBC_FWD_N(4, 2) VBC_FWD_N(4, 3)
#undef VBC_FWD_N
    return (int)hipErrorInvalidValue;
}

int launch_planar_f64n(const SlotBin &hb, bool faste, bool staged, const void *x, void *y, double alpha, double beta,
                       bool rd, hipStream_t s)
{
    // only the plain chunk-planar bins store narrow values: a missing kernel is an error, never another
    // kernel on the wrong bytes
    if (hb.vsz != 4 || !hb.planar || hb.lanes || hb.pair || hb.split > 1 || hb.fused || hb.holes)
        return (int)hipErrorInvalidValue;
    const double *xs = static_cast<const double *>(x);
    double *ys = static_cast<double *>(y);
    if (hb.kind == 1)
        return hb.kc ? launch_fwd_n<true>(hb, faste, staged, xs, ys, alpha, beta, rd, s)
                     : launch_fwd_n<false>(hb, faste, staged, xs, ys, alpha, beta, rd, s);
    return hb.kc ? launch_t_n<true>(hb, faste, staged, xs, ys, alpha, beta, rd, s)
                 : launch_t_n<false>(hb, faste, staged, xs, ys, alpha, beta, rd, s);
}

}  // namespace vbc
