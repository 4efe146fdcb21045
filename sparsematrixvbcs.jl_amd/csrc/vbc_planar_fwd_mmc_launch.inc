// spmm_planar_fwd_col / spmm_pair_col<..., DOT> launchers for one value type (included by vbc_planar_fwd_mmc_f64.hip /
// vbc_planar_fwd_mmc_f32.hip / vbc_planar_fwd_mmc_f64n.hip, which define VBC_PLANAR_T and VBC_PLANAR_SUFFIX, and
// VBC_PLANAR_S when the stored values are narrower than VBC_PLANAR_T): one translation unit per type so they
// compile in parallel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vbc_planar_fwd_mmc.h"

#ifndef VBC_PLANAR_S
#define VBC_PLANAR_S VBC_PLANAR_T
#endif

namespace vbc {

// NR = 2 or 4, the smallest that holds the nr live columns (every instance is free of scratch and spills at NR = 4:
// DESIGN.md §11.3 has the compiler's table, so no (type, w, R) falls back to NR = 2 chunks)
template <typename T, typename S, int W_, int R, bool KC>
static void launch_pfmmc_wr(const SlotBin &hb, const T *x, int64_t ldx, T *y, int64_t ldy, int nr, double alpha,
                            double beta, bool rd, hipStream_t s)
{
    const dim3 grid((hb.nranges + kWavesPerBlock - 1) / kWavesPerBlock), blk(kBlockThreads);
#define VBC_PFMMC(MASK)                                                                                                \
    do {                                                                                                               \
        if (nr <= 2)                                                                                                   \
            hipLaunchKernelGGL((spmm_planar_fwd_col<T, W_, R, KC, MASK, S, 2>), grid, blk, 0, s, hb, x, ldx, y, ldy,   \
                               nr, (T)alpha, (T)beta, (int)rd);                                                        \
        else                                                                                                           \
            hipLaunchKernelGGL((spmm_planar_fwd_col<T, W_, R, KC, MASK, S, 4>), grid, blk, 0, s, hb, x, ldx, y, ldy,   \
                               nr, (T)alpha, (T)beta, (int)rd);                                                        \
    } while (0)
    if (hb.mask) VBC_PFMMC(true);
    else VBC_PFMMC(false);
#undef VBC_PFMMC
}

// forward row runs: w in {2, 3, 4}, R in {2, 3} (spmv_planar_fwd's forms)
template <typename T, typename S, bool KC>
static int launch_pfmmc(const SlotBin &hb, const T *x, int64_t ldx, T *y, int64_t ldy, int nr, double alpha,
                        double beta, bool rd, hipStream_t s)
{
#define VBC_PFMMC_WR(W, RR)                                                        \
    if (hb.wkey == W && hb.run == RR) {                                            \
        launch_pfmmc_wr<T, S, W, RR, KC>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s); \
        return (int)hipGetLastError();                                             \
    }
    VBC_PFMMC_WR(2, 2) VBC_PFMMC_WR(2, 3) VBC_PFMMC_WR(3, 2) VBC_PFMMC_WR(3, 3) VBC_PFMMC_WR(4, 2) VBC_PFMMC_WR(4, 3)
#undef VBC_PFMMC_WR
    return (int)hipErrorInvalidValue;
}

template <typename S, bool KC>
static int launch_pair_fmmc(const SlotBin &hb, const double *x, int64_t ldx, double *y, int64_t ldy, int nr,
                            double alpha, double beta, bool rd, hipStream_t s)
{
    const dim3 grid((hb.nranges + kWavesPerBlock - 1) / kWavesPerBlock), blk(kBlockThreads);
#define VBC_PAIR_FMMC(MASK)                                                                                            \
    do {                                                                                                               \
        if (nr <= 2)                                                                                                   \
            hipLaunchKernelGGL((spmm_pair_col<KC, MASK, S, 2, true>), grid, blk, 0, s, hb, x, ldx, y, ldy, nr, alpha,  \
                               beta, (int)rd);                                                                         \
        else                                                                                                           \
            hipLaunchKernelGGL((spmm_pair_col<KC, MASK, S, 4, true>), grid, blk, 0, s, hb, x, ldx, y, ldy, nr, alpha,  \
                               beta, (int)rd);                                                                         \
    } while (0)
    if (hb.mask) VBC_PAIR_FMMC(true);
    else VBC_PAIR_FMMC(false);
#undef VBC_PAIR_FMMC
    return (int)hipGetLastError();
}

// forward lane pairs: fp64, w = 3, runs of 3 (no fp32 form: a missing kernel is an error)
template <typename T, typename S>
static int launch_pair_fmmc_t(const SlotBin &hb, const T *x, int64_t ldx, T *y, int64_t ldy, int nr, double alpha,
                              double beta, bool rd, hipStream_t s)
{
    if constexpr (sizeof(T) == 8) {
        if (hb.wkey != 3 || hb.run != 3) return (int)hipErrorInvalidValue;
        return hb.kc ? launch_pair_fmmc<S, true>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s)
                     : launch_pair_fmmc<S, false>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s);
    } else {
        return (int)hipErrorInvalidValue;
    }
}

#define VBC_CAT2(a, b) a##b
#define VBC_CAT(a, b) VBC_CAT2(a, b)

// One forward planar bin (row runs of kind 1, or lane pairs with SlotBin::dot; not split, no lane streams), nr <= 4
// live columns at x / y (column strides ldx / ldy).  The bin's stored value type must be this unit's (the caller
// picks the unit by SlotBin::vsz).
int VBC_CAT(launch_planar_fwd_mmc_, VBC_PLANAR_SUFFIX)(const SlotBin &hb, const void *x, int64_t ldx, void *y,
                                                       int64_t ldy, int nr, double alpha, double beta, bool rd,
                                                       hipStream_t stream)
{
    typedef VBC_PLANAR_T T;
    typedef VBC_PLANAR_S S;
    const T *xs = static_cast<const T *>(x);
    T *ys = static_cast<T *>(y);
    if (nr < 1 || nr > 4) return (int)hipErrorInvalidValue;
    if (hb.nranges <= 0) return (int)hipSuccess;
    if (hb.split > 1 || hb.lanes || hb.fused) return (int)hipErrorInvalidValue;
    if ((hb.vsz == 4) != (sizeof(S) < sizeof(T)) || (hb.vsz != 0 && hb.vsz != 4)) return (int)hipErrorInvalidValue;
    if (hb.pair) {
        if (!hb.dot) return (int)hipErrorInvalidValue;
        return launch_pair_fmmc_t<T, S>(hb, xs, ldx, ys, ldy, nr, alpha, beta, rd, stream);
    }
    if (hb.kind != 1) return (int)hipErrorInvalidValue;
    return hb.kc ? launch_pfmmc<T, S, true>(hb, xs, ldx, ys, ldy, nr, alpha, beta, rd, stream)
                 : launch_pfmmc<T, S, false>(hb, xs, ldx, ys, ldy, nr, alpha, beta, rd, stream);
}

}  // namespace vbc
