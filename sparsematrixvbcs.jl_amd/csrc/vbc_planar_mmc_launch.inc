// spmm_planar_col / spmm_pair_col launchers for one value type (included by vbc_planar_mmc_f64.hip /
// vbc_planar_mmc_f32.hip / vbc_planar_mmc_f64n.hip, which define VBC_PLANAR_T and VBC_PLANAR_SUFFIX, and
// VBC_PLANAR_S when the stored values are narrower than VBC_PLANAR_T): one translation unit per type so they
// compile in parallel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vbc_planar_mmc.h"

#ifndef VBC_PLANAR_S
#define VBC_PLANAR_S VBC_PLANAR_T
#endif

namespace vbc {

template <typename T, typename S, int W_, bool KC, int RUN, int NR>
static void launch_pmmc_nr(const SlotBin &hb, const T *x, int64_t ldx, T *y, int64_t ldy, int nr, double alpha,
                           double beta, bool rd, hipStream_t s)
{
    const int grid = (hb.nranges + kWavesPerBlock - 1) / kWavesPerBlock;
    if (hb.mask)
        hipLaunchKernelGGL((spmm_planar_col<T, W_, KC, RUN, true, S, NR>), dim3(grid), dim3(kBlockThreads), 0, s, hb, x,
                           ldx, y, ldy, nr, (T)alpha, (T)beta, (int)rd);
    else
        hipLaunchKernelGGL((spmm_planar_col<T, W_, KC, RUN, false, S, NR>), dim3(grid), dim3(kBlockThreads), 0, s, hb, x,
                           ldx, y, ldy, nr, (T)alpha, (T)beta, (int)rd);
}

// NR = 2 or 4, the smallest that holds the nr live columns (every instance is free of scratch at NR = 4: DESIGN.md
// §11.2 has the compiler's table, so no width falls back to NR = 2 chunks)
template <typename T, typename S, int W_, bool KC, int RUN>
static void launch_pmmc_w(const SlotBin &hb, const T *x, int64_t ldx, T *y, int64_t ldy, int nr, double alpha,
                          double beta, bool rd, hipStream_t s)
{
    if (nr <= 2) launch_pmmc_nr<T, S, W_, KC, RUN, 2>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s);
    else launch_pmmc_nr<T, S, W_, KC, RUN, 4>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s);
}

template <typename T, typename S, bool KC, int RUN>
static int launch_pmmc_r(const SlotBin &hb, const T *x, int64_t ldx, T *y, int64_t ldy, int nr, double alpha,
                         double beta, bool rd, hipStream_t s)
{
    switch (hb.wkey) {
    case 3: launch_pmmc_w<T, S, 3, KC, RUN>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s); break;
    case 4: launch_pmmc_w<T, S, 4, KC, RUN>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s); break;
    case 5: launch_pmmc_w<T, S, 5, KC, RUN>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s); break;
    case 6: launch_pmmc_w<T, S, 6, KC, RUN>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s); break;
    case 7: launch_pmmc_w<T, S, 7, KC, RUN>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s); break;
    case 8: launch_pmmc_w<T, S, 8, KC, RUN>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

template <typename T, typename S, bool KC>
static int launch_pmmc_t(const SlotBin &hb, const T *x, int64_t ldx, T *y, int64_t ldy, int nr, double alpha,
                         double beta, bool rd, hipStream_t s)
{
    switch (hb.run) {
    case 1: return launch_pmmc_r<T, S, KC, 1>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s);
    case 2: return launch_pmmc_r<T, S, KC, 2>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s);
    case 3: return launch_pmmc_r<T, S, KC, 3>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s);
    default: return (int)hipErrorInvalidValue;
    }
}

template <typename S, bool KC>
static int launch_pair_mmc(const SlotBin &hb, const double *x, int64_t ldx, double *y, int64_t ldy, int nr,
                           double alpha, double beta, bool rd, hipStream_t s)
{
    const dim3 grid((hb.nranges + kWavesPerBlock - 1) / kWavesPerBlock), blk(kBlockThreads);
#define VBC_PAIR_MMC(MASK)                                                                                             \
    do {                                                                                                               \
        if (nr <= 2)                                                                                                   \
            hipLaunchKernelGGL((spmm_pair_col<KC, MASK, S, 2>), grid, blk, 0, s, hb, x, ldx, y, ldy, nr, alpha, beta,  \
                               (int)rd);                                                                               \
        else                                                                                                           \
            hipLaunchKernelGGL((spmm_pair_col<KC, MASK, S, 4>), grid, blk, 0, s, hb, x, ldx, y, ldy, nr, alpha, beta,  \
                               (int)rd);                                                                               \
    } while (0)
    if (hb.mask) VBC_PAIR_MMC(true);
    else VBC_PAIR_MMC(false);
#undef VBC_PAIR_MMC
    return (int)hipGetLastError();
}

// lane pairs: fp64, w = 3, runs of 3 (no fp32 form: a missing kernel is an error)
template <typename T, typename S>
static int launch_pair_mmc_t(const SlotBin &hb, const T *x, int64_t ldx, T *y, int64_t ldy, int nr, double alpha,
                             double beta, bool rd, hipStream_t s)
{
    if constexpr (sizeof(T) == 8) {
        if (hb.wkey != 3 || hb.run != 3) return (int)hipErrorInvalidValue;
        return hb.kc ? launch_pair_mmc<S, true>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s)
                     : launch_pair_mmc<S, false>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s);
    } else {
        return (int)hipErrorInvalidValue;
    }
}

#define VBC_CAT2(a, b) a##b
#define VBC_CAT(a, b) VBC_CAT2(a, b)

// One planar bin (plain or lane-pair, kind 0, not split, no lane streams), nr <= 4 live columns at x / y (column
// strides ldx / ldy).  The bin's stored value type must be this unit's (the caller picks the unit by SlotBin::vsz).
int VBC_CAT(launch_planar_mmc_, VBC_PLANAR_SUFFIX)(const SlotBin &hb, const void *x, int64_t ldx, void *y, int64_t ldy,
                                                   int nr, double alpha, double beta, bool rd, hipStream_t stream)
{
    typedef VBC_PLANAR_T T;
    typedef VBC_PLANAR_S S;
    const T *xs = static_cast<const T *>(x);
    T *ys = static_cast<T *>(y);
    if (nr < 1 || nr > 4) return (int)hipErrorInvalidValue;
    if (hb.nranges <= 0) return (int)hipSuccess;
    if (hb.kind != 0 || hb.split > 1 || hb.lanes || hb.dot) return (int)hipErrorInvalidValue;
    if ((hb.vsz == 4) != (sizeof(S) < sizeof(T)) || (hb.vsz != 0 && hb.vsz != 4)) return (int)hipErrorInvalidValue;
    if (hb.pair) return launch_pair_mmc_t<T, S>(hb, xs, ldx, ys, ldy, nr, alpha, beta, rd, stream);
    return hb.kc ? launch_pmmc_t<T, S, true>(hb, xs, ldx, ys, ldy, nr, alpha, beta, rd, stream)
                 : launch_pmmc_t<T, S, false>(hb, xs, ldx, ys, ldy, nr, alpha, beta, rd, stream);
}

}  // namespace vbc
