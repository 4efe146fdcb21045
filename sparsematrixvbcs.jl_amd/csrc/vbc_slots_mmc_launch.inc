// spmm_slots_col launchers for one value type (included by vbc_slots_mmc_f64.hip / vbc_slots_mmc_f32.hip /
// vbc_slots_mmc_f64n.hip, which define VBC_SLOTS_T and VBC_SLOTS_SUFFIX, and VBC_SLOTS_S when the stored values
// are narrower than VBC_SLOTS_T): one translation unit per type so they compile in parallel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vbc_slots_mmc.h"

#ifndef VBC_SLOTS_S
#define VBC_SLOTS_S VBC_SLOTS_T
#endif

namespace vbc {

template <typename T, typename S, bool KC, int NR, int WONLY>
static void launch_mmc_t(const SlotBin *d_bins, int nbins, int total_ranges, int xcd, const T *x, int64_t ldx, T *y,
                         int64_t ldy, int nr, double alpha, double beta, bool rd, hipStream_t s)
{
    const int grid = (total_ranges + kWavesPerBlock - 1) / kWavesPerBlock;
    const int xcd_chunk = (xcd && grid >= 16) ? 1 : 0;
    hipLaunchKernelGGL((spmm_slots_col<T, KC, S, NR, WONLY>), dim3(grid), dim3(kBlockThreads), 0, s, d_bins, nbins,
                       total_ranges, xcd_chunk, x, ldx, y, ldy, nr, (T)alpha, (T)beta, (int)rd);
}

#define VBC_CAT2(a, b) a##b
#define VBC_CAT(a, b) VBC_CAT2(a, b)

// nr <= 8 live columns at x / y (column strides ldx / ldy).  wonly: 2 or kWonlyNarrow2 when every bin of the launch
// has that form, else -1.  d_fill / nfill: the launch's fill list, applied to the same columns.
int VBC_CAT(launch_slots_mmc_, VBC_SLOTS_SUFFIX)(const SlotBin *d_bins, int nbins, int total_ranges, int xcd, bool kc,
                                                 int wonly, const int32_t *d_fill, int nfill, const void *x,
                                                 int64_t ldx, void *y, int64_t ldy, int nr, double alpha, double beta,
                                                 bool rd, hipStream_t stream)
{
    typedef VBC_SLOTS_T T;
    typedef VBC_SLOTS_S S;
    const T *xs = static_cast<const T *>(x);
    T *ys = static_cast<T *>(y);
    if (nr < 1 || nr > 8) return hipErrorInvalidValue;
    constexpr bool kNarrow2 = sizeof(T) == 4;  // (the two-segment form exists in fp32 only)
    if (wonly == kWonlyNarrow2 && !kNarrow2) return hipErrorInvalidValue;
#define VBC_MMC(KC, NR, W) launch_mmc_t<T, S, KC, NR, W>(d_bins, nbins, total_ranges, xcd, xs, ldx, ys, ldy, nr, alpha, beta, rd, stream)
#define VBC_MMC_NR(KC, W)                    \
    do {                                     \
        if (nr <= 2) VBC_MMC(KC, 2, W);      \
        else if (nr <= 4) VBC_MMC(KC, 4, W); \
        else VBC_MMC(KC, 8, W);              \
    } while (0)
#define VBC_MMC_W(KC)                                                                \
    do {                                                                             \
        if (wonly == 2) VBC_MMC_NR(KC, 2);                                           \
        else if (wonly == kWonlyNarrow2) VBC_MMC_NR(KC, (kNarrow2 ? kWonlyNarrow2 : -1)); \
        else VBC_MMC_NR(KC, -1);                                                     \
    } while (0)
    if (total_ranges > 0) {
        if (kc) VBC_MMC_W(true);
        else VBC_MMC_W(false);
    }
#undef VBC_MMC_W
#undef VBC_MMC_NR
#undef VBC_MMC
    if (nfill > 0)
        hipLaunchKernelGGL((fill_cols<T>), dim3((nfill + kBlockThreads - 1) / kBlockThreads, nr), dim3(kBlockThreads), 0,
                           stream, d_fill, nfill, ys, ldy, (T)beta, (int)rd);
    return hipGetLastError();
}

}  // namespace vbc
