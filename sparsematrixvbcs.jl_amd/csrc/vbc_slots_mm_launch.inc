// spmm_slots launchers for one value type (included by vbc_slots_mm_f64.hip / vbc_slots_mm_f32.hip /
// vbc_slots_mm_f64n.hip) and, with VBC_SLOTS_COL defined, spmm_slots_col launchers (vbc_slots_mmc_*.hip).  The unit
// defines VBC_SLOTS_T and VBC_SLOTS_SUFFIX, and VBC_SLOTS_S when the stored values are narrower than VBC_SLOTS_T: one
// translation unit per operand layout and type so they compile in parallel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vbc_slots_mm.h"

#ifndef VBC_SLOTS_S
#define VBC_SLOTS_S VBC_SLOTS_T
#endif

namespace vbc {

template <typename T, typename S, bool KC, int NR, int WONLY>
static void launch_mm_t(const SlotBin *d_bins, int nbins, int total_ranges, int xcd, const T *x, int64_t ldx, T *y,
                        int64_t ldy, int nr, double alpha, double beta, bool rd, hipStream_t s)
{
    const int grid = (total_ranges + kWavesPerBlock - 1) / kWavesPerBlock;
    const int xcd_chunk = (xcd && grid >= 16) ? 1 : 0;
#ifdef VBC_SLOTS_COL
    hipLaunchKernelGGL((spmm_slots_col<T, KC, S, NR, WONLY>), dim3(grid), dim3(kBlockThreads), 0, s, d_bins, nbins,
                       total_ranges, xcd_chunk, x, ldx, y, ldy, nr, (T)alpha, (T)beta, (int)rd);
#else
    // vector moves of a lane's X / Y row: every live column, both bases and both row pitches on the vector's bytes
    constexpr uintptr_t kVecBytes = NR * sizeof(T) >= 16 ? 16 : NR * sizeof(T);
    const bool vec = nr == NR && ((uintptr_t)x | (uintptr_t)y | (uintptr_t)(ldx * (int64_t)sizeof(T)) |
                                  (uintptr_t)(ldy * (int64_t)sizeof(T))) % kVecBytes == 0;
    if (vec)
        hipLaunchKernelGGL((spmm_slots<T, KC, S, NR, true, WONLY>), dim3(grid), dim3(kBlockThreads), 0, s, d_bins, nbins,
                           total_ranges, xcd_chunk, x, ldx, y, ldy, nr, (T)alpha, (T)beta, (int)rd);
    else
        hipLaunchKernelGGL((spmm_slots<T, KC, S, NR, false, WONLY>), dim3(grid), dim3(kBlockThreads), 0, s, d_bins, nbins,
                           total_ranges, xcd_chunk, x, ldx, y, ldy, nr, (T)alpha, (T)beta, (int)rd);
#endif
}

#define VBC_CAT2(a, b) a##b
#define VBC_CAT(a, b) VBC_CAT2(a, b)

#ifdef VBC_SLOTS_COL
#define VBC_SLOTS_ENTRY VBC_CAT(launch_slots_mmc_, VBC_SLOTS_SUFFIX)
#else
#define VBC_SLOTS_ENTRY VBC_CAT(launch_slots_mm_, VBC_SLOTS_SUFFIX)
#endif

// The slotted bins of a launch (total_ranges > 0), nr <= 8 live columns at x / y (row pitches, or column strides,
// ldx / ldy).  wonly: 2 or kWonlyNarrow2 when every bin of the launch has that form, else -1.
int VBC_SLOTS_ENTRY(const SlotBin *d_bins, int nbins, int total_ranges, int xcd, bool kc, int wonly, const void *x,
                    int64_t ldx, void *y, int64_t ldy, int nr, double alpha, double beta, bool rd, hipStream_t stream)
{
    typedef VBC_SLOTS_T T;
    typedef VBC_SLOTS_S S;
    const T *xs = static_cast<const T *>(x);
    T *ys = static_cast<T *>(y);
    if (nr < 1 || nr > 8) return hipErrorInvalidValue;
    constexpr bool kNarrow2 = sizeof(T) == 4;  // (the two-segment form exists in fp32 only)
    if (wonly == kWonlyNarrow2 && !kNarrow2) return hipErrorInvalidValue;
#define VBC_MM(KC, NR, W) launch_mm_t<T, S, KC, NR, W>(d_bins, nbins, total_ranges, xcd, xs, ldx, ys, ldy, nr, alpha, beta, rd, stream)
#define VBC_MM_NR(KC, W)                    \
    do {                                    \
        if (nr <= 2) VBC_MM(KC, 2, W);      \
        else if (nr <= 4) VBC_MM(KC, 4, W); \
        else VBC_MM(KC, 8, W);              \
    } while (0)
#define VBC_MM_W(KC)                                                                \
    do {                                                                            \
        if (wonly == 2) VBC_MM_NR(KC, 2);                                           \
        else if (wonly == kWonlyNarrow2) VBC_MM_NR(KC, (kNarrow2 ? kWonlyNarrow2 : -1)); \
        else VBC_MM_NR(KC, -1);                                                     \
    } while (0)
    if (kc) VBC_MM_W(true);
    else VBC_MM_W(false);
#undef VBC_MM_W
#undef VBC_MM_NR
#undef VBC_MM
    return hipGetLastError();
}

}  // namespace vbc
