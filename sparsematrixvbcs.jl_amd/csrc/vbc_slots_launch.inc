// Slotted-kernel launchers for one value type (included by vbc_slots_f64.hip / vbc_slots_f32.hip /
// vbc_slots_f64n.hip, which define VBC_SLOTS_T, VBC_SLOTS_U and VBC_SLOTS_SUFFIX, and VBC_SLOTS_S when the
// stored values are narrower than VBC_SLOTS_T): one translation unit per type so they compile in parallel.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include <type_traits>

#include "vbc_slots.h"

#ifndef VBC_SLOTS_S
#define VBC_SLOTS_S VBC_SLOTS_T
#endif

namespace vbc {

template <typename T, int U, bool KC, int WONLY, typename S>
static void launch_t(int kind, const SlotBin *d_bins, int nbins, int total_ranges, bool faste, int xcd, int diag, int stage,
                     const void *x, void *y, double alpha, double beta, bool rd, hipStream_t s)
{
    const int grid = (total_ranges + kWavesPerBlock - 1) / kWavesPerBlock;
    const int xcd_chunk = (xcd && grid >= 16) ? 1 : 0;
    const T *xs = static_cast<const T *>(x);
    T *ys = static_cast<T *>(y);
#define VBC_SLOTS(KIND, F)                                                                               \
    hipLaunchKernelGGL((spmv_slots<T, KIND, U, F, 0, 0, KC, WONLY, S>), dim3(grid), dim3(kBlockThreads), 0, s, d_bins, nbins, \
                       total_ranges, xcd_chunk, xs, ys, (T)alpha, (T)beta, (int)rd)
#ifdef VBC_ABLATION
    if constexpr (sizeof(T) == 8 && !KC && WONLY < 0 && std::is_same<S, T>::value) {  // ablations (the VBC_ABLATION build only)
        if (kind == 0 && faste && diag == 1) {
            hipLaunchKernelGGL((spmv_slots<T, 0, U, true, 1>), dim3(grid), dim3(kBlockThreads), 0, s, d_bins, nbins,
                               total_ranges, xcd_chunk, xs, ys, (T)alpha, (T)beta, (int)rd);
            return;
        }
        if (kind == 0 && faste && diag == 2) {
            hipLaunchKernelGGL((spmv_slots<T, 0, U, true, 2>), dim3(grid), dim3(kBlockThreads), 0, s, d_bins, nbins,
                               total_ranges, xcd_chunk, xs, ys, (T)alpha, (T)beta, (int)rd);
            return;
        }
        if (kind == 0 && faste && diag == 4) {
            hipLaunchKernelGGL((spmv_slots<T, 0, U, true, 4>), dim3(grid), dim3(kBlockThreads), 0, s, d_bins, nbins,
                               total_ranges, xcd_chunk, xs, ys, (T)alpha, (T)beta, (int)rd);
            return;
        }
        if (kind == 0 && faste && diag == 3) {
            hipLaunchKernelGGL((spmv_slots<T, 0, U, true, 3>), dim3(grid), dim3(kBlockThreads), 0, s, d_bins, nbins,
                               total_ranges, xcd_chunk, xs, ys, (T)alpha, (T)beta, (int)rd);
            return;
        }
    }
#else
    (void)diag;
#endif
#define VBC_STAGED(KIND, NB)                                                                             \
    hipLaunchKernelGGL((spmv_slots<T, KIND, U, true, 0, NB, KC, WONLY, S>), dim3(grid), dim3(kBlockThreads), 0, s, d_bins, nbins, \
                       total_ranges, xcd_chunk, xs, ys, (T)alpha, (T)beta, (int)rd)
    if (faste && stage == 8) { if (kind == 0) VBC_STAGED(0, 8); else VBC_STAGED(1, 8); return; }
#undef VBC_STAGED
    if (kind == 0) { if (faste) VBC_SLOTS(0, true); else VBC_SLOTS(0, false); }
    else { if (faste) VBC_SLOTS(1, true); else VBC_SLOTS(1, false); }
#undef VBC_SLOTS
}

#define VBC_CAT2(a, b) a##b
#define VBC_CAT(a, b) VBC_CAT2(a, b)

// wonly: the common width of every bin of the launch (-1: mixed), selecting a one-width kernel for the
// widths of FE (2) and CSC columns (1)
int VBC_CAT(launch_slots_, VBC_SLOTS_SUFFIX)(int kind, const SlotBin *d_bins, int nbins, int total_ranges, bool faste,
                                             int xcd, int diag, int stage, bool kc, int wonly, const void *x, void *y,
                                             double alpha, double beta, bool rd, hipStream_t stream)
{
#define VBC_LT(KC, W) launch_t<VBC_SLOTS_T, VBC_SLOTS_U, KC, W, VBC_SLOTS_S>(kind, d_bins, nbins, total_ranges, faste, xcd, diag, stage, \
                                                              x, y, alpha, beta, rd, stream)
#ifdef VBC_SLOTS_NO_NARROW2  // (a TU whose T is never fp32: no instantiation for the two-segment form)
#define VBC_LT_N2(KC) VBC_LT(KC, -1)
#else
#define VBC_LT_N2(KC) VBC_LT(KC, kWonlyNarrow2)
#endif
    if (VBC_ABL((diag & 15) != 0)) wonly = -1;  // (bit 16, streaming y stores, keeps the kernel)
    if (kc) {
        if (wonly == 2) VBC_LT(true, 2);
        else if (wonly == 1) VBC_LT(true, 1);
        else if (wonly == kWonlyNarrow2 && sizeof(VBC_SLOTS_T) == 4) VBC_LT_N2(true);
        else VBC_LT(true, -1);
    } else {
        if (wonly == 2) VBC_LT(false, 2);
        else if (wonly == 1) VBC_LT(false, 1);
        else if (wonly == kWonlyNarrow2 && sizeof(VBC_SLOTS_T) == 4) VBC_LT_N2(false);
        else VBC_LT(false, -1);
    }
#undef VBC_LT_N2
#undef VBC_LT
    return hipGetLastError();
}

#ifndef VBC_SLOTS_NO_OCCUPANCY
int VBC_CAT(occupancy_slots_, VBC_SLOTS_SUFFIX)(int kind)
{
    int occ = 0;
    if (kind == 0) (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, spmv_slots<VBC_SLOTS_T, 0, VBC_SLOTS_U, true>, kBlockThreads, 0);
    else (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, spmv_slots<VBC_SLOTS_T, 1, VBC_SLOTS_U, true>, kBlockThreads, 0);
    return occ;
}
#endif

}  // namespace vbc
