// Launchers of the row-swept SpMV kernel (vbc_sweep.h) for a compute type T on stored values S: included by
// vbc_sweep.hip (S = T) and vbc_sweep_f64n.hip (fp64 on Float32 stored values).  Every width 1..8 and both key forms
// are inside the kernel; the instances are the two kinds by the three tile sizes.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "vbc_sweep.h"

namespace vbc {

template <typename T, typename S, int KIND, int TB, int DIAG = 0>
static void launch_t(const SweepBin *d_bins, int nbins, int total_tiles, const void *x, void *y, double alpha,
                     double beta, bool rd, hipStream_t s)
{
    hipLaunchKernelGGL((spmv_sweep<T, KIND, TB, DIAG, S>), dim3(total_tiles), dim3(64), 0, s, d_bins, nbins, total_tiles,
                       static_cast<const T *>(x), static_cast<T *>(y), (T)alpha, (T)beta, (int)rd);
}

template <typename T, typename S, int KIND>
static void launch_any(const SweepBin *d_bins, int nbins, int total_tiles, int tile_bytes, int diag, const void *x,
                       void *y, double alpha, double beta, bool rd, hipStream_t s)
{
#ifdef VBC_ABLATION
    if constexpr (sizeof(T) == 8 && KIND == 0 && std::is_same_v<S, T>) {  // ablations (the VBC_ABLATION build only)
        if (diag == 1 && tile_bytes == 2 * kSweepTileBytes) return launch_t<T, S, KIND, 2 * kSweepTileBytes, 1>(d_bins, nbins, total_tiles, x, y, alpha, beta, rd, s);
        if (diag == 2 && tile_bytes == 2 * kSweepTileBytes) return launch_t<T, S, KIND, 2 * kSweepTileBytes, 2>(d_bins, nbins, total_tiles, x, y, alpha, beta, rd, s);
    }
#else
    (void)diag;
#endif
    if (tile_bytes >= 4 * kSweepTileBytes) launch_t<T, S, KIND, 4 * kSweepTileBytes>(d_bins, nbins, total_tiles, x, y, alpha, beta, rd, s);
    else if (tile_bytes >= 2 * kSweepTileBytes) launch_t<T, S, KIND, 2 * kSweepTileBytes>(d_bins, nbins, total_tiles, x, y, alpha, beta, rd, s);
    else launch_t<T, S, KIND, kSweepTileBytes>(d_bins, nbins, total_tiles, x, y, alpha, beta, rd, s);
}

}  // namespace vbc
