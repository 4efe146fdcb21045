// Launchers of the row-swept SpMV kernel (vbc_sweep.h) on values of the compute eltype; a bin of Float32 values
// under fp64 compute (VBC_CREATE_NARROW_SWEPT) goes to vbc_sweep_f64n.hip.
#include <hip/hip_runtime.h>

#include "vbc_sweep.h"

namespace vbc {

// vbc_sweep_f64n.hip: spmv_sweep<double, KIND, TB, 0, float> (swept bins with SweepBin::vsz = 4)
int launch_sweep_f64n(int kind, const SweepBin *d_bins, int nbins, int total_tiles, int tile_bytes, const void *x, void *y,
                      double alpha, double beta, bool rd, hipStream_t stream);

template <typename T, int KIND, int TB, int DIAG = 0>
static void launch_t(const SweepBin *d_bins, int nbins, int total_tiles, const void *x, void *y, double alpha,
                     double beta, bool rd, hipStream_t s)
{
    hipLaunchKernelGGL((spmv_sweep<T, KIND, TB, DIAG>), dim3(total_tiles), dim3(64), 0, s, d_bins, nbins, total_tiles,
                       static_cast<const T *>(x), static_cast<T *>(y), (T)alpha, (T)beta, (int)rd);
}

template <typename T, int KIND>
static void launch_any(const SweepBin *d_bins, int nbins, int total_tiles, int tile_bytes, int diag, const void *x,
                       void *y, double alpha, double beta, bool rd, hipStream_t s)
{
#ifdef VBC_ABLATION
    if constexpr (sizeof(T) == 8 && KIND == 0) {  // ablations (the VBC_ABLATION build only)
        if (diag == 1 && tile_bytes == 2 * kSweepTileBytes) return launch_t<T, KIND, 2 * kSweepTileBytes, 1>(d_bins, nbins, total_tiles, x, y, alpha, beta, rd, s);
        if (diag == 2 && tile_bytes == 2 * kSweepTileBytes) return launch_t<T, KIND, 2 * kSweepTileBytes, 2>(d_bins, nbins, total_tiles, x, y, alpha, beta, rd, s);
    }
#else
    (void)diag;
#endif
    if (tile_bytes >= 4 * kSweepTileBytes) launch_t<T, KIND, 4 * kSweepTileBytes>(d_bins, nbins, total_tiles, x, y, alpha, beta, rd, s);
    else if (tile_bytes >= 2 * kSweepTileBytes) launch_t<T, KIND, 2 * kSweepTileBytes>(d_bins, nbins, total_tiles, x, y, alpha, beta, rd, s);
    else launch_t<T, KIND, kSweepTileBytes>(d_bins, nbins, total_tiles, x, y, alpha, beta, rd, s);
}

int launch_sweep(int esz, int vsz, int kind, const SweepBin *d_bins, int nbins, int total_tiles, int tile_bytes, int diag,
                 const void *x, void *y, double alpha, double beta, bool rd, hipStream_t stream)
{
    if (total_tiles <= 0) return hipSuccess;
    if (vsz != esz) {  // Float32 values on an fp64 launch; any other pair has no kernel and is an error
        if (esz != 8 || vsz != 4) return (int)hipErrorInvalidValue;
        return launch_sweep_f64n(kind, d_bins, nbins, total_tiles, tile_bytes, x, y, alpha, beta, rd, stream);
    }
#define VBC_SWEEP_ARGS d_bins, nbins, total_tiles, tile_bytes, diag, x, y, alpha, beta, rd, stream
    if (esz == 8) { if (kind == 0) launch_any<double, 0>(VBC_SWEEP_ARGS); else launch_any<double, 1>(VBC_SWEEP_ARGS); }
    else { if (kind == 0) launch_any<float, 0>(VBC_SWEEP_ARGS); else launch_any<float, 1>(VBC_SWEEP_ARGS); }
#undef VBC_SWEEP_ARGS
    return hipGetLastError();
}

}  // namespace vbc
