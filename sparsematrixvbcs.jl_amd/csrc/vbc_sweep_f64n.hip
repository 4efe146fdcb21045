// Row-swept kernel launchers, fp64 compute on Float32 stored values (VBC_CREATE_NARROW_SWEPT): spmv_sweep of
// vbc_sweep.h with the value rows read as floats and widened in registers.  A translation unit of its own, so
// vbc_sweep.hip compiles as before.  The variants are those launch_sweep picks for a wide fp64 launch: both kinds,
// the three tile sizes; every width 1..8 and both key forms are inside the kernel.
#include <hip/hip_runtime.h>

#include "vbc_sweep.h"

namespace vbc {

template <int KIND, int TB>
static void launch_t_n(const SweepBin *d_bins, int nbins, int total_tiles, const void *x, void *y, double alpha,
                       double beta, bool rd, hipStream_t s)
{
    hipLaunchKernelGGL((spmv_sweep<double, KIND, TB, 0, float>), dim3(total_tiles), dim3(64), 0, s, d_bins, nbins,
                       total_tiles, static_cast<const double *>(x), static_cast<double *>(y), alpha, beta, (int)rd);
}

template <int KIND>
static void launch_any_n(const SweepBin *d_bins, int nbins, int total_tiles, int tile_bytes, const void *x, void *y,
                         double alpha, double beta, bool rd, hipStream_t s)
{
    if (tile_bytes >= 4 * kSweepTileBytes) launch_t_n<KIND, 4 * kSweepTileBytes>(d_bins, nbins, total_tiles, x, y, alpha, beta, rd, s);
    else if (tile_bytes >= 2 * kSweepTileBytes) launch_t_n<KIND, 2 * kSweepTileBytes>(d_bins, nbins, total_tiles, x, y, alpha, beta, rd, s);
    else launch_t_n<KIND, kSweepTileBytes>(d_bins, nbins, total_tiles, x, y, alpha, beta, rd, s);
}

int launch_sweep_f64n(int kind, const SweepBin *d_bins, int nbins, int total_tiles, int tile_bytes, const void *x, void *y,
                      double alpha, double beta, bool rd, hipStream_t stream)
{
    if (kind == 0) launch_any_n<0>(d_bins, nbins, total_tiles, tile_bytes, x, y, alpha, beta, rd, stream);
    else if (kind == 1) launch_any_n<1>(d_bins, nbins, total_tiles, tile_bytes, x, y, alpha, beta, rd, stream);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

}  // namespace vbc
