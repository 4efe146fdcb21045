// Row-swept kernel launchers, fp64 compute on Float32 stored values (VBC_CREATE_NARROW_SWEPT): spmv_sweep of
// vbc_sweep.h with the value rows read as floats and widened in registers.  A translation unit of its own, so it
// compiles beside vbc_sweep.hip.
#include "vbc_sweep_launch.inc"

namespace vbc {

int launch_sweep_f64n(int kind, const SweepBin *d_bins, int nbins, int total_tiles, int tile_bytes, const void *x, void *y,
                      double alpha, double beta, bool rd, hipStream_t stream)
{
    if (kind == 0) launch_any<double, float, 0>(d_bins, nbins, total_tiles, tile_bytes, 0, x, y, alpha, beta, rd, stream);
    else if (kind == 1) launch_any<double, float, 1>(d_bins, nbins, total_tiles, tile_bytes, 0, x, y, alpha, beta, rd, stream);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

}  // namespace vbc
