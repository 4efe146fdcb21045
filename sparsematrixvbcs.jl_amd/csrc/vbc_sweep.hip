// Launchers of the row-swept SpMV kernel (vbc_sweep.h) on values of the compute eltype; a bin of Float32 values
// under fp64 compute (VBC_CREATE_NARROW_SWEPT) goes to vbc_sweep_f64n.hip.
#include "vbc_sweep_launch.inc"

namespace vbc {

// vbc_sweep_f64n.hip: spmv_sweep<double, KIND, TB, 0, float> (swept bins with SweepBin::vsz = 4)
int launch_sweep_f64n(int kind, const SweepBin *d_bins, int nbins, int total_tiles, int tile_bytes, const void *x, void *y,
                      double alpha, double beta, bool rd, hipStream_t stream);

int launch_sweep(int esz, int vsz, int kind, const SweepBin *d_bins, int nbins, int total_tiles, int tile_bytes, int diag,
                 const void *x, void *y, double alpha, double beta, bool rd, hipStream_t stream)
{
    if (total_tiles <= 0) return hipSuccess;
    if (vsz != esz) {  // Float32 values on an fp64 launch; any other pair has no kernel and is an error
        if (esz != 8 || vsz != 4) return (int)hipErrorInvalidValue;
        return launch_sweep_f64n(kind, d_bins, nbins, total_tiles, tile_bytes, x, y, alpha, beta, rd, stream);
    }
#define VBC_SWEEP_ARGS d_bins, nbins, total_tiles, tile_bytes, diag, x, y, alpha, beta, rd, stream
    if (esz == 8) { if (kind == 0) launch_any<double, double, 0>(VBC_SWEEP_ARGS); else launch_any<double, double, 1>(VBC_SWEEP_ARGS); }
    else { if (kind == 0) launch_any<float, float, 0>(VBC_SWEEP_ARGS); else launch_any<float, float, 1>(VBC_SWEEP_ARGS); }
#undef VBC_SWEEP_ARGS
    return hipGetLastError();
}

}  // namespace vbc
