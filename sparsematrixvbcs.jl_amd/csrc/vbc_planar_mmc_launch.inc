// The column-major multi-RHS launchers of one planar bin for one value type: spmm_planar_col / spmm_pair_col (B'X;
// included by vbc_planar_mmc_f64.hip / vbc_planar_mmc_f32.hip / vbc_planar_mmc_f64n.hip) and, with VBC_PLANAR_FWD
// defined, spmm_planar_fwd_col / spmm_pair_col<..., DOT> (forward; vbc_planar_fwd_mmc_*.hip).  The unit defines
// VBC_PLANAR_T and VBC_PLANAR_SUFFIX, and VBC_PLANAR_S when the stored values are narrower than VBC_PLANAR_T: one
// translation unit per family and type so they compile in parallel, each with the kernels of its own family only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "vbc_planar_fwd_mmc.h"  // (includes vbc_planar_mmc.h)

#ifndef VBC_PLANAR_S
#define VBC_PLANAR_S VBC_PLANAR_T
#endif

namespace vbc {

// A bin form at its compile-time parameters: kernel<NR, MASK> is its instance for NR columns in the natural or the
// masked chunk order.
template <typename T, typename S, int W_, int RUN, bool KC>
struct RunsCol {  // B'X row chunks: w in 3..8, runs of 1..3 (spmv_planar's forms)
    template <int NR, bool MASK>
    static constexpr auto kernel = spmm_planar_col<T, W_, KC, RUN, MASK, S, NR>;
};
template <typename T, typename S, int W_, int R, bool KC>
struct RunsFwdCol {  // forward row runs: w in {2, 3, 4}, R in {2, 3} (spmv_planar_fwd's forms)
    template <int NR, bool MASK>
    static constexpr auto kernel = spmm_planar_fwd_col<T, W_, R, KC, MASK, S, NR>;
};
template <typename S, bool KC, bool DOT>
struct PairCol {  // lane pairs: fp64, w = 3, runs of 3; DOT: the forward ones
    template <int NR, bool MASK>
    static constexpr auto kernel = spmm_pair_col<KC, MASK, S, NR, DOT>;
};

// NR = 2 or 4, the smallest that holds the nr live columns (every instance is free of scratch at NR = 4: DESIGN.md
// §11.2 and §11.3 have the compiler's tables, so no form falls back to NR = 2 chunks), by MASK.
template <typename FORM, typename T>
static int launch_form(const SlotBin &hb, const T *x, int64_t ldx, T *y, int64_t ldy, int nr, double alpha, double beta,
                       bool rd, hipStream_t s)
{
    const dim3 grid((hb.nranges + kWavesPerBlock - 1) / kWavesPerBlock), blk(kBlockThreads);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, blk, 0, s, hb, x, ldx, y, ldy, nr, (T)alpha, (T)beta, (int)rd);
    };
    if (hb.mask) nr <= 2 ? go(FORM::template kernel<2, true>) : go(FORM::template kernel<4, true>);
    else nr <= 2 ? go(FORM::template kernel<2, false>) : go(FORM::template kernel<4, false>);
    return (int)hipGetLastError();
}

template <bool FWD, typename T, typename S, bool KC>
static int launch_runs(const SlotBin &hb, const T *x, int64_t ldx, T *y, int64_t ldy, int nr, double alpha, double beta,
                       bool rd, hipStream_t s)
{
#define VBC_WR(W, R)                    \
    if (hb.wkey == W && hb.run == R)    \
        return launch_form<std::conditional_t<FWD, RunsFwdCol<T, S, W, R, KC>, RunsCol<T, S, W, R, KC>>>( \
            hb, x, ldx, y, ldy, nr, alpha, beta, rd, s);
    if constexpr (FWD) {
        VBC_WR(2, 2) VBC_WR(2, 3) VBC_WR(3, 2) VBC_WR(3, 3) VBC_WR(4, 2) VBC_WR(4, 3)
    } else {
#define VBC_W(W) VBC_WR(W, 1) VBC_WR(W, 2) VBC_WR(W, 3)
        VBC_W(3) VBC_W(4) VBC_W(5) VBC_W(6) VBC_W(7) VBC_W(8)
#undef VBC_W
    }
#undef VBC_WR
    return (int)hipErrorInvalidValue;
}

// lane pairs: fp64, w = 3, runs of 3 (no fp32 form: a missing kernel is an error)
template <bool DOT, typename T, typename S>
static int launch_pairs(const SlotBin &hb, const T *x, int64_t ldx, T *y, int64_t ldy, int nr, double alpha, double beta,
                        bool rd, hipStream_t s)
{
    if constexpr (sizeof(T) == 8) {
        if (hb.wkey != 3 || hb.run != 3) return (int)hipErrorInvalidValue;
        return hb.kc ? launch_form<PairCol<S, true, DOT>>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s)
                     : launch_form<PairCol<S, false, DOT>>(hb, x, ldx, y, ldy, nr, alpha, beta, rd, s);
    } else {
        return (int)hipErrorInvalidValue;
    }
}

#define VBC_CAT2(a, b) a##b
#define VBC_CAT(a, b) VBC_CAT2(a, b)
#ifdef VBC_PLANAR_FWD
#define VBC_PLANAR_ENTRY VBC_CAT(launch_planar_fwd_mmc_, VBC_PLANAR_SUFFIX)
constexpr bool kFwd = true;
#else
#define VBC_PLANAR_ENTRY VBC_CAT(launch_planar_mmc_, VBC_PLANAR_SUFFIX)
constexpr bool kFwd = false;
#endif

// One planar bin, one wave per range and chunk rows (not split, no lane streams), nr <= 4 live columns at x / y (column
// strides ldx / ldy): of kind 0 in row chunks or lane pairs (B'X), or of kind 1 in row runs or the lane pairs with
// SlotBin::dot (forward).  The bin's stored value type must be this unit's (the caller picks the unit by SlotBin::vsz).
// A form without a kernel is an error.
int VBC_PLANAR_ENTRY(const SlotBin &hb, const void *x, int64_t ldx, void *y, int64_t ldy, int nr, double alpha,
                     double beta, bool rd, hipStream_t stream)
{
    typedef VBC_PLANAR_T T;
    typedef VBC_PLANAR_S S;
    const T *xs = static_cast<const T *>(x);
    T *ys = static_cast<T *>(y);
    if (nr < 1 || nr > 4) return (int)hipErrorInvalidValue;
    if (hb.nranges <= 0) return (int)hipSuccess;
    if (hb.split > 1 || hb.lanes) return (int)hipErrorInvalidValue;
    if ((hb.vsz == 4) != (sizeof(S) < sizeof(T)) || (hb.vsz != 0 && hb.vsz != 4)) return (int)hipErrorInvalidValue;
    const bool form = kFwd ? !hb.fused && (hb.pair ? hb.dot != 0 : hb.kind == 1) : hb.kind == 0 && !hb.dot;
    if (!form) return (int)hipErrorInvalidValue;
    if (hb.pair) return launch_pairs<kFwd, T, S>(hb, xs, ldx, ys, ldy, nr, alpha, beta, rd, stream);
    return hb.kc ? launch_runs<kFwd, T, S, true>(hb, xs, ldx, ys, ldy, nr, alpha, beta, rd, stream)
                 : launch_runs<kFwd, T, S, false>(hb, xs, ldx, ys, ldy, nr, alpha, beta, rd, stream);
}

}  // namespace vbc
