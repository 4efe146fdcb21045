// The single-vector launchers of one planar bin for one value type (the kernels of vbc_planar.h; included by
// vbc_planar_f64.hip / vbc_planar_f32.hip / vbc_planar_f64n.hip).  The unit defines VBC_PLANAR_T and VBC_PLANAR_SUFFIX,
// and VBC_PLANAR_S when the stored values are narrower than VBC_PLANAR_T: one translation unit per type so they compile
// in parallel, each with the kernels of its own type only.  A unit whose stored type is its compute type also has the
// split kernels, the fused split launch and the occupancy queries; lane pairs exist for fp64 compute only.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "vbc_planar.h"

#ifndef VBC_PLANAR_S
#define VBC_PLANAR_S VBC_PLANAR_T
#define VBC_PLANAR_WIDE
#endif

namespace vbc {

template <int I>
using ic = std::integral_constant<int, I>;

// A chunk form at its compile-time parameters: kernel<FASTE, NB, MASK> is its instance on one write path, kNB the NB
// of its staged one.
template <typename T, typename S, int W_, int RUN, bool KC>
struct Runs {  // row chunks: w in 3..8, runs of 1..3
    static constexpr int kNB = planar_nb<T, W_>();
    template <bool FASTE, int NB, bool MASK>
    static constexpr auto kernel = spmv_planar<T, W_, FASTE, NB, KC, RUN, MASK, S>;
};
template <typename T, typename S, int W_, int R, bool KC>
struct RunsFwd {  // forward row runs: w in {2, 3, 4}, R in {2, 3}
    static constexpr int kNB = 8192 / (64 * R * (int)sizeof(T)) > 8 ? 8 : 8192 / (64 * R * (int)sizeof(T));
    template <bool FASTE, int NB, bool MASK>
    static constexpr auto kernel = spmv_planar_fwd<T, W_, R, FASTE, NB, KC, MASK, S>;
};
template <typename S, bool KC, bool DOT>
struct Pairs {  // lane pairs: fp64, w = 3, runs of 3; DOT: the forward product of 3 x 3 node blocks (SlotBin::dot)
    static constexpr int kNB = 8;
    template <bool FASTE, int NB, bool MASK>
    static constexpr auto kernel = spmv_planar_pair<FASTE, NB, KC, MASK, DOT, S>;
};

// The write path of a chunk form: the y-offset table of the chunk-local length order (never the affine path), the
// staged affine path, the affine path, or read-modify-write.
template <typename FORM, typename T>
static int launch_path(const SlotBin &hb, bool faste, bool staged, const T *x, T *y, double alpha, double beta, bool rd,
                       hipStream_t s)
{
    const dim3 grid((hb.nranges + kWavesPerBlock - 1) / kWavesPerBlock), blk(kBlockThreads);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, blk, 0, s, hb, x, y, (T)alpha, (T)beta, (int)rd); };
    if (hb.mask) go(FORM::template kernel<false, 0, true>);
    else if (faste && staged) go(FORM::template kernel<true, FORM::kNB, false>);
    else if (faste) go(FORM::template kernel<true, 0, false>);
    else go(FORM::template kernel<false, 0, false>);
    return (int)hipGetLastError();
}

// A lane-stream form (B'x): kernel<DEEP, RD> is its instance.
template <typename T, typename S, int W_, int RUN, int DIAG = 0>
struct Lanes {  // per-lane compacted streams: w in 3..8, runs of 1..3
    template <bool DEEP, bool RD>
    static constexpr auto kernel = spmv_planar_lanes<T, W_, RUN, DEEP, RD, DIAG, S>;
};
template <typename S>
struct PairLanes {  // lane-pair streams: fp64, w = 3, runs of 3 (no DEEP form)
    template <bool DEEP, bool RD>
    static constexpr auto kernel = spmv_pair_lanes<RD, S>;
};

template <typename FORM, typename T>
static int launch_stream(const SlotBin &hb, const T *x, T *y, double alpha, double beta, bool rd, hipStream_t s)
{
    const dim3 grid((hb.nranges + kWavesPerBlock - 1) / kWavesPerBlock), blk(kBlockThreads);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, blk, 0, s, hb, x, y, (T)alpha, (T)beta); };
    if (rd) go(FORM::template kernel<false, true>);
    else if (hb.deep) go(FORM::template kernel<true, false>);
    else go(FORM::template kernel<false, false>);
    return (int)hipGetLastError();
}

// f(w, run) at the bin's width and row run (SlotBin::run: 1 (none), 2 or 3 consecutive x rows per gather), both as
// integral constants, for widths WLO..WHI and runs RLO..3; any other (w, run) has no kernel.
template <int WLO, int WHI, int RLO, typename F>
static int by_width_run(const SlotBin &hb, F f)
{
#define VBC_WR(W, R)                                    \
    if constexpr (W >= WLO && W <= WHI && R >= RLO)     \
        if (hb.wkey == W && hb.run == R) return f(ic<W>{}, ic<R>{});
#define VBC_W(W) VBC_WR(W, 1) VBC_WR(W, 2) VBC_WR(W, 3)
    VBC_W(1) VBC_W(2) VBC_W(3) VBC_W(4) VBC_W(5) VBC_W(6) VBC_W(7) VBC_W(8)
#undef VBC_W
#undef VBC_WR
    return (int)hipErrorInvalidValue;
}

// f(P) at P = 2, 4 or 8 waves per workgroup (anything else as 8), as an integral constant
template <typename F>
static void by_waves(int p, F f)
{
    p == 2 ? f(ic<2>{}) : p == 4 ? f(ic<4>{}) : f(ic<8>{});
}

// few chunks: P waves per chunk (SlotBin::split), w in 1..8, runs of 1..3 (no narrow form)
template <typename T, int W_, int RUN, bool KC, int DIAG = 0>
static int launch_split(const SlotBin &hb, const T *x, T *y, double alpha, double beta, bool rd, hipStream_t s)
{
#ifdef VBC_ABLATION
    if constexpr (W_ == 3 && RUN == 3 && !KC && DIAG == 0) {  // ablations (the VBC_ABLATION build only, VBC_DIAG=1..4)
        if (hb.diag == 1) return launch_split<T, 3, 3, false, 1>(hb, x, y, alpha, beta, rd, s);
        if (hb.diag == 2) return launch_split<T, 3, 3, false, 2>(hb, x, y, alpha, beta, rd, s);
        if (hb.diag == 3) return launch_split<T, 3, 3, false, 3>(hb, x, y, alpha, beta, rd, s);
        if (hb.diag == 4) return launch_split<T, 3, 3, false, 4>(hb, x, y, alpha, beta, rd, s);
    }
#endif
    by_waves(hb.split, [&](auto p) {
        hipLaunchKernelGGL((spmv_planar_split<T, W_, KC, RUN, p, DIAG>), dim3(hb.nranges), dim3(64 * p), 0, s, hb, x, y,
                           (T)alpha, (T)beta, (int)rd);
    });
    return (int)hipGetLastError();
}

template <typename T, int W_, int R>
static int launch_fwd_split(const SlotBin &hb, const T *x, T *y, double alpha, double beta, bool rd, hipStream_t s)
{
    by_waves(hb.split, [&](auto p) {
        hipLaunchKernelGGL((spmv_planar_fwd_split<T, W_, R, p>), dim3(hb.nranges), dim3(64 * p), 0, s, hb, x, y,
                           (T)alpha, (T)beta, (int)rd);
    });
    return (int)hipGetLastError();
}

#define VBC_CAT2(a, b) a##b
#define VBC_CAT(a, b) VBC_CAT2(a, b)

#ifdef VBC_PLANAR_WIDE
// The fused split bins of a launch, P waves per chunk.
int VBC_CAT(launch_split_multi_, VBC_PLANAR_SUFFIX)(const SplitMulti &M, int P, const void *x, void *y, double alpha,
                                                    double beta, bool rd, hipStream_t s)
{
    typedef VBC_PLANAR_T T;
    if (P != 2 && P != 4 && P != 8) return (int)hipErrorInvalidValue;
    by_waves(P, [&](auto p) {
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(M.nchunks), dim3(64 * p), 0, s, M, static_cast<const T *>(x),
                               static_cast<T *>(y), (T)alpha, (T)beta, (int)rd);
        };
        switch (M.pad0) {  // SplitMulti::pad0: slice loop 0 plain, 1 pipelined, 2 batched, 3 batched non-temporal
        case 3: go(spmv_split_multi<T, p, 3>); break;
        case 2: go(spmv_split_multi<T, p, 2>); break;
        case 1: go(spmv_split_multi<T, p, 1>); break;
        default: go(spmv_split_multi<T, p, 0>); break;
        }
    });
    return (int)hipGetLastError();
}

// Resident waves per CU of the fused split launch (batched slice loop) with P waves per workgroup.
int VBC_CAT(occupancy_split_multi_, VBC_PLANAR_SUFFIX)(int P)
{
    int nb = 0;
    by_waves(P, [&](auto p) {
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, spmv_split_multi<VBC_PLANAR_T, p, 2>, 64 * p, 0);
    });
    return nb * P;
}

int VBC_CAT(occupancy_planar_, VBC_PLANAR_SUFFIX)()
{
    int occ = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, spmv_planar<VBC_PLANAR_T, 3, true, 0, true, 1>, kBlockThreads, 0);
    return occ;
}

int VBC_CAT(occupancy_lanes_, VBC_PLANAR_SUFFIX)()
{
    int occ = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, spmv_planar_lanes<VBC_PLANAR_T, 3, 3, false, false>, kBlockThreads, 0);
    return occ;
}
#endif  // VBC_PLANAR_WIDE

// The chunk forms (one wave per range, or P waves per chunk of a split bin) at one key form.
template <typename T, typename S, bool KC>
static int launch_chunks(const SlotBin &hb, bool faste, bool staged, const T *x, T *y, double alpha, double beta,
                         bool rd, hipStream_t s)
{
    constexpr bool kWide = std::is_same_v<S, T>;
    if (hb.kind == 1)  // forward with row runs (vbc_planar.h run_planar_fwd)
        return by_width_run<2, 4, 2>(hb, [&](auto w, auto r) {
            if constexpr (kWide && !KC)
                if (hb.split > 1) return launch_fwd_split<T, w, r>(hb, x, y, alpha, beta, rd, s);
            return launch_path<RunsFwd<T, S, w, r, KC>>(hb, faste, staged, x, y, alpha, beta, rd, s);
        });
    if constexpr (sizeof(T) == 8)
        if (hb.pair)  // lane pairs (vbc_planar.h run_pair)
            return hb.dot ? launch_path<Pairs<S, KC, true>>(hb, faste, staged, x, y, alpha, beta, rd, s)
                          : launch_path<Pairs<S, KC, false>>(hb, faste, staged, x, y, alpha, beta, rd, s);
    if constexpr (kWide)
        if (hb.split > 1)
            return by_width_run<1, 8, 1>(hb, [&](auto w, auto r) {
                return launch_split<T, w, r, KC>(hb, x, y, alpha, beta, rd, s);
            });
    return by_width_run<3, 8, 1>(hb, [&](auto w, auto r) {
        return launch_path<Runs<T, S, w, r, KC>>(hb, faste, staged, x, y, alpha, beta, rd, s);
    });
}

// One planar bin with at least one range.  The bin's stored value type must be this unit's (the caller picks the unit
// by SlotBin::vsz).  A form without a kernel is an error, never another kernel on the wrong bytes.
int VBC_CAT(launch_planar_, VBC_PLANAR_SUFFIX)(const SlotBin &hb, bool faste, bool staged, const void *x, void *y,
                                               double alpha, double beta, bool rd, hipStream_t s)
{
    typedef VBC_PLANAR_T T;
    typedef VBC_PLANAR_S S;
    constexpr bool kNarrow = sizeof(S) < sizeof(T);
    const T *xs = static_cast<const T *>(x);
    T *ys = static_cast<T *>(y);
    if ((hb.vsz == 4) != kNarrow || (hb.vsz != 0 && hb.vsz != 4)) return (int)hipErrorInvalidValue;
    // narrow values: only in planar bins of one wave per range, never fused or with holes
    if (kNarrow && (!hb.planar || hb.split > 1 || hb.fused || hb.holes)) return (int)hipErrorInvalidValue;
    if (hb.pair && (sizeof(T) != 8 || hb.wkey != 3 || hb.run != 3)) return (int)hipErrorInvalidValue;
    if (hb.lanes && hb.kind != 0) return (int)hipErrorInvalidValue;
    if (kNarrow && hb.pair && hb.kind != 0) return (int)hipErrorInvalidValue;  // (the forward form is SlotBin::dot)
    if (hb.lanes) {  // the lane streams (B'x)
        if constexpr (sizeof(T) == 8)
            if (hb.pair) return launch_stream<PairLanes<S>>(hb, xs, ys, alpha, beta, rd, s);
        return by_width_run<3, 8, 1>(hb, [&](auto w, auto r) {
#ifdef VBC_ABLATION
            if constexpr (!kNarrow && w == 3 && r == 3) {  // ablations (the VBC_ABLATION build only, VBC_DIAG=1..3)
                const dim3 grid((hb.nranges + kWavesPerBlock - 1) / kWavesPerBlock), blk(kBlockThreads);
                auto go = [&](auto kernel) {
                    hipLaunchKernelGGL(kernel, grid, blk, 0, s, hb, xs, ys, (T)alpha, (T)beta);
                    return (int)hipGetLastError();
                };
                if (hb.diag == 1) return go(Lanes<T, S, 3, 3, 1>::template kernel<false, false>);
                if (hb.diag == 2) return go(Lanes<T, S, 3, 3, 2>::template kernel<false, false>);
                if (hb.diag == 3) return go(Lanes<T, S, 3, 3, 3>::template kernel<false, false>);
            }
#endif
            return launch_stream<Lanes<T, S, w, r>>(hb, xs, ys, alpha, beta, rd, s);
        });
    }
    return hb.kc ? launch_chunks<T, S, true>(hb, faste, staged, xs, ys, alpha, beta, rd, s)
                 : launch_chunks<T, S, false>(hb, faste, staged, xs, ys, alpha, beta, rd, s);
}

}  // namespace vbc
