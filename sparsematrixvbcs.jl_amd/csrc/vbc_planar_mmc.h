// gfx950 planar and lane-pair multi-RHS kernels on column-major operands: Y = alpha * B' X + beta * Y over the
// planar chunks (run_planar) and the lane-pair run-rows (run_pair) of vbc_planar.h (device code, included by the
// vbc_planar_mmc_*.hip translation units only).
//
// X (m x nrhs) and Y (n x nrhs) are column-major: X[i + j * ldx], Y[i + j * ldy] with ldx >= m, ldy >= n (a Julia
// Matrix).  run_planar_mmc is run_planar<T, W_, U, false, 0, KC, RUN, MASK, S> and run_pair_mmc is
// run_pair<NRS, false, 0, KC, MASK, false, S> with the accumulators widened by a column index, the step
// run_slots_mm (vbc_slots_mm.h, kRhsCols) took from run_slots: the same SlotBin, ranges, chunks, RUN-aligned clamped
// unconditional loads, keys in both forms, nlive masking, `live` / `pad` selects, two-stage ping-pong and the
// y-offset table staged through LDS (kSlotOutEntries).  Each stored value is loaded once and meets the NR
// right-hand sides of its x row in NR fused multiply-adds, rows in stored order, and every column keeps
// accumulators of its own: column j of Y is, bit for bit, what spmv_planar / spmv_planar_pair gives for column j of
// X, whichever write path (staged or direct) that product takes -- a staged chunk holds alpha * acc, the value the
// direct flush writes when beta = 0.  A launch covers nr <= NR live columns starting at the X / Y pointers it is
// given; columns j >= nr are neither read nor written.
//   gather: per run, NR gathers of the single-vector kernel's form at x + min(j, nr - 1) * ldx + gi (the column
//       bases are wave-uniform and the loads stay unconditional).
//   flush:  per live column at y + j * ldy + o with the single-vector direct-flush expressions: q = alpha * acc,
//       then fmadd(beta, y, q) only when beta != 0; columns e >= wst are never written.
//   The staged-burst write path (NB > 0) has no counterpart here.
#pragma once
#include "vbc_planar.h"

namespace vbc {

template <typename T, int W_, int U, bool KC, int RUN, bool MASK, typename S, int NR>
__device__ __forceinline__ void run_planar_mmc(const SlotBin &b, int r, int lane, const T *__restrict__ x, int64_t ldx,
                                               T *__restrict__ y, int64_t ldy, int nr, T alpha, T beta, bool rd,
                                               int *lds_out)
{
    const int R0 = G(b.rrow)[r], R1 = G(b.rrow)[r + 1];
    if (R0 >= R1) return;
    int c = G(b.rchunk)[r];
    const gptr<const S> val = G(static_cast<const S *>(b.val));
    const gptr<const uint32_t> key = G(b.key);
    // the columns of X a launch reads: base j of a dead column (j >= nr) is the last live column's
    gptr<const T> xc[NR];
#pragma unroll
    for (int j = 0; j < NR; j++) xc[j] = G(x) + (int64_t)min(j, nr - 1) * ldx;
    typedef __attribute__((address_space(4))) const uint32_t *cptr;
    const cptr bases = (cptr)b.base;
    const cptr doffs = (cptr)b.kdoff;
    const cptr nlive = (cptr)b.nlive;
    constexpr int NRUN = U / RUN;  // runs per step (ranges start and end on run boundaries)
    static_assert(NRUN * RUN == U, "a step holds whole runs");
    constexpr int XS = xrun_slots<T, RUN>();
    auto load = [&](int R, uint32_t (&kk)[NRUN], uint32_t (&bs)[NRUN], int (&nl)[NRUN], S (&v)[U][W_]) {
#pragma unroll
        for (int j = 0; j < NRUN; j++) {
            const int Rk = min(R + j * RUN, R1 - RUN);  // the run's first row (clamped: rows past the range)
            int ln = lane;
            if constexpr (MASK) {
                nl[j] = (int)nlive[Rk];
                ln = lane < nl[j] ? lane : 0;
            }
            if constexpr (KC) {
                kk[j] = (uint32_t)(int32_t)((gptr<const int16_t>)key)[(size_t)doffs[Rk] + ln];
                bs[j] = bases[Rk];
            } else {
                kk[j] = __builtin_nontemporal_load(key + (size_t)Rk * 64 + ln);
                bs[j] = 0;
            }
#pragma unroll
            for (int d = 0; d < RUN; d++) {
                const int Rc = min(R + j * RUN + d, R1 - 1);
                ld_row<S, W_, 0>(val + (size_t)Rc * 64 * W_, ln, v[j * RUN + d]);
            }
        }
    };
    constexpr uint32_t kPad16 = 0xFFFF8000u;
    auto gather = [&](const uint32_t (&kk)[NRUN], const uint32_t (&bs)[NRUN], T (&xv)[NRUN][NR][XS]) {
#pragma unroll
        for (int j = 0; j < NRUN; j++) {
            const uint32_t gi = KC ? (bs[j] & kSlotIdx) + (kk[j] == kPad16 ? 0u : kk[j]) : kk[j] & kSlotIdx;
#pragma unroll
            for (int q = 0; q < NR; q++) ld_xrun<T, RUN>(xc[q], gi, xv[j][q]);
        }
    };
    T acc[NR][W_];
#pragma unroll
    for (int q = 0; q < NR; q++)
#pragma unroll
        for (int e = 0; e < W_; e++) acc[q][e] = T(0);
    const int c0 = c;
    if (!b.out_affine) {
        const int n = min(kSlotOutEntries, b.nseg - c0 * 64);
        for (int i = lane; i < n; i += 64) lds_out[i] = G(b.out)[c0 * 64 + i];
    }
    auto flush = [&]() {
        const int seg = c * 64 + lane;
        if (seg < b.nseg) {
            const int o = b.out_affine ? b.out_base + seg * b.out_stride : lds_out[(c - c0) * 64 + lane];
            const int lim = b.wst;  // padding columns (w > wst) are never written
#pragma unroll
            for (int q = 0; q < NR; q++) {
                if (q < nr) {
                    gptr<T> yo = G(y) + (int64_t)q * ldy + o;
#pragma unroll
                    for (int e = 0; e < W_; e++) {
                        if (e < lim) {
                            T t = alpha * acc[q][e];
                            if (rd) t = fmadd(beta, yo[e], t);
                            yo[e] = t;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NR; q++)
#pragma unroll
            for (int e = 0; e < W_; e++) acc[q][e] = T(0);
        c++;
    };
    int R1v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(R1v) : "s"(R1));
    auto compute = [&](int R, const uint32_t (&kk)[NRUN], const uint32_t (&bs)[NRUN], const int (&nl)[NRUN],
                       const S (&v)[U][W_], const T (&xv)[NRUN][NR][XS]) {
#pragma unroll
        for (int j = 0; j < NRUN; j++) {
            const bool pad = MASK ? lane >= nl[j] : (KC ? kk[j] == kPad16 : (kk[j] & kPad) != 0);
            const bool live = R + j * RUN < R1v && !(MASK && pad);  // MASK: lane 0's values, never folded
            T xr[NR][RUN];
#pragma unroll
            for (int q = 0; q < NR; q++) xrun_values<T, RUN>(xv[j][q], xr[q]);
#pragma unroll
            for (int d = 0; d < RUN; d++) {  // the run's rows in stored (reference) order
#pragma unroll
                for (int e = 0; e < W_; e++) {
                    const T ve = (T)v[j * RUN + d][e];  // loaded once, folded into every column
#pragma unroll
                    for (int q = 0; q < NR; q++) {
                        const T xe = pad ? T(0) : xr[q][d];
                        const T nv = fmadd(ve, xe, acc[q][e]);
                        acc[q][e] = live ? nv : acc[q][e];
                    }
                }
            }
            const uint32_t lastw = KC ? bs[j] : (uint32_t)__builtin_amdgcn_readfirstlane((int)kk[j]);
            if (R + j * RUN < R1 && (lastw & kLast)) flush();
        }
    };
    uint32_t kA[NRUN], kB[NRUN], bA[NRUN], bB[NRUN];
    int nA[NRUN], nB[NRUN];
    S vA[U][W_], vB[U][W_];
    T xv[NRUN][NR][XS];
    load(R0, kA, bA, nA, vA);
    __builtin_amdgcn_s_waitcnt(0);
    for (int R = R0; R < R1; R += 2 * U) {
        gather(kA, bA, xv);
        load(R + U, kB, bB, nB, vB);
        compute(R, kA, bA, nA, vA, xv);
        gather(kB, bB, xv);
        load(R + 2 * U, kA, bA, nA, vA);
        compute(R + U, kB, bB, nB, vB, xv);
    }
}

// Rows per pipeline step: planar_step scaled down by NR as slot_mm_step does (the x values of a step and the
// NR * W_ accumulators are the register cost that grows with NR), whole runs, at least one run per stage.  No
// instance uses scratch (DESIGN.md §11.2 has the compiler's table).
template <typename T, int W_, int RUN>
__host__ __device__ constexpr int planar_mmc_step(int NR)
{
    const int u = planar_step<T, W_, RUN>() / NR / RUN * RUN;
    return u < RUN ? RUN : u;
}

// One wave per range of one planar bin (each planar bin is a launch of its own, as spmv_planar).
template <typename T, int W_, bool KC, int RUN, bool MASK, typename S, int NR>
__global__ __launch_bounds__(kBlockThreads) void spmm_planar_col(const SlotBin b, const T *__restrict__ x, int64_t ldx,
                                                                 T *__restrict__ y, int64_t ldy, int nr, T alpha,
                                                                 T beta, int rd_i)
{
    const int blk = b.xcd ? xcd_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int rg = __builtin_amdgcn_readfirstlane((int)(blk * kWavesPerBlock + (threadIdx.x >> 6)));
    if (rg >= b.nranges) return;
    const int lane = threadIdx.x & 63;
    __shared__ int outs[kWavesPerBlock * kSlotOutEntries];
    int *lds_out = outs + (threadIdx.x >> 6) * kSlotOutEntries;
    run_planar_mmc<T, W_, planar_mmc_step<T, W_, RUN>(NR), KC, RUN, MASK, S, NR>(b, rg, lane, x, ldx, y, ldy, nr, alpha,
                                                                                beta, rd_i != 0, lds_out);
}

// The lane-pair form (SlotBin::pair: fp64, 3-wide stripes, runs of 3).  Per column one d2 gather at
// x_j + gi + odd, its own DPP swap and its own acc0[j] / acc1[j]; the fmadd chains are run_pair's.
// DOT (SlotBin::dot, the forward product of 3 x 3 node blocks; vbc_planar_fwd_mmc.h's units launch it): run_pair's
// DOT expressions per column -- the block's dot products d0 / d1 first, then acc = (live && !pad) ? acc + d : acc --
// with the same loads, keys, gathers, swap and flush.
template <int NRS, bool KC, bool MASK, typename S, int NR, bool DOT = false>
__device__ __forceinline__ void run_pair_mmc(const SlotBin &b, int r, int lane, const double *__restrict__ x,
                                             int64_t ldx, double *__restrict__ y, int64_t ldy, int nr, double alpha,
                                             double beta, bool rd, int *lds_out)
{
    typedef double d2 __attribute__((ext_vector_type(2)));
    typedef S s2 __attribute__((ext_vector_type(2)));
    const int R0 = G(b.rrow)[r], R1 = G(b.rrow)[r + 1];
    if (R0 >= R1) return;
    int c = G(b.rchunk)[r];
    const bool odd = (lane & 1) != 0;
    const int ps = lane >> 1;  // stripe slot of the pair
    const gptr<const S> val = G(static_cast<const S *>(b.val));
    const gptr<const uint32_t> key = G(b.key);
    gptr<const double> xc[NR];
#pragma unroll
    for (int q = 0; q < NR; q++) xc[q] = G(x) + (int64_t)min(q, nr - 1) * ldx;
    typedef __attribute__((address_space(4))) const uint32_t *cptr;
    const cptr bases = (cptr)b.base;
    const cptr doffs = (cptr)b.kdoff;
    const cptr nlive = (cptr)b.nlive;
    // per-lane element offsets of the three value loads inside a run-row
    const int o0 = 2 * lane, o1 = odd ? 192 + ps : 128 + 2 * ps, o2 = 224 + 2 * ps;
    auto load = [&](int R, uint32_t (&kk)[NRS], uint32_t (&bs)[NRS], int (&nl)[NRS], s2 (&v)[NRS][3]) {
#pragma unroll
        for (int j = 0; j < NRS; j++) {
            const int Rc = min(R + j, R1 - 1);
            int mps = ps, m0 = o0, m1 = o1, m2 = o2, mlane = lane;
            if constexpr (MASK) {  // dead pairs: pair 0's addresses (lane parity kept)
                nl[j] = (int)nlive[Rc];
                const bool dead = ps >= nl[j];
                mps = dead ? 0 : ps;
                mlane = dead ? (odd ? 1 : 0) : lane;
                m0 = dead ? (odd ? 1 : 0) * 2 : o0;
                m1 = dead ? (odd ? 192 : 128) : o1;
                m2 = dead ? 224 : o2;
            }
            if constexpr (KC) {
                kk[j] = (uint32_t)(int32_t)((gptr<const int16_t>)key)[(size_t)doffs[Rc] + mps];
                bs[j] = bases[Rc];
            } else {
                kk[j] = key[(size_t)Rc * 32 + mps];
                bs[j] = 0;
            }
            const gptr<const S> rowp = val + (size_t)Rc * 288;
            pair_load<S>(rowp, m0, m1, m2, odd, mlane, mps, v[j]);
        }
    };
    constexpr uint32_t kPad16 = 0xFFFF8000u;
    auto gather = [&](const uint32_t (&kk)[NRS], const uint32_t (&bs)[NRS], d2 (&xv)[NRS][NR]) {
#pragma unroll
        for (int j = 0; j < NRS; j++) {
            const uint32_t gi = KC ? (bs[j] & kSlotIdx) + (kk[j] == kPad16 ? 0u : kk[j]) : kk[j] & kSlotIdx;
#pragma unroll
            for (int q = 0; q < NR; q++)
                xv[j][q] = *(const __attribute__((address_space(1))) d2 *)(xc[q] + gi + (odd ? 1 : 0));  // 8-B aligned
        }
    };
    double acc0[NR], acc1[NR];  // even: columns 0, 1; odd: column 2 in acc0
#pragma unroll
    for (int q = 0; q < NR; q++) acc0[q] = acc1[q] = 0.0;
    const int c0 = c;
    if (!b.out_affine) {
        const int n = min(kSlotOutEntries, b.nseg - c0 * 32);
        for (int i = lane; i < n; i += 64) lds_out[i] = G(b.out)[c0 * 32 + i];
    }
    auto flush = [&]() {
        const int seg = c * 32 + ps;
        if (seg < b.nseg) {
            const int o = b.out_affine ? b.out_base + seg * b.out_stride : lds_out[(c - c0) * 32 + ps];
#pragma unroll
            for (int q = 0; q < NR; q++) {
                if (q < nr) {
                    gptr<double> yo = G(y) + (int64_t)q * ldy + o;
                    if (odd) {
                        double t = alpha * acc0[q];
                        if (rd) t = fmadd(beta, yo[2], t);
                        yo[2] = t;
                    } else {
                        double t0 = alpha * acc0[q], t1 = alpha * acc1[q];
                        if (rd) {
                            t0 = fmadd(beta, yo[0], t0);
                            t1 = fmadd(beta, yo[1], t1);
                        }
                        yo[0] = t0;
                        yo[1] = t1;
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NR; q++) acc0[q] = acc1[q] = 0.0;
        c++;
    };
    int R1v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(R1v) : "s"(R1));
    auto compute = [&](int R, const uint32_t (&kk)[NRS], const uint32_t (&bs)[NRS], const int (&nl)[NRS],
                       const s2 (&v)[NRS][3], const d2 (&xv)[NRS][NR]) {
#pragma unroll
        for (int j = 0; j < NRS; j++) {
            const bool pad = MASK ? ps >= nl[j] : (KC ? kk[j] == kPad16 : (kk[j] & kPad) != 0);
            const bool live = R + j < R1v && !(MASK && pad);  // MASK: pair 0's values, never folded
            const s2 r2 = pair_r2<S>(v[j]);
            // even: v[0] = {r0c0, r0c1}, v[1] = {r1c0, r1c1}, r2 = {r2c0, r2c1}
            // odd:  v[0] = {r0c2, r1c2}, v[1].x = r2c2
#pragma unroll
            for (int q = 0; q < NR; q++) {
                // even sends x[g] (its .x), odd sends x[g+2] (its .y); each receives the element it lacks
                const double t = odd ? xv[j][q].y : xv[j][q].x;
                const uint64_t tb = __builtin_bit_cast(uint64_t, t);
                const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)tb, 0xB1, 0xF, 0xF, true);
                const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(tb >> 32), 0xB1, 0xF, 0xF, true);
                const double other = __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
                double x0 = odd ? other : xv[j][q].x, x1 = odd ? xv[j][q].x : xv[j][q].y, x2 = odd ? xv[j][q].y : other;
                if (pad) x0 = x1 = x2 = 0.0;
                if constexpr (DOT) {
                    const double d0 = odd ? fmadd((double)v[j][1].x, x2, fmadd((double)v[j][0].y, x1, (double)v[j][0].x * x0))
                                          : fmadd((double)r2.x, x2, fmadd((double)v[j][1].x, x1, (double)v[j][0].x * x0));
                    const double d1 = fmadd((double)r2.y, x2, fmadd((double)v[j][1].y, x1, (double)v[j][0].y * x0));
                    acc0[q] = (live && !pad) ? acc0[q] + d0 : acc0[q];
                    acc1[q] = (live && !pad) ? acc1[q] + d1 : acc1[q];
                } else {
                    const double n0 = odd ? fmadd((double)v[j][1].x, x2, fmadd((double)v[j][0].y, x1, fmadd((double)v[j][0].x, x0, acc0[q])))
                                          : fmadd((double)r2.x, x2, fmadd((double)v[j][1].x, x1, fmadd((double)v[j][0].x, x0, acc0[q])));
                    const double n1 = fmadd((double)r2.y, x2, fmadd((double)v[j][1].y, x1, fmadd((double)v[j][0].y, x0, acc1[q])));
                    acc0[q] = live ? n0 : acc0[q];
                    acc1[q] = live ? n1 : acc1[q];
                }
            }
            const uint32_t lastw = KC ? bs[j] : (uint32_t)__builtin_amdgcn_readfirstlane((int)kk[j]);
            if (R + j < R1 && (lastw & kLast)) flush();
        }
    };
    uint32_t kA[NRS], kB[NRS], bA[NRS], bB[NRS];
    int nA[NRS], nB[NRS];
    s2 vA[NRS][3], vB[NRS][3];
    d2 xv[NRS][NR];
    load(R0, kA, bA, nA, vA);
    __builtin_amdgcn_s_waitcnt(0);
    for (int R = R0; R < R1; R += 2 * NRS) {
        gather(kA, bA, xv);
        load(R + NRS, kB, bB, nB, vB);
        compute(R, kA, bA, nA, vA, xv);
        gather(kB, bB, xv);
        load(R + 2 * NRS, kA, bA, nA, vA);
        compute(R + NRS, kB, bB, nB, vB, xv);
    }
}

// Run-rows per pipeline stage: spmv_planar_pair's (VBC_PAIR_NRS = 4) scaled down by NR, at least one.
__host__ __device__ constexpr int pair_mmc_step(int NR) { return VBC_PAIR_NRS / NR < 1 ? 1 : VBC_PAIR_NRS / NR; }

template <bool KC, bool MASK, typename S, int NR, bool DOT = false>
__global__ __launch_bounds__(kBlockThreads) void spmm_pair_col(const SlotBin b, const double *__restrict__ x,
                                                               int64_t ldx, double *__restrict__ y, int64_t ldy, int nr,
                                                               double alpha, double beta, int rd_i)
{
    const int blk = b.xcd ? xcd_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int rg = __builtin_amdgcn_readfirstlane((int)(blk * kWavesPerBlock + (threadIdx.x >> 6)));
    if (rg >= b.nranges) return;
    const int lane = threadIdx.x & 63;
    __shared__ int outs[kWavesPerBlock * kSlotOutEntries];
    int *lds_out = outs + (threadIdx.x >> 6) * kSlotOutEntries;
    run_pair_mmc<pair_mmc_step(NR), KC, MASK, S, NR, DOT>(b, rg, lane, x, ldx, y, ldy, nr, alpha, beta, rd_i != 0,
                                                          lds_out);
}

}  // namespace vbc
