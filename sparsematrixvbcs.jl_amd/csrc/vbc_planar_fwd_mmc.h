// gfx950 forward multi-RHS kernels on column-major operands: Y = alpha * B X + beta * Y over the forward row runs
// (run_planar_fwd, SlotBin kind 1) and the forward lane pairs (run_pair DOT, SlotBin::dot) of vbc_planar.h (device
// code, included by the vbc_planar_fwd_mmc_*.hip translation units only).
//
// X (n x nrhs) and Y (m x nrhs) are column-major: X[i + j * ldx], Y[i + j * ldy] with ldx >= n, ldy >= m (a Julia
// Matrix).  run_planar_fwd_mmc is run_planar_fwd<T, W_, R, U, false, 0, KC, MASK, S>, the direct-flush form (no
// FASTE, no staged chunks, no LDS at all), with the accumulators widened by a column index, the step
// run_planar_mmc (vbc_planar_mmc.h) took from run_planar: the same SlotBin, ranges, chunks, clamped unconditional
// loads, keys in both forms, nlive masking, `live` / `pad` selects, two-stage ping-pong and kLast flush test.  A
// block's R x w stored values are loaded once and meet the NR right-hand sides of the block's x slice in NR sets of
// R dot products, blocks in stored order, and every column keeps accumulators of its own: column j of Y is, bit for
// bit, what spmv_planar_fwd gives for column j of X, whichever write path (staged or direct) that product takes -- a
// staged chunk holds alpha * acc, the value the direct flush writes when beta = 0.  A launch covers nr <= NR live
// columns starting at the X / Y pointers it is given; columns j >= nr are neither read nor written.
//   gather: per block, NR gathers of the single-vector kernel's form at x + min(j, nr - 1) * ldx + gi (the column
//       bases are wave-uniform and the loads stay unconditional).
//   dot:    per column and output row q, run_planar_fwd's expressions: d = v[q*w] * x[0], then
//       d = fmadd(v[q*w+e], x[e], d) for e = 1 .. w-1, then acc[j][q] = (live && !pad) ? acc[j][q] + d : acc[j][q].
//   flush:  per live column at y + j * ldy + o: v = alpha * acc, then fmadd(beta, y, v) only when beta != 0.
// The forward lane pairs are spmm_pair_col<KC, MASK, S, NR, DOT = true> of vbc_planar_mmc.h.
#pragma once
#include "vbc_planar_mmc.h"

namespace vbc {

template <typename T, int W_, int R, int U, bool KC, bool MASK, typename S, int NR>
__device__ __forceinline__ void run_planar_fwd_mmc(const SlotBin &b, int r, int lane, const T *__restrict__ x,
                                                   int64_t ldx, T *__restrict__ y, int64_t ldy, int nr, T alpha,
                                                   T beta, bool rd)
{
    constexpr int WV = R * W_;
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
    constexpr int XS = xrun_slots<T, W_>();
    auto load = [&](int Rr, uint32_t (&kk)[U], uint32_t (&bs)[U], int (&nl)[U], S (&v)[U][WV]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int Rc = min(Rr + u, R1 - 1);
            int ln = lane;
            if constexpr (MASK) {
                nl[u] = (int)nlive[Rc];
                ln = lane < nl[u] ? lane : 0;
            }
            if constexpr (KC) {
                kk[u] = (uint32_t)(int32_t)((gptr<const int16_t>)key)[(size_t)doffs[Rc] + ln];
                bs[u] = bases[Rc];
            } else {
                kk[u] = __builtin_nontemporal_load(key + (size_t)Rc * 64 + ln);
                bs[u] = 0;
            }
            ld_row<S, WV, 0>(val + (size_t)Rc * 64 * WV, ln, v[u]);
        }
    };
    constexpr uint32_t kPad16 = 0xFFFF8000u;
    auto gather = [&](const uint32_t (&kk)[U], const uint32_t (&bs)[U], T (&xv)[U][NR][XS]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t gi = KC ? (bs[u] & kSlotIdx) + (kk[u] == kPad16 ? 0u : kk[u]) : kk[u] & kSlotIdx;
#pragma unroll
            for (int j = 0; j < NR; j++) ld_xrun<T, W_>(xc[j], gi, xv[u][j]);
        }
    };
    T acc[NR][R];
#pragma unroll
    for (int j = 0; j < NR; j++)
#pragma unroll
        for (int q = 0; q < R; q++) acc[j][q] = T(0);
    auto flush = [&]() {
        const int seg = c * 64 + lane;
        if (seg < b.nseg) {  // affine (natural order) or the table of a length-sorted layout
            const int64_t o = b.out_affine ? b.out_base + (int64_t)seg * R : (int64_t)G(b.out)[seg];
#pragma unroll
            for (int j = 0; j < NR; j++) {
                if (j < nr) {
                    gptr<T> yo = G(y) + (int64_t)j * ldy + o;
#pragma unroll
                    for (int q = 0; q < R; q++) {
                        T v = alpha * acc[j][q];
                        if (rd) v = fmadd(beta, yo[q], v);
                        yo[q] = v;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NR; j++)
#pragma unroll
            for (int q = 0; q < R; q++) acc[j][q] = T(0);
        c++;
    };
    int R1v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(R1v) : "s"(R1));
    auto compute = [&](int Rr, const uint32_t (&kk)[U], const uint32_t (&bs)[U], const int (&nl)[U],
                       const S (&v)[U][WV], const T (&xv)[U][NR][XS]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool live = Rr + u < R1v;
            const bool pad = MASK ? lane >= nl[u] : (KC ? kk[u] == kPad16 : (kk[u] & kPad) != 0);
#pragma unroll
            for (int j = 0; j < NR; j++) {
                T xr[W_];
                xrun_values<T, W_>(xv[u][j], xr);
#pragma unroll
                for (int q = 0; q < R; q++) {  // one dot product per output row of the run (values loaded once)
                    T d = (T)v[u][q * W_] * xr[0];
#pragma unroll
                    for (int e = 1; e < W_; e++) d = fmadd((T)v[u][q * W_ + e], xr[e], d);
                    acc[j][q] = (live && !pad) ? acc[j][q] + d : acc[j][q];
                }
            }
            const uint32_t lastw = KC ? bs[u] : (uint32_t)__builtin_amdgcn_readfirstlane((int)kk[u]);
            if (Rr + u < R1 && (lastw & kLast)) flush();
        }
    };
    uint32_t kA[U], kB[U], bA[U], bB[U];
    int nA[U], nB[U];
    S vA[U][WV], vB[U][WV];
    T xv[U][NR][XS];
    load(R0, kA, bA, nA, vA);
    __builtin_amdgcn_s_waitcnt(0);
    for (int Rr = R0; Rr < R1; Rr += 2 * U) {
        gather(kA, bA, xv);
        load(Rr + U, kB, bB, nB, vB);
        compute(Rr, kA, bA, nA, vA, xv);
        gather(kB, bB, xv);
        load(Rr + 2 * U, kA, bA, nA, vA);
        compute(Rr + U, kB, bB, nB, vB, xv);
    }
}

// Blocks per pipeline stage: spmv_planar_fwd's (VBC_FWD_VALS / (R * w) values per lane, at least 2) scaled down by
// NR (the x slices of a stage and the NR * R accumulators are the register cost that grows with NR), at least one.
// No instance uses scratch at this step (DESIGN.md §11.3 has the compiler's table), so none is lowered further.
template <int W_, int R>
__host__ __device__ constexpr int planar_fwd_mmc_step(int NR)
{
    const int u1 = (VBC_FWD_VALS / (R * W_)) < 2 ? 2 : (VBC_FWD_VALS / (R * W_));
    return u1 / NR < 1 ? 1 : u1 / NR;
}

// One wave per range of one forward run bin (each planar bin is a launch of its own, as spmv_planar_fwd).
template <typename T, int W_, int R, bool KC, bool MASK, typename S, int NR>
__global__ __launch_bounds__(kBlockThreads) void spmm_planar_fwd_col(const SlotBin b, const T *__restrict__ x,
                                                                     int64_t ldx, T *__restrict__ y, int64_t ldy,
                                                                     int nr, T alpha, T beta, int rd_i)
{
    const int blk = b.xcd ? xcd_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int rg = __builtin_amdgcn_readfirstlane((int)(blk * kWavesPerBlock + (threadIdx.x >> 6)));
    if (rg >= b.nranges) return;
    const int lane = threadIdx.x & 63;
    run_planar_fwd_mmc<T, W_, R, planar_fwd_mmc_step<W_, R>(NR), KC, MASK, S, NR>(b, rg, lane, x, ldx, y, ldy, nr, alpha,
                                                                                 beta, rd_i != 0);
}

}  // namespace vbc
