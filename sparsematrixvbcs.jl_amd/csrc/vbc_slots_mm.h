// gfx950 slotted-segment multi-RHS kernels: Y = alpha * B' X + beta * Y over the slotted B'x layout of
// vbc_slots.h (device code, included by the vbc_slots_mm_*.hip and vbc_slots_mmc_*.hip translation units only).
//
// One body (run_slots_mm, and run_slots_narrow_mm for the fp32 w = 2 two-segment rows) serves both operand layouts;
// the layout is a compile-time parameter (RhsLayout) that decides only how a lane fetches the NR right-hand sides
// of a stored row and how it writes its outputs.  The kernels read the SlotBin arena of spmv_slots -- no layout of
// their own -- and keep run_slots's lane -> (slot, sub) map, chunks, ranges, PAD / LAST handling, clamped
// unconditional loads, two-stage ping-pong and `live` select (kind 0 only).  Each stored value is loaded once and
// meets the NR right-hand sides of its x row in NR fused multiply-adds, so the matrix is streamed once per NR
// columns.  A slot still folds its stripe serially in stored row order and every column j keeps an accumulator of
// its own, so column j of Y is, bit for bit, what spmv_slots gives for column j of X.  A launch covers nr <= NR
// live columns starting at the X / Y pointers it is given; columns j >= nr are neither read nor written.
//   Row-major (spmm_slots; kRhsRows, kRhsRowsVec): X (m x nrhs) and Y (n x nrhs) with the right-hand sides
//       interleaved, X[i * ldx + j].  A lane moves its X row and its Y row with ld_rhs / st_rhs: with 8- / 16-B
//       vector accesses under kRhsRowsVec (chosen by the host per launch, nr == NR only: X, Y and both leading
//       dimensions aligned to the vector), otherwise element by element, the column index clamped to nr - 1 on
//       loads so they stay unconditional.
//   Column-major (spmm_slots_col; kRhsCols): X[i + j * ldx], Y[i + j * ldy] with ldx >= m, ldy >= n (a Julia
//       Matrix), the operand addressing of run_slots per column.
//       gather: NR element loads x[gi + j * ldx] per stored row, the column index clamped to nr - 1 so the loads
//           stay unconditional (the column bases are wave-uniform: one vector offset serves the NR loads).
//       flush:  per live column the lane writes its V contiguous outputs at y + j * ldy + o + sub * V with
//           run_slots's direct-flush forms -- one 8- / 16-B store when the lane owns its whole vector, element
//           stores under e < lim otherwise; q = alpha * acc, then fmadd(beta, y, q) only when beta != 0.
//   y offsets: affine, or table-mapped and staged through LDS per range (kSlotOutEntries, as run_slots).
//   The staged-burst write path of spmv_slots (NB > 0) has no counterpart here.
#pragma once
#include "vbc_slots.h"

namespace vbc {

// The operand layout of an instance: row-major element by element, row-major with vector moves, column-major.
enum RhsLayout { kRhsRows, kRhsRowsVec, kRhsCols };

// One row of NR right-hand sides: p[0 .. nr).
template <typename T, int NR, bool VEC>
__device__ __forceinline__ void ld_rhs(gptr<const T> p, int nr, T (&r)[NR])
{
    if constexpr (VEC) {
        constexpr int VE = NR * (int)sizeof(T) >= 16 ? 16 / (int)sizeof(T) : NR;
        typedef T vt __attribute__((ext_vector_type(VE)));
#pragma unroll
        for (int j = 0; j < NR; j += VE) {
            const vt t = *(gptr<const vt>)(p + j);
#pragma unroll
            for (int e = 0; e < VE; e++) r[j + e] = t[e];
        }
    } else {
#pragma unroll
        for (int j = 0; j < NR; j++) r[j] = p[min(j, nr - 1)];
    }
}

// One row of Y: p[j] = alpha * a[j] (+ beta * p[j]) for j < nr.
template <typename T, int NR, bool VEC>
__device__ __forceinline__ void st_rhs(gptr<T> p, int nr, const T (&a)[NR], T alpha, T beta, bool rd)
{
    T q[NR];
#pragma unroll
    for (int j = 0; j < NR; j++) q[j] = alpha * a[j];
    if constexpr (VEC) {
        constexpr int VE = NR * (int)sizeof(T) >= 16 ? 16 / (int)sizeof(T) : NR;
        typedef T vt __attribute__((ext_vector_type(VE)));
#pragma unroll
        for (int j = 0; j < NR; j += VE) {
            vt t;
            if (rd) {
                const vt o = *(gptr<const vt>)(p + j);
#pragma unroll
                for (int e = 0; e < VE; e++) t[e] = fmadd(beta, o[e], q[j + e]);
            } else {
#pragma unroll
                for (int e = 0; e < VE; e++) t[e] = q[j + e];
            }
            *(gptr<vt>)(p + j) = t;
        }
    } else {
#pragma unroll
        for (int j = 0; j < NR; j++)
            if (j < nr) p[j] = rd ? fmadd(beta, p[j], q[j]) : q[j];
    }
}

template <typename T, int W_, int U, bool KC, typename S, int NR, RhsLayout LAY>
__device__ __forceinline__ void run_slots_mm(const SlotBin &b, int r, int lane, const T *__restrict__ x, int64_t ldx,
                                             T *__restrict__ y, int64_t ldy, int nr, T alpha, T beta, bool rd,
                                             int *lds_out)
{
    constexpr int V = vec_elems(sizeof(T), W_);
    constexpr int LPR = W_ / V;  // lanes per row (slot-major: lane = slot * LPR + sub)
    const int RPI = b.rpi;
    const int slot = lane / LPR, sub = lane - slot * LPR;
    const bool active = slot < RPI;
    const int R0 = G(b.rrow)[r], R1 = G(b.rrow)[r + 1];
    if (R0 >= R1) return;
    int c = G(b.rchunk)[r];
    const int lslot = active ? slot : 0, lsub = active ? sub : 0;
    const gptr<const S> val = G(static_cast<const S *>(b.val));
    const gptr<const uint32_t> key = G(b.key);
    constexpr bool COL = LAY == kRhsCols, VEC = LAY == kRhsRowsVec;
    // column-major: the columns of X a launch reads, base j of a dead column (j >= nr) being the last live column's
    gptr<const T> xc[COL ? NR : 1];
    if constexpr (COL) {
#pragma unroll
        for (int j = 0; j < NR; j++) xc[j] = G(x) + (int64_t)min(j, nr - 1) * ldx;
    } else {
        xc[0] = G(x);
    }

    // Loads are unconditional (rows past the range re-read its last row and are never folded), as in run_slots.
    typedef __attribute__((address_space(4))) const uint32_t *cptr;  // scalar (constant) loads
    const cptr bases = (cptr)b.base;
    const cptr doffs = (cptr)b.kdoff;
    auto load = [&](int R, uint32_t (&kk)[U], uint32_t (&bs)[U], S (&v)[U][V]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int Rc = min(R + u, R1 - 1);
            const size_t p = (size_t)Rc * RPI + lslot;
            if constexpr (KC) {
                kk[u] = (uint32_t)(int32_t)((gptr<const int16_t>)key)[(size_t)doffs[Rc] + lslot];
                bs[u] = bases[Rc];
            } else {
                kk[u] = __builtin_nontemporal_load(key + p);
                bs[u] = 0;
            }
            ld_stream<S, V>(val + p * W_ + lsub * V, v[u]);
        }
    };
    constexpr uint32_t kPad16 = 0xFFFF8000u;  // INT16_MIN sign-extended
    auto gather = [&](const uint32_t (&kk)[U], const uint32_t (&bs)[U], T (&xv)[U][NR]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t gi = KC ? (bs[u] & kSlotIdx) + (kk[u] == kPad16 ? 0u : kk[u]) : kk[u] & kSlotIdx;
            if constexpr (COL) {
#pragma unroll
                for (int j = 0; j < NR; j++) xv[u][j] = xc[j][gi];
            } else {
                ld_rhs<T, NR, VEC>(xc[0] + (size_t)gi * ldx, nr, xv[u]);
            }
        }
    };
    T acc[NR][V];
#pragma unroll
    for (int j = 0; j < NR; j++)
#pragma unroll
        for (int e = 0; e < V; e++) acc[j][e] = T(0);
    // table-mapped y offsets: the range's entries staged in LDS by the prologue (bins are cut so a range holds
    // <= kSlotOutEntries segments)
    const int c0 = c;
    if (!b.out_affine) {
        const int n = min(kSlotOutEntries, b.nseg - c0 * RPI);
        for (int i = lane; i < n; i += 64) lds_out[i] = G(b.out)[c0 * RPI + i];
    }
    auto flush = [&]() {
        const int seg = c * RPI + slot;
        if (active && seg < b.nseg) {
            const int o = b.out_affine ? b.out_base + seg * b.out_stride : lds_out[(c - c0) * RPI + slot];
            const int lim = b.wst - sub * V;  // padding columns (w > wst) are never written
            if constexpr (COL) {
#pragma unroll
                for (int j = 0; j < NR; j++) {
                    if (j < nr) {
                        gptr<T> yo = G(y) + (int64_t)j * ldy + o + sub * V;
                        T q[V];
#pragma unroll
                        for (int e = 0; e < V; e++) {
                            q[e] = alpha * acc[j][e];
                            if (rd && e < lim) q[e] = fmadd(beta, yo[e], q[e]);
                        }
                        if (V > 1 && lim >= V) {  // the lane's whole vector: one 8- / 16-B store
                            typedef T vt __attribute__((ext_vector_type(V)));
                            vt t;
#pragma unroll
                            for (int e = 0; e < V; e++) t[e] = q[e];
                            *(gptr<vt>)yo = t;
                        } else {
#pragma unroll
                            for (int e = 0; e < V; e++)
                                if (e < lim) yo[e] = q[e];
                        }
                    }
                }
            } else {
#pragma unroll
                for (int e = 0; e < V; e++) {
                    if (e < lim) {
                        T a[NR];
#pragma unroll
                        for (int j = 0; j < NR; j++) a[j] = acc[j][e];
                        st_rhs<T, NR, VEC>(G(y) + (size_t)(o + sub * V + e) * ldy, nr, a, alpha, beta, rd);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NR; j++)
#pragma unroll
            for (int e = 0; e < V; e++) acc[j][e] = T(0);
        c++;
    };
    // rows past the range are folded as no-ops by a select (run_slots: every loaded register is consumed on
    // every path); R1 in a VGPR keeps `live` a per-lane select
    int R1v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(R1v) : "s"(R1));
    auto compute = [&](int R, const uint32_t (&kk)[U], const uint32_t (&bs)[U], const S (&v)[U][V],
                       const T (&xv)[U][NR]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool live = R + u < R1v;
            const bool pad = KC ? kk[u] == kPad16 : (kk[u] & kPad) != 0;
#pragma unroll
            for (int j = 0; j < NR; j++) {
                const T xe = pad ? T(0) : xv[u][j];  // a padding row contributes 0 by a select, never a product
#pragma unroll
                for (int e = 0; e < V; e++) {
                    const T nv = fmadd((T)v[u][e], xe, acc[j][e]);
                    acc[j][e] = live ? nv : acc[j][e];
                }
            }
            const uint32_t lastw = KC ? bs[u] : (uint32_t)__builtin_amdgcn_readfirstlane((int)kk[u]);
            if (R + u < R1 && (lastw & kLast)) flush();
        }
    };

    // two-stage ping-pong as run_slots: the gathers of step i are issued before the stream loads of step i+1
    uint32_t kA[U], kB[U], bA[U], bB[U];
    S vA[U][V], vB[U][V];
    T xv[U][NR];
    load(R0, kA, bA, vA);
    __builtin_amdgcn_s_waitcnt(0);
    for (int R = R0; R < R1; R += 2 * U) {
        gather(kA, bA, xv);
        load(R + U, kB, bB, vB);
        compute(R, kA, bA, vA, xv);
        gather(kB, bB, xv);
        load(R + 2 * U, kA, bA, vA);
        compute(R + U, kB, bB, vB, xv);
    }
}

// The narrow rows of run_slots_narrow (fp32 w = 2: one lane holds two consecutive segments, 128 slots per
// chunk, a row's values one 16-B load per lane and its keys one 4- / 8-B load).
template <int U, bool KC, int NR, RhsLayout LAY>
__device__ __forceinline__ void run_slots_narrow_mm(const SlotBin &b, int r, int lane, const float *__restrict__ x,
                                                    int64_t ldx, float *__restrict__ y, int64_t ldy, int nr,
                                                    float alpha, float beta, bool rd, int *lds_out)
{
    typedef float T;
    constexpr int W_ = 2, SPL = 2, NV = SPL * W_;
    const int RPI = b.rpi;  // = 64 * SPL
    const int R0 = G(b.rrow)[r], R1 = G(b.rrow)[r + 1];
    if (R0 >= R1) return;
    int c = G(b.rchunk)[r];
    const gptr<const T> val = G(static_cast<const T *>(b.val));
    constexpr bool COL = LAY == kRhsCols, VEC = LAY == kRhsRowsVec;
    gptr<const T> xc[COL ? NR : 1];
    if constexpr (COL) {
#pragma unroll
        for (int j = 0; j < NR; j++) xc[j] = G(x) + (int64_t)min(j, nr - 1) * ldx;
    } else {
        xc[0] = G(x);
    }
    typedef __attribute__((address_space(4))) const uint32_t *cptr;
    const cptr bases = (cptr)b.base;
    const cptr doffs = (cptr)b.kdoff;
    typedef T vt __attribute__((ext_vector_type(NV)));
    auto load = [&](int R, uint32_t (&kk)[U][SPL], uint32_t (&bs)[U], T (&v)[U][NV]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int Rc = min(R + u, R1 - 1);
            const size_t p = (size_t)Rc * RPI + (size_t)lane * SPL;
            if constexpr (KC) {
                typedef int16_t hv __attribute__((ext_vector_type(SPL)));
                const hv d = *(gptr<const hv>)((gptr<const int16_t>)b.key + (size_t)doffs[Rc] + (size_t)lane * SPL);
#pragma unroll
                for (int k = 0; k < SPL; k++) kk[u][k] = (uint32_t)(int32_t)d[k];
                bs[u] = bases[Rc];
            } else {
                typedef uint32_t kv __attribute__((ext_vector_type(SPL)));
                const kv d = __builtin_nontemporal_load((gptr<const kv>)(G(b.key) + p));
#pragma unroll
                for (int k = 0; k < SPL; k++) kk[u][k] = d[k];
                bs[u] = 0;
            }
            const vt t = __builtin_nontemporal_load((gptr<const vt>)(val + p * W_));
#pragma unroll
            for (int e = 0; e < NV; e++) v[u][e] = t[e];
        }
    };
    constexpr uint32_t kPad16 = 0xFFFF8000u;
    auto is_pad = [&](uint32_t k) { return KC ? k == kPad16 : (k & kPad) != 0; };
    auto gather = [&](const uint32_t (&kk)[U][SPL], const uint32_t (&bs)[U], T (&xv)[U][SPL][NR]) {
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int k = 0; k < SPL; k++) {
                const uint32_t gi = KC ? (bs[u] & kSlotIdx) + (kk[u][k] == kPad16 ? 0u : kk[u][k]) : kk[u][k] & kSlotIdx;
                if constexpr (COL) {
#pragma unroll
                    for (int j = 0; j < NR; j++) xv[u][k][j] = xc[j][gi];
                } else {
                    ld_rhs<T, NR, VEC>(xc[0] + (size_t)gi * ldx, nr, xv[u][k]);
                }
            }
    };
    T acc[NR][NV];
#pragma unroll
    for (int j = 0; j < NR; j++)
#pragma unroll
        for (int e = 0; e < NV; e++) acc[j][e] = T(0);
    const int c0 = c;
    if (!b.out_affine) {
        const int n = min(kSlotOutEntries, b.nseg - c0 * RPI);
        for (int i = lane; i < n; i += 64) lds_out[i] = G(b.out)[c0 * RPI + i];
    }
    auto flush = [&]() {
        const int seg0 = c * RPI + lane * SPL;
#pragma unroll
        for (int k = 0; k < SPL; k++) {
            const int seg = seg0 + k;
            if (seg < b.nseg) {
                const int o = b.out_affine ? b.out_base + seg * b.out_stride : lds_out[(c - c0) * RPI + lane * SPL + k];
                if constexpr (COL) {
                    const int lim = b.wst;
#pragma unroll
                    for (int j = 0; j < NR; j++) {
                        if (j < nr) {
                            gptr<T> yo = G(y) + (int64_t)j * ldy + o;
                            T q[W_];
#pragma unroll
                            for (int e = 0; e < W_; e++) {
                                q[e] = alpha * acc[j][k * W_ + e];
                                if (rd && e < lim) q[e] = fmadd(beta, yo[e], q[e]);
                            }
                            if (lim >= W_) {  // the segment's whole width: one 8-B store
                                typedef T st __attribute__((ext_vector_type(W_)));
                                st t;
#pragma unroll
                                for (int e = 0; e < W_; e++) t[e] = q[e];
                                *(gptr<st>)yo = t;
                            } else {
#pragma unroll
                                for (int e = 0; e < W_; e++)
                                    if (e < lim) yo[e] = q[e];
                            }
                        }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < W_; e++) {
                        if (e < b.wst) {
                            T a[NR];
#pragma unroll
                            for (int j = 0; j < NR; j++) a[j] = acc[j][k * W_ + e];
                            st_rhs<T, NR, VEC>(G(y) + (size_t)(o + e) * ldy, nr, a, alpha, beta, rd);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NR; j++)
#pragma unroll
            for (int e = 0; e < NV; e++) acc[j][e] = T(0);
        c++;
    };
    int R1v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(R1v) : "s"(R1));
    auto compute = [&](int R, const uint32_t (&kk)[U][SPL], const uint32_t (&bs)[U], const T (&v)[U][NV],
                       const T (&xv)[U][SPL][NR]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool live = R + u < R1v;
#pragma unroll
            for (int k = 0; k < SPL; k++) {
                const bool pad = is_pad(kk[u][k]);
#pragma unroll
                for (int j = 0; j < NR; j++) {
                    const T xe = pad ? T(0) : xv[u][k][j];
#pragma unroll
                    for (int e = 0; e < W_; e++) {
                        const T nv = fmadd(v[u][k * W_ + e], xe, acc[j][k * W_ + e]);
                        acc[j][k * W_ + e] = live ? nv : acc[j][k * W_ + e];
                    }
                }
            }
            const uint32_t lastw = KC ? bs[u] : (uint32_t)__builtin_amdgcn_readfirstlane((int)kk[u][0]);
            if (R + u < R1 && (lastw & kLast)) flush();
        }
    };
    uint32_t kA[U][SPL], kB[U][SPL], bA[U], bB[U];
    T vA[U][NV], vB[U][NV], xv[U][SPL][NR];
    load(R0, kA, bA, vA);
    __builtin_amdgcn_s_waitcnt(0);
    for (int R = R0; R < R1; R += 2 * U) {
        gather(kA, bA, xv);
        load(R + U, kB, bB, vB);
        compute(R, kA, bA, vA, xv);
        gather(kB, bB, xv);
        load(R + 2 * U, kA, bA, vA);
        compute(R + U, kB, bB, vB, xv);
    }
}

// Rows per pipeline step of an instance: the x rows of a step (U * NR elements per lane) are the register
// cost that grows with NR, so U halves as NR doubles; compressed keys (KC) hold a base and a pattern offset
// per row in SGPRs for both pipeline stages and take half again.  No instance uses scratch (DESIGN.md has the
// compiler's resource table).  fp32 rows of 16-B lane vectors and the narrow rows take half, as in spmv_slots.
template <typename T, bool KC>
__host__ __device__ constexpr int slot_mm_step(int NR)
{
    const int u = (sizeof(T) == 8 ? 16 : 32) / NR / (KC ? 2 : 1);
    return u < 2 ? 2 : u;
}

// One wave per range, bins and XCD-aware block order as spmv_slots.  WONLY = 2 / kWonlyNarrow2: every bin of the
// launch has width 2 in the plain / the narrow-row form (the FE width), so only that case is compiled.
template <typename T, bool KC, typename S, int NR, RhsLayout LAY, int WONLY>
__device__ __forceinline__ void slots_mm_wave(const SlotBin *bins, int nbins, int total_ranges, int xcd_chunk, const T *x,
                                              int64_t ldx, T *y, int64_t ldy, int nr, T alpha, T beta, int rd_i)
{
    int blk = blockIdx.x;
    if (xcd_chunk > 0) blk = xcd_block(blk, gridDim.x);
    const int rg = __builtin_amdgcn_readfirstlane((int)(blk * kWavesPerBlock + (threadIdx.x >> 6)));
    if (rg >= total_ranges) return;
    int bi = 0;
    while (bi + 1 < nbins && bins[bi + 1].range0 <= rg) bi++;
    const SlotBin b = bins[bi];
    const int r = rg - b.range0;
    const int lane = threadIdx.x & 63;
    const bool rd = rd_i != 0;
    __shared__ int outs[kWavesPerBlock * kSlotOutEntries];
    int *lds_out = outs + (threadIdx.x >> 6) * kSlotOutEntries;
    constexpr int U = slot_mm_step<T, KC>(NR);
#define VBC_MM_W(W) run_slots_mm<T, W, slot_step<T>(W, U), KC, S, NR, LAY>(b, r, lane, x, ldx, y, ldy, nr, alpha, beta, rd, lds_out)
    if constexpr (WONLY == 2) {
        VBC_MM_W(2);
    } else if constexpr (WONLY == kWonlyNarrow2) {
        run_slots_narrow_mm<U / 2, KC, NR, LAY>(b, r, lane, x, ldx, y, ldy, nr, alpha, beta, rd, lds_out);
    } else {
        if constexpr (sizeof(T) == 4 && sizeof(S) == 4) {
            if (b.spl == 2 && b.wkey == 2) {
                run_slots_narrow_mm<U / 2, KC, NR, LAY>(b, r, lane, x, ldx, y, ldy, nr, alpha, beta, rd, lds_out);
                return;
            }
        }
        switch (b.wkey) {
        case 1: VBC_MM_W(1); break;
        case 2: VBC_MM_W(2); break;
        case 3: VBC_MM_W(3); break;
        case 4: VBC_MM_W(4); break;
        case 5: VBC_MM_W(5); break;
        case 6: VBC_MM_W(6); break;
        case 7: VBC_MM_W(7); break;
        case 8: VBC_MM_W(8); break;
        default: break;
        }
    }
#undef VBC_MM_W
}

// Row-major operands; VEC: kRhsRowsVec.
template <typename T, bool KC, typename S, int NR, bool VEC, int WONLY = -1>
__global__ __launch_bounds__(kBlockThreads) void spmm_slots(const SlotBin *__restrict__ bins, int nbins,
                                                            int total_ranges, int xcd_chunk, const T *__restrict__ x,
                                                            int64_t ldx, T *__restrict__ y, int64_t ldy, int nr,
                                                            T alpha, T beta, int rd_i)
{
    slots_mm_wave<T, KC, S, NR, VEC ? kRhsRowsVec : kRhsRows, WONLY>(bins, nbins, total_ranges, xcd_chunk, x, ldx, y, ldy,
                                                                     nr, alpha, beta, rd_i);
}

// Column-major operands.
template <typename T, bool KC, typename S, int NR, int WONLY = -1>
__global__ __launch_bounds__(kBlockThreads) void spmm_slots_col(const SlotBin *__restrict__ bins, int nbins,
                                                                int total_ranges, int xcd_chunk,
                                                                const T *__restrict__ x, int64_t ldx,
                                                                T *__restrict__ y, int64_t ldy, int nr, T alpha,
                                                                T beta, int rd_i)
{
    slots_mm_wave<T, KC, S, NR, kRhsCols, WONLY>(bins, nbins, total_ranges, xcd_chunk, x, ldx, y, ldy, nr, alpha, beta,
                                                 rd_i);
}

}  // namespace vbc
