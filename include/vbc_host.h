/*
 * vbc_host.h -- host-side layout producers of libvbc (no GPU needed).
 *
 * These build the reference's own data structures (1-based Int64 fields of SparseMatrix1DVBC /
 * SparseMatrixVBC) from a SparseMatrixCSC, so that a host without Julia (the Python mirror, tests,
 * bench) can produce exactly what `SparseMatrix1DVBC{W}(A, Φ)` / `SparseMatrixVBC{U,W}(A, Π, Φ)`
 * produce, and hand them to vbc1d_create / vbc2d_create.  A Julia caller does not need them: it
 * builds the struct with the reference's constructors and passes the fields straight to vbc.h.
 *
 * Partitioners stand in for the external ChainPartitioners.jl 1.1.6 (`pack_stripe`, Manifest.toml:
 * 23-29), which is absent from the container; partition parity is UNPINNED -- all
 * parity is defined per given partition.  Layout parity (given Φ / Π) is exact and is checked
 * against the oracle restatement of constructors_1DVBC.jl / constructors_VBC.jl.
 *
 * Conventions: colptr[n+1], rowval[nnz] are 1-based Int64 (SparseMatrixCSC fields), rows sorted
 * ascending within a column.  Output spl arrays are 1-based, spl[0] = 1, spl[L] = n+1; the caller
 * provides n+1 slots.  Return: vbc_status (vbc.h).
 */
#ifndef VBC_HOST_H
#define VBC_HOST_H

#ifndef VBC_API
#define VBC_API __attribute__((visibility("default")))  /* the library builds with -fvisibility=hidden */
#endif

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* EquiChunker(w): stripes of exactly w columns (last one shorter). */
VBC_API int vbcx_partition_equi(int64_t n, int64_t w, int64_t *spl, int64_t *L);

/* StrictChunker(W): maximal runs of consecutive columns with identical row patterns, width <= W. */
VBC_API int vbcx_partition_strict(int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval,
                          int64_t W, int64_t *spl, int64_t *L);

/* OverlapChunker(ρ, W): greedy; column j joins the open stripe while
 * |S(j) ∩ S(first)| >= ρ · max(|S(j)|, |S(first)|) and width < W (S = row pattern). */
VBC_API int vbcx_partition_overlap(int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval,
                           double rho, int64_t W, int64_t *spl, int64_t *L);

/* DynamicTotalChunker(model, W): optimal (minimum total cost) contiguous partition with width <= W
 * by dynamic programming, for the affine per-stripe cost
 *     cost(stripe) = c_stripe + c_col·w + c_pin·pins + c_row·rows + c_cell·w·rows
 * where rows = distinct rows of the stripe.  model_SparseMatrix1DVBC_memory(Tv, Ti) (costs.jl:10)
 * is (3Ti, 0, 0, Ti, Tv); model_SparseMatrix1DVBC_blocks() (costs.jl:8) is (0, 0, 0, 1, 0). */
VBC_API int vbcx_partition_dynamic(int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval,
                           int64_t W, double c_stripe, double c_col, double c_pin, double c_row,
                           double c_cell, int64_t *spl, int64_t *L);

/* DynamicTotalChunker over a ColumnBlockComponentCostModel (costs.jl:12, the TrSpMV time model):
 *     cost(stripe of width w with R distinct rows) = alpha[w-1] + beta[w-1]·R,   1 <= w <= W,
 * alpha / beta hold W entries (model_SparseMatrix1DVBC_TrSpMV_time fits them, costs.py). */
VBC_API int vbcx_partition_dynamic_table(int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval,
                                         int64_t W, const double *alpha, const double *beta, int64_t *spl,
                                         int64_t *L);

/* DynamicTotalChunker over a BlockComponentCostModel (costs.jl:138-142, the SparseMatrixVBC models):
 * the columns of A are partitioned while its rows are grouped into G block rows (grp[i] = 1-based
 * block row of row i, the other dimension's partition; NULL = every row its own group, G = m):
 *     cost(stripe of width w) = alpha[w-1] + Σ_r colw[r·W + w-1] · Σ_{block rows g it touches} gw[r·G + g]
 * i.e. the stripe's own cost plus, for every u_g × w block it stores, Σ_r β_row[r](u_g)·β_col[r](w)
 * (gw = β_row[r] evaluated at each group's height, colw = β_col[r] at each width; R <= 64 components,
 * the rank of the time model's SVD).  The row partition of pack_plaid's alternation is this call on
 * Aᵀ with the permuted model (permutedims swaps the row and column terms).  Optimal by dynamic
 * programming, width <= W. */
VBC_API int vbcx_partition_block(int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval,
                                 const int64_t *grp, int64_t G, int64_t R, const double *gw, int64_t W,
                                 const double *alpha, const double *colw, int64_t *spl, int64_t *L);

/* SparseMatrix1DVBC{W}(A, Φ) (constructors_1DVBC.jl:9-92): pass 1 fills pos[L+1], ofs[L+1]. */
VBC_API int vbcx_1dvbc_count(int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, int64_t L,
                     const int64_t *spl, int64_t *pos, int64_t *ofs);
/* pass 2 fills idx[pos[L]-1] and val[ofs[L]-1 + pad] (pad trailing zeros, :35-39).
 * dtype: any vbc_dtype (nzval and val have that eltype; values are copied, never converted). */
VBC_API int vbcx_1dvbc_fill(int64_t m, int64_t n, int64_t W, const int64_t *colptr, const int64_t *rowval,
                    const void *nzval, int dtype, int64_t L, const int64_t *spl, const int64_t *pos,
                    const int64_t *ofs, int64_t *idx, void *val, int64_t pad);

/* SparseMatrixVBC{U,W}(A, Π, Φ) (constructors_VBC.jl:15-133). */
VBC_API int vbcx_vbc_count(int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, int64_t K,
                   const int64_t *pspl, int64_t L, const int64_t *spl, int64_t *pos, int64_t *ofs);
VBC_API int vbcx_vbc_fill(int64_t m, int64_t n, int64_t U, int64_t W, const int64_t *colptr,
                  const int64_t *rowval, const void *nzval, int dtype, int64_t K,
                  const int64_t *pspl, int64_t L, const int64_t *spl, const int64_t *pos,
                  const int64_t *ofs, int64_t *idx, void *val, int64_t pad);

/* Row pattern of Aᵀ (CSR of A) for row partitioning: rowptr[m+1], colval[nnz], 1-based. */
VBC_API int vbcx_transpose_pattern(int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval,
                           int64_t *rowptr, int64_t *colval);

/* The value plan of a sharded handle (vbc.h VBC_CREATE_UPDATABLE_SHARDS): which elements of val each of the
 * `ngpus` shards of vbc1d_create_sharded / vbc2d_create_sharded holds -- the function those creates build their
 * shards with.  Matrix fields as vbc1d_create (pspl = NULL; K ignored) or vbc2d_create; compute_size = bytes of
 * the compute eltype (4 / 8: the byte balance of the cuts); split = VBC_SPLIT_STRIPES or VBC_SPLIT_ROWS.
 * Outputs (each may be NULL):
 *   cuts[ngpus+1]       0-based ranges of the split dimension (columns / rows), as vbc_sharded_shard reports;
 *   vbase[ngpus+1]      shard g holds vbase[g+1] - vbase[g] values: the slice [vbase[g], vbase[g+1]) of the packed
 *                       order (shard 0's values, then shard 1's, ...); for the stripe split that is val's own
 *                       order, shard g = val[vbase[g] : vbase[g+1]), and there are no runs;
 *   run_begin[ngpus+1]  row split: shard g's runs are run_begin[g] .. run_begin[g+1]-1;
 *   *nruns              number of runs (always written);
 *   runs[3*nruns]       (src element, dst element, length) per run, 0-based, dst in packed order and ascending;
 *                       kept blocks adjacent in val are one run.  Written only when run_capacity >= *nruns
 *                       (call once with runs = NULL for the count). */
VBC_API int vbcx_sharded_value_plan(int64_t m, int64_t n, int64_t K, const int64_t *pspl, int64_t L,
                                    const int64_t *spl, const int64_t *pos, const int64_t *idx, const int64_t *ofs,
                                    int compute_size, int ngpus, int split, int64_t *cuts, int64_t *vbase,
                                    int64_t *run_begin, int64_t *nruns, int64_t *runs, int64_t run_capacity);

/* ---- the layout planner on the host (for tests and tools; a product caller needs neither) ----
 * A create asks the device a handful of facts, then plans the whole layout on the host (the arena image it
 * uploads).  These two entries separate the steps, so that a layout can be checked on a machine without a GPU
 * under the facts recorded on one.
 *
 * vbcx_facts: compute units and the occupancy (resident workgroups per CU, as the runtime reports them) of every
 * kernel family, first index 0 = Float64, 1 = Float32. */
typedef struct vbcx_facts {
    int32_t cus;
    int32_t occ_ranges[2][2][2][2];  /* merge kernel: [eltype][tile K = 8][pipeline depth = 3][B'x, Bx] */
    int32_t occ_slots[2][2];         /* slotted kernels: [eltype][B'x, Bx] */
    int32_t occ_planar[2];
    int32_t occ_lanes[2];
    int32_t occ_split_multi[2][3];   /* fused split launch: [eltype][P = 2, 4, 8] */
    int32_t occ_panel[2];            /* the two multi-RHS kernels: asked only by VBC_CREATE_MULTI(_FORWARD) creates */
    int32_t occ_tiles[2];
} vbcx_facts;

/* The facts of `device`, every row filled (needs the device). */
VBC_API int vbcx_device_facts(int device, vbcx_facts *out);

/* The arena image a create with these arguments would upload under `facts` (needs no device): the fields of
 * vbc1d_create (pspl = NULL; U, K ignored) or vbc2d_create, checked as those do; dtype = the compute eltype of
 * val; flags = vbc_create_flags without VBC_CREATE_UPDATABLE(_SHARDS) (VBC_CREATE_NARROW_VALUES, alone or with
 * VBC_CREATE_NARROW_PLANAR [| VBC_CREATE_NARROW_PAIRS [| VBC_CREATE_NARROW_STREAMS]]: val holds Float32 values widened
 * to Float64; 0x100 without 0x80, 0x400 without 0x180 and 0x800 without 0x580 are refused; VBC_CREATE_NARROW_SWEPT
 * may join any of them and is refused without 0x80;
 * VBC_CREATE_NARROW_UPDATABLE is accepted together with 0x80 and changes nothing, and is refused without it).  The
 * environment knobs of INTEGRATION.md apply as in a create.  *bytes receives the image size; image = NULL
 * returns only that, else capacity must hold it. */
VBC_API int vbcx_plan_image(int64_t m, int64_t n, int64_t U, int64_t W, int64_t K, const int64_t *pspl, int64_t L,
                            const int64_t *spl, const int64_t *pos, const int64_t *idx, const int64_t *ofs,
                            const void *val, int64_t nval, int dtype, unsigned flags, const vbcx_facts *facts,
                            void *image, size_t capacity, size_t *bytes);

/* One chunk of a value map: `n` 16-byte quads of stored value slots, `vsz` bytes each (0: the compute eltype's
 * size, 4: Float32 slots of a narrow bucket), starting at slot `dst` of the arena image (in units of the chunk's
 * stored size) and at entry `map` of the map. */
typedef struct vbcx_map_chunk {
    uint64_t dst;
    uint64_t map;
    uint32_t n;
    uint32_t vsz;
} vbcx_map_chunk;
#define VBCX_MAP_ZERO 0xFFFFFFFFu  /* a padding slot: rewritten with zero */
#define VBCX_MAP_SKIP 0xFFFFFFFEu  /* no value slot (a region's alignment to 16 bytes): never written */
#define VBCX_MAP_CANON 0x80000000u /* with a source index: the slot holds 0 + v (-0 becomes +0) */

/* The value map an updatable create with these arguments would keep under `facts` (needs no device; the creates
 * run the same host code): the arguments of vbcx_plan_image, flags including VBC_CREATE_NARROW_VALUES [|
 * VBC_CREATE_NARROW_PLANAR] where the handle would be created with VBC_CREATE_NARROW_UPDATABLE (the three
 * UPDATABLE bits themselves are ignored).  One 32-bit entry per stored value slot, in arena order: the 0-based
 * index of the source element of val, VBCX_MAP_CANON set where create stores 0 + v, or VBCX_MAP_ZERO /
 * VBCX_MAP_SKIP.  *nentries and *nchunks are always written; a buffer is written only when it is not NULL and its
 * capacity holds the count (call once with NULL buffers for the counts). */
VBC_API int vbcx_value_map(int64_t m, int64_t n, int64_t U, int64_t W, int64_t K, const int64_t *pspl, int64_t L,
                           const int64_t *spl, const int64_t *pos, const int64_t *idx, const int64_t *ofs,
                           const void *val, int64_t nval, int dtype, unsigned flags, const vbcx_facts *facts,
                           uint32_t *map, int64_t map_capacity, int64_t *nentries, vbcx_map_chunk *chunks,
                           int64_t chunk_capacity, int64_t *nchunks);

#ifdef __cplusplus
}
#endif
#endif /* VBC_HOST_H */
