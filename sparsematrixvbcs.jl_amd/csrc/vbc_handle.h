// The host-side handle, shared by libvbc's translation units: vbc_create.hip (the create entry points),
// vbc_device.hip (the device part of a create and the rest of the C ABI), vbc_launch.hip / vbc_panel_launch.hip
// (the kernel launches).  The layout planner (vbc_plan.h and its units vbc_plan*.hip) does not depend on it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <utility>
#include <vector>

#include "vbc_config.h"
#include "vbc_internal.h"
#include "vbc_kernels.h"
#include "vbc_launch_desc.h"
#include "vbc_panel.h"
#include "vbc_tiles.h"

namespace vbc {

#define VBC_HIP(call)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            set_error("%s failed: %s", #call, hipGetErrorString(e_));                             \
            return VBC_HIP_ERROR;                                                                 \
        }                                                                                         \
    } while (0)

// Restores the caller's current device on scope exit.
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

inline bool is_float(int dt) { return dt == VBC_F64 || dt == VBC_F32; }
inline bool known_dtype(int dt) { return dt >= VBC_F64 && dt <= VBC_BOOL; }

// Integer-eltype layout (vbc_generic.hip): the reference layout itself, 0-based, on the device.
struct IntLayout {
    int64_t L = 0, nrows = 0;
    const int32_t *col0 = nullptr, *w = nullptr, *rows = nullptr;  // per stripe / per stored row
    const int32_t *col2stripe = nullptr;  // per column j: its stripe
    const int32_t *row2stripe = nullptr;  // per stored row: its stripe
    const int64_t *rbeg = nullptr;        // L+1 prefix into rows
    const int64_t *voff = nullptr;        // per stripe: first value
    const int64_t *val = nullptr;         // values as Int64
};

// VBC_CREATE_UPDATABLE (vbc_update.hip): the value map of a handle.  `map` holds one 32-bit entry per stored
// value slot, in arena order: the index of the source element of the caller's val, kUpdCanon set where the
// create path stores 0 + v (transpose_stripes), kUpdZero for a padding slot (rewritten with zero) or kUpdSkip
// for a word that is no value slot (alignment of a region to 16 bytes; never written).  The entries are cut
// into chunks of at most kUpdChunkQuads 16-byte quads: `dst` and `map` are element offsets (multiples of a
// quad) into the arena and the map, 64 bits wide, so only the source index is limited to 32 bits.
// VBC_CREATE_NARROW_UPDATABLE: a chunk inside a value region stored as Float32 on a Float64 handle has vsz = 4 --
// its quads are four floats with four entries and `dst` counts floats; every other chunk has vsz = 0 (the
// compute eltype).  A handle may mix both (vbc_host.h vbcx_map_chunk is this struct).
struct UpdChunk {
    uint64_t dst;
    uint64_t map;
    uint32_t n;  // quads
    uint32_t vsz;
};
constexpr uint32_t kUpdZero = 0xFFFFFFFFu, kUpdSkip = 0xFFFFFFFEu, kUpdCanon = 0x80000000u;
constexpr int64_t kUpdMaxSource = 0x7FFFFFFE;  // largest nval an updatable handle takes (entries keep bit 31 free)
constexpr int kUpdChunkQuads = 1024;
struct ValueMap {
    void *d_buf = nullptr;  // map entries, then the chunk table
    size_t bytes = 0;
    const uint32_t *d_map = nullptr;
    const UpdChunk *d_chunks = nullptr;
    int64_t nchunks = 0, entries = 0;
    bool mixed = false;  // VBC_CREATE_NARROW_UPDATABLE: chunks say their stored size, Float32 sources only
};

}  // namespace vbc

struct vbc_handle {
    explicit vbc_handle(const vbc::LayoutConfig &c) : cfg(c) {}
    const vbc::LayoutConfig cfg;  // knobs and device-derived targets of the create (vbc_config.h)
    int64_t m = 0, n = 0, L = 0, K = 0, nblocks = 0, nrows = 0, nval = 0, nnz = 0;
    int dtype = 0, esz = 8, device = 0;
    void *d_arena = nullptr;
    size_t arena_bytes = 0;
    size_t arena_used = 0;        // bytes of the host image the arena was uploaded from
    bool updatable = false;       // VBC_CREATE_UPDATABLE: `umap` is built, vbc_update_values is allowed
    vbc::ValueMap umap;
    bool has_t = false, has_f = false, has_m = false;
    vbc::PanelLaunch lm;          // multi-RHS transposed product on matrix cores (VBC_CREATE_MULTI)
    int64_t bytes_m = 0;          // matrix bytes one panel product streams
    vbc::PanelLaunch lmf;         // multi-RHS forward product on matrix cores (VBC_CREATE_MULTI_FORWARD): the
                                  // panel layout of Bᵀ (output row groups as stripes, tile columns as rows)
    bool has_mf = false;
    int64_t bytes_mf = 0;         // matrix bytes one forward panel product streams
    int32_t mf_group = 0;         // forward panel: widest output row group
    int64_t panel_val_bytes = 0;  // largest bin val array of the panel layout
    vbc::IntLayout li;            // integer eltypes (dtype VBC_I64): exact wrapping products
    vbc::Launch lt;               // transposed product: all buckets in one launch
    vbc::Launch lft;              // forward product as the transposed product of C = Bᵀ (small mixed widths)
    bool has_ft = false;
    std::vector<vbc::Launch> lf;  // forward product: one launch per width bucket
    bool f_scale = false;         // forward with several buckets: scale y by beta first
    int64_t bytes_t = 0, bytes_f = 0;
    void *d_carry_mm = nullptr;   // multi-RHS carry slots (allocated on first use)
    size_t carry_mm_bytes = 0;
    int cus = 256;                // compute units of the device (cfg.cus; read at product time)
    int panel_nobuf = 0;          // cfg.panel_nobuf, read by the panel and tile launches

    // Mutable per-handle state, guarded by `mu` (the layout itself is immutable after create):
    //  * host-pointer staging buffers, grown on demand and reused across calls (VBC_MEM_HOST);
    //  * the product order of handles whose layout has shared scratch (the merge layout's carry
    //    slots and the fused multi-RHS carries): a product enqueued on a different stream than the
    //    previous one first waits for that one's completion event, so concurrent products on
    //    distinct streams stay correct.  Slotted / swept / panel layouts hold no scratch and skip it.
    std::mutex mu;
    std::mutex fork_mu;               // the fork / join event sequence of a forked B'x launch (Launch::fork_*)
    void *d_stage[4] = {nullptr, nullptr, nullptr, nullptr};  // x / X, y / Y staging; 2, 3: column temporaries
    size_t stage_bytes[4] = {0, 0, 0, 0};
    bool has_scratch = false;         // set at create: some launch of this handle uses carry slots
    hipEvent_t order_ev = nullptr;    // recorded after each product with scratch
    hipStream_t order_stream = nullptr;
    bool order_valid = false;
};


namespace vbc {

// vbc_device.hip: the device part of a create.  gather_facts: what a create asks the current device; instantiate:
// a handle around a plan's uploaded arena (vbc_plan.h); release: the handle and everything it holds on its device.
struct Plan;
int gather_facts(int device, unsigned eltypes, bool multi, DeviceFacts &f);
int instantiate(Plan &P, const LayoutConfig &cfg, int device, vbc_handle **out);
void release(vbc_handle *h);
// vbc_launch.hip
int launch_groups(const Launch &L);  // independent launch groups of a B'x launch (vbc_launch.hip)
int mul_dispatch(const vbc_handle *h, int trans, const void *x, void *y, double alpha, double beta,
                 hipStream_t stream);
// Row-major B'X with nrhs >= kMmSlotsMinRhs columns runs fused over the handle's B'x layout (mulmat_rowmajor): merge
// bins of compile-time widths, and slotted bins through spmm_slots unless VBC_MM_SLOTS=0.  The one predicate of the
// dispatch (vbc_mul_mat) and of vbc_info.planar_mask bit 22 (*slotted: the layout has a slotted bucket).
bool mulmat_fuses(const vbc_handle *h, bool *slotted);
constexpr int64_t kMmSlotsMinRhs = 2;  // smallest nrhs the slotted part runs fused at (profiles/mm_slots_time.json)
// Column-major operands run fused when the launch of the product -- the B'x launch, or the one launch of a forward
// product on B's own layout (no forward on C = B', one width bucket) -- has one of three forms (mulmat_col_form), on a
// float handle with no merge bucket (spmm_ranges is row-major only), no swept bucket and no fused small-matrix split:
//   kColSlots  B'X, slotted buckets alone, of mulmat_fuses's forms (spmm_slots_col), unless VBC_MM_SLOTS_COL=0;
//   kColPlanar B'X, planar buckets of kind 0 with one wave per range and chunk rows (no lane streams), widths 3..8,
//              plain or lane pairs (spmm_planar_col / spmm_pair_col), slotted buckets of kColSlots's forms beside them
//              or none; VBC_MM_PLANAR_COL=1 (opt-in);
//   kColFwd    B X, planar buckets alone, with one wave per range and chunk rows, of kind 1 with w in {2, 3, 4} and
//              runs of 2 or 3 (spmm_planar_fwd_col) or the fp64 forward lane pairs (spmm_pair_col<DOT>);
//              VBC_MM_FWD_COL=1 (opt-in).
// VBC_MM_SLOTS=0 turns all three off, VBC_MM_SLOTS_COL=0 too (vbc_config.cpp).  The one classification of the dispatch
// (from the form's smallest nrhs on) and of vbc_info.planar_mask bits 23 / 24 (trans) / 25 (forward).
enum ColForm { kColNone, kColSlots, kColPlanar, kColFwd };
ColForm mulmat_col_form(const vbc_handle *h, int trans);
constexpr int64_t kMmSlotsColMinRhs = 2;  // smallest nrhs the column-major form runs fused at (profiles/mm_slots_col_time.json)
// columns per launch, 4 or 8: 8 columns as two NR = 4 launches sum to 1805.9 us over the three forms on FE-2D, as one
// NR = 8 launch to 1833.6 us (profiles/mm_slots_col_time_cap8.json, measured on a build with 8 here)
constexpr int64_t kMmSlotsColChunk = 4;
// smallest nrhs the planar column-major form runs fused at: it beats nrhs x vbc_mul by more than the spread from
// nrhs = 2 on in fp64, fp32 and narrow on the ldoor stand-in (profiles/mm_planar_col_time.json)
constexpr int64_t kMmPlanarColMinRhs = 2;
// columns per launch, 2 or 4: 8 columns as two NR = 4 launches sum to 723.5 us over the three forms, as four NR = 2
// launches to 833.5 us (the same record, `fused` against `fused_by2`)
constexpr int64_t kMmPlanarColChunk = 4;
// smallest nrhs the forward column-major form runs fused at: it beats nrhs x vbc_mul by more than the spread from
// nrhs = 2 on in every form of both workloads -- FE-2D in fp64, fp32 and narrow, the ldoor stand-in in fp64 and narrow
// (profiles/mm_fwd_col_time.json)
constexpr int64_t kMmFwdColMinRhs = 2;
// columns per launch, 2 or 4: 8 columns as two NR = 4 launches sum to less over the five forms than as four NR = 2
// launches (the same record, `fused` against `fused_by2`: nrhs8_sum_over_forms_us; FE-2D narrow alone is 2 % faster by 2)
constexpr int64_t kMmFwdColChunk = 4;
// The table of the forms, indexed by ColForm: smallest fused nrhs, columns per launch, the kernels (for messages).
struct ColFormRow {
    int64_t min_rhs, chunk;
    const char *kernel;
};
constexpr ColFormRow kColForms[] = {{0, 0, ""},
                                    {kMmSlotsColMinRhs, kMmSlotsColChunk, "spmm_slots_col"},
                                    {kMmPlanarColMinRhs, kMmPlanarColChunk, "spmm_planar_col"},
                                    {kMmFwdColMinRhs, kMmFwdColChunk, "spmm_planar_fwd_col"}};
// The fused column-major product of a handle with a form (trans: B'X, else B X), on the caller's stream alone.
int mulmat_colmajor(const vbc_handle *h, int trans, int64_t nrhs, const char *X, int64_t ldx, char *Y, int64_t ldy,
                    double alpha, double beta, hipStream_t s);
int mulmat_rowmajor(vbc_handle *h, int64_t nrhs, const char *X, int64_t ldx, char *Y, int64_t ldy, double alpha,
                    double beta, hipStream_t s);
// A cached buffer of the handle (`what`) has to grow for a product on `s`.  hipFree / hipMalloc are not stream
// operations, so a product on a capturing stream is refused before either is called (the capture stays valid);
// asked only when a buffer must grow, so a handle whose paths have each run once pays nothing.
inline int may_grow(hipStream_t s, const char *what)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) return fail(VBC_HIP_ERROR, "hipStreamIsCapturing failed");
    if (cs == hipStreamCaptureStatusNone) return VBC_OK;
    set_error("%s must be allocated and the stream is capturing: run the product once outside the capture", what);
    return VBC_INVALID_ARG;
}
void occupancy_ranges(int esz, int K, int P, int occ[2]);
// vbc_generic.hip
int mul_int(const vbc_handle *h, int trans, const void *x, void *y, double alpha, double beta, hipStream_t s);
int convert_gather(const void *src, int src_dtype, int64_t inc, void *dst, int dst_dtype, int64_t n, hipStream_t s);
int convert_scatter(const void *src, int src_dtype, void *dst, int dst_dtype, int64_t inc, int64_t n, hipStream_t s);
// vbc_update.hip
int value_map_host(int esz, int64_t nval, const std::vector<char> &tagged, const std::vector<char> &zeroed,
                   const ByteRanges &canon, const ByteRanges &narrow, std::vector<uint32_t> &map,
                   std::vector<UpdChunk> &chunks);
int upload_value_map(vbc_handle *h, const std::vector<uint32_t> &map, const std::vector<UpdChunk> &chunks);
int update_launch(const vbc_handle *h, const void *d_val, int val_dtype, hipStream_t s);
// vbc_panel_launch.hip
int mulmat_panel_any(const vbc_handle *h, int trans, int64_t nrhs, const char *X, int64_t sxr, int64_t sxc, char *Y,
                     int64_t syr, int64_t syc, double alpha, double beta, hipStream_t s);
int occupancy_panel(int esz);
// vbc_tiles.hip
int mulmat_tiles_any(const vbc_handle *h, int trans, int64_t nrhs, const char *X, int64_t sxr, int64_t sxc, char *Y,
                     int64_t syr, int64_t syc, double alpha, double beta, hipStream_t s);
int occupancy_tiles(int esz);

}  // namespace vbc
