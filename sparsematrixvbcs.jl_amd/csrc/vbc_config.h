// Create-time configuration of a handle: what the device reports (DeviceFacts) and every layout / tuning
// knob with the targets derived from them (LayoutConfig).  make_config is the one place that reads the
// environment; the layout planner (vbc_plan.hip plan_layout) takes the result and reads neither the environment nor the device.
#pragma once
#include <cstdint>

#include "vbc_host.h"
#include "vbc_kernels.h"
#include "vbc_tiles.h"

namespace vbc {

// Raw answers of the device (vbc_host.h vbcx_facts: compute units and the occupancy of every kernel family, per
// eltype).  A create fills the rows of its own eltype (vbc_device.hip gather_facts), the panel / tile rows only
// under VBC_CREATE_MULTI / VBC_CREATE_MULTI_FORWARD; rows nobody asked for stay 0.
using DeviceFacts = vbcx_facts;

struct LayoutConfig {
    int dtype = 0, esz = 8;
    bool narrow_values = false;   // VBC_CREATE_NARROW_VALUES (fp64 handle of Float32 values): slotted bins store floats
    bool narrow_planar = false;   // VBC_CREATE_NARROW_PLANAR (only with narrow_values): so do the chunk-planar bins of
                                  // spmv_planar / spmv_planar_fwd (not pair, lanes or split)
    bool narrow_pairs = false;    // VBC_CREATE_NARROW_PAIRS (only with narrow_planar): so do the lane-pair bins of
                                  // spmv_planar_pair / spmv_pair_lanes (288 floats per run-row)
    bool narrow_streams = false;  // VBC_CREATE_NARROW_STREAMS (only with narrow_pairs): so do the plain lane-stream bins
                                  // of spmv_planar_lanes, B'x and forward (rows of 64 * w floats)
    bool narrow_swept = false;    // VBC_CREATE_NARROW_SWEPT (only with narrow_values, whatever the bits between): so do
                                  // the row-swept bins of spmv_sweep, B'x and forward (rows of w floats per lane slot)
    int target_ranges_m = 4096;
    int panel_valu = 0;           // ablation bits of the panel kernel (VBC_PANEL_VALU / VBC_PANEL_DIAG, the VBC_ABLATION
                                  // build only; 0 in the product library)
    int panel_nobuf = 0;          // VBC_PANEL_NOBUF=1: 64-bit addressing variant (tests / A/B)
    int panel_tiles = -1;         // VBC_PANEL_TILES: small-tile buckets tile-granular (vbc_tiles.h): -1 auto, 0 never,
                                  // 1 whenever representable (any fill)
    int occ_tiles = 24;           // resident waves per CU of the tile kernel (the layout's range count)
    int tile_nbt = vbc::kTileBatch;  // VBC_TILE_NBT: tiles per stream per pipeline stage of the tile kernel (4 / 8)
    int tile_depth = 2;  // VBC_TILE_DEPTH (VBC_ABLATION build): register sets of the tile kernel's pipeline (2 / 3)
    int tile_cluster = 1;             // VBC_TILE_CLUSTER=0: tile ranges launched in natural stripe order (no X-locality balls);
                                      // 2: balls at any range count (tests)
    int tile_spr = vbc::kTileStripes;  // VBC_TILE_SPR: stripes per range (wave) of the tile layout
    int fwd_t = 1;                // VBC_FWD_T: 0 never build the forward product on C = Bᵀ, 2 always
    int target_ranges_k[2] = {4096, 4096};  // resident waves of the B'x / Bx kernels (one range each)
    int tile_k = vbc::kTileKDefault;  // entries per slot per tile
    int lanes_rdiv = 2;               // VBC_LANES_RDIV: lane-stream tiles sized for target_ranges_l / this many ranges
    int pipe = vbc::kPipeDefault;     // software-pipeline depth (2 or 3 tiles)
    int diag = 0;                     // ablation variant (VBC_DIAG; tools/ab.py only)
    int target_ranges_s[2] = {4096, 4096};  // resident waves of the slotted kernels
    int slots_mode = -1;              // VBC_SLOTS: -1 auto, 0 never, 1 always (when representable)
    double slots_pad = 1.10;          // auto: largest padded/real row ratio of a slotted bucket
    int slot_narrow = 1;              // VBC_SLOT_NARROW=0: one segment per lane slot for narrow B'x rows too
    int slots_sort = 1;               // VBC_SLOTS_SORT: 0 natural order only, 1 sort when needed, 2 always sort
    int xcd = 1;                      // VBC_XCD=0: identity block order in the slotted kernel (XCD-contiguous ranges:
                                      // FE 170.3 -> 169.2 us, its 1/8 stripe shard 28.1 -> 26.0 us)
    int64_t range_bytes = 192 << 10;  // VBC_RANGE_KB: a slotted bucket with fewer layout bytes per range at full
                                      // occupancy runs half the waves per SIMD (longer ranges)
    int xcd_p = 1;                    // VBC_XCD_P=0: identity workgroup order in the planar kernels (XCD-contiguous:
                                      // ldoor stand-in fp64 76.8 -> 70.2 us, fp32 44.6 -> 39.8, TrSpMV! 44.6 -> 39.3)
    int occ_s[2] = {4, 4};            // workgroups per CU of the slotted kernels (occupancy)
    int slot_u = 0;                   // rows per step of the slotted kernel (VBC_SLOT_U)
    bool slot_dedup = true;           // VBC_SLOT_DEDUP=0: one stored delta pattern per compressed row
    bool mm_slots = true;             // VBC_MM_SLOTS=0: row-major B'X of a slotted layout runs per column (no spmm_slots)
    bool mm_slots_col = true;         // VBC_MM_SLOTS_COL=0: column-major B'X of a slotted layout runs per column (no
                                      // spmm_slots_col); VBC_MM_SLOTS=0 turns this off too
    bool mm_planar_col = false;       // VBC_MM_PLANAR_COL=1: column-major B'X of a planar layout runs fused
                                      // (spmm_planar_col / spmm_pair_col; planar_mask bit 24).  Opt-in, although it wins
                                      // at every nrhs measured: tests/test_gpu_planar.py asserts the
                                      // exact planar_mask of planar handles created under the default knobs.
                                      // VBC_MM_SLOTS=0 and VBC_MM_SLOTS_COL=0 turn it off too
    bool mm_fwd_col = false;          // VBC_MM_FWD_COL=1: column-major B X of a forward layout of row runs or lane pairs
                                      // runs fused (spmm_planar_fwd_col / spmm_pair_col<DOT>; planar_mask bit 25).
                                      // Opt-in whatever the measurement says, for the reason above:
                                      // older tests assert the exact planar_mask of handles created under the default
                                      // knobs.  VBC_MM_SLOTS=0 and VBC_MM_SLOTS_COL=0 turn it off too
    int slot_keys16 = 1;              // VBC_SLOT_KEYS16: 0 keep 32-bit keys, 1 auto, 2 compress whenever possible
    int fork = 1;                     // VBC_FORK=0: B'x launch groups queue on the caller's stream (Launch::fork_*)
    int slot_stage = -1;              // VBC_SLOT_STAGE = 0 / 4 / 8: chunks staged in LDS per y write (-1 auto)
    int slot_planar = -1;             // VBC_SLOT_PLANAR: -1 auto (B'x, w = 3..8 wider than a lane vector), 0 never, 1 w >= 3
    int slot_runs = 1;                // VBC_SLOT_RUNS=0: no row-run gathers in planar buckets
    int planar_pair = 1;              // VBC_PLANAR_PAIR: 0 never, 1 auto (>= 8 runs per stripe), 2 always (fp64 w = 3 runs)
    int planar_mask = 1;              // VBC_PLANAR_MASK: planar B'x buckets whose natural order pads > slots_pad: 1 masked
                                      // chunk-local length order (SlotBin::mask), 0 length-sorted windows of 32 chunks
    int planar_mask_pair = 1;         // VBC_PLANAR_MASK_PAIR=0: the lane-pair kernel folds its padding rows (no nlive)
    int mask_window = 2;              // VBC_MASK_WINDOW: chunks per length-sort window of the masked order (a prefix
                                      // of live lanes holds in every chunk of a window sorted by decreasing length;
                                      // fe3d fp64 1 / 2 / 4 / 8: 284 / 276 / 284 / 287 us, fp32 145 / 145 / 152 / 159,
                                      // ldoor fp32 37.2 / 37.1 / 36.5 / 36.3)
    int planar_split = -1;            // VBC_PLANAR_SPLIT: -1 auto (few chunks), 0 never, 2 / 4 / 8 waves per chunk
    int target_ranges_p = 4096;       // resident waves of the planar kernel
    int target_ranges_l = 4096;       // resident waves of the lane-stream planar kernel
    int slot_wonly = 1;               // VBC_SLOT_WONLY=0: the all-width slotted kernel even for one-width launches
    int split_kc = 0;                 // VBC_SPLIT_KC=1: compressed keys for split planar bins too
    int small_fuse = 1;               // VBC_SMALL_FUSE: 0 = never fuse the buckets of a small matrix
    int side_fuse = -1;               // VBC_SIDE_FUSE: the dominant bucket outside the fused split (-1 auto, 0 never,
                                      // 1 whenever one width holds >= 80 % of the chunks)
    int colsplit = 1;                 // VBC_COLSPLIT=0: no column pieces (side stripes of a multiple of the
                                      // dominant width run as that many dominant-width stripes)
    double fork_side_bytes = 1 << 20; // VBC_FORK_SIDE_KB: beside a group with >= 90 % of the bytes, the others fork only
                                      // while they hold at most this many bytes
    int fuse_pmax = 8;                // VBC_FUSE_PMAX: most waves per chunk of the fused split launch (2 / 4 / 8; P = 16,
                                      // 1024-thread workgroups, measured 1.4-1.9x slower: profiles/r04_ab20_*.log)
    int colsplit_w = 0;               // VBC_COLSPLIT_W=c: every stripe wider than c as c-wide pieces (A/B)
    int64_t split_nt_bytes = 0;       // VBC_SPLIT_NT_MB: value bytes above which split bins stream nt (0: never)
    int small_rows = 8;               // VBC_SMALL_ROWS: fewest chunk rows per wave (fp64) of the fused small split
    int cus = 256;                    // compute units of the device
    int occ_multi[4] = {0, 0, 0, 0};  // resident waves per CU of the fused split launch, P = 2 / 4 / 8 (index log2 P)
    double ksplit = 1.0;              // VBC_KSPLIT: fused split stripes above this x the mean chunk work are cut
                                      // into 2 / 4 lane parts (SlotBin::ks; 0: never)
    int split_pipe = -1;              // VBC_SPLIT_PIPE: split bins' pipelined slice loop (-1 auto, 0 off, 1 on)
    double split_deep = 2.0;          // VBC_SPLIT_DEEP: auto slice loop batched above this many steps per wave
    int split_rows = 12;              // VBC_SPLIT_ROWS: fewest chunk rows per wave of an automatic split
    int fwd_min_rows = 16;            // VBC_FWD_MIN_ROWS: fewest chunk rows per range of the forward run layout
    int planar_wps = 2;               // VBC_PLANAR_WPS: most resident waves per SIMD of a plain planar bin (0: occupancy)
    int planar_wps_pair = 1;          // VBC_PLANAR_WPS_PAIR: the same for the fp64 lane-pair layout
    int lanes_pair = 0;               // VBC_LANES_PAIR=1: a lane pair per stream in the lane-stream layout (fp64 w = 3,
                                      // runs of 3; one 16-B x gather per lane per run).  FE-3D measured 217 -> 223 us
                                      // with pairs (profiles/r03_ab_pairlanes_fe3d.log), so off by default
    int lanes_deep = 0;               // VBC_LANES_DEEP=1: the lanes kernel's deeper pipeline (gathers a step ahead)
    int planar_lanes = -1;            // VBC_PLANAR_LANES: -1 auto, 0 never, 1 always (planar B'x buckets with
                                      // natural contiguous outputs): per-lane compacted streams (run_planar_lanes)
    int occ_p = 4;                    // workgroups per CU of the planar kernel
    int sweep_mode = -1;              // VBC_SWEEP: -1 auto (no x locality), 0 never, 1 always (w <= 8)
    int sweep_tile = vbc::kSweepTileBytes;  // VBC_SWEEP_TILE=16: 16 KB of LDS accumulators per wave
    int sweep_pack = 1;               // VBC_SWEEP_PACK=0/1: swept keys as gather index + 16-bit segment (6 B per
                                      // entry, two loads) or one packed 32-bit key per entry (default: fp64)
    // knobs the builders used to read themselves
    bool pad_set = false;             // VBC_PAD="w:wp,...": padded widths of the merge layout (A/B); pad_w[w] = wp,
    uint8_t pad_w[65] = {};           // 0: w itself
    int64_t tile_ranges = 0;          // VBC_TILE_RANGES: ranges of a tile bucket (0: the layout's own count)
    bool no_affine = false;           // VBC_NO_AFFINE ablation: y offsets from the table even when affine
    int sweep_diag = 0;               // VBC_SWEEP_DIAG ablation (tools/ab.py only)
    int tile_diag = 0;                // VBC_TILE_DIAG ablation (tools/ab.py only)
    bool verbose = false;             // VBC_VERBOSE: the builders print their choices to stderr
};

// The whole environment block of a create.  `flags`: vbc_create_flags (VBC_CREATE_SERIAL overrides two knobs, the
// MULTI flags enable the panel / tile knobs).  `narrow`: the narrow-storage bits the create accepted
// (VBC_CREATE_NARROW_VALUES, VBC_CREATE_NARROW_PLANAR, VBC_CREATE_NARROW_PAIRS, VBC_CREATE_NARROW_STREAMS,
// VBC_CREATE_NARROW_SWEPT; 0: none) -- they are not part of `flags`.
LayoutConfig make_config(int dtype, unsigned flags, unsigned narrow, const DeviceFacts &facts);

}  // namespace vbc
