// make_config: every environment knob of a create and the targets derived from the device's facts.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "vbc_config.h"
#include "vbc_internal.h"

namespace vbc {

LayoutConfig make_config(int dtype, unsigned flags, unsigned narrow, const DeviceFacts &f)
{
    LayoutConfig c;
    c.dtype = dtype;
    c.esz = elem_size(dtype);
    c.narrow_values = (narrow & VBC_CREATE_NARROW_VALUES) && dtype == VBC_F64;
    c.narrow_planar = c.narrow_values && (narrow & VBC_CREATE_NARROW_PLANAR);
    c.narrow_pairs = c.narrow_planar && (narrow & VBC_CREATE_NARROW_PAIRS);
    c.narrow_streams = c.narrow_pairs && (narrow & VBC_CREATE_NARROW_STREAMS);
    c.narrow_swept = c.narrow_values && (narrow & VBC_CREATE_NARROW_SWEPT);
    if (dtype == VBC_I64) return c;  // the integer layout has no knobs
    const int e32 = c.esz == 4;      // row of the facts
    c.tile_k = dtype == VBC_F64 ? 4 : 8;  // measured best (tools/ab.py, FE workload)
    if (const char *e = tuning_knob("VBC_TILE_K")) {
        const int k = atoi(e);
        c.tile_k = (k == 4 || k == 8) ? k : c.tile_k;
    }
    if (const char *e = tuning_knob("VBC_PIPE")) c.pipe = atoi(e) == 3 ? 3 : 2;
    if (const char *e = ablation_knob("VBC_DIAG")) c.diag = atoi(e);
    // one range per resident wave: occupancy of the kernel variant this handle will launch
    const int32_t *occ = f.occ_ranges[e32][c.tile_k == 8][c.pipe == 3];
    for (int kd = 0; kd < 2; kd++)
        c.target_ranges_k[kd] = f.cus * std::max(1, std::min(occ[kd], 8)) * kWavesPerBlock;
    if (const char *e = tuning_knob("VBC_TARGET_RANGES")) c.target_ranges_k[0] = c.target_ranges_k[1] = std::max(1, atoi(e));
    for (int kd = 0; kd < 2; kd++) {
        c.occ_s[kd] = std::max(1, std::min(f.occ_slots[e32][kd], 8));
        c.target_ranges_s[kd] = f.cus * c.occ_s[kd] * kWavesPerBlock;
    }
    if (const char *e = tuning_knob("VBC_TARGET_RANGES_S")) {  // an explicit range count is taken as is
        c.target_ranges_s[0] = c.target_ranges_s[1] = std::max(1, atoi(e));
        c.occ_s[0] = c.occ_s[1] = 1;
    }
    if (const char *e = layout_knob("VBC_RANGE_KB")) c.range_bytes = (int64_t)std::max(0, atoi(e)) << 10;
    if (const char *e = layout_knob("VBC_SLOTS")) c.slots_mode = atoi(e) == 0 ? 0 : atoi(e) == 1 ? 1 : -1;
    if (const char *e = layout_knob("VBC_SLOTS_PAD")) c.slots_pad = atof(e);
    if (const char *e = layout_knob("VBC_SLOTS_SORT")) c.slots_sort = atoi(e);
    if (const char *e = tuning_knob("VBC_SLOT_NARROW")) c.slot_narrow = atoi(e) != 0;
    if (const char *e = layout_knob("VBC_XCD")) c.xcd = atoi(e) != 0;
    if (const char *e = layout_knob("VBC_XCD_P")) c.xcd_p = atoi(e) != 0;
    if (const char *e = layout_knob("VBC_SLOT_KEYS16")) c.slot_keys16 = atoi(e);  // 0 off, 1 auto, 2 always
    if (const char *e = layout_knob("VBC_SLOT_DEDUP")) c.slot_dedup = atoi(e) != 0;
    if (const char *e = layout_knob("VBC_MM_SLOTS")) c.mm_slots = atoi(e) != 0;
    if (const char *e = layout_knob("VBC_MM_SLOTS_COL")) c.mm_slots_col = atoi(e) != 0;
    if (!c.mm_slots) c.mm_slots_col = false;
    if (const char *e = layout_knob("VBC_MM_PLANAR_COL")) c.mm_planar_col = atoi(e) != 0;
    if (!c.mm_slots_col) c.mm_planar_col = false;
    if (const char *e = layout_knob("VBC_MM_FWD_COL")) c.mm_fwd_col = atoi(e) != 0;
    if (!c.mm_slots_col) c.mm_fwd_col = false;
    if (const char *e = layout_knob("VBC_SWEEP")) c.sweep_mode = atoi(e) == 0 ? 0 : atoi(e) == 1 ? 1 : -1;
    c.sweep_tile = (c.esz == 8 ? 4 : 2) * kSweepTileBytes;  // measured on NS: fp64 32 KB 473 us (16 KB 508), fp32 16 KB 313 us (32 KB 353)
    // packed swept keys: NS fp64 464.5 -> 456.2 us, mixed widths 553 -> 539 us; fp32 311 -> 316 us, so
    // fp64 only (profiles/r03_sweeppack_*.log)
    c.sweep_pack = c.esz == 8;
    if (const char *e = layout_knob("VBC_FORK")) c.fork = atoi(e) != 0;
    if (const char *e = tuning_knob("VBC_FORK_SIDE_KB")) c.fork_side_bytes = atof(e) * 1024.0;
    if (const char *e = layout_knob("VBC_SWEEP_PACK")) c.sweep_pack = atoi(e) != 0;
    if (const char *e = layout_knob("VBC_SWEEP_TILE")) c.sweep_tile = atoi(e) >= 32 ? 4 * kSweepTileBytes : atoi(e) >= 16 ? 2 * kSweepTileBytes : kSweepTileBytes;
    if (const char *e = layout_knob("VBC_SLOT_STAGE")) c.slot_stage = (atoi(e) == 4 || atoi(e) == 8) ? atoi(e) : 0;
    if (const char *e = layout_knob("VBC_SLOT_PLANAR")) c.slot_planar = atoi(e) == 0 ? 0 : atoi(e) == 1 ? 1 : -1;
    if (const char *e = layout_knob("VBC_SLOT_RUNS")) c.slot_runs = atoi(e) != 0;
    if (const char *e = layout_knob("VBC_PLANAR_PAIR")) c.planar_pair = atoi(e) == 0 ? 0 : atoi(e) == 2 ? 2 : 1;  // 2: always
    if (const char *e = layout_knob("VBC_PLANAR_MASK")) c.planar_mask = atoi(e) != 0;
    if (const char *e = layout_knob("VBC_PLANAR_MASK_PAIR")) c.planar_mask_pair = atoi(e) != 0;
    if (const char *e = layout_knob("VBC_MASK_WINDOW")) c.mask_window = std::max(1, std::min(64, atoi(e)));
    if (const char *e = layout_knob("VBC_PLANAR_SPLIT")) {  // 0 never, 1 auto, 2 / 4 / 8 forced
        const int v = atoi(e);
        c.planar_split = v == 0 ? 0 : (v == 2 || v == 4 || v == 8) ? v : -1;
    }
    if (flags & VBC_CREATE_SERIAL) {  // every stripe summed serially in stored row order:
        c.planar_split = 0;            // no split planar product (P slices meeting in LDS),
        if (c.slots_mode < 0) c.slots_mode = 1;  // and no merge layout (its segmented scan joins slot sums)
    }
    c.occ_p = std::max(1, std::min(f.occ_planar[e32], 8));
    c.target_ranges_l = f.cus * std::max(1, std::min(f.occ_lanes[e32], 8)) * kWavesPerBlock;
    if (const char *e = layout_knob("VBC_PLANAR_LANES")) c.planar_lanes = atoi(e) == 0 ? 0 : atoi(e) == 1 ? 1 : -1;
    if (const char *e = layout_knob("VBC_TARGET_RANGES_L")) c.target_ranges_l = std::max(1, atoi(e));
    if (const char *e = tuning_knob("VBC_LANES_DEEP")) c.lanes_deep = atoi(e) != 0;
    if (const char *e = tuning_knob("VBC_LANES_RDIV")) c.lanes_rdiv = std::max(1, atoi(e));
    if (const char *e = layout_knob("VBC_LANES_PAIR")) c.lanes_pair = atoi(e) != 0;
    if (const char *e = tuning_knob("VBC_SPLIT_KC")) c.split_kc = atoi(e) != 0;
    if (const char *e = tuning_knob("VBC_SPLIT_ROWS")) c.split_rows = std::max(1, atoi(e));
    if (const char *e = layout_knob("VBC_SMALL_FUSE")) c.small_fuse = atoi(e);
    if (const char *e = layout_knob("VBC_SIDE_FUSE")) c.side_fuse = atoi(e) < 0 ? -1 : atoi(e) != 0;
    if (const char *e = layout_knob("VBC_COLSPLIT")) c.colsplit = atoi(e) != 0;
    if (const char *e = tuning_knob("VBC_FUSE_PMAX")) c.fuse_pmax = atoi(e) >= 8 ? 8 : atoi(e) >= 4 ? 4 : 2;
    if (const char *e = tuning_knob("VBC_COLSPLIT_W")) c.colsplit_w = std::max(0, atoi(e));
    if (const char *e = tuning_knob("VBC_SPLIT_PIPE")) c.split_pipe = atoi(e);
    if (const char *e = tuning_knob("VBC_SMALL_ROWS")) c.small_rows = std::max(1, atoi(e));
    if (const char *e = layout_knob("VBC_KSPLIT")) c.ksplit = std::max(0.0, atof(e));
    if (const char *e = layout_knob("VBC_FWD_T")) c.fwd_t = atoi(e);
    if (const char *e = tuning_knob("VBC_SPLIT_DEEP")) c.split_deep = std::max(0.0, atof(e));
    if (const char *e = tuning_knob("VBC_SPLIT_NT_MB")) c.split_nt_bytes = (int64_t)(atof(e) * (1 << 20));
    if (const char *e = tuning_knob("VBC_FWD_MIN_ROWS")) c.fwd_min_rows = std::max(1, atoi(e));
    if (const char *e = tuning_knob("VBC_PLANAR_WPS")) c.planar_wps = c.planar_wps_pair = std::max(0, atoi(e));
    if (const char *e = tuning_knob("VBC_PLANAR_WPS_PAIR")) c.planar_wps_pair = std::max(0, atoi(e));
    if (const char *e = tuning_knob("VBC_SLOT_WONLY")) c.slot_wonly = atoi(e) != 0;
    c.target_ranges_p = f.cus * c.occ_p * kWavesPerBlock;
    c.cus = std::max(1, (int)f.cus);
    for (int lp = 1; lp <= 3; lp++) c.occ_multi[lp] = f.occ_split_multi[e32][lp - 1];
    if (const char *e = tuning_knob("VBC_TARGET_RANGES_P")) {
        c.target_ranges_p = std::max(1, atoi(e));
        c.occ_p = 1;
    }
    c.slot_u = c.esz == 8 ? 8 : 16;  // rows per step (measured on FE: 4 / 8 rows are 4-8 % slower)
    if (flags & (VBC_CREATE_MULTI | VBC_CREATE_MULTI_FORWARD)) {
        // (round 5: half as many ranges measured 195.5 against 206.5 us in tools/ab.py's interleaved graph replays,
        // but 213-216 against 208-210 us in bench.py's own C5 line, each setting in a fresh process --
        // profiles/r05zo_c5_ranges_ab.log; the bench decides, the count stays one round of resident waves)
        const int om = f.occ_panel[e32];
        c.target_ranges_m = f.cus * std::max(1, std::min(om, 8)) * kWavesPerBlock;
        if (const char *e = tuning_knob("VBC_TARGET_RANGES_M")) c.target_ranges_m = std::max(1, atoi(e));
        if (const char *e = ablation_knob("VBC_PANEL_VALU")) c.panel_valu = atoi(e) != 0;
        if (const char *e = ablation_knob("VBC_PANEL_DIAG")) c.panel_valu |= atoi(e) & ~1;
        if (const char *e = tuning_knob("VBC_PANEL_NOBUF")) c.panel_nobuf = atoi(e) != 0;
        if (const char *e = layout_knob("VBC_PANEL_TILES")) c.panel_tiles = atoi(e) < 0 ? -1 : atoi(e) != 0;
        if (const char *e = tuning_knob("VBC_TILE_NBT")) c.tile_nbt = atoi(e) >= 8 ? 8 : 4;
        if (const char *e = tuning_knob("VBC_TILE_SPR")) c.tile_spr = std::max(1, atoi(e));
        if (const char *e = layout_knob("VBC_TILE_CLUSTER")) c.tile_cluster = atoi(e) == 2 ? 2 : atoi(e) != 0;
        if (const char *e = tuning_knob("VBC_TILE_DEPTH")) c.tile_depth = atoi(e) == 3 ? 3 : 2;
        c.occ_tiles = f.occ_tiles[e32];
    }

    if (const char *e = tuning_knob("VBC_PAD")) {  // "w:wp,..."
        c.pad_set = true;
        for (const char *p = e; *p;) {
            int a = 0, b = 0, n = 0;
            if (sscanf(p, "%d:%d%n", &a, &b, &n) != 2) break;
            if (a >= 0 && a <= 64 && b >= a && b <= 64) c.pad_w[a] = (uint8_t)b;
            p += n;
            if (*p == ',') p++;
        }
    }
    if (const char *e = tuning_knob("VBC_TILE_RANGES")) c.tile_ranges = std::max<int64_t>(1, atoll(e));
    c.no_affine = ablation_knob("VBC_NO_AFFINE") != nullptr;  // (the VBC_ABLATION build only)
    if (const char *e = ablation_knob("VBC_SWEEP_DIAG")) c.sweep_diag = atoi(e);
    if (const char *e = ablation_knob("VBC_TILE_DIAG")) c.tile_diag = atoi(e);
    c.verbose = layout_knob("VBC_VERBOSE") != nullptr;
    return c;
}

}  // namespace vbc
