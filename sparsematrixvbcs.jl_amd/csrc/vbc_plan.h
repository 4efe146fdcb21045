// The layout planner's interface: from the input stripes and a LayoutConfig to the arena image and the launch
// descriptors without device pointers.  Pure host code: the planner calls no HIP runtime function and reads no
// environment.  The create entry points (vbc_create.hip) make the plans; the device part of a create (instantiate)
// uploads one.  The planner is three units of its own -- vbc_plan.hip (plan_layout and the per-direction planners),
// vbc_plan_bins.hip (the per-bucket builders), vbc_plan_panel.hip (the panel layouts) -- which share
// vbc_plan_impl.h; tests/test_plan_host.py checks that their objects reference no HIP runtime function and no getenv.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "vbc_config.h"
#include "vbc_internal.h"
#include "vbc_launch_desc.h"

namespace vbc {

// Host description of the input stripes, common to 1D, 2D (expanded) and CSC inputs.
struct Stripes {
    int64_t m = 0, n = 0, L = 0;
    std::vector<int64_t> col0;  // 0-based first column of stripe l
    std::vector<int32_t> w;     // width
    std::vector<int64_t> rbeg;  // L+1 prefix into rows
    std::vector<int32_t> rows;  // 0-based x row of each stored w-wide row
    std::vector<int64_t> voff;  // element offset of the stripe's first value in the input val
    std::vector<int32_t> vst;   // per stripe: elements between its stored rows' values (empty: the width;
                                // a column piece keeps its source stripe's stride)
    int64_t vstride(int64_t l) const { return vst.empty() ? w[l] : vst[l]; }
    std::vector<int64_t> grp;   // 2D input: Π's block-row starts (K + 1, 0-based); empty for 1D / CSC
};

// The reference's fields as Stripes, with the checks of its inner constructors: shared by the creates and
// vbcx_plan_image.  nval: the elements of val the stripes address.
struct StripesInput {
    Stripes s;
    int64_t nval = 0, K = 0, nblocks = 0;
};

// The recorder of VBC_CREATE_UPDATABLE's recording plans (vbc_create.hip plan_value_map): the byte ranges of the
// arena filled from transpose_stripes' values (the value map marks their slots, vbc_handle.h).  With a recorder
// transpose_stripes copies the (tag) values instead of summing them.  `narrow`: the byte ranges of the value
// regions stored as Float32 on a Float64 handle (VBC_CREATE_NARROW_UPDATABLE), in arena order; the builders that
// narrow copy a tag's low 4 bytes there (narrow_value).  `ft_narrow`: whether the handle's own plan kept narrow
// storage in the forward-on-Bᵀ layout (plan_layout's guard reads values, which a recording plan does not have).
struct Recorder {
    ByteRanges canon;
    ByteRanges narrow;
    bool ft_narrow = false;
};

// What the builders write besides the arena: which layouts exist and their statistics.
struct PlanStats {
    bool has_t = false, has_f = false, has_ft = false, has_m = false, has_mf = false;
    bool f_scale = false;          // forward with several buckets: scale y by beta first
    int64_t bytes_t = 0, bytes_f = 0, bytes_m = 0, bytes_mf = 0;  // matrix bytes one product streams
    int32_t mf_group = 0;          // forward panel: widest output row group
    int64_t panel_val_bytes = 0;   // largest bin val array of the panel layout
    bool ft_narrow = false;        // the forward-on-Bᵀ layout kept narrow storage (plan_layout's guard)
    // scratch of build_transposed, rebuilt by each call:
    int small_split = 0;           // > 1: this B'x layout is the fused small-matrix split with P waves per chunk
    uint32_t fuse_w = 0;           // bit w: the width-w bucket belongs to the fused split (all, or the side buckets)
};

// Arena builder: reserves aligned regions, fills a host image, uploads once.
struct Arena {
    std::vector<char> host;
    size_t reserve(size_t bytes)
    {
        size_t off = (host.size() + 255) & ~size_t(255);
        host.resize(off + std::max<size_t>(bytes, 1));
        return off;
    }
    template <typename U>
    U *at(size_t off) { return reinterpret_cast<U *>(host.data() + off); }
};

// A planned bin: its descriptor without device pointers and the arena offsets they will point to.
struct PendingBin {
    Bin b;
    size_t o_key, o_val, o_rseg, o_out, o_carry, o_cseg;
    double work = 0;  // matrix bytes the bin streams (launch-group ordering)
};

struct PendingSlot {
    SlotBin b;
    size_t o_key, o_val, o_out, o_rrow, o_rchunk, o_base = 0, o_doff = 0, o_nlive = 0;
    size_t o_trow = 0, o_tseg = 0, o_lseg = 0;  // lanes layout (build_lanes)
    bool lanes_done = false;                    // keys already stored (build_lanes: 32-bit keys per run)
    int64_t key_bytes = 0;       // index bytes as stored (keys, deltas, bases, delta offsets)
    std::vector<uint32_t> keys;  // full keys until commit_slot_keys picks the stored form
    int64_t rows = 0;
    int64_t real = 0;            // entries without padding
    bool kc_ok = false;          // every row's keys fit base + int16 deltas
};

struct PendingSweep {
    SweepBin b;
    size_t o_tstep, o_key, o_loc, o_val, o_out, o_sbase;
    double work = 0;  // matrix bytes the bin streams (launch-group ordering)
};

struct PendingPanel {
    PanelBin b;
    TileBin tb;  // tile: a small-tile bucket (vbc_tiles.h; o_rgrp = its range table)
    bool tile = false;
    size_t o_key, o_val, o_out, o_rgrp, o_rseg;
};

// Integer eltypes: arena offsets of IntLayout.
struct IntPlan {
    int64_t L = 0, nrows = 0;
    size_t o_col0 = 0, o_w = 0, o_rows = 0, o_c2s = 0, o_r2s = 0, o_rbeg = 0, o_voff = 0, o_val = 0;
};

// One planned launch: its pending bins (arena offsets) and the host descriptor without device pointers.
struct LaunchPlan {
    std::vector<PendingBin> bins;
    std::vector<PendingSlot> slots;
    std::vector<PendingSweep> sweeps;
    Launch L;
};
struct PanelPlan {
    std::vector<PendingPanel> bins;
    PanelLaunch L;
};

// What plan_layout makes and instantiate uploads: the arena image, the planned launches per direction --
// transposed (t), forward as the transposed product of C = Bᵀ (tf), forward with one launch per width bucket
// (f), panels (m, mf) -- and the statistics.
struct Plan {
    Arena ar;
    bool is_int = false;
    IntPlan li;
    LaunchPlan t, tf;
    std::vector<LaunchPlan> f;
    PanelPlan m, mf;
    PlanStats st;
};

int check_plan_input(int dtype, const Stripes &s);
// Plans every layout `flags` asks for (none of the four layout flags: the transposed one).  v: nval elements
// of cfg.dtype.  Pure host code: no HIP call, no environment.
int plan_layout(const LayoutConfig &cfg, const Stripes &s, const char *v, int64_t nval, unsigned flags, Plan &P,
                Recorder *rec);

}  // namespace vbc
