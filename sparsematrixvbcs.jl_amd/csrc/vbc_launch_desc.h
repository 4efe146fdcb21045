// The launch descriptors of a handle: filled by the layout planner (vbc_plan.h, everything but the device
// pointers, streams and events), completed by the device part of a create (vbc_device.hip) and read by the
// kernel launches (vbc_launch.hip / vbc_panel_launch.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "vbc_kernels.h"
#include "vbc_panel.h"
#include "vbc_tiles.h"

namespace vbc {

// One fused launch of spmv_ranges (+ its fix-up pass).
struct Launch {
    std::vector<Bin> bins;
    Bin *d_bins = nullptr;
    int total_ranges = 0;
    int nfill = 0;
    size_t o_fill = 0;             // arena offset of the fill list (y indices)
    const int32_t *d_fill = nullptr;
    std::vector<SlotBin> sbins;    // slotted buckets (vbc_slots.h), launched before the merge kernel
    SlotBin *d_sbins = nullptr;
    int slot_ranges = 0;
    std::vector<SlotBin> pbins;    // planar slotted buckets (vbc_planar.h), one launch each
    SlotBin *d_pbins = nullptr;  // (uploaded, but no kernel reads it: the planar kernels take their bin by value)
    std::vector<SweepBin> wbins;   // row-swept buckets (vbc_sweep.hip, B'x only), launched first
    SweepBin *d_wbins = nullptr;
    int sweep_tiles = 0;
    int sweep_tile_bytes = 0;      // LDS accumulator bytes per wave the layout was cut for
    int sweep_diag = 0;            // VBC_SWEEP_DIAG ablation (tools/ab.py only)
    // B'x with several independent launch groups (swept, slotted, each planar bucket, merge + fix-up:
    // disjoint stripes of y): the groups after the first run on side streams forked from the caller's
    // stream by an event and joined back, so small buckets overlap instead of queueing one after the
    // other (graph capture records them as parallel branches).  Empty when one group or VBC_FORK=0.
    // small mixed-width B'x (vbc_plan.hip build_transposed): every planar split bin in ONE launch of
    // spmv_split_multi with fuse_split waves per chunk (0: one launch per planar bin)
    int fuse_split = 0;
    int fuse_p = 0;  // the fused split's P as build_transposed chose it (finalize_launch builds `multi`)
    SplitMulti multi{};
    std::vector<double> gwork;  // matrix bytes of each launch group (launch_groups order): the heaviest is
                                // submitted last, so the small groups are already dispatched when it fills the chip
    std::vector<hipStream_t> fork_streams;
    std::vector<hipEvent_t> fork_events;  // [0]: the fork, [1 + i]: side stream i done
    void free_device();  // the bin arrays, streams and events (vbc_device.hip)
};

// The panel layout of the MFMA multi-RHS transposed product (vbc_panel.h): one launch.
struct PanelLaunch {
    std::vector<PanelBin> bins;
    PanelBin *d_bins = nullptr;
    std::vector<TileBin> tbins;  // small-tile buckets (vbc_tiles.h, u, w <= 4): one launch each
    int total_ranges = 0;
    int nfill = 0;
    size_t o_fill = 0;
    const int32_t *d_fill = nullptr;
    void free_device();
};

}  // namespace vbc
