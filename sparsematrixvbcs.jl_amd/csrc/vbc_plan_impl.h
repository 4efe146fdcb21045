// Private to the layout planner's units (vbc_plan.hip, vbc_plan_bins.hip, vbc_plan_panel.hip): what the builders
// see and the builders that are called from another unit than their own.  Pure host code, as vbc_plan.h promises:
// no HIP call, no environment.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "vbc_plan.h"

namespace vbc {

// What the builders see (as `h`): the configuration, the statistics they fill, the recorder (NULL outside a
// recording plan).  No handle, no device.
struct PlanCtx : LayoutConfig {
    PlanCtx(const LayoutConfig &c, PlanStats &stats, Recorder *r, int64_t nv) : LayoutConfig(c), st(stats), rec(r), nval(nv) {}
    PlanStats &st;
    Recorder *rec;
    int64_t nval;  // elements of the input val
};

// The Float32 a narrow value slot stores for the fp64 value at `src`.  In a recording plan `src` holds a tag
// (i + 1 <= 2^31 - 1 as an integer, a denormal as a double): its low 4 bytes are the tag and are never zero.
inline void narrow_value(const PlanCtx *h, const double *src, void *dst)
{
    if (h->rec) {
        std::memcpy(dst, src, 4);  // little-endian
    } else {
        const float f = (float)*src;
        std::memcpy(dst, &f, 4);
    }
}

// A logical entry of a bucket's stream: gather index + where its w values come from.
struct Entry {
    uint32_t key;   // gather index | HEAD
    int64_t voff;   // element offset into the input val
};

// What a builder that may decline returns when it built nothing (build_slots with pair_only); no status code.
constexpr int kBuildDeclined = -1;

// Padded / real rows a masked planar bucket may carry: padding costs instructions, not lines.
constexpr double kMaskPad = 3.0;

// vbc_plan_bins.hip: the per-bucket builders
int build_bucket(PlanCtx *h, int kind, int w, const std::vector<Entry> &ents,
                 const std::vector<int32_t> &out, int64_t total_entries, const char *val,
                 Arena &ar, int &range0, PendingBin &pb, int wsrc = 0);
bool slot_keys_compressible(const std::vector<uint32_t> &keys, int64_t rows, int RPI);
bool slot_planar(const PlanCtx *h, int kind, int w);
std::vector<int32_t> chunk_rows(const std::vector<int64_t> &sbeg, int RPI);
std::vector<int64_t> sorted_order(const std::vector<int64_t> &sbeg, int RPI);
std::vector<int64_t> permuted_sbeg(const std::vector<int64_t> &sbeg, const std::vector<int64_t> &ord);
std::vector<int64_t> chunk_sorted_order(const std::vector<int64_t> &sbeg, int win);
int want_slots(const PlanCtx *h, int kind, int w, const std::vector<int64_t> &sbeg,
               int64_t total_entries, int64_t gather_limit, std::vector<int64_t> &order,
               bool *mask = nullptr, int wsrc = -1);
int slot_runs(const PlanCtx *h, const std::vector<Entry> &ents, const std::vector<int64_t> &sbeg);
int build_slots(PlanCtx *h, int kind, int w, int wsrc, const std::vector<Entry> &ents,
                const std::vector<int64_t> &sbeg0, const std::vector<int32_t> &out0, int64_t total_entries,
                const char *val, Arena &ar, int &range0, PendingSlot &ps,
                const std::vector<int64_t> &order = {}, bool mask = false, int ks = 1, bool pair_only = false);
bool want_lanes(const PlanCtx *h, int wps, int w, const std::vector<int64_t> &sbeg,
                const std::vector<int32_t> &out, int64_t total_entries, bool mask);
int build_lanes(PlanCtx *h, int w, const std::vector<Entry> &ents, const std::vector<int64_t> &sbeg,
                const std::vector<int32_t> &out, int run, int64_t total_entries, const char *val, Arena &ar,
                PendingSlot &ps);
void commit_launch_keys(const PlanCtx *h, std::vector<PendingSlot> &pss, Arena &ar);
bool sweep_possible(const PlanCtx *h, int w, int64_t nx);
bool want_sweep(const PlanCtx *h, int w, int64_t nx, const std::vector<int64_t> &sbeg,
                const std::vector<Entry> &ents);
int build_sweep(PlanCtx *h, int kind, int w, const std::vector<int64_t> &sbeg,
                const std::vector<Entry> &ents, const std::vector<int32_t> &out, const char *val, Arena &ar,
                int &tile0, PendingSweep &pw);

// vbc_plan_panel.hip: the panel layouts and C = Bᵀ as stripes
int build_panel(PlanCtx *h, const Stripes &s, const char *val, Arena &ar, PanelPlan &plan,
                std::vector<int32_t> &fill, const std::vector<int64_t> *tgrp);
int transpose_stripes(const PlanCtx *h, const Stripes &s, const char *val, int maxu, Stripes &c,
                      std::vector<char> &cv);
int build_forward_panel(PlanCtx *h, const Stripes &s, const char *val, Arena &ar, PanelPlan &plan);

}  // namespace vbc
