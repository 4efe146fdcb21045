// The device part of libvbc's C ABI (include/vbc.h).  Of a create's three steps (vbc_create.hip: the entry points
// and their host-side checks) the first and the last are here: the device's facts (gather_facts) and the device
// part (instantiate: upload of the planned arena image, device pointers, fork streams and events); the layout is
// planned between them on the host alone (vbc_plan.h plan_layout; vbc_plan.hip, vbc_plan_bins.hip,
// vbc_plan_panel.hip).  Also here: the thread's error message (set_error), release, the products, vbc_get_info and
// vbc_update_values.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>

#include "vbc_handle.h"
#include "vbc_plan.h"

namespace vbc {

static thread_local std::string g_err;

void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

// A bin table on the device.
template <typename B>
static int upload_bins(const std::vector<B> &bins, B *&d_bins)
{
    if (bins.empty()) return VBC_OK;
    VBC_HIP(hipMalloc(&d_bins, bins.size() * sizeof(B)));
    VBC_HIP(hipMemcpy(d_bins, bins.data(), bins.size() * sizeof(B), hipMemcpyHostToDevice));
    return VBC_OK;
}

// The device pointers of a planned panel launch, into L: the handle's descriptor, moved there from the plan.
static int finalize_panel(vbc_handle *h, const PanelPlan &plan, PanelLaunch &L)
{
    L.bins.clear();
    L.tbins.clear();
    char *base = static_cast<char *>(h->d_arena);
    for (const PendingPanel &pp : plan.bins) {
        if (pp.tile) {
            TileBin t = pp.tb;
            t.key = reinterpret_cast<const uint32_t *>(base + pp.o_key);
            t.val = base + pp.o_val;
            t.out = reinterpret_cast<const int32_t *>(base + pp.o_out);
            t.rinfo = reinterpret_cast<const int32_t *>(base + pp.o_rgrp);
            L.tbins.push_back(t);
            continue;
        }
        PanelBin b = pp.b;
        b.key = reinterpret_cast<const uint32_t *>(base + pp.o_key);
        b.val = base + pp.o_val;
        b.out = reinterpret_cast<const int32_t *>(base + pp.o_out);
        b.rgrp = reinterpret_cast<const int32_t *>(base + pp.o_rgrp);
        b.rseg = reinterpret_cast<const int32_t *>(base + pp.o_rseg);
        L.bins.push_back(b);
    }
    L.d_fill = reinterpret_cast<const int32_t *>(base + L.o_fill);
    return upload_bins(L.bins, L.d_bins);
}

// The same for a planned launch (an empty plan: a forward product with no entries, its fill list alone writes y).
static int finalize_launch(vbc_handle *h, const LaunchPlan &plan, Launch &L)
{
    L.bins.clear();
    L.sbins.clear();
    L.wbins.clear();
    char *base = static_cast<char *>(h->d_arena);
    for (const PendingSweep &pw : plan.sweeps) {
        SweepBin b = pw.b;
        b.tstep = reinterpret_cast<const int32_t *>(base + pw.o_tstep);
        b.key = reinterpret_cast<const uint32_t *>(base + pw.o_key);
        b.loc = reinterpret_cast<const uint16_t *>(base + pw.o_loc);
        b.sbase = reinterpret_cast<const uint32_t *>(base + pw.o_sbase);
        b.val = base + pw.o_val;
        b.out = reinterpret_cast<const int32_t *>(base + pw.o_out);
        L.wbins.push_back(b);
    }
    if (int st = upload_bins(L.wbins, L.d_wbins)) return st;
    for (const PendingBin &pb : plan.bins) {
        Bin b = pb.b;
        b.key = reinterpret_cast<const uint32_t *>(base + pb.o_key);
        b.val = base + pb.o_val;
        b.rseg = reinterpret_cast<const int32_t *>(base + pb.o_rseg);
        b.out = reinterpret_cast<const int32_t *>(base + pb.o_out);
        b.carry = base + pb.o_carry;
        b.carry_seg = reinterpret_cast<int32_t *>(base + pb.o_cseg);
        L.bins.push_back(b);
    }
    L.pbins.clear();
    for (const PendingSlot &ps : plan.slots) {
        SlotBin b = ps.b;
        b.key = reinterpret_cast<const uint32_t *>(base + ps.o_key);
        b.val = base + ps.o_val;
        b.out = reinterpret_cast<const int32_t *>(base + ps.o_out);
        b.rrow = reinterpret_cast<const int32_t *>(base + ps.o_rrow);
        b.rchunk = reinterpret_cast<const int32_t *>(base + ps.o_rchunk);
        b.base = reinterpret_cast<const uint32_t *>(base + ps.o_base);
        b.kdoff = reinterpret_cast<const uint32_t *>(base + ps.o_doff);
        b.nlive = reinterpret_cast<const uint32_t *>(base + ps.o_nlive);
        b.trow = reinterpret_cast<const int32_t *>(base + ps.o_trow);
        b.tseg = reinterpret_cast<const int32_t *>(base + ps.o_tseg);
        b.lseg = reinterpret_cast<const int16_t *>(base + ps.o_lseg);
        (b.planar ? L.pbins : L.sbins).push_back(b);
    }
    if (int st = upload_bins(L.pbins, L.d_pbins)) return st;
    // the fused small-matrix split (build_transposed): every planar bin a split bin of the common P, all
    // of them one launch of spmv_split_multi (their chunks concatenated)
    L.fuse_split = 0;
    if (L.fuse_p > 1) {
        int nfb = 0;
        bool all = true;
        for (const SlotBin &b : L.pbins) {
            if (!b.fused) continue;
            nfb++;
            all = all && b.kind == 0 && b.split == L.fuse_p && !b.kc && !b.lanes && !b.pair && !b.mask &&
                  b.diag == 0 && b.wkey >= 1 && b.wkey <= 8 && b.w == b.wkey && b.run >= 1 && b.run <= 3;
        }
        if (nfb > 0 && nfb <= kSplitParts && all) {
            SplitMulti M{};
            int c0 = 0, i = 0;
            for (const SlotBin &b : L.pbins) {
                if (!b.fused) continue;
                M.p[i++] = SplitPart{b.wkey, b.run, c0, b.nseg, b.out_affine, b.out_base, b.out_stride, b.wst, b.holes, b.ks,
                                     b.rrow, b.key, b.val, b.out};
                c0 += b.nranges;  // a split bin's ranges are its chunks
                M.pad0 = std::max<int32_t>(M.pad0, b.deep);  // slice loop (build_slots)
            }
            M.nparts = nfb;
            M.nchunks = c0;
            L.multi = M;
            L.fuse_split = L.fuse_p;
        } else {
            for (SlotBin &b : L.pbins) b.fused = 0;  // each split bin on its own launch
        }
    }
    L.d_fill = reinterpret_cast<const int32_t *>(base + L.o_fill);
    if (int st = upload_bins(L.bins, L.d_bins)) return st;
    if (int st = upload_bins(L.sbins, L.d_sbins)) return st;
    // bytes per launch group, in launch_group's order (sweep, slots, fused split, planar bins, merge)
    L.gwork.clear();
    {
        std::vector<double> pw_planar;
        double slots = 0, fused = 0, sweep = 0, merge = 0;
        size_t pi = 0;
        for (const PendingSlot &ps : plan.slots) {
            const double wk = (double)ps.rows * ps.b.rpi * ps.b.w * h->esz + (double)ps.key_bytes;
            if (!ps.b.planar) slots += wk;
            else if (L.fuse_split && L.pbins[pi++].fused) fused += wk;
            else pw_planar.push_back(wk);
        }
        for (const PendingSweep &pw : plan.sweeps) sweep += pw.work;
        for (const PendingBin &pb : plan.bins) merge += pb.work;
        if (L.sweep_tiles > 0) L.gwork.push_back(sweep);
        if (L.slot_ranges > 0) L.gwork.push_back(slots);
        if (L.fuse_split) L.gwork.push_back(fused);
        for (double wk : pw_planar) L.gwork.push_back(wk);
        if (L.total_ranges > 0 || L.nfill > 0) L.gwork.push_back(merge + 1.0);
    }
    return VBC_OK;
}

// Side streams for the independent groups of a transposed launch.
static int fork_streams(const vbc_handle *h, Launch &Lx)
{
    if (!h->cfg.fork || launch_groups(Lx) < 2) return VBC_OK;
    // no fork beside one dominant group when the others are more than a few waves of work: they are
    // latency-bound, and beside a launch that saturates HBM their dependent loads wait on a loaded
    // memory system while holding its wave slots (the ldoor stand-in's fp64 'min blocks': merge
    // kernel 131.5 us + fused side launch 11.5 us one after another, 160.3 / 88.7 us side by side;
    // 154 against 188 us per product, profiles/r04_bprof_*).  A side group of a few chunks still
    // forks (its one wave hides under the big launch).
    if ((int)Lx.gwork.size() == launch_groups(Lx)) {
        double tot = 0, big = 0;
        for (double wk : Lx.gwork) { tot += wk; big = std::max(big, wk); }
        if (big >= 0.9 * tot && tot - big > h->cfg.fork_side_bytes) return VBC_OK;
    }
    const int ns = std::min(launch_groups(Lx) - 1, 3);
    for (int i = 0; i < ns; i++) {
        hipStream_t q = nullptr;
        if (hipStreamCreateWithFlags(&q, hipStreamNonBlocking) != hipSuccess) return fail(VBC_HIP_ERROR, "hipStreamCreate failed");
        Lx.fork_streams.push_back(q);
    }
    for (int i = 0; i <= ns; i++) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(VBC_HIP_ERROR, "hipEventCreate failed");
        Lx.fork_events.push_back(e);
    }
    return VBC_OK;
}

void Launch::free_device()
{
    if (d_bins) (void)hipFree(d_bins);
    if (d_sbins) (void)hipFree(d_sbins);
    if (d_wbins) (void)hipFree(d_wbins);
    if (d_pbins) (void)hipFree(d_pbins);
    for (hipStream_t q : fork_streams) (void)hipStreamDestroy(q);
    for (hipEvent_t e : fork_events) (void)hipEventDestroy(e);
}

void PanelLaunch::free_device()
{
    if (d_bins) (void)hipFree(d_bins);
}

void release(vbc_handle *h)
{
    if (!h) return;
    DeviceGuard g(h->device);
    h->lft.free_device();
    h->lm.free_device();
    h->lmf.free_device();
    for (Launch &l : h->lf) l.free_device();
    if (h->d_arena) (void)hipFree(h->d_arena);
    if (h->umap.d_buf) (void)hipFree(h->umap.d_buf);
    if (h->d_carry_mm) (void)hipFree(h->d_carry_mm);
    for (void *p : h->d_stage)
        if (p) (void)hipFree(p);
    if (h->order_ev) (void)hipEventDestroy(h->order_ev);
    h->lt.free_device();
    delete h;
}

// What a create asks the device (the current one, ordinal `device`): the rows of the eltypes in `eltypes`
// (bit 0: Float64, bit 1: Float32), the panel / tile rows only with `multi`.
int gather_facts(int device, unsigned eltypes, bool multi, DeviceFacts &f)
{
    f = DeviceFacts{};
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(VBC_HIP_ERROR, "hipGetDeviceProperties failed");
    f.cus = prop.multiProcessorCount;
    for (int e = 0; e < 2; e++) {
        if (!((eltypes >> e) & 1)) continue;
        const int esz = e ? 4 : 8;
        for (int k = 0; k < 2; k++)
            for (int p = 0; p < 2; p++) occupancy_ranges(esz, k ? 8 : 4, p ? 3 : 2, f.occ_ranges[e][k][p]);
        for (int kd = 0; kd < 2; kd++) f.occ_slots[e][kd] = occupancy_slots(esz, kd);
        f.occ_planar[e] = occupancy_planar(esz);
        f.occ_lanes[e] = occupancy_lanes(esz);
        for (int lp = 1; lp <= 3; lp++) f.occ_split_multi[e][lp - 1] = occupancy_split_multi(esz, 1 << lp);
        if (multi) {
            f.occ_panel[e] = occupancy_panel(esz);
            f.occ_tiles[e] = occupancy_tiles(esz);
        }
    }
    return VBC_OK;
}

// The device side of the handle: the caller's current device is `h->device`.
static int instantiate_on_device(vbc_handle *h, Plan &P)
{
    if (hipEventCreateWithFlags(&h->order_ev, hipEventDisableTiming) != hipSuccess)
        return fail(VBC_HIP_ERROR, "hipEventCreate failed");
    const std::vector<char> &image = P.ar.host;
    h->arena_used = image.size();
    h->arena_bytes = P.is_int ? image.size() : std::max<size_t>(image.size(), 256);
    if (hipMalloc(&h->d_arena, h->arena_bytes) != hipSuccess) return fail(VBC_HIP_ERROR, "hipMalloc of the matrix arena failed");
    if (!image.empty() && hipMemcpy(h->d_arena, image.data(), image.size(), hipMemcpyHostToDevice) != hipSuccess)
        return fail(VBC_HIP_ERROR, "hipMemcpy of the matrix arena failed");
    if (P.is_int) {
        const char *b = static_cast<const char *>(h->d_arena);
        IntLayout &li = h->li;
        li.L = P.li.L;
        li.nrows = P.li.nrows;
        li.col0 = reinterpret_cast<const int32_t *>(b + P.li.o_col0);
        li.w = reinterpret_cast<const int32_t *>(b + P.li.o_w);
        li.rows = reinterpret_cast<const int32_t *>(b + P.li.o_rows);
        li.col2stripe = reinterpret_cast<const int32_t *>(b + P.li.o_c2s);
        li.row2stripe = reinterpret_cast<const int32_t *>(b + P.li.o_r2s);
        li.rbeg = reinterpret_cast<const int64_t *>(b + P.li.o_rbeg);
        li.voff = reinterpret_cast<const int64_t *>(b + P.li.o_voff);
        li.val = reinterpret_cast<const int64_t *>(b + P.li.o_val);
        return VBC_OK;
    }
    h->lt = std::move(P.t.L);
    h->lft = std::move(P.tf.L);
    for (LaunchPlan &lp : P.f) h->lf.push_back(std::move(lp.L));
    h->lm = std::move(P.m.L);
    h->lmf = std::move(P.mf.L);
    int st = VBC_OK;
    if (h->has_t && (st = finalize_launch(h, P.t, h->lt))) return st;
    if (h->has_ft && (st = finalize_launch(h, P.tf, h->lft))) return st;
    if (h->has_t && (st = fork_streams(h, h->lt))) return st;
    if (h->has_ft && (st = fork_streams(h, h->lft))) return st;
    if (h->has_m && (st = finalize_panel(h, P.m, h->lm))) return st;
    if (h->has_mf && (st = finalize_panel(h, P.mf, h->lmf))) return st;
    // (a forward layout with no entries is one empty LaunchPlan: the fill list alone writes y)
    for (size_t b = 0; b < P.f.size(); b++)
        if ((st = finalize_launch(h, P.f[b], h->lf[b]))) return st;
    h->has_scratch = (h->has_t && !h->lt.bins.empty()) || (h->has_ft && !h->lft.bins.empty());
    for (const Launch &l : h->lf) h->has_scratch = h->has_scratch || (h->has_f && !l.bins.empty());
    return VBC_OK;
}

// Uploads a plan's arena to `device` and builds the handle around it (the caller fills the matrix dimensions).
int instantiate(Plan &P, const LayoutConfig &cfg, int device, vbc_handle **out)
{
    vbc_handle *h = new vbc_handle(cfg);
    h->dtype = cfg.dtype;
    h->esz = cfg.esz;
    h->device = device;
    h->cus = cfg.cus;
    h->panel_nobuf = cfg.panel_nobuf;
    h->has_t = P.st.has_t, h->has_f = P.st.has_f, h->has_ft = P.st.has_ft, h->has_m = P.st.has_m, h->has_mf = P.st.has_mf;
    h->f_scale = P.st.f_scale;
    h->bytes_t = P.st.bytes_t, h->bytes_f = P.st.bytes_f, h->bytes_m = P.st.bytes_m, h->bytes_mf = P.st.bytes_mf;
    h->mf_group = P.st.mf_group;
    h->panel_val_bytes = P.st.panel_val_bytes;
    DeviceGuard g(device);
    const int st = g.ok ? instantiate_on_device(h, P) : fail(VBC_HIP_ERROR, "hipSetDevice failed");
    if (st != VBC_OK) {
        release(h);
        return st;
    }
    *out = h;
    return VBC_OK;
}

}  // namespace vbc

using namespace vbc;

extern "C" {

static_assert(sizeof(vbc_info) == VBC_INFO_SIZE, "vbc_info layout changed: bump VBC_VERSION and VBC_INFO_SIZE");

int vbc_version(void) { return VBC_VERSION; }

int vbc_last_error(char *buf, size_t n)
{
    if (buf && n) {
        std::strncpy(buf, g_err.c_str(), n - 1);
        buf[n - 1] = 0;
    }
    return (int)g_err.size();
}

int vbc_destroy(vbc_handle *h)
{
    release(h);
    return VBC_OK;
}

// The planar_mask bit of a planar bucket of Float32 values: 14 / 15 a B'x / forward bucket of the plain planar
// kernels (VBC_CREATE_NARROW_PLANAR), 16 / 17 a lane-pair one (VBC_CREATE_NARROW_PAIRS), 18 / 19 a plain lane-stream
// one (VBC_CREATE_NARROW_STREAMS).
static int narrow_bit(const SlotBin &b, bool fwd)
{
    return (b.pair ? 16 : b.lanes ? 18 : 14) + (fwd ? 1 : 0);
}

int vbc_get_info(const vbc_handle *h, vbc_info *info)
{
    if (!h || !info) return fail(VBC_INVALID_ARG, "NULL handle or info");
    std::memset(info, 0, sizeof(*info));
    info->m = h->m;
    info->n = h->n;
    info->L = h->L;
    info->K = h->K;
    info->nblocks = h->nblocks;
    info->nrows = h->nrows;
    info->nval = h->nval;
    info->nnz_hint = h->nnz;
    info->dtype = h->dtype;
    info->device = h->device;
    info->bins_t = h->has_t ? (int32_t)h->lt.bins.size() : 0;
    int32_t bf = 0;
    for (auto &l : h->lf) bf += (int32_t)l.bins.size();
    if (h->has_ft) bf += (int32_t)(h->lft.bins.size() + h->lft.sbins.size() + h->lft.pbins.size() + h->lft.wbins.size());
    info->bins_f = h->has_f ? bf : 0;
    if (h->has_ft) info->planar_mask |= 256;  // the forward product runs on the transposed layout of C = Bᵀ
    info->device_bytes = (int64_t)(h->arena_bytes + h->umap.bytes);  // the value map of an updatable handle included
    info->bytes_t = h->bytes_t;
    info->bytes_f = h->bytes_f;
    info->bins_m = h->has_m ? (int32_t)(h->lm.bins.size() + h->lm.tbins.size())
                 : h->has_mf ? (int32_t)(h->lmf.bins.size() + h->lmf.tbins.size()) : 0;
    if ((h->has_m && !h->lm.tbins.empty()) || (h->has_mf && !h->lmf.tbins.empty()))
        info->planar_mask |= 512;  // multi-RHS buckets in the tile-granular layout (spmm_tiles)
    int32_t sl = h->has_t ? (int32_t)(h->lt.sbins.size() + h->lt.pbins.size()) : 0;  // planar bins are slotted too
    for (auto &l : h->lf) sl += h->has_f ? (int32_t)(l.sbins.size() + l.pbins.size()) : 0;  // + planar forward
    if (h->has_ft) sl += (int32_t)(h->lft.sbins.size() + h->lft.pbins.size());  // forward on C = Bᵀ's layout
    info->slot_bins = sl;
    int32_t sw = h->has_t ? (int32_t)h->lt.wbins.size() : 0;
    for (auto &l : h->lf) sw += h->has_f ? (int32_t)l.wbins.size() : 0;
    info->sweep_bins = sw;
    int32_t pl = h->has_t ? (int32_t)h->lt.pbins.size() : 0;
    info->planar_bins = pl;
    info->planar_run = 1;
    info->planar_split = 1;
    if (h->has_t)
        for (const auto &b : h->lt.pbins) {
            info->planar_run = std::max<int32_t>(info->planar_run, b.run);
            info->planar_split = std::max<int32_t>(info->planar_split, b.split);
            info->planar_pair = std::max<int32_t>(info->planar_pair, b.pair);
            info->planar_mask = std::max<int32_t>(info->planar_mask & 1, b.mask) | (info->planar_mask & ~1);
            if (b.lanes) info->planar_mask |= 4;
        }
    if (h->has_t && h->lt.fuse_split) info->planar_mask |= 32;  // the B'x planar bins run as one fused split launch
    if (h->has_t)
        for (const SlotBin &b : h->lt.pbins)
            if (b.ks > 1) info->planar_mask |= 64;  // long stripes cut into lane parts (SlotBin::ks)
    info->fwd_run = 1;
    if (h->has_f)
        for (const auto &l : h->lf)
            for (const auto &b : l.pbins) {
                info->fwd_run = std::max<int32_t>(info->fwd_run, b.lanes ? b.wkey : b.run);  // lanes: W = R rows
                if (b.mask && !b.lanes) info->planar_mask |= 2;
                if (b.split > 1) info->planar_mask |= 8;
                if (b.lanes) info->planar_mask |= 16;
                if (b.dot) info->planar_mask |= 2048;  // forward lane pairs (run_pair DOT)
            }
    if (h->has_ft)  // the forward product on C = Bᵀ: its split bins sum P slices too (bit 3, as a split forward)
        for (const SlotBin &b : h->lft.pbins)
            if (b.split > 1) info->planar_mask |= 8;
    if (h->has_t)
        for (const SlotBin &b : h->lt.sbins)
            if (b.vsz) info->planar_mask |= 1 << 12;  // B'x slotted buckets of Float32 values (VBC_CREATE_NARROW_VALUES)
    if (h->has_f)
        for (const auto &l : h->lf)
            for (const SlotBin &b : l.sbins)
                if (b.vsz) info->planar_mask |= 1 << 13;  // forward ones
    if (h->has_ft)
        for (const SlotBin &b : h->lft.sbins)
            if (b.vsz) info->planar_mask |= 1 << 13;
    if (h->has_t)
        for (const SlotBin &b : h->lt.pbins)
            if (b.vsz) info->planar_mask |= 1 << narrow_bit(b, false);
    if (h->has_f)
        for (const auto &l : h->lf)
            for (const SlotBin &b : l.pbins)
                if (b.vsz) info->planar_mask |= 1 << narrow_bit(b, true);
    if (h->has_ft)
        for (const SlotBin &b : h->lft.pbins)
            if (b.vsz) info->planar_mask |= 1 << narrow_bit(b, true);
    if (h->has_t)
        for (const SweepBin &b : h->lt.wbins)
            if (b.vsz) info->planar_mask |= 1 << 20;  // B'x row-swept buckets of Float32 values (VBC_CREATE_NARROW_SWEPT)
    if (h->has_f)
        for (const auto &l : h->lf)
            for (const SweepBin &b : l.wbins)
                if (b.vsz) info->planar_mask |= 1 << 21;  // forward ones
    if (h->has_ft)
        for (const SweepBin &b : h->lft.wbins)
            if (b.vsz) info->planar_mask |= 1 << 21;
    bool mm_slotted = false;
    if (mulmat_fuses(h, &mm_slotted) && mm_slotted)
        info->planar_mask |= 1 << 22;  // row-major B'X runs fused over the slotted buckets (spmm_slots)
    const ColForm ct = mulmat_col_form(h, 1), cf = mulmat_col_form(h, 0);
    if (ct == kColSlots)
        info->planar_mask |= 1 << 23;  // column-major B'X runs fused over the slotted buckets (spmm_slots_col)
    if (ct == kColPlanar)
        info->planar_mask |= 1 << 24;  // column-major B'X runs fused over the planar buckets (spmm_planar_col / spmm_pair_col)
    if (cf == kColFwd)
        info->planar_mask |= 1 << 25;  // column-major B X runs fused over forward row runs (spmm_planar_fwd_col) or
                                       // forward lane pairs (spmm_pair_col with DOT)
    info->bytes_m = h->has_m ? h->bytes_m : h->bytes_mf;  // a forward-only multi handle: its Bᵀ panel layout
    return VBC_OK;
}

static int check_mul(const vbc_handle *h, int trans, int64_t nx, int64_t ny, bool mat = false)
{
    if (!h) return fail(VBC_INVALID_ARG, "NULL handle");
    // DimensionMismatch checks: multiply_1DVBC.jl:44-45 (forward), :139-140 (transposed)
    const int64_t want_x = trans ? h->m : h->n, want_y = trans ? h->n : h->m;
    if (nx != want_x || ny != want_y) return fail(VBC_DIM_MISMATCH, "DimensionMismatch");
    if (trans && !h->has_t && !(mat && h->has_m))
        return fail(VBC_INVALID_ARG, mat ? "handle built without VBC_CREATE_TRANSPOSED or VBC_CREATE_MULTI"
                                         : "handle built without VBC_CREATE_TRANSPOSED");
    if (!trans && !h->has_f && !(mat && h->has_mf))
        return fail(VBC_INVALID_ARG, mat ? "handle built without VBC_CREATE_FORWARD or VBC_CREATE_MULTI_FORWARD"
                                         : "handle built without VBC_CREATE_FORWARD");
    return VBC_OK;
}

static void apply_quirks(int trans, unsigned flags, double &alpha, double &beta)
{
    if (!(flags & VBC_MUL_REFERENCE_QUIRKS)) return;
    alpha = 1.0;             // forward drops α; transposed overwrites y
    if (trans) beta = 0.0;
}

// Orders the products of a handle whose layout has shared scratch (vbc_handle::has_scratch):
// a product on a different stream than the previous one waits for that one's completion event.
// The caller holds h->mu from before begin() until after end().  Inside a stream capture the
// captured order is the stream's own, so the event chain is skipped.
struct ProductOrder {
    vbc_handle *h;
    hipStream_t s;
    bool active = false;
    bool force = false;  // the call uses the handle's staging buffers (host operands or staged device ones)
    ProductOrder(vbc_handle *h_, hipStream_t s_, bool force_ = false) : h(h_), s(s_), force(force_) {}
    int begin()
    {
        if (!h->has_scratch && !force) return VBC_OK;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) != hipSuccess) return fail(VBC_HIP_ERROR, "hipStreamIsCapturing failed");
        if (cs != hipStreamCaptureStatusNone) return VBC_OK;
        active = true;
        if (h->order_valid && h->order_stream != s && hipStreamWaitEvent(s, h->order_ev, 0) != hipSuccess)
            return fail(VBC_HIP_ERROR, "hipStreamWaitEvent failed");
        return VBC_OK;
    }
    int end()
    {
        if (!active) return VBC_OK;
        if (hipEventRecord(h->order_ev, s) != hipSuccess) return fail(VBC_HIP_ERROR, "hipEventRecord failed");
        h->order_stream = s;
        h->order_valid = true;
        return VBC_OK;
    }
};

// Cached device staging buffer `which` (0: x / X, 1: y / Y; 2, 3: column temporaries) of at least `bytes` for a
// product on `s` (caller holds h->mu).  Growing it is refused while `s` is capturing (may_grow).
static int stage_buffer(vbc_handle *h, int which, size_t bytes, hipStream_t s, void **out)
{
    bytes = std::max<size_t>(bytes, 256);
    if (h->stage_bytes[which] < bytes) {
        if (int st = may_grow(s, "a staging buffer")) return st;
        // hipFree waits for the device: a product still using the old buffer on another stream has finished
        const size_t grow = std::max(bytes, h->stage_bytes[which] + h->stage_bytes[which] / 2);
        if (h->d_stage[which]) (void)hipFree(h->d_stage[which]);
        h->d_stage[which] = nullptr;
        h->stage_bytes[which] = 0;
        if (hipMalloc(&h->d_stage[which], grow) != hipSuccess)
            return fail(VBC_HIP_ERROR, "hipMalloc of a staging buffer failed");
        h->stage_bytes[which] = grow;
    }
    *out = h->d_stage[which];
    return VBC_OK;
}

int vbc_mul(vbc_handle *h, int trans, const void *x, int64_t nx, void *y, int64_t ny, double alpha,
            double beta, int mem, void *stream, unsigned flags)
{
    if (int st = check_mul(h, trans, nx, ny)) return st;
    apply_quirks(trans, flags, alpha, beta);
    const int64_t esz = h->esz;
    if (ny > 0 && x == y) return fail(VBC_INVALID_ARG, "x and y must not alias");
    if ((nx > 0 && !x) || (ny > 0 && !y)) return fail(VBC_INVALID_ARG, "NULL x or y");
    if (mem != VBC_MEM_DEVICE && mem != VBC_MEM_HOST)
        return fail(VBC_INVALID_ARG, "mem must be VBC_MEM_DEVICE or VBC_MEM_HOST");
    DeviceGuard g(h->device);
    if (!g.ok) return fail(VBC_HIP_ERROR, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    if (mem == VBC_MEM_DEVICE) {
        if (!h->has_scratch) return mul_dispatch(h, trans, x, y, alpha, beta, s);  // lock-free: no shared state
        std::lock_guard<std::mutex> lk(h->mu);
        ProductOrder po(h, s);
        int st = po.begin();
        if (st == VBC_OK) st = mul_dispatch(h, trans, x, y, alpha, beta, s);
        if (st == VBC_OK) st = po.end();
        return st;
    }
    // Host pointers: stage through the handle's cached device buffers (no per-call allocation).
    std::lock_guard<std::mutex> lk(h->mu);
    void *dx = nullptr, *dy = nullptr;
    if (int st = stage_buffer(h, 0, nx * esz, s, &dx)) return st;
    if (int st = stage_buffer(h, 1, ny * esz, s, &dy)) return st;
    ProductOrder po(h, s, true);  // a staged product on another stream may be using the same two buffers
    if (int st = po.begin()) return st;
    if (nx > 0 && hipMemcpyAsync(dx, x, nx * esz, hipMemcpyHostToDevice, s) != hipSuccess)
        return fail(VBC_HIP_ERROR, "staging copy of x failed");
    if (beta != 0.0 && ny > 0 && hipMemcpyAsync(dy, y, ny * esz, hipMemcpyHostToDevice, s) != hipSuccess)
        return fail(VBC_HIP_ERROR, "staging copy of y failed");
    if (int st = mul_dispatch(h, trans, dx, dy, alpha, beta, s)) return st;
    if (ny > 0 && hipMemcpyAsync(y, dy, ny * esz, hipMemcpyDeviceToHost, s) != hipSuccess)
        return fail(VBC_HIP_ERROR, "result copy failed");
    if (int st = po.end()) return st;
    if (hipStreamSynchronize(s) != hipSuccess) return fail(VBC_HIP_ERROR, "hipStreamSynchronize failed");
    return VBC_OK;
}

// 2D copy of `rows` rows of `width` bytes between pitched buffers (no-op when empty).
static bool copy2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows,
                   hipMemcpyKind kind, hipStream_t s)
{
    if (width == 0 || rows == 0) return true;
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, kind, s) == hipSuccess;
}

// The path of a multi-RHS product on device operands: the one dispatch of mul_mat_device, and what vbc_mul_mat
// orders (only kMatColumnTemps touches the handle's staging buffers; kMatFused's carries set has_scratch;
// kMatFusedCol holds no shared state and stays on the caller's stream).
enum MatPath { kMatPanels, kMatFused, kMatFusedCol, kMatColumns, kMatColumnTemps };
static MatPath mat_path(const vbc_handle *h, int trans, int64_t nrhs, bool rowmajor)
{
    if (trans ? (h->has_m && nrhs > 0 && h->n > 0) : (h->has_mf && nrhs > 0 && h->m > 0)) return kMatPanels;
    // the fused vector kernels read the merge layout and, from kMmSlotsMinRhs columns on, the slotted one
    bool slotted = false;
    bool fused = rowmajor && trans && nrhs > 0 && mulmat_fuses(h, &slotted);
    if (slotted && nrhs < kMmSlotsMinRhs) fused = false;
    if (fused) return kMatFused;
    // column-major: a launch with one of mulmat_col_form's forms, from the form's smallest nrhs on
    const ColForm cf = rowmajor ? kColNone : mulmat_col_form(h, trans);
    if (cf != kColNone && nrhs >= kColForms[cf].min_rhs) return kMatFusedCol;
    return rowmajor ? kMatColumnTemps : kMatColumns;
}

static int mul_mat_device(vbc_handle *h, int trans, int64_t nrhs, const char *dX, int64_t ldx, int64_t nx,
                          char *dY, int64_t ldy, int64_t ny, double alpha, double beta, bool rowmajor,
                          hipStream_t s)
{
    const int64_t esz = h->esz;
    int st = VBC_OK;
    const MatPath path = mat_path(h, trans, nrhs, rowmajor);
    if (path == kMatPanels) {  // matrix-core panels
        const int64_t sxr = rowmajor ? ldx : 1, sxc = rowmajor ? 1 : ldx;
        const int64_t syr = rowmajor ? ldy : 1, syc = rowmajor ? 1 : ldy;
        return mulmat_panel_any(h, trans, nrhs, dX, sxr, sxc, dY, syr, syc, alpha, beta, s);
    }
    if (path == kMatFused) return mulmat_rowmajor(h, nrhs, dX, ldx, dY, ldy, alpha, beta, s);
    if (path == kMatFusedCol) return mulmat_colmajor(h, trans, nrhs, dX, ldx, dY, ldy, alpha, beta, s);
    if (path == kMatColumns) {
        for (int64_t r = 0; r < nrhs && st == VBC_OK; r++)
            st = mul_dispatch(h, trans, dX + r * ldx * esz, dY + r * ldy * esz, alpha, beta, s);
        return st;
    }
    // row-major, per column through the handle's cached contiguous temporaries (strided 2D copies);
    // the caller holds h->mu, and the stream orders the columns -- no allocation, no synchronisation
    void *tx = nullptr, *ty = nullptr;
    if (int e = stage_buffer(h, 2, std::max<int64_t>(nx, 1) * esz, s, &tx)) return e;
    if (int e = stage_buffer(h, 3, std::max<int64_t>(ny, 1) * esz, s, &ty)) return e;
    for (int64_t r = 0; r < nrhs && st == VBC_OK; r++) {
        if (!copy2d(tx, esz, dX + r * esz, ldx * esz, esz, nx, hipMemcpyDeviceToDevice, s))
            st = fail(VBC_HIP_ERROR, "column gather failed");
        if (st == VBC_OK && beta != 0.0 && !copy2d(ty, esz, dY + r * esz, ldy * esz, esz, ny, hipMemcpyDeviceToDevice, s))
            st = fail(VBC_HIP_ERROR, "column gather failed");
        if (st == VBC_OK) st = mul_dispatch(h, trans, tx, ty, alpha, beta, s);
        if (st == VBC_OK && !copy2d(dY + r * esz, ldy * esz, ty, esz, esz, ny, hipMemcpyDeviceToDevice, s))
            st = fail(VBC_HIP_ERROR, "column scatter failed");
    }
    return st;
}

int vbc_mul_mat(vbc_handle *h, int trans, int64_t nrhs, const void *X, int64_t ldx, int64_t nx,
                void *Y, int64_t ldy, int64_t ny, double alpha, double beta, int mem, void *stream,
                unsigned flags)
{
    if (int st = check_mul(h, trans, nx, ny, true)) return st;
    const bool rowmajor = (flags & VBC_MAT_ROWMAJOR) != 0;
    if (nrhs < 0 || (!rowmajor && (ldx < std::max<int64_t>(nx, 1) || ldy < std::max<int64_t>(ny, 1))) ||
        (rowmajor && (ldx < std::max<int64_t>(nrhs, 1) || ldy < std::max<int64_t>(nrhs, 1))))
        return fail(VBC_INVALID_ARG, "bad nrhs / leading dimensions");
    if (X == Y && nrhs > 0) return fail(VBC_INVALID_ARG, "X and Y must not alias");
    if (nrhs > 0 && ((nx > 0 && !X) || (ny > 0 && !Y))) return fail(VBC_INVALID_ARG, "NULL X or Y");
    if (mem != VBC_MEM_DEVICE && mem != VBC_MEM_HOST)
        return fail(VBC_INVALID_ARG, "mem must be VBC_MEM_DEVICE or VBC_MEM_HOST");
    apply_quirks(trans, flags, alpha, beta);
    const int64_t esz = h->esz;
    DeviceGuard g(h->device);
    if (!g.ok) return fail(VBC_HIP_ERROR, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(h->mu);  // the fused kernel's carry buffer and the staging buffers
    // host operands share the X / Y staging buffers, row-major per-column products the column temporaries;
    // panels hold no shared state
    ProductOrder po(h, s, mem == VBC_MEM_HOST || mat_path(h, trans, nrhs, rowmajor) == kMatColumnTemps);
    if (mem == VBC_MEM_DEVICE) {
        int st = po.begin();
        if (st == VBC_OK)
            st = mul_mat_device(h, trans, nrhs, static_cast<const char *>(X), ldx, nx, static_cast<char *>(Y), ldy,
                                ny, alpha, beta, rowmajor, s);
        if (st == VBC_OK) st = po.end();
        return st;
    }
    // Host operands: only the logical extent moves (pitched 2D copies into packed device buffers),
    // so the padding of a caller's view (ld > extent) is never read or written.
    const int64_t xr = rowmajor ? nx : nrhs, xw = rowmajor ? nrhs : nx;  // rows x row-width (elements)
    const int64_t yr = rowmajor ? ny : nrhs, yw = rowmajor ? nrhs : ny;
    void *sx = nullptr, *sy = nullptr;
    if (int st = stage_buffer(h, 0, xr * xw * esz, s, &sx)) return st;
    if (int st = stage_buffer(h, 1, yr * yw * esz, s, &sy)) return st;
    if (int st = po.begin()) return st;
    if (!copy2d(sx, xw * esz, X, ldx * esz, xw * esz, xr, hipMemcpyHostToDevice, s))
        return fail(VBC_HIP_ERROR, "staging copy of X failed");
    if (beta != 0.0 && !copy2d(sy, yw * esz, Y, ldy * esz, yw * esz, yr, hipMemcpyHostToDevice, s))
        return fail(VBC_HIP_ERROR, "staging copy of Y failed");
    if (int st = mul_mat_device(h, trans, nrhs, static_cast<const char *>(sx), std::max<int64_t>(xw, 1), nx,
                                static_cast<char *>(sy), std::max<int64_t>(yw, 1), ny, alpha, beta, rowmajor, s))
        return st;
    if (!copy2d(Y, ldy * esz, sy, yw * esz, yw * esz, yr, hipMemcpyDeviceToHost, s))
        return fail(VBC_HIP_ERROR, "result copy failed");
    if (int st = po.end()) return st;
    if (hipStreamSynchronize(s) != hipSuccess) return fail(VBC_HIP_ERROR, "hipStreamSynchronize failed");
    return VBC_OK;
}

// ---------------------------------------------------------------------------------------------
// Generic eltypes (vbc_types), strided operands
// ---------------------------------------------------------------------------------------------

int vbc_mul_ex(vbc_handle *h, int trans, const void *x, int x_dtype, int64_t incx, int64_t nx, void *y, int y_dtype,
               int64_t incy, int64_t ny, double alpha, double beta, int mem, void *stream, unsigned flags)
{
    if (int st = check_mul(h, trans, nx, ny)) return st;
    const int cdt = h->dtype;
    if (!known_dtype(x_dtype) || !known_dtype(y_dtype)) return fail(VBC_UNSUPPORTED_DTYPE, "unknown eltype");
    if (cdt == VBC_I64 && is_float(x_dtype))
        return fail(VBC_UNSUPPORTED_DTYPE, "floating-point x on an integer handle (InexactError)");
    if (is_float(cdt) ? y_dtype != cdt : (y_dtype != VBC_I64 && y_dtype != VBC_I32))
        return fail(VBC_UNSUPPORTED_DTYPE, "eltype(y) must be the handle's compute eltype (or Int32 on an Int64 handle)");
    if ((nx > 0 && incx == 0) || (ny > 0 && incy == 0)) return fail(VBC_INVALID_ARG, "zero stride");
    if ((nx > 0 && !x) || (ny > 0 && !y)) return fail(VBC_INVALID_ARG, "NULL x or y");
    if (cdt == VBC_I64 && (alpha != std::trunc(alpha) || beta != std::trunc(beta)))
        return fail(VBC_INVALID_ARG, "alpha and beta must be integers on an integer handle (InexactError)");
    if (mem != VBC_MEM_DEVICE && mem != VBC_MEM_HOST)
        return fail(VBC_INVALID_ARG, "mem must be VBC_MEM_DEVICE or VBC_MEM_HOST");
    const bool direct_x = x_dtype == cdt && (incx == 1 || nx <= 1);
    const bool direct_y = y_dtype == cdt && (incy == 1 || ny <= 1);
    if (direct_x && direct_y) return vbc_mul(h, trans, x, nx, y, ny, alpha, beta, mem, stream, flags);
    const int64_t esz = h->esz;
    if (mem == VBC_MEM_HOST) {  // convert on the host, then the contiguous host path
        std::vector<char> xs, ys((size_t)std::max<int64_t>(ny, 1) * esz);
        const void *xp = x;
        if (!direct_x) {
            xs.resize((size_t)std::max<int64_t>(nx, 1) * esz);
            host_convert_to(x, x_dtype, nx, incx, xs.data(), cdt);
            xp = xs.data();
        }
        if (beta != 0.0) host_convert_to(y, y_dtype, ny, incy, ys.data(), cdt);
        if (int st = vbc_mul(h, trans, xp, nx, ys.data(), ny, alpha, beta, mem, stream, flags)) return st;
        host_store(ys.data(), cdt, ny, y, y_dtype, incy);
        return VBC_OK;
    }
    // device operands: conversion kernels into / out of the handle's staging buffers
    apply_quirks(trans, flags, alpha, beta);
    DeviceGuard g(h->device);
    if (!g.ok) return fail(VBC_HIP_ERROR, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(h->mu);
    ProductOrder po(h, s, true);
    void *dx = const_cast<void *>(x), *dy = y;
    if (!direct_x) {
        if (int st = stage_buffer(h, 0, nx * esz, s, &dx)) return st;
    }
    if (!direct_y) {
        if (int st = stage_buffer(h, 1, ny * esz, s, &dy)) return st;
    }
    if (int st = po.begin()) return st;
    if (!direct_x) {
        if (int st = convert_gather(x, x_dtype, incx, dx, cdt, nx, s)) return st;
    }
    if (!direct_y && beta != 0.0) {
        if (int st = convert_gather(y, y_dtype, incy, dy, cdt, ny, s)) return st;
    }
    if (int st = mul_dispatch(h, trans, dx, dy, alpha, beta, s)) return st;
    if (!direct_y) {
        if (int st = convert_scatter(dy, cdt, y, y_dtype, incy, ny, s)) return st;
    }
    return po.end();
}

int vbc_mul_mat_ex(vbc_handle *h, int trans, int64_t nrhs, const void *X, int X_dtype, int64_t ldx, int64_t nx,
                   void *Y, int Y_dtype, int64_t ldy, int64_t ny, double alpha, double beta, int mem, void *stream,
                   unsigned flags)
{
    if (!h) return fail(VBC_INVALID_ARG, "NULL handle");
    if (!known_dtype(X_dtype) || !known_dtype(Y_dtype)) return fail(VBC_UNSUPPORTED_DTYPE, "unknown eltype");
    if (X_dtype != h->dtype || Y_dtype != h->dtype)
        return fail(VBC_UNSUPPORTED_DTYPE, "the matrix product takes X and Y of the handle's compute eltype "
                                           "(other eltypes: vbc_mul_ex column by column)");
    return vbc_mul_mat(h, trans, nrhs, X, ldx, nx, Y, ldy, ny, alpha, beta, mem, stream, flags);
}

// ---------------------------------------------------------------------------------------------
// Value updates of a handle with an unchanged pattern (VBC_CREATE_UPDATABLE)
// ---------------------------------------------------------------------------------------------

int vbc_update_values(vbc_handle *h, const void *val, int64_t nval, int val_dtype, int mem, void *stream)
{
    if (!h) return fail(VBC_INVALID_ARG, "NULL handle");
    if (!h->updatable) return fail(VBC_INVALID_ARG, "handle created without VBC_CREATE_UPDATABLE");
    if (!known_dtype(val_dtype)) return fail(VBC_UNSUPPORTED_DTYPE, "unknown val_dtype");
    if (h->umap.mixed && val_dtype != VBC_F32)  // a Float64 val would be rounded in the narrow buckets only
        return fail(VBC_UNSUPPORTED_DTYPE, "a handle created with VBC_CREATE_NARROW_UPDATABLE takes val_dtype VBC_F32 only "
                                           "(its narrow buckets store Float32, its wide ones the same values widened)");
    if (h->dtype == VBC_I64 && is_float(val_dtype))
        return fail(VBC_UNSUPPORTED_DTYPE, "floating-point values on an integer handle (InexactError)");
    if (nval < h->nval) return fail(VBC_DIM_MISMATCH, "DimensionMismatch: val shorter than at create");
    if (h->nval > 0 && !val) return fail(VBC_INVALID_ARG, "NULL val");
    if (mem != VBC_MEM_DEVICE && mem != VBC_MEM_HOST)
        return fail(VBC_INVALID_ARG, "mem must be VBC_MEM_DEVICE or VBC_MEM_HOST");
    if (h->nval == 0) return VBC_OK;
    DeviceGuard g(h->device);
    if (!g.ok) return fail(VBC_HIP_ERROR, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    if (mem == VBC_MEM_DEVICE) return update_launch(h, val, val_dtype, s);  // one kernel, ordered by the stream
    // host val: through the x staging buffer, in the handle's product order (a product on another stream
    // may be reading that buffer)
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t bytes = (size_t)h->nval * elem_size(val_dtype);
    void *dv = nullptr;
    if (int st = stage_buffer(h, 0, bytes, s, &dv)) return st;
    ProductOrder po(h, s, true);
    if (int st = po.begin()) return st;
    if (hipMemcpyAsync(dv, val, bytes, hipMemcpyHostToDevice, s) != hipSuccess)
        return fail(VBC_HIP_ERROR, "staging copy of val failed");
    if (int st = update_launch(h, dv, val_dtype, s)) return st;
    if (int st = po.end()) return st;
    if (hipStreamSynchronize(s) != hipSuccess) return fail(VBC_HIP_ERROR, "hipStreamSynchronize failed");
    return VBC_OK;
}

}  // extern "C"
