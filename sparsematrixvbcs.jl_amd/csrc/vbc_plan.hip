// The layout planner's entry (vbc_plan.h plan_layout) and its per-direction planners: the transposed layout
// (build_transposed, with the fused small-matrix split and its long-stripe cut, build_ksplit), the forward layouts
// (build_forward and its row-run, lane-stream and lane-pair forms) and the integer layout (plan_int).  The
// per-bucket builders are vbc_plan_bins.hip, the panel layouts and C = Bᵀ vbc_plan_panel.hip.  Pure host code: no
// HIP call, no environment.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <vector>

#include "vbc_plan_impl.h"
#include "vbc_planar.h"

namespace vbc {

// Whether every value of an fp64 array is a widened Float32 (NaNs included), so that storing it as a
// float and widening it again gives the same bits.
static bool all_float_exact(const char *val, int64_t n)
{
    const double *d = reinterpret_cast<const double *>(val);
    for (int64_t i = 0; i < n; i++) {
        const double back = (double)(float)d[i];
        if (std::memcmp(&back, &d[i], 8) != 0) return false;
    }
    return true;
}

static int check_limits(const Stripes &s)
{
    if (s.m >= (int64_t(1) << 31) || s.n >= (int64_t(1) << 31))
        return fail(VBC_INVALID_ARG, "m and n must be < 2^31 on the GPU path");
    for (int32_t w : s.w)
        if (w > 64) return fail(VBC_UNSUPPORTED_DTYPE, "stripe width > 64 is not supported on the GPU path");
    return VBC_OK;
}

// Stored width of a transposed bucket.  Widths whose rows do not split into 16-B lane vectors
// with a power-of-two slot count (w = 3, 5, 6, 7) run the shuffle-scan path with 4-8-B loads; padding
// them with zero columns buys 16-B loads and the DPP scan for 14-60 % more value bytes.  The padding
// columns multiply x[row] by 0 into outputs that are never written (the forward product, which would
// gather x beyond the stripe, is never padded).  VBC_PAD="w:wp,..." overrides (A/B).
static int padded_width(const PlanCtx *h, int w)
{
    static const int def64[9] = {0, 1, 2, 4, 4, 5, 6, 8, 8};
    static const int def32[9] = {0, 1, 2, 4, 4, 5, 8, 8, 8};
    int wp = w <= 8 ? (h->esz == 8 ? def64[w] : def32[w]) : w;
    if (h->pad_set) wp = (w <= 64 && h->pad_w[w]) ? h->pad_w[w] : w;
    return wp;
}

// Runs with holes (SlotBin::holes) for a bucket of the fused small-matrix split: when the stripes' rows do
// not all come in aligned runs of R consecutive rows (slot_runs) but grouping every stripe's rows by
// row / R adds at most kHoleFill padding rows, each group becomes a whole run of R entries -- the absent
// rows with voff = -1 (zero values; their x is taken as 0 by the kernel, so a non-finite x of a row the
// stripe does not store never reaches it, as in the reference).  One key and one R-wide x gather per
// run instead of one per row.  Fills hents / hsbeg (empty: no runs worth it).
constexpr double kHoleFill = 0.15;
static void hole_runs(const PlanCtx *h, const Stripes &s, const std::vector<int64_t> &stripes, int w,
                      std::vector<Entry> &hents, std::vector<int64_t> &hsbeg)
{
    hents.clear();
    hsbeg.clear();
    if (h->slot_runs == 0 || s.m >= (int64_t)kHoleIdx - 3) return;
    int64_t real = 0;
    for (int64_t l : stripes) real += s.rbeg[l + 1] - s.rbeg[l];
    if (real == 0) return;
    for (int R = 3; R >= 2; R--) {
        int64_t expanded = 0;
        bool exact = true, past = false;
        for (int64_t l : stripes) {
            int64_t prev = -1, groups = 0;
            for (int64_t r = s.rbeg[l]; r < s.rbeg[l + 1]; r++) {
                const int64_t k = s.rows[r] / R;
                if (k != prev) { groups++; prev = k; }
                // the kernels gather a run's R x values with one unconditional R-wide load: a run whose
                // last row lies past the operand (m % R != 0) would read beyond x's allocation
                past = past || k * R + R > s.m;
            }
            expanded += groups * R;
            exact = exact && groups * R == s.rbeg[l + 1] - s.rbeg[l];
        }
        if (exact) return;  // whole runs already: slot_runs finds them
        if (past || (double)(expanded - real) > kHoleFill * (double)real) continue;
        hsbeg.assign(1, 0);
        hents.reserve(expanded);
        for (int64_t l : stripes) {
            for (int64_t r = s.rbeg[l]; r < s.rbeg[l + 1];) {
                const int64_t k = s.rows[r] / R;
                for (int d = 0; d < R; d++) {
                    const int64_t row = k * R + d;
                    if (r < s.rbeg[l + 1] && s.rows[r] == row) {
                        hents.push_back({(uint32_t)row, s.voff[l] + (r - s.rbeg[l]) * s.vstride(l)});
                        r++;
                    } else {
                        hents.push_back({(uint32_t)row, -1});  // a hole of the run
                    }
                }
            }
            hsbeg.push_back((int64_t)hents.size());
        }
        if (h->verbose)
            fprintf(stderr, "[vbc] runs with holes: w %d R %d rows %lld -> %lld\n", w, R, (long long)real,
                    (long long)expanded);
        return;
    }
}

// Long stripes of the fused split cut into ks parts (SlotBin::ks): each stripe's rows split at run
// boundaries into ks parts of equal run counts (the last may be shorter), the stripes by decreasing
// length, 64 / ks of them per chunk, part p of the chunk's stripe i in lane p * (64 / ks) + i; lanes past
// the last stripe hold empty segments.  ents[sbeg[q] ..] are stripe q's rows, out[q] its first column.
static int build_ksplit(PlanCtx *h, int w, int ks, const std::vector<Entry> &ents, const std::vector<int64_t> &sbeg,
                        const std::vector<int32_t> &out, int64_t total, const char *val, Arena &ar, int &range0,
                        PendingSlot &ps)
{
    const int64_t n = (int64_t)sbeg.size() - 1, m = 64 / ks;
    const int R = slot_runs(h, ents, sbeg);
    std::vector<int64_t> sx{0};  // segment bounds in ents order: stripe q's part p is segment q * ks + p
    std::vector<int32_t> ox;
    for (int64_t q = 0; q < n; q++) {
        const int64_t runs = (sbeg[q + 1] - sbeg[q]) / R, per = (runs + ks - 1) / ks;
        for (int p = 0; p < ks; p++) {
            sx.push_back(sbeg[q] + std::min<int64_t>(runs, (p + 1) * per) * R);
            ox.push_back(out[q]);
        }
    }
    const int64_t nchk = (n + m - 1) / m;
    for (int64_t t = n; t < nchk * m; t++)  // empty segments: stripe slots t >= n of the last chunk
        for (int p = 0; p < ks; p++) {
            sx.push_back(sx.back());
            ox.push_back(-1);
        }
    std::vector<int64_t> byl(n);
    for (int64_t q = 0; q < n; q++) byl[q] = q;
    std::stable_sort(byl.begin(), byl.end(),
                     [&](int64_t a, int64_t b) { return sbeg[a + 1] - sbeg[a] > sbeg[b + 1] - sbeg[b]; });
    std::vector<int64_t> order((size_t)(nchk * 64));
    for (int64_t c = 0; c < nchk; c++)
        for (int p = 0; p < ks; p++)
            for (int64_t i = 0; i < m; i++) {
                const int64_t t = c * m + i;
                order[c * 64 + p * m + i] = (t < n ? byl[t] : t) * ks + p;
            }
    if (h->verbose)
        fprintf(stderr, "[vbc] long stripes: w %d, %lld stripes cut into %d parts (runs of %d), %lld chunks\n", w,
                (long long)n, ks, R, (long long)nchk);
    return build_slots(h, 0, w, w, ents, sx, ox, total, val, ar, range0, ps, order, false, ks);
}

// Column pieces (B'x layouts only): when one width wd holds >= 80 % of the stripes, a side stripe whose
// width is a multiple k·wd runs as k wd-wide stripes over the same stored rows (values addressed in
// place through Stripes::vst).  The ldoor stand-in's 'min memory' partition is 317,337 3-wide stripes
// and 32 6-wide ones: as two buckets, the 6-wide one is a single chunk whose wave walks 51 rows of
// dependent loads at the loaded-memory latency of the streaming bucket beside it (42.6 us against the
// strict partition's 33.8 us, profiles/r04_ab11_ldoor32_*.log).  Every output column keeps its
// stripe's rows in stored order, so each column is summed exactly as before (multiply_1DVBC.jl:101-104).
static bool column_pieces(const PlanCtx *h, const Stripes &s, Stripes &c)
{
    if (h->colsplit == 0 || s.L < 1) return false;
    std::map<int, int64_t> cnt;
    for (int64_t l = 0; l < s.L; l++) cnt[s.w[l]]++;
    int wd = 0;
    int64_t nd = 0;
    for (auto &kv : cnt)
        if (kv.second > nd) { nd = kv.second; wd = kv.first; }
    // VBC_COLSPLIT_W=c (A/B): every stripe wider than c as pieces of c columns (+ the remainder)
    const int cw = h->colsplit_w;
    bool any = false;
    if (cw > 0) {
        wd = cw;
        for (auto &kv : cnt) any = any || kv.first > cw;
    } else {
        if (cnt.size() < 2 || (double)nd < 0.8 * (double)s.L) return false;
        for (auto &kv : cnt) any = any || (kv.first > wd && kv.first % wd == 0);
    }
    if (!any) return false;
    c.m = s.m;
    c.n = s.n;
    c.grp = s.grp;
    c.rbeg.assign(1, 0);
    for (int64_t l = 0; l < s.L; l++) {
        const int wl = s.w[l];
        const bool cut = wl > wd && (cw > 0 || wl % wd == 0);
        for (int c0 = 0; c0 < wl; c0 += cut ? wd : wl) {
            const int wp = cut ? std::min(wd, wl - c0) : wl;
            c.col0.push_back(s.col0[l] + c0);
            c.w.push_back(wp);
            c.voff.push_back(s.voff[l] + c0);
            c.vst.push_back((int32_t)s.vstride(l));
            c.rows.insert(c.rows.end(), s.rows.begin() + s.rbeg[l], s.rows.begin() + s.rbeg[l + 1]);
            c.rbeg.push_back((int64_t)c.rows.size());
        }
    }
    c.L = (int64_t)c.w.size();
    if (h->verbose)
        fprintf(stderr, "[vbc] column pieces: %lld stripes -> %lld (dominant width %d)\n", (long long)s.L,
                (long long)c.L, wd);
    return true;
}

// Transposed layout: segments = stripes of each width, entries = their stored rows.  A bucket runs
// slotted (vbc_slots.h, every stripe of the width a segment, empty ones included) when its row counts
// are near-uniform, else merged (non-empty stripes; empty ones go to the fill list).
static int build_transposed(PlanCtx *h, const Stripes &s0, const char *val, Arena &ar, LaunchPlan &plan,
                            std::vector<int32_t> &fill)
{
    Stripes sp;
    const Stripes &s = column_pieces(h, s0, sp) ? sp : s0;
    std::map<int, std::vector<int64_t>> buckets;  // w -> stripes
    for (int64_t l = 0; l < s.L; l++) buckets[s.w[l]].push_back(l);
    const int64_t total = (int64_t)s.rows.size();
    int range0 = 0, srange0 = 0, tile0 = 0;
    // Small matrices with several width buckets (a SuiteSparse operator's strict stripes: ct20stif's are
    // 1..6 wide; filled / mixed partitions): every bucket planar (any width 1..8, one stripe per lane)
    // and split, P waves per 64-stripe chunk, all buckets in ONE launch (Launch::fuse_split) -- instead
    // of a slotted launch, one launch per planar bucket and the merge kernel for the buckets whose
    // chunks are too long to balance one wave each.  Taken when the chunks of all buckets together fill
    // at most half the wave slots (the split rule of build_slots) and every chunk keeps >= split_rows
    // (fp64) rows per wave; P is common to the launch.  VBC_SMALL_FUSE=0 turns it off.
    h->st.small_split = 0;
    h->st.fuse_w = 0;
    // A single-width small matrix runs the fused split when its bucket would otherwise take the merge
    // layout (chunks too long to balance one wave each: the 3dtube stand-in's 'overlap' partition, 15,110
    // 3-wide stripes of ~71 rows, fp64 16.4 -> 7.8 us, fp32 14.2 -> 6.8 us); a bucket the planar layouts
    // take keeps them (ldoor's 1/8 stripe shard: masked planar 12.4 us, fused 14.3 us,
    // profiles/r04_ab13_*.log, r04_ab15_*.log).  VBC_SMALL_FUSE=2 fuses every single-width one.
    // (a bucket headed for the merge layout: no slotted / planar layout balances its chunks)
    auto merge_bound = [&](int w, const std::vector<int64_t> &stripes) {
        if (w > 8 || sweep_possible(h, w, s.m)) return false;
        const int wps = slot_planar(h, 0, w) ? w : (h->esz == 8 && w == 3) ? 3 : padded_width(h, w);
        std::vector<int64_t> sb{0}, order;
        for (int64_t l : stripes) sb.push_back(sb.back() + s.rbeg[l + 1] - s.rbeg[l]);
        bool mask = false;
        return want_slots(h, 0, wps, sb, total, s.m, order, &mask, w) == 0;
    };
    int fuse_min = h->small_fuse >= 2 ? 1 : 2;
    if (fuse_min == 2 && h->small_fuse == 1 && buckets.size() == 1 && merge_bound(buckets.begin()->first, buckets.begin()->second))
        fuse_min = 1;
    // Long stripes (SlotBin::ks): a chunk runs on one CU and costs its longest stripe's rows, so a few
    // chunks of long stripes (a 'min blocks' partition's widest, fullest stripes: 3.4x the mean chunk on
    // the ct20stif stand-in) set the product's time.  A stripe whose work (rows x width, values per
    // lane) exceeds ksplit x the mean chunk's is cut into 2 (4 above twice that) parts of whole runs,
    // laid side by side in the lanes of one chunk and summed across them before the store.
    std::vector<uint8_t> kst;  // per stripe: parts (empty: none cut)
    // (auto layouts only: a forced VBC_SLOTS / VBC_SLOT_PLANAR keeps the layout the tests ask for)
    if (h->planar_split != 0 && h->small_fuse != 0 && h->slot_planar < 0 && h->slots_mode < 0 && (int)buckets.size() >= fuse_min &&
        (int)buckets.size() <= kSplitParts && buckets.rbegin()->first <= 8 && !sweep_possible(h, 1, s.m)) {
        // the fused buckets: all of them; or, when their chunks would overflow the launch and one bucket
        // holds most of them, every bucket but that one (a large operator's dominant width keeps its
        // streaming layout, and its small side buckets -- a time-model partition's few 1-, 4- and 5-wide
        // stripes beside 305,000 3-wide ones -- run as one fused launch instead of one launch each)
        const double slots0 = (double)h->target_ranges_p;
        int64_t nall = 0, nmax = 0;
        int wmax = 0;
        for (auto &kv : buckets) {
            const int64_t c = ((int64_t)kv.second.size() + 63) / 64;
            nall += c;
            if (c > nmax) { nmax = c; wmax = kv.first; }
        }
        for (auto &kv : buckets) h->st.fuse_w |= 1u << kv.first;
        // a dominant bucket headed for the merge layout is better fused too, up to one chunk per wave slot
        // (the ldoor stand-in's fp64 'min blocks', 2,358 chunks of 6-wide stripes of 69 rows: merge kernel
        // 131.5 us + the fused side launch 11.5 us; all fused 131.5 us, profiles/r04_ab17_ldoor64_blocks.log)
        const bool dom_merge = h->side_fuse < 0 && (double)nmax >= 0.8 * (double)nall && (double)nall <= slots0 &&
                               merge_bound(wmax, buckets[wmax]);
        const bool side = h->side_fuse < 0 ? (double)nall * 2 > slots0 && buckets.size() >= 3 && (double)nmax >= 0.8 * (double)nall && !dom_merge
                                           : h->side_fuse == 1 && (double)nmax >= 0.8 * (double)nall;
        if (side) h->st.fuse_w &= ~(1u << wmax);
        auto fused_w = [&](int w) { return ((h->st.fuse_w >> w) & 1) != 0; };
        if (h->ksplit > 0) {
            double work = 0;
            int64_t nw = 0;
            for (auto &kv : buckets) {  // chunks of the length-sorted buckets
                if (!fused_w(kv.first)) continue;
                std::vector<int64_t> len;
                for (int64_t l : kv.second) len.push_back(s.rbeg[l + 1] - s.rbeg[l]);
                std::sort(len.begin(), len.end(), std::greater<int64_t>());
                for (size_t i = 0; i < len.size(); i += 64, nw++) work += (double)len[i] * kv.first;
            }
            // never below a CU's share of the whole: with many chunks per CU (the ldoor stand-in's 'min
            // blocks', 2550 chunks) a long chunk is averaged out, and cutting only adds chunks (70 -> 107 us)
            const double thr = std::max(h->ksplit * work / (double)std::max<int64_t>(nw, 1), work / (double)h->cus);
            kst.assign(s.L, 1);
            int parts = 0, cut = 0;
            for (auto &kv : buckets) {
                if (!fused_w(kv.first)) continue;
                int cls = 0;
                for (int64_t l : kv.second) {
                    const double wk = (double)(s.rbeg[l + 1] - s.rbeg[l]) * kv.first;
                    kst[l] = wk > 2 * thr ? 4 : wk > thr ? 2 : 1;
                    cls |= kst[l];
                }
                parts += __builtin_popcount(cls);
                cut += cls > 1;
            }
            if (parts > kSplitParts || cut == 0 || !(thr > 0)) kst.clear();
        }
        int64_t nch = 0, rows = 0;
        int nf = 0;
        for (auto &kv : buckets) {
            if (!fused_w(kv.first)) continue;
            nf++;
            int64_t cnt[5] = {0, 0, 0, 0, 0};
            for (int64_t l : kv.second) {
                cnt[kst.empty() ? 1 : kst[l]]++;
                rows += s.rbeg[l + 1] - s.rbeg[l];
            }
            for (int k = 1; k <= 4; k *= 2) nch += (cnt[k] * k + 63) / 64;
        }
        const double slots = (double)h->target_ranges_p;
        const double avg = (double)rows / (double)std::max<int64_t>(nch, 1) / 64.0 * 1.1;  // rows per chunk (sorted)
        // (the batched slice loop costs a round trip per batch, not per step: thinner slices than the
        // single-bucket rule's split_rows pay off -- ct20stif 'min blocks' P = 4 / 8: 15.7 / 14.7 us)
        const double minrows = (double)h->small_rows * h->esz / 8.0;
        if ((double)nch * (dom_merge ? 1 : 2) <= slots && nf >= fuse_min) {
            int P = 1;
            while (P < h->fuse_pmax && (double)nch * P * 2 <= 2 * slots && avg / (P * 2) >= minrows) P *= 2;
            // fusing pays even when the chunks are too short to split: one launch instead of one per
            // bucket (the thermal1 stand-in's 'min blocks', 8 buckets of 16-row chunks: 41 us unfused)
            P = std::max(P, 2);
            // many chunks (more waves than one round of the chip): P that fills whole rounds of resident
            // waves -- the ldoor stand-in's 'min blocks', 2550 chunks: P = 2 / 4 / 8 give 1.25 / 2.5 / 5.0
            // rounds of 4096 fp32 waves (70.9 / 70.1 / 66.0 us, profiles/r04_ab7_ldoor32_blocks.log)
            auto rounds = [&](int p) {
                const double cap = (double)h->cus * std::max(1, h->occ_multi[p == 2 ? 1 : p == 4 ? 2 : 3]);
                return (double)nch * p / cap;
            };
            if (rounds(P) > 1.0) {
                auto eff = [&](int p) { const double r = rounds(p); return r / std::ceil(r); };
                for (int p = 2; p <= h->fuse_pmax; p *= 2)
                    if (eff(p) > eff(P) + 0.05) P = p;
            }
            if (h->planar_split > 1) P = h->planar_split;
            if (P > 1) h->st.small_split = P;
        }
        if (h->st.small_split <= 1) {
            kst.clear();
            h->st.fuse_w = 0;
        }
        if (h->verbose)
            fprintf(stderr, "[vbc] small fused split: %d of %d buckets (width mask 0x%x), %lld chunks, %.1f rows per "
                    "chunk -> P = %d%s\n", nf, (int)buckets.size(), h->st.fuse_w, (long long)nch, avg, h->st.small_split,
                    kst.empty() ? "" : ", long stripes cut");
    }
    // the bins: a width bucket, or (long stripes cut) its stripes of each part count ks
    std::vector<std::pair<int, std::vector<int64_t>>> subs;
    std::vector<int> subk;
    for (auto &kv : buckets) {
        if (kst.empty()) {
            subs.emplace_back(kv.first, std::move(kv.second));
            subk.push_back(1);
            continue;
        }
        for (int k = 1; k <= 4; k *= 2) {
            std::vector<int64_t> v;
            for (int64_t l : kv.second)
                if (kst[l] == k) v.push_back(l);
            if (v.empty()) continue;
            subs.emplace_back(kv.first, std::move(v));
            subk.push_back(k);
        }
    }
    for (size_t si = 0; si < subs.size(); si++) {
        const auto &kv = subs[si];
        const int ks = subk[si];
        const int w = kv.first;
        if (sweep_possible(h, w, s.m)) {
            std::vector<int64_t> sb{0};
            std::vector<Entry> ents;
            std::vector<int32_t> out;
            ents.reserve(s.rbeg[s.L] - s.rbeg[0]);
            for (int64_t l : kv.second) {
                sb.push_back(sb.back() + s.rbeg[l + 1] - s.rbeg[l]);
                out.push_back((int32_t)s.col0[l]);
                for (int64_t r = s.rbeg[l]; r < s.rbeg[l + 1]; r++)
                    ents.push_back({(uint32_t)s.rows[r], s.voff[l] + (r - s.rbeg[l]) * s.vstride(l)});
            }
            if (want_sweep(h, w, s.m, sb, ents)) {
                PendingSweep pw;
                if (int st = build_sweep(h, 0, w, sb, ents, out, val, ar, tile0, pw)) return st;
                pw.work = (double)ents.size() * (4.0 + (double)w * h->esz);
                plan.sweeps.push_back(pw);
                continue;
            }
        }
        const int wp = padded_width(h, w);
        // the slotted kernel has no scan to feed: fp64 w = 3 runs unpadded (8-B lanes), measured
        // 117 -> 106 us on the ldoor stand-in (fp32 keeps 3 -> 4: 73 vs 84 us unpadded)
        const int wps = slot_planar(h, 0, w) ? w : (h->esz == 8 && w == 3 && !h->pad_set) ? 3 : wp;
        std::vector<int64_t> sbeg{0}, order;
        for (int64_t l : kv.second) sbeg.push_back(sbeg.back() + s.rbeg[l + 1] - s.rbeg[l]);
        bool mask = false;
        // fused small split: rows that ALMOST come in aligned runs (a stiffness operator's dof rows, some
        // stripes missing one of a node's rows -- the structural zeros of ct20stif-like matrices) are
        // padded to whole runs, the absent rows marked in the run's key (hole_runs)
        // Only a bucket of the fused launch takes them: its bins run the split product (build_slots gives a
        // fused bucket split = small_split), the one kernel family that folds absent rows (voff < 0); a
        // side bucket, a lane-stream or an unfused slotted / pair layout keeps the plain rows.
        std::vector<Entry> hents;
        std::vector<int64_t> hsbeg;
        const bool fused_bucket = h->st.small_split > 1 && w <= 8 && ((h->st.fuse_w >> w) & 1) != 0;
        if (fused_bucket && slot_planar(h, 0, w)) hole_runs(h, s, kv.second, w, hents, hsbeg);
        if (!hsbeg.empty()) {
            std::vector<int32_t> out0;
            for (int64_t l : kv.second) out0.push_back((int32_t)s.col0[l]);
            std::vector<int64_t> order0;
            bool mask0 = false;
            if (want_slots(h, 0, wps, sbeg, total, s.m, order0, &mask0, w) && want_lanes(h, wps, w, sbeg, out0, total, mask0)) {
                hents.clear();
                hsbeg.clear();
            }
        }
        const std::vector<int64_t> &sb = hsbeg.empty() ? sbeg : hsbeg;
        if (ks > 1) {  // long stripes of the fused split, cut into ks lane parts
            std::vector<Entry> ents;
            std::vector<int32_t> out;
            for (int64_t l : kv.second) out.push_back((int32_t)s.col0[l]);
            if (!hsbeg.empty()) {
                ents.swap(hents);
                sbeg.swap(hsbeg);
            } else {
                for (int64_t l : kv.second)
                    for (int64_t r = s.rbeg[l]; r < s.rbeg[l + 1]; r++)
                        ents.push_back({(uint32_t)s.rows[r], s.voff[l] + (r - s.rbeg[l]) * s.vstride(l)});
            }
            PendingSlot ps;
            if (int st = build_ksplit(h, w, ks, ents, sbeg, out, total, val, ar, srange0, ps)) return st;
            plan.slots.push_back(std::move(ps));
            continue;
        }
        if (want_slots(h, 0, wps, sb, hsbeg.empty() ? total : total + (hsbeg.back() - sbeg.back()), s.m, order, &mask, w)) {
            std::vector<Entry> ents;
            std::vector<int32_t> out;
            for (int64_t l : kv.second) out.push_back((int32_t)s.col0[l]);
            const bool holes = !hsbeg.empty();
            if (holes) {
                ents.swap(hents);
                sbeg.swap(hsbeg);
            } else {
                ents.reserve(sbeg.back());
                for (int64_t l : kv.second)
                    for (int64_t r = s.rbeg[l]; r < s.rbeg[l + 1]; r++)
                        ents.push_back({(uint32_t)s.rows[r], s.voff[l] + (r - s.rbeg[l]) * s.vstride(l)});
            }
            PendingSlot ps;
            if (!holes && want_lanes(h, wps, w, sbeg, out, total, mask)) {
                if (int st = build_lanes(h, w, ents, sbeg, out, slot_runs(h, ents, sbeg), total, val, ar, ps)) return st;
            } else if (int st = build_slots(h, 0, wps, w, ents, sbeg, out, total, val, ar, srange0, ps, order, mask)) {
                return st;
            }
            plan.slots.push_back(std::move(ps));
            continue;
        }
        std::vector<Entry> ents;
        std::vector<int32_t> out;
        for (int64_t l : kv.second) {
            if (s.rbeg[l + 1] == s.rbeg[l]) {
                for (int c = 0; c < s.w[l]; c++) fill.push_back((int32_t)(s.col0[l] + c));
                continue;
            }
            out.push_back((int32_t)s.col0[l]);
            for (int64_t r = s.rbeg[l]; r < s.rbeg[l + 1]; r++)
                ents.push_back({(uint32_t)s.rows[r] | (r == s.rbeg[l] ? kHead : 0u),
                                s.voff[l] + (r - s.rbeg[l]) * s.vstride(l)});
        }
        if (ents.empty()) continue;
        PendingBin pb;
        if (int st = build_bucket(h, 0, wp, ents, out, total, val, ar, range0, pb, w)) return st;
        h->st.bytes_t += (int64_t)ents.size() * (4 + (int64_t)wp * h->esz) + (int64_t)out.size() * 4;
        pb.work = (double)ents.size() * (4.0 + (double)wp * h->esz);
        plan.bins.push_back(pb);
    }
    commit_launch_keys(h, plan.slots, ar);
    for (const PendingSlot &ps : plan.slots) {  // slotted bins: padded rows x (index bytes + values)
        if (ps.b.lanes) {  // lanes: real rows' values, one key per run, nlive per row, the tile tables
            h->st.bytes_t += ps.real * (int64_t)ps.b.w * (ps.b.vsz ? ps.b.vsz : h->esz) + ps.key_bytes + ps.rows * 4 + (int64_t)ps.b.ntiles * (8 + 128);
        } else if (ps.b.mask) {  // masked: padding lanes fetch nothing; + the per-row live counts
            const double f = (double)ps.real / (double)std::max<int64_t>(1, ps.rows * ps.b.rpi);
            h->st.bytes_t += ps.real * (int64_t)ps.b.w * (ps.b.vsz ? ps.b.vsz : h->esz) + (int64_t)(f * (double)ps.key_bytes) + ps.rows * 4;
        } else {  // (a pair bin's rows are run-rows: 3 rows of every stripe slot, 288 values)
            h->st.bytes_t += ps.rows * ps.b.rpi * (int64_t)ps.b.w * (ps.b.pair ? 3 : 1) * (ps.b.vsz ? ps.b.vsz : h->esz) + ps.key_bytes;
        }
    }
    plan.L.total_ranges = range0;
    plan.L.slot_ranges = srange0;
    plan.L.sweep_tiles = tile0;
    plan.L.fuse_p = h->st.small_split;  // (the handle's field is rebuilt by the next build_transposed call)
    plan.L.sweep_tile_bytes = h->sweep_tile;
    plan.L.sweep_diag = h->sweep_diag;
    h->st.bytes_t += (s.m + s.n) * h->esz;  // x read once, y written once
    return VBC_OK;
}

// Forward row runs (the forward counterpart of slot_runs): the largest R in {3, 2} such that the
// output rows come in aligned runs of R (rows R*q .. R*q+R-1, m divisible by R) with identical stripe
// lists -- the dof rows of a node in a stiffness operator.  sbeg: every row a segment (natural order).
static int fwd_runs(const PlanCtx *h, int w, int64_t m, const std::vector<Entry> &ents,
                    const std::vector<int64_t> &sbeg)
{
    if (h->slot_runs == 0 || h->slot_planar == 0 || w < 2 || w > 4 || m <= 0) return 1;
    for (int R = 3; R >= 2; R--) {
        if (m % R || R * w > 12) continue;
        bool ok = true;
        for (int64_t q = 0; q < m && ok; q += R) {
            const int64_t b0 = sbeg[q], len = sbeg[q + 1] - b0;
            for (int r = 1; r < R && ok; r++) {
                const int64_t br = sbeg[q + r];
                if (sbeg[q + r + 1] - br != len) { ok = false; break; }
                for (int64_t k = 0; k < len; k++)
                    if ((ents[br + k].key & kSlotIdx) != (ents[b0 + k].key & kSlotIdx)) { ok = false; break; }
            }
        }
        if (ok) return R;
    }
    return 1;
}

// Planar forward bin (vbc_planar.h run_planar_fwd): segment q = output rows R*q .. R*q+R-1, one per
// lane, 64 per chunk; chunk row k = the k-th block (stripe) of each segment, its R x w values stored
// column-group-major over the chunk (planar_off with width R*w, element r*w + c); one key per block =
// the stripe's first column (the gathered x slice).  Natural order: y offsets affine (R*q).
// Returns false (and builds nothing) when the padded rows exceed slots_pad x the real ones.
static bool build_fwd_runs(PlanCtx *h, int w, int R, const std::vector<Entry> &ents, const std::vector<int64_t> &sbeg,
                           int64_t m, const char *val, Arena &ar, int &range0, PendingSlot &ps)
{
    const int esz = h->esz, RPI = 64, WV = R * w;
    const int64_t nseg = m / R;
    const int64_t nch = (nseg + RPI - 1) / RPI;
    // run-segment lengths; natural order first, else sorted by length in windows of kSortWindow chunks
    // (y offsets from a table then)
    std::vector<int64_t> rb(nseg + 1, 0), order;
    for (int64_t q = 0; q < nseg; q++) rb[q + 1] = rb[q] + sbeg[R * q + 1] - sbeg[R * q];
    const int64_t real = rb[nseg];
    std::vector<int32_t> cr = chunk_rows(rb, RPI);
    int64_t rows = 0;
    for (int32_t c : cr) rows += c;
    if (real == 0) return false;
    bool mask = false;
    // few chunks: natural order for the split product below, unless it pads by more than half
    const bool few = h->planar_split != 0 && (double)nch * 2 <= (double)h->target_ranges_p &&
                     (double)(rows * RPI) <= 1.5 * (double)real;
    if (!few && (double)(rows * RPI) > h->slots_pad * (double)real) {
        if (h->slots_sort == 0) return false;
        if (h->planar_mask != 0) {  // masked chunk-local length order (SlotBin::mask, as the B'x planar bins)
            order = chunk_sorted_order(rb, RPI * h->mask_window);
            cr = chunk_rows(permuted_sbeg(rb, order), RPI);
            rows = 0;
            for (int32_t c : cr) rows += c;
            mask = (double)(rows * RPI) <= kMaskPad * (double)real;
        }
        if (!mask) {
            order = sorted_order(rb, RPI);
            cr = chunk_rows(permuted_sbeg(rb, order), RPI);
            rows = 0;
            for (int32_t c : cr) rows += c;
            if ((double)(rows * RPI) > h->slots_pad * (double)real) return false;
        }
    }
    auto seg_of = [&](int64_t p) { return order.empty() ? p : order[p]; };  // layout position -> run-segment
    // few chunks (natural order): P waves per chunk (spmv_planar_fwd_split), the rule of the B'x split
    // product with its rows counted in values (>= 36 fp64 / 18 fp32 values per lane per wave: 4 blocks
    // of a 3 x 3 node block in fp64)
    int split = 1;
    if (h->planar_split != 0 && order.empty()) {
        const double share = (double)h->target_ranges_p;
        if (h->planar_split > 1) split = h->planar_split;
        else if ((double)nch * 2 <= share) {
            const double avg = (double)rows / (double)std::max<int64_t>(nch, 1);
            const double minrows = std::max(1.0, (double)h->split_rows * 3.0 * esz / 8.0 / WV);
            while (split < 8 && (double)nch * split * 2 <= 2 * share && avg / (split * 2) >= minrows) split *= 2;
        }
    }
    // ranges of >= fwd_min_rows chunk rows: the kernel's two-stage pipeline loads up to 3U rows past a
    // short range's end (clamped duplicates); ldoor's 1/8 stripe shard (4.8 rows per range at 3072
    // ranges) ran 30.8 us, 16.0 us as 1024 ranges (profiles/r03_fwdshard2.log)
    // (the B'x rule of at most planar_wps waves per SIMD does not carry over: ldoor fp32 B·x 34.3 ->
    // 37.9 us with it, profiles/r03_wps_fwd_*.log)
    const int64_t nr = split > 1 ? nch
                                 : std::max<int64_t>(1, std::min<int64_t>({(int64_t)h->target_ranges_p, nch,
                                                                           rows / std::max(1, h->fwd_min_rows)}));
    std::vector<int32_t> rrow{0}, rchunk{0};
    int64_t acc = 0;
    for (int64_t c = 0; c < nch; c++) {
        acc += cr[c];
        if (c + 1 < nch && (split > 1 || ((int64_t)rrow.size() < nr && acc * nr >= (int64_t)rrow.size() * rows))) {
            rrow.push_back((int32_t)acc);
            rchunk.push_back((int32_t)(c + 1));
        }
    }
    rrow.push_back((int32_t)rows);
    if (h->verbose)
        fprintf(stderr, "[vbc] forward runs bin w %d R %d segments %lld chunks %lld rows %lld (real %lld) mask %d sorted %d "
                "split %d ranges %zu\n", w, R, (long long)nseg, (long long)nch, (long long)rows, (long long)real, (int)mask,
                (int)(!order.empty() && !mask), split, rchunk.size());
    ps = PendingSlot{};
    SlotBin &b = ps.b;
    b.kind = 1;
    b.wkey = w;
    b.w = w;
    b.wst = w;
    b.rpi = RPI;
    b.range0 = 0;  // its own launch
    b.nranges = (int32_t)rchunk.size();
    b.nseg = (int32_t)nseg;
    b.u = h->slot_u;
    b.diag = h->diag;
    b.xcd = split > 1 ? 0 : h->xcd_p;
    b.spl = 1;
    b.planar = 1;
    b.run = R;
    b.split = split;
    b.pair = 0;
    b.mask = mask ? 1 : 0;
    b.out_affine = order.empty() ? 1 : 0;
    b.out_base = 0;
    b.out_stride = R;
    b.contig = b.out_affine;
    const int64_t E = rows * RPI;
    ps.rows = rows;
    ps.real = real;
    if (mask) ps.o_nlive = ar.reserve((size_t)rows * 4);
    ps.keys.resize(E);
    // VBC_CREATE_NARROW_PLANAR (build_slots): the non-split bin (spmv_planar_fwd) stores floats, in the Float32
    // column-group arrangement of width R * w; everything above was decided with esz
    const bool narrow = h->narrow_planar && esz == 8 && split == 1;
    const int vsz = narrow ? 4 : esz;
    b.vsz = narrow ? 4 : 0;
    ps.o_val = ar.reserve(E * WV * vsz);
    if (narrow && h->rec) h->rec->narrow.emplace_back(ps.o_val, ps.o_val + (size_t)E * WV * vsz);
    ps.o_out = ar.reserve(std::max<int64_t>(order.size(), 1) * 4);
    for (size_t p = 0; p < order.size(); p++) ar.at<int32_t>(ps.o_out)[p] = (int32_t)(R * order[p]);
    ps.o_rrow = ar.reserve(rrow.size() * 4);
    ps.o_rchunk = ar.reserve(rchunk.size() * 4);
    std::memcpy(ar.at<int32_t>(ps.o_rrow), rrow.data(), rrow.size() * 4);
    std::memcpy(ar.at<int32_t>(ps.o_rchunk), rchunk.data(), rchunk.size() * 4);
    char *vv = ar.at<char>(ps.o_val);
    int64_t row = 0;
    for (int64_t c = 0; c < nch; c++) {
        for (int32_t k = 0; k < cr[c]; k++, row++) {
            const uint32_t last = k + 1 == cr[c] ? kLast : 0u;
            char *rowp = vv + row * RPI * WV * vsz;
            if (mask) {  // live lanes of this chunk row: a prefix in chunk-local length order
                uint32_t nl = 0;
                for (int sl = 0; sl < RPI; sl++) {
                    const int64_t p = c * RPI + sl;
                    if (p < nseg && sbeg[R * seg_of(p)] + k < sbeg[R * seg_of(p) + 1]) {
                        if (nl != (uint32_t)sl) return false;
                        nl++;
                    }
                }
                ar.at<uint32_t>(ps.o_nlive)[row] = nl;
            }
            for (int sl = 0; sl < RPI; sl++) {
                const int64_t p = c * RPI + sl, e = row * RPI + sl;
                const int64_t q = p < nseg ? seg_of(p) : 0;
                const bool real_blk = p < nseg && sbeg[R * q] + k < sbeg[R * q + 1];
                ps.keys[e] = real_blk ? ((ents[sbeg[R * q] + k].key & kSlotIdx) | last) : (kPad | last);
                for (int r = 0; r < R; r++)
                    for (int cc = 0; cc < w; cc++) {
                        char *dst = rowp + planar_off(vsz, WV, sl, r * w + cc) * vsz;
                        if (real_blk && narrow) {
                            narrow_value(h, reinterpret_cast<const double *>(val) + ents[sbeg[R * q + r] + k].voff + cc, dst);
                        } else if (real_blk) {
                            std::memcpy(dst, val + (ents[sbeg[R * q + r] + k].voff + cc) * esz, (size_t)esz);
                        } else {
                            std::memset(dst, 0, (size_t)vsz);
                        }
                    }
            }
        }
    }
    ps.kc_ok = h->slot_keys16 != 0 && (split == 1 || h->split_kc) && slot_keys_compressible(ps.keys, rows, RPI);
    (void)range0;
    return true;
}

// Forward lane streams (VBC_PLANAR_LANES as for B'x): the B'x lane-stream kernel (run_planar_lanes) with
// a node block's rows and columns exchanged.  Segment q = output rows R*q .. R*q+R-1 (the kernel's W = R
// outputs per stripe slot); the k-th block of the segment (stripe j, w columns) is one "run" of w
// consecutive x rows (the kernel's RUN = w, one w-wide gather) whose d-th row holds A[R*q + 0..R-1][j + d],
// so the kernel folds acc[r] += A[R*q + r][j + d] * x[j + d] for d = 0..w-1, blocks in stripe order.
// Chosen where the forward run layout would need the masked order (natural chunks pad beyond
// slots_pad), with few empty segments and >= 256 segments per resident wave -- FE-3D.
static bool want_fwd_lanes(const PlanCtx *h, int w, int R, int64_t m, const std::vector<int64_t> &sbeg)
{
    if (h->planar_lanes == 0 || w < 1 || w > 3 || !slot_planar(h, 0, R) || m % R) return false;
    const int64_t nseg = m / R;
    if (nseg < 64 || nseg >= (int64_t(1) << 31)) return false;
    if (h->planar_lanes == 1) return true;
    std::vector<int64_t> rb(nseg + 1, 0);
    int64_t empty = 0;
    for (int64_t q = 0; q < nseg; q++) {
        rb[q + 1] = rb[q] + sbeg[R * q + 1] - sbeg[R * q];
        empty += sbeg[R * q + 1] == sbeg[R * q];
    }
    int64_t rows = 0;
    for (int32_t c : chunk_rows(rb, 64)) rows += c;
    if ((double)(rows * 64) <= h->slots_pad * (double)rb[nseg] || empty * 100 > nseg) return false;
    return (double)nseg >= 256.0 * std::max(1, h->target_ranges_l);
}

static int build_fwd_lanes(PlanCtx *h, int w, int R, const std::vector<Entry> &ents, const std::vector<int64_t> &sbeg,
                           int64_t m, const char *val, Arena &ar, PendingSlot &ps)
{
    const int esz = h->esz;
    const int64_t nseg = m / R;
    std::vector<int64_t> sb(nseg + 1, 0);
    for (int64_t q = 0; q < nseg; q++) sb[q + 1] = sb[q] + (sbeg[R * q + 1] - sbeg[R * q]) * w;
    std::vector<Entry> e2((size_t)sb[nseg]);
    std::vector<char> tv((size_t)sb[nseg] * R * esz);  // the blocks transposed: [block][d][r]
    for (int64_t q = 0; q < nseg; q++) {
        const int64_t nb = sbeg[R * q + 1] - sbeg[R * q];
        for (int64_t k = 0; k < nb; k++) {
            const uint32_t col = ents[sbeg[R * q] + k].key & kSlotIdx;
            for (int d = 0; d < w; d++) {
                const int64_t i = sb[q] + k * w + d;
                e2[i] = {col + (uint32_t)d, i * R};
                for (int r = 0; r < R; r++)
                    std::memcpy(tv.data() + (i * R + r) * esz, val + (ents[sbeg[R * q + r] + k].voff + d) * esz, (size_t)esz);
            }
        }
    }
    std::vector<int32_t> out(nseg);
    for (int64_t q = 0; q < nseg; q++) out[q] = (int32_t)(R * q);
    return build_lanes(h, R, e2, sb, out, w, sb[nseg], tv.data(), ar, ps);
}

// Forward lane pairs (round 6): fp64 3 x 3 node blocks (w = 3 stripes, output rows in runs of R = 3) in the
// lane-pair layout of the B'x product (run_pair) with every block TRANSPOSED -- a "stripe" of that layout is
// an output node run q (rows 3q .. 3q+2), its runs the node's blocks in stripe order, a run's 3 "rows" the
// block's columns d gathering x[j + d] -- folded in DOT mode (SlotBin::dot: each output row's dot product with
// the block's x slice added per block, the reference's forward association, multiply_1DVBC.jl:34, :62-71).
// The forward row-run layout (build_fwd_runs) gathers a 24-B x slice per lane per block in two requests; the
// lane pair shares one 16-B gather per lane (ldoor stand-in fp64: its B'x in this layout runs 0.81 of the
// HBM roofline, the forward row runs 0.69).  Returns kBuildDeclined (nothing built) when the bucket would not
// take the pair layout (too few blocks per node, or a small matrix that takes the split product).
static int build_fwd_pair(PlanCtx *h, int w, int R, const std::vector<Entry> &ents, const std::vector<int64_t> &sbeg,
                          int64_t m, int64_t n, const char *val, Arena &ar, PendingSlot &ps)
{
    if (h->esz != 8 || w != 3 || R != 3 || h->planar_pair == 0 || h->slot_planar == 0 || h->slot_runs == 0 || m % R)
        return kBuildDeclined;
    const int esz = h->esz;
    const int64_t nseg = m / R;
    std::vector<int64_t> sb(nseg + 1, 0);
    for (int64_t q = 0; q < nseg; q++) sb[q + 1] = sb[q] + (sbeg[R * q + 1] - sbeg[R * q]) * w;
    if (sb[nseg] == 0 || sb[nseg] >= (int64_t(1) << 31)) return kBuildDeclined;
    std::vector<Entry> e2((size_t)sb[nseg]);
    std::vector<char> tv((size_t)sb[nseg] * R * esz);  // the blocks transposed: [block][d][r]
    for (int64_t q = 0; q < nseg; q++) {
        const int64_t nb = sbeg[R * q + 1] - sbeg[R * q];
        for (int64_t k = 0; k < nb; k++) {
            const uint32_t col = ents[sbeg[R * q] + k].key & kSlotIdx;
            for (int d = 0; d < w; d++) {
                const int64_t i = sb[q] + k * w + d;
                e2[i] = {col + (uint32_t)d, i * R};
                for (int r = 0; r < R; r++)
                    std::memcpy(tv.data() + (i * R + r) * esz, val + (ents[sbeg[R * q + r] + k].voff + d) * esz, (size_t)esz);
            }
        }
    }
    std::vector<int32_t> out(nseg);
    for (int64_t q = 0; q < nseg; q++) out[q] = (int32_t)(R * q);
    std::vector<int64_t> order;
    bool mask = false;
    if (!want_slots(h, 0, w, sb, sb[nseg], n, order, &mask, w)) return kBuildDeclined;
    int zero = 0;
    const int st = build_slots(h, 0, w, w, e2, sb, out, sb[nseg], tv.data(), ar, zero, ps, order, mask, 1, true);
    if (st == VBC_OK) ps.b.dot = 1;
    return st;
}

// Forward layout: per width bucket, segments = output rows with entries of that width (ascending),
// entries = (row, stripe) blocks ordered by stripe within the row.  With a single bucket, a slotted
// layout takes every row as a segment (affine, no fill list).
// Whether the forward product is built as the transposed product of C = Bᵀ (transpose_stripes): stripes
// of two or more widths (the forward layouts would need a scale pass plus one launch per width, each
// adding into y), at most 2^23 stored rows, float eltypes, not VBC_CREATE_SERIAL (C sums each output over
// B's columns in ascending order, not stripe by stripe), VBC_FWD_T != 0.
static bool fwd_via_t_wanted(const PlanCtx *h, const Stripes &s, unsigned flags)
{
    if (h->fwd_t == 0 || (flags & VBC_CREATE_SERIAL) || h->dtype == VBC_I64) return false;
    // a forced layout family (VBC_SLOTS / VBC_SWEEP / VBC_SLOT_PLANAR) keeps the forward layouts the tests ask for
    if (h->fwd_t != 2 && (h->slots_mode >= 0 || h->sweep_mode >= 0 || h->slot_planar >= 0)) return false;
    if ((int64_t)s.rows.size() > (int64_t(1) << 23)) return false;
    int w0 = -1;
    bool mixed = false;
    for (int64_t l = 0; l < s.L && !mixed; l++) {
        if (s.rbeg[l + 1] == s.rbeg[l]) continue;
        if (w0 < 0) w0 = s.w[l];
        mixed = s.w[l] != w0;
    }
    return mixed || h->fwd_t == 2;
}

// One LaunchPlan per width bucket.
static int build_forward(PlanCtx *h, const Stripes &s, const char *val, Arena &ar, std::vector<LaunchPlan> &plans,
                         std::vector<int32_t> &fill)
{
    std::map<int, std::vector<int64_t>> buckets;  // w -> stripes
    for (int64_t l = 0; l < s.L; l++)
        if (s.rbeg[l + 1] > s.rbeg[l]) buckets[s.w[l]].push_back(l);
    std::vector<int64_t> cnt(s.m + 1), cur(s.m);
    std::vector<char> any(s.m, 0);
    for (auto &kv : buckets) {
        const int w = kv.first;
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int64_t l : kv.second)
            for (int64_t r = s.rbeg[l]; r < s.rbeg[l + 1]; r++) cnt[s.rows[r] + 1]++;
        for (int64_t i = 0; i < s.m; i++) cnt[i + 1] += cnt[i];
        const bool single = buckets.size() == 1;
        // swept only as the single bucket: with several, every bucket's launch would sweep x and all of
        // y again (mixed-width NS fp64: 904 -> 1280 us measured)
        if ((single || h->sweep_mode == 1) && sweep_possible(h, w, s.n)) {
            // every output row a segment (rows without blocks in this bucket keep beta * y)
            std::vector<Entry> ents(cnt[s.m]);
            for (int64_t i = 0; i < s.m; i++) cur[i] = cnt[i];
            for (int64_t l : kv.second)
                for (int64_t r = s.rbeg[l]; r < s.rbeg[l + 1]; r++)
                    ents[cur[s.rows[r]]++] = {(uint32_t)s.col0[l], s.voff[l] + (r - s.rbeg[l]) * w};
            std::vector<int64_t> sb(cnt.begin(), cnt.end());
            if (want_sweep(h, w, s.n, sb, ents)) {
                std::vector<int32_t> out(s.m);
                for (int64_t i = 0; i < s.m; i++) out[i] = (int32_t)i;
                PendingSweep pw;
                int tile0 = 0;
                if (int st = build_sweep(h, 1, w, sb, ents, out, val, ar, tile0, pw)) return st;
                h->st.bytes_f += s.m * h->esz;  // y written once per bucket
                std::fill(any.begin(), any.end(), 1);
                plans.emplace_back();
                plans.back().L.sweep_tiles = tile0;
                plans.back().L.sweep_tile_bytes = h->sweep_tile;
                plans.back().L.sweep_diag = h->sweep_diag;
                plans.back().sweeps.push_back(pw);
                continue;
            }
        }
        std::vector<int64_t> sbeg{0};
        std::vector<int32_t> sout;
        for (int64_t i = 0; i < s.m; i++)
            if (single || cnt[i + 1] > cnt[i]) { sbeg.push_back(cnt[i + 1]); sout.push_back((int32_t)i); }
        std::vector<int64_t> order;
        const bool slotted = want_slots(h, 1, w, sbeg, (int64_t)cnt[s.m], s.n, order) != 0;
        std::vector<Entry> ents(cnt[s.m]);
        for (int64_t i = 0; i < s.m; i++) cur[i] = cnt[i];
        for (int64_t l : kv.second)
            for (int64_t r = s.rbeg[l]; r < s.rbeg[l + 1]; r++) {
                const int64_t i = s.rows[r];
                const int64_t e = cur[i]++;
                ents[e] = {(uint32_t)s.col0[l] | (!slotted && e == cnt[i] ? kHead : 0u), s.voff[l] + (r - s.rbeg[l]) * w};
            }
        plans.emplace_back();
        if (single) {  // node-blocked rows: the planar forward layout with row runs (or lane streams)
            const int R = fwd_runs(h, w, s.m, ents, sbeg);
            PendingSlot ps;
            int zero = 0;
            const bool lanes = R > 1 && want_fwd_lanes(h, w, R, s.m, sbeg);
            if (lanes) {
                if (int st = build_fwd_lanes(h, w, R, ents, sbeg, s.m, val, ar, ps)) return st;
            }
            bool fpair = false;
            if (!lanes && R == 3) {
                const int st = build_fwd_pair(h, w, R, ents, sbeg, s.m, s.n, val, ar, ps);
                if (st != VBC_OK && st != kBuildDeclined) return st;
                fpair = st == VBC_OK;
            }
            if (lanes || fpair || (R > 1 && build_fwd_runs(h, w, R, ents, sbeg, s.m, val, ar, zero, ps))) {
                std::vector<PendingSlot> one;
                one.push_back(std::move(ps));
                commit_launch_keys(h, one, ar);
                const PendingSlot &p1 = one[0];
                if (lanes)  // real values, one key per block, nlive per row, the tile tables, y
                    h->st.bytes_f += p1.real * (int64_t)R * (p1.b.vsz ? p1.b.vsz : h->esz) + p1.key_bytes + p1.rows * 4 +
                                  (int64_t)p1.b.ntiles * (8 + 128) + s.m * h->esz;
                else if (fpair)  // run-rows of 32 blocks (288 values), one key per block, y
                    h->st.bytes_f += p1.rows * 288 * (int64_t)(p1.b.vsz ? p1.b.vsz : h->esz) + p1.key_bytes + (p1.b.mask ? p1.rows * 4 : 0) +
                                  s.m * h->esz;
                else
                    h->st.bytes_f += p1.rows * p1.b.rpi * (int64_t)w * R * (p1.b.vsz ? p1.b.vsz : h->esz) + p1.key_bytes +
                                     s.m * h->esz;
                std::fill(any.begin(), any.end(), 1);
                plans.back().slots = std::move(one);
                continue;
            }
        }
        if (slotted) {
            PendingSlot ps;
            int srange0 = 0;
            if (int st = build_slots(h, 1, w, w, ents, sbeg, sout, (int64_t)ents.size(), val, ar, srange0, ps, order)) return st;
            std::vector<PendingSlot> one;
            one.push_back(std::move(ps));
            commit_launch_keys(h, one, ar);
            const PendingSlot &p1 = one[0];
            h->st.bytes_f += p1.rows * p1.b.rpi * (int64_t)w * (p1.b.vsz ? p1.b.vsz : h->esz) + p1.key_bytes +
                          (int64_t)sout.size() * h->esz;
            for (int32_t i : sout) any[i] = 1;
            plans.back().slots = std::move(one);
            plans.back().L.slot_ranges = srange0;
            continue;
        }
        std::vector<int32_t> out;
        for (int64_t i = 0; i < s.m; i++)
            if (cnt[i + 1] > cnt[i]) { out.push_back((int32_t)i); any[i] = 1; }
        PendingBin pb;
        int range0 = 0;
        if (int st = build_bucket(h, 1, w, ents, out, (int64_t)ents.size(), val, ar, range0, pb)) return st;
        h->st.bytes_f += (int64_t)ents.size() * (4 + (int64_t)w * h->esz) + (int64_t)out.size() * (4 + h->esz);
        plans.back().bins.push_back(pb);
        plans.back().L.total_ranges = range0;
    }
    h->st.f_scale = buckets.size() > 1;
    if (buckets.size() <= 1)
        for (int64_t i = 0; i < s.m; i++)
            if (!any[i]) fill.push_back((int32_t)i);
    if (h->st.f_scale) h->st.bytes_f += s.m * h->esz * 2 * (int64_t)buckets.size();
    h->st.bytes_f += s.n * h->esz;
    return VBC_OK;
}

int check_plan_input(int dtype, const Stripes &s)
{
    if (dtype != VBC_F64 && dtype != VBC_F32 && dtype != VBC_I64)
        return fail(VBC_UNSUPPORTED_DTYPE, "GPU products compute in Float64, Float32 or Int64 (see vbc_types)");
    return check_limits(s);
}

// Integer eltypes: the reference layout itself (0-based) in one arena, read by vbc_generic.hip.
static void plan_int(const Stripes &s, const int64_t *val, int64_t nval, Plan &P)
{
    Arena &ar = P.ar;
    IntPlan &li = P.li;
    const int64_t L = s.L, q = (int64_t)s.rows.size();
    li.L = L;
    li.nrows = q;
    li.o_col0 = ar.reserve(L * 4), li.o_w = ar.reserve(L * 4), li.o_rows = ar.reserve(q * 4);
    li.o_c2s = ar.reserve(s.n * 4), li.o_r2s = ar.reserve(q * 4);
    li.o_rbeg = ar.reserve((L + 1) * 8), li.o_voff = ar.reserve(L * 8), li.o_val = ar.reserve(nval * 8);
    for (int64_t l = 0; l < L; l++) {
        ar.at<int32_t>(li.o_col0)[l] = (int32_t)s.col0[l];
        ar.at<int32_t>(li.o_w)[l] = s.w[l];
        ar.at<int64_t>(li.o_voff)[l] = s.voff[l];
        for (int64_t c = 0; c < s.w[l]; c++) ar.at<int32_t>(li.o_c2s)[s.col0[l] + c] = (int32_t)l;
        for (int64_t r = s.rbeg[l]; r < s.rbeg[l + 1]; r++) ar.at<int32_t>(li.o_r2s)[r] = (int32_t)l;
    }
    std::memcpy(ar.at<int64_t>(li.o_rbeg), s.rbeg.data(), (L + 1) * 8);
    if (q) std::memcpy(ar.at<int32_t>(li.o_rows), s.rows.data(), q * 4);
    if (nval) std::memcpy(ar.at<int64_t>(li.o_val), val, nval * 8);
    P.st.bytes_t = P.st.bytes_f = nval * 8 + q * 4 + (s.m + s.n) * 8;
}


// The fill list of a launch (y entries no bin writes): into the arena, after the launch's bins.
template <typename LaunchT>
static void place_fill(Arena &ar, LaunchT &L, const std::vector<int32_t> &fill)
{
    L.nfill = (int)fill.size();
    L.o_fill = ar.reserve(fill.size() * 4);
    if (!fill.empty()) std::memcpy(ar.at<int32_t>(L.o_fill), fill.data(), fill.size() * 4);
}

int plan_layout(const LayoutConfig &cfg, const Stripes &s, const char *v, int64_t nval, unsigned flags, Plan &P,
                Recorder *rec)
{
    if (int st = check_plan_input(cfg.dtype, s)) return st;
    if ((flags & (VBC_CREATE_TRANSPOSED | VBC_CREATE_FORWARD | VBC_CREATE_MULTI | VBC_CREATE_MULTI_FORWARD)) == 0)
        flags |= VBC_CREATE_TRANSPOSED;
    P = Plan{};
    if (cfg.dtype == VBC_I64) {  // exact integer products (vbc_generic.hip): one layout, both directions
        P.is_int = true;
        plan_int(s, reinterpret_cast<const int64_t *>(v), nval, P);
        P.st.has_t = (flags & (VBC_CREATE_TRANSPOSED | VBC_CREATE_MULTI)) != 0;
        P.st.has_f = (flags & (VBC_CREATE_FORWARD | VBC_CREATE_MULTI_FORWARD)) != 0;
        return VBC_OK;
    }
    PlanCtx ctx(cfg, P.st, rec, nval);
    PlanCtx *h = &ctx;
    Arena &ar = P.ar;
    std::vector<int32_t> fill;
    int st = VBC_OK;
    if (flags & VBC_CREATE_MULTI) {
        st = build_panel(h, s, v, ar, P.m, fill, nullptr);
        h->st.has_m = st == VBC_OK;
        if (st == VBC_OK) place_fill(ar, P.m.L, fill);
    }
    if (st == VBC_OK && (flags & VBC_CREATE_MULTI_FORWARD)) {
        const size_t c0 = ar.host.size();
        st = build_forward_panel(h, s, v, ar, P.mf);
        if (rec) rec->canon.emplace_back(c0, ar.host.size());
        h->st.has_mf = st == VBC_OK;
        if (st == VBC_OK) P.mf.L.o_fill = ar.reserve(4);
    }
    if (st == VBC_OK && (flags & VBC_CREATE_TRANSPOSED)) {
        fill.clear();
        st = build_transposed(h, s, v, ar, P.t, fill);
        h->st.has_t = st == VBC_OK;
        if (st == VBC_OK) place_fill(ar, P.t.L, fill);
    }
    fill.clear();
    if (st == VBC_OK && (flags & VBC_CREATE_FORWARD) && fwd_via_t_wanted(h, s, flags)) {
        // small mixed-width forward product as the transposed product of C = Bᵀ (one fused launch instead
        // of a scale pass and one forward launch per width bucket, each adding into y)
        Stripes c;
        std::vector<char> cv;
        st = transpose_stripes(h, s, v, 8, c, cv);
        if (st == VBC_OK) {
            const int64_t bt = h->st.bytes_t;
            const size_t c0 = ar.host.size();
            // (a stripe that stores one row twice had its copies summed in fp64: such values stay wide)
            // A recording plan holds tags, not values: it takes the answer the handle's own plan gave.  (That
            // answer is always yes there -- a recording plan refuses a row stored twice, so every slot of cv is
            // 0 + v of one widened float, which is a float -- but the plans must agree whatever it is.)
            LayoutConfig cfg_c = cfg;
            cfg_c.narrow_values = cfg.narrow_values &&
                                  (rec ? rec->ft_narrow : all_float_exact(cv.data(), (int64_t)(cv.size() / 8)));
            cfg_c.narrow_planar = cfg.narrow_planar && cfg_c.narrow_values;
            cfg_c.narrow_pairs = cfg.narrow_pairs && cfg_c.narrow_planar;
            cfg_c.narrow_streams = cfg.narrow_streams && cfg_c.narrow_pairs;
            cfg_c.narrow_swept = cfg.narrow_swept && cfg_c.narrow_values;
            h->st.ft_narrow = cfg_c.narrow_values;
            PlanCtx hc(cfg_c, P.st, rec, nval);
            st = build_transposed(&hc, c, cv.data(), ar, P.tf, fill);
            if (rec) rec->canon.emplace_back(c0, ar.host.size());
            h->st.bytes_f = h->st.bytes_t - bt;
            h->st.bytes_t = bt;
        }
        if (st == VBC_OK) {
            h->st.has_f = h->st.has_ft = true;
            place_fill(ar, P.tf.L, fill);
        }
    } else if (st == VBC_OK && (flags & VBC_CREATE_FORWARD)) {
        st = build_forward(h, s, v, ar, P.f, fill);
        h->st.has_f = st == VBC_OK;
        if (st == VBC_OK) {
            if (P.f.empty()) P.f.emplace_back();  // no entries: the fill list alone writes y
            place_fill(ar, P.f[0].L, fill);
        }
    }
    return st;
}

}  // namespace vbc
