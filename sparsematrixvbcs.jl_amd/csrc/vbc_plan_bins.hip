// The layout planner's per-bucket builders: one bucket's entries laid out for the merge kernel (build_bucket), the
// slotted / planar / lane-pair layouts (build_slots), the lane streams (build_lanes) and the row-swept layout
// (build_sweep), with the rules that choose among them (want_*).  The per-direction planners of vbc_plan.hip call
// them.  Pure host code (vbc_plan.h): no HIP call, no environment.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

#include "vbc_plan_impl.h"
#include "vbc_planar.h"

namespace vbc {

// Lay out one bucket's entry stream (segment-ordered) as tiles, ranges and fix-up slots.
int build_bucket(PlanCtx *h, int kind, int w, const std::vector<Entry> &ents,
                 const std::vector<int32_t> &out, int64_t total_entries, const char *val,
                 Arena &ar, int &range0, PendingBin &pb, int wsrc)
{
    // wsrc < w: the entries carry wsrc values each, stored w wide with zero padding columns
    if (wsrc <= 0) wsrc = w;
    const int esz = h->esz;
    const int V = w <= 8 ? vec_elems(esz, w) : 1;
    const int LPR = w / V;
    const int RPI = 64 / LPR;
    const int K = h->tile_k;
    const int64_t tile_rows = (int64_t)RPI * K;
    const int64_t R = (int64_t)ents.size();
    const int64_t ntiles = (R + tile_rows - 1) / tile_rows;
    if (ntiles >= (int64_t(1) << 31)) return fail(VBC_INVALID_ARG, "bucket too large");
    if ((int64_t)out.size() >= (int64_t(1) << 31)) return fail(VBC_INVALID_ARG, "too many segments");
    // ranges: one wave each, about target_ranges over the whole launch, >= 2 tiles per range
    int64_t nr = (int64_t)std::llround((double)h->target_ranges_k[kind] * (double)R / (double)std::max<int64_t>(total_entries, 1));
    nr = std::max<int64_t>(1, std::min<int64_t>(nr, (ntiles + 1) / 2));
    const int64_t tpr = ntiles > 0 ? (ntiles + nr - 1) / nr : 1;
    nr = ntiles > 0 ? (ntiles + tpr - 1) / tpr : 0;
    pb = PendingBin{};
    pb.b.kind = kind;
    pb.b.wkey = w <= 8 ? w : 0;
    pb.b.w = w;
    pb.b.wst = wsrc;
    pb.b.rpi = RPI;
    pb.b.range0 = range0;
    pb.b.nranges = (int32_t)nr;
    pb.b.tiles_per_range = (int32_t)tpr;
    pb.b.ntiles = (int32_t)ntiles;
    pb.b.tile_k = K;
    pb.b.pipe = h->pipe;
    pb.b.diag = h->diag;
    pb.b.out_affine = 1;
    pb.b.out_base = out.empty() ? 0 : out[0];
    pb.b.out_stride = out.size() > 1 ? out[1] - out[0] : 0;
    for (size_t q = 1; q < out.size() && pb.b.out_affine; q++)
        pb.b.out_affine = (int64_t)out[q] == (int64_t)out[0] + (int64_t)q * pb.b.out_stride;
    if (h->no_affine) pb.b.out_affine = 0;  // (the VBC_ABLATION build only)
    range0 += (int)nr;
    const int64_t Rp = ntiles * tile_rows;
    pb.o_key = ar.reserve(Rp * 4);
    pb.o_val = ar.reserve(Rp * w * esz);
    pb.o_rseg = ar.reserve(std::max<int64_t>(nr, 1) * 4);
    pb.o_out = ar.reserve(std::max<size_t>(out.size(), 1) * 4);
    pb.o_carry = ar.reserve(std::max<int64_t>(nr, 1) * (kind == 0 ? w : 1) * esz);
    pb.o_cseg = ar.reserve(std::max<int64_t>(nr, 1) * 4);
    uint32_t *key = ar.at<uint32_t>(pb.o_key);
    char *vv = ar.at<char>(pb.o_val);
    int32_t *rseg = ar.at<int32_t>(pb.o_rseg);
    std::memcpy(ar.at<int32_t>(pb.o_out), out.data(), out.size() * 4);
    int64_t heads = 0;
    const int GV = val_group(esz, w);  // grouped tile layout (vbc_kernels.h key_pos / val_pos)
    for (int64_t t = 0; t < Rp; t++) {
        const int64_t tile = t / tile_rows, within = t - tile * tile_rows;
        const int slot = (int)(within / K), k = (int)(within - (int64_t)slot * K);
        const size_t pk = key_pos((size_t)(tile * tile_rows), k, slot, RPI);
        const size_t pv = val_pos((size_t)(tile * tile_rows), k, slot, RPI, GV);
        if (within == 0 && tile % tpr == 0) rseg[tile / tpr] = (int32_t)heads;
        if (t < R) {
            key[pk] = ents[t].key;
            heads += (ents[t].key >> 31);
            std::memcpy(vv + pv * w * esz, val + ents[t].voff * esz, (size_t)wsrc * esz);
            if (wsrc < w) std::memset(vv + (pv * w + wsrc) * esz, 0, (size_t)(w - wsrc) * esz);
        } else {
            key[pk] = 0;  // padding extends the last segment by zeros
            std::memset(vv + pv * w * esz, 0, (size_t)w * esz);
        }
    }
    return VBC_OK;
}

// ---- slotted layout (vbc_slots.h) ----------------------------------------------------------------

// Per-row base of the compressed form: the first non-padding key of the row (0 if none).
bool slot_keys_compressible(const std::vector<uint32_t> &keys, int64_t rows, int RPI)
{
    for (int64_t r = 0; r < rows; r++) {
        const uint32_t *k = keys.data() + r * RPI;
        int64_t base = -1;
        for (int s = 0; s < RPI; s++) {
            if (k[s] & kPad) continue;
            const int64_t g = k[s] & kSlotIdx;
            if (base < 0) base = g;
            if (g - base < -32767 || g - base > 32767) return false;
        }
    }
    return true;
}

// Store a slotted bin's keys: full 32-bit keys, or (kc) per-row bases + int16 deltas.  Compressed rows
// with identical delta patterns are stored once (a mesh operator's interior chunks all share one --
// FE: [0, 2, 4, ...] -- so its delta stream collapses to a few KB that stay in L2); each row carries
// the offset of its pattern.  VBC_SLOT_DEDUP=0 keeps one pattern per row (A/B).
static void commit_slot_keys(PendingSlot &ps, bool kc, Arena &ar, bool dedup)
{
    const int RPI = ps.b.rpi;
    const int64_t E = ps.rows * RPI;
    ps.b.kc = kc ? 1 : 0;
    if (!kc) {
        ps.o_key = ar.reserve(E * 4);
        std::memcpy(ar.at<uint32_t>(ps.o_key), ps.keys.data(), E * 4);
        ps.key_bytes = E * 4;
    } else {
        std::vector<int16_t> d(E);
        std::vector<uint32_t> bs(ps.rows), doff(ps.rows);
        for (int64_t r = 0; r < ps.rows; r++) {
            const uint32_t *k = ps.keys.data() + r * RPI;
            uint32_t base = 0;
            for (int s = 0; s < RPI; s++)
                if (!(k[s] & kPad)) { base = k[s] & kSlotIdx; break; }
            bs[r] = base | (k[0] & kLast);
            for (int s = 0; s < RPI; s++)
                d[r * RPI + s] = (k[s] & kPad) ? INT16_MIN : (int16_t)((int64_t)(k[s] & kSlotIdx) - (int64_t)base);
        }
        std::unordered_map<std::string, uint32_t> seen;
        int64_t stored = 0;  // distinct patterns, in rows
        for (int64_t r = 0; r < ps.rows; r++) {
            const int16_t *row = d.data() + r * RPI;
            if (dedup) {
                std::string kbytes(reinterpret_cast<const char *>(row), (size_t)RPI * 2);
                auto it = seen.find(kbytes);
                if (it != seen.end()) { doff[r] = it->second; continue; }
                seen.emplace(std::move(kbytes), (uint32_t)(stored * RPI));
            }
            if (stored != r) std::memmove(d.data() + stored * RPI, row, (size_t)RPI * 2);
            doff[r] = (uint32_t)(stored * RPI);
            stored++;
        }
        ps.o_key = ar.reserve(stored * RPI * 2);
        ps.o_base = ar.reserve(ps.rows * 4);
        ps.o_doff = ar.reserve(ps.rows * 4);
        std::memcpy(ar.at<int16_t>(ps.o_key), d.data(), (size_t)stored * RPI * 2);
        std::memcpy(ar.at<uint32_t>(ps.o_base), bs.data(), (size_t)ps.rows * 4);
        std::memcpy(ar.at<uint32_t>(ps.o_doff), doff.data(), (size_t)ps.rows * 4);
        ps.key_bytes = stored * RPI * 2 + ps.rows * 8;
    }
    std::vector<uint32_t>().swap(ps.keys);
}

// Segments per lane of a B'x bucket whose rows are narrower than a 16-B lane vector: fp32 w = 2 folds
// two segments side by side (run_slots_narrow); w = 1 (CSC) keeps one segment per lane (faster).
static int slot_spl(const PlanCtx *h, int kind, int w)
{
    if (kind != 0 || !h->slot_narrow) return 1;
    return (h->esz == 4 && w == 2) ? 2 : 1;  // the only narrow form that measured faster (vbc_slots.h)
}

// Planar chunk rows (vbc_planar.h) for a B'x bucket of width w: one stripe per lane whenever a row
// is wider than one 16-B lane vector would hold with a single lane (fp64 w >= 3, fp32 w >= 5) and for
// fp32 w = 3 (12-B rows, no padding to 4).
bool slot_planar(const PlanCtx *h, int kind, int w)
{
    if (kind == 0 && h->st.small_split > 1 && w >= 1 && w <= 8 && ((h->st.fuse_w >> w) & 1)) return true;  // fused split (below)
    if (kind != 0 || h->slot_planar == 0 || w < 3 || w > 8) return false;
    return h->esz == 8 || w != 4;
}

// Slots per chunk of a bucket stored w wide (lane-vector width as in the kernel).
static int slot_rpi(const PlanCtx *h, int kind, int w)
{
    if (slot_planar(h, kind, w)) return 64;
    const int spl = slot_spl(h, kind, w);
    if (spl > 1) return 64 * spl;
    const int V = w <= 8 ? vec_elems(h->esz, w) : 1;
    return 64 / (w / V);
}

// Rows of each chunk: the longest segment of its RPI (>= 1, so every chunk closes).
std::vector<int32_t> chunk_rows(const std::vector<int64_t> &sbeg, int RPI)
{
    const int64_t nseg = (int64_t)sbeg.size() - 1;
    std::vector<int32_t> cr((nseg + RPI - 1) / RPI, 1);
    for (int64_t q = 0; q < nseg; q++)
        cr[q / RPI] = (int32_t)std::max<int64_t>(cr[q / RPI], sbeg[q + 1] - sbeg[q]);
    return cr;
}

// Segment order of a sorted slotted bucket: by decreasing length inside windows of kSortWindow
// chunks (neighbouring segments stay near each other, so x locality survives the sort).
constexpr int kSortWindow = 32;
std::vector<int64_t> sorted_order(const std::vector<int64_t> &sbeg, int RPI)
{
    const int64_t nseg = (int64_t)sbeg.size() - 1, win = (int64_t)kSortWindow * RPI;
    std::vector<int64_t> ord(nseg);
    for (int64_t i = 0; i < nseg; i++) ord[i] = i;
    for (int64_t a = 0; a < nseg; a += win) {
        const int64_t e = std::min(nseg, a + win);
        std::stable_sort(ord.begin() + a, ord.begin() + e, [&](int64_t p, int64_t q) {
            return sbeg[p + 1] - sbeg[p] > sbeg[q + 1] - sbeg[q];
        });
    }
    return ord;
}

std::vector<int64_t> permuted_sbeg(const std::vector<int64_t> &sbeg, const std::vector<int64_t> &ord)
{
    std::vector<int64_t> p(sbeg.size());
    p[0] = 0;
    for (size_t i = 0; i < ord.size(); i++) p[i + 1] = p[i] + sbeg[ord[i] + 1] - sbeg[ord[i]];
    return p;
}

// Whether a bucket (segments sbeg over `real` entries) runs slotted: auto mode asks for a padded row
// count within slots_pad of the real one and chunks short enough to balance over the ranges, first
// in the natural segment order (affine y map), then sorted by length (y offsets from the table).
// Returns 0 (merge layout), 1 (slotted, natural order) or 2 (slotted, `order`).
// Chunk-local length order (SlotBin::mask): the segments of each window of `win` consecutive natural
// segments (mask_window chunks) by decreasing length -- the window keeps its segments (most of the
// x locality of the natural order: the sort over windows of 32 chunks lost it, FE-3D's x is fetched
// ~10x), and every chunk row's live lanes are a prefix, so the kernel points the dead lanes at lane
// 0's lines.
std::vector<int64_t> chunk_sorted_order(const std::vector<int64_t> &sbeg, int win)
{
    const int64_t nseg = (int64_t)sbeg.size() - 1;
    std::vector<int64_t> ord(nseg);
    for (int64_t i = 0; i < nseg; i++) ord[i] = i;
    for (int64_t a = 0; a < nseg; a += win)
        std::stable_sort(ord.begin() + a, ord.begin() + std::min(nseg, a + win), [&](int64_t p, int64_t q) {
            return sbeg[p + 1] - sbeg[p] > sbeg[q + 1] - sbeg[q];
        });
    return ord;
}

// Padded / real rows a bucket of the fused small-matrix split may carry in length-sorted order: a chunk
// costs its longest stripe's rows / P whatever its padding, and the padding rows read cached zeros.
constexpr double kSmallPad = 4.0;

int want_slots(const PlanCtx *h, int kind, int w, const std::vector<int64_t> &sbeg,
               int64_t total_entries, int64_t gather_limit, std::vector<int64_t> &order,
               bool *mask, int wsrc)
{
    const bool fused = kind == 0 && h->st.small_split > 1 && wsrc >= 1 && wsrc <= 8 && ((h->st.fuse_w >> wsrc) & 1);
    if (mask) *mask = false;
    const int64_t nseg = (int64_t)sbeg.size() - 1;
    const int64_t real = nseg > 0 ? sbeg[nseg] - sbeg[0] : 0;
    order.clear();
    if (h->slots_mode == 0 || real == 0 || gather_limit >= (int64_t)kSlotIdxLimit) return 0;
    if (nseg >= (int64_t(1) << 31)) return 0;
    const int RPI = slot_rpi(h, kind, w);
    double pad_limit = 0;
    // (not for buckets small enough for the split product, which folds every padding row: build_slots)
    const double share_p = (double)h->target_ranges_p * (double)real / (double)std::max<int64_t>(total_entries, 1);
    // (P >= 4; a masked bucket skips P = 2: ldoor's 1/8 stripe shard, 615 chunks, masked lane pairs
    // 15.3 us vs split P = 2 16.3 us; the ct20stif stand-in, 273 chunks, keeps P = 4: 10.9 vs 12.8 us)
    const bool split_likely = h->planar_split != 0 && (double)((nseg + RPI - 1) / RPI) * 8 <= share_p;
    auto fits = [&](const std::vector<int64_t> &sb, bool force) {
        const std::vector<int32_t> cr = chunk_rows(sb, RPI);
        int64_t rows = 0, longest = 0;
        for (int32_t c : cr) { rows += c; longest = std::max<int64_t>(longest, c); }
        if (rows * RPI >= (int64_t(1) << 31)) return false;
        if (force) return true;
        const double ratio = (double)(rows * RPI) / (double)real;
        const double share = (double)h->target_ranges_s[kind] * (double)real / (double)std::max<int64_t>(total_entries, 1);
        const double rows_per_range = (double)rows / std::max(1.0, share);
        // (chunks are atomic: a planar w = 6 bucket of the ldoor stand-in with chunks up to 2x the rows
        // per range ran 193 us against the merge kernel's 171 us, profiles/r03_fork_ab2.log)
        return ratio <= (pad_limit > 0 ? pad_limit : h->slots_pad) && (double)longest <= std::max(64.0, 0.5 * rows_per_range);
    };
    if (fused && h->slots_mode != 0) {
        // fused small-matrix split (build_transposed): P waves fold every chunk, so a chunk longer than
        // the rows of a range does not unbalance anything; padding rows cost instructions and a few
        // cached lines of a matrix that stays in L2, so a sorted order may pad up to kSmallPad
        auto pad = [&](const std::vector<int64_t> &sb) {  // rows the chunks' lanes that hold a segment step through
            const std::vector<int32_t> cr = chunk_rows(sb, RPI);
            int64_t padded = 0;
            for (size_t c = 0; c < cr.size(); c++)
                padded += (int64_t)cr[c] * std::min<int64_t>(RPI, nseg - (int64_t)c * RPI);
            return (double)padded / (double)real;
        };
        // a bucket's padding counts against the whole launch: a few-chunk bucket (one chunk of 5 stripes,
        // one of them long) may pad far beyond kSmallPad and still add only a few workgroups' rows
        auto ok = [&](double p) { return p <= kSmallPad || (p - 1.0) * (double)real <= 0.05 * (double)total_entries; };
        if (h->slots_sort != 2 && (pad(sbeg) <= h->slots_pad || (h->slots_sort == 0 && ok(pad(sbeg))))) return 1;
        if (h->slots_sort == 0) return 0;
        order = sorted_order(sbeg, RPI);
        if (ok(pad(permuted_sbeg(sbeg, order)))) return 2;
        order.clear();
        return 0;
    }
    if (h->slots_sort != 2 && fits(sbeg, h->slots_mode == 1)) return 1;
    if (h->slots_sort == 0) return 0;
    if (mask && kind == 0 && h->planar_mask != 0 && slot_planar(h, 0, w) && !split_likely) {
        order = chunk_sorted_order(sbeg, RPI * h->mask_window);
        pad_limit = kMaskPad;
        if (fits(permuted_sbeg(sbeg, order), h->slots_mode == 1)) {
            *mask = true;
            return 2;
        }
        pad_limit = 0;
    }
    order = sorted_order(sbeg, RPI);
    if (fits(permuted_sbeg(sbeg, order), h->slots_mode == 1)) return 2;
    order.clear();
    return 0;
}

// Row runs of a planar bucket (SlotBin::run): the largest R in {3, 2} such that every segment's rows
// come in aligned runs of R consecutive x rows -- the dof rows of a node in a stiffness operator
// stored by node stripes (fe3d, the ldoor / ct20stif stand-ins).  The kernel then reads one key per
// run and gathers the run's R x values at once.  VBC_SLOT_RUNS=0 disables it (A/B, tests).
int slot_runs(const PlanCtx *h, const std::vector<Entry> &ents, const std::vector<int64_t> &sbeg)
{
    if (h->slot_runs == 0) return 1;
    const int64_t nseg = (int64_t)sbeg.size() - 1;
    for (int R = 3; R >= 2; R--) {
        bool ok = sbeg[nseg] > sbeg[0];
        for (int64_t q = 0; q < nseg && ok; q++) {
            const int64_t b = sbeg[q], len = sbeg[q + 1] - b;
            if (len % R) { ok = false; break; }
            for (int64_t t = 0; t < len && ok; t += R)
                for (int d = 1; d < R; d++)
                    if (ents[b + t + d].key != ents[b + t].key + (uint32_t)d) { ok = false; break; }
        }
        if (ok) return R;
    }
    return 1;
}

// Lay out a slotted bucket: chunk rows row-major over the slots, PAD / LAST keys, ranges of whole
// chunks balanced by rows.  ents[sbeg[q] ...] are segment q's entries (keys = gather index only).
// pair_only: build nothing and return kBuildDeclined unless the bucket takes the lane-pair layout.

// One run's 3 x 3 values v[row][column] at stripe (stream) slot sl of the pair run-row at `blk` (vbc_planar.h
// run_pair: segments A, B, C, D of 288 values).  narrow (VBC_CREATE_NARROW_PAIRS): the run-row holds floats, in the
// arrangement VBC_PAIR_FORM names (vbc_kernels.h; vbc_planar.h pair_load reads it).
static void put_pair_run(const PlanCtx *h, bool narrow, char *blk, int sl, const double (&v)[3][3])
{
    auto put = [&](int e, const double &src) {
        if (narrow) narrow_value(h, &src, blk + (size_t)e * 4);
        else std::memcpy(blk + (size_t)e * 8, &src, 8);
    };
    if (narrow && VBC_PAIR_FORM == 1) {  // 16 B per lane: even {r0c0, r0c1, r1c0, r1c1}, odd {r0c2, r1c2, r2c2, r2c0}; r2c1 tail
        put(8 * sl + 0, v[0][0]);
        put(8 * sl + 1, v[0][1]);
        put(8 * sl + 2, v[1][0]);
        put(8 * sl + 3, v[1][1]);
        put(8 * sl + 4, v[0][2]);
        put(8 * sl + 5, v[1][2]);
        put(8 * sl + 6, v[2][2]);
        put(8 * sl + 7, v[2][0]);
        put(256 + sl, v[2][1]);
        return;
    }
    put(4 * sl + 0, v[0][0]);
    put(4 * sl + 1, v[0][1]);
    put(4 * sl + 2, v[0][2]);
    put(4 * sl + 3, v[1][2]);
    put(128 + 2 * sl + 0, v[1][0]);
    put(128 + 2 * sl + 1, v[1][1]);
    put(192 + sl, v[2][2]);
    put(224 + 2 * sl + 0, v[2][0]);
    put(224 + 2 * sl + 1, v[2][1]);
}
int build_slots(PlanCtx *h, int kind, int w, int wsrc, const std::vector<Entry> &ents,
                const std::vector<int64_t> &sbeg0, const std::vector<int32_t> &out0, int64_t total_entries,
                const char *val, Arena &ar, int &range0, PendingSlot &ps,
                const std::vector<int64_t> &order, bool mask, int ks, bool pair_only)
{
    const int esz = h->esz;
    // segment q of the layout is input segment order[q] (natural order when `order` is empty)
    const std::vector<int64_t> sbeg = order.empty() ? sbeg0 : permuted_sbeg(sbeg0, order);
    std::vector<int64_t> pstart(sbeg.size() - 1);
    std::vector<int32_t> out(out0.size());
    for (size_t q = 0; q < pstart.size(); q++) {
        const int64_t o = order.empty() ? (int64_t)q : order[q];
        pstart[q] = sbeg0[o];
        out[q] = out0[o];
    }
    const int64_t nseg = (int64_t)sbeg.size() - 1;
    int64_t nstripes = nseg;
    if (ks > 1) {  // stripes cut into ks parts (build_ksplit): out / nseg per stripe, lanes 0 .. 64/ks - 1
        const int m = 64 / ks;
        std::vector<int32_t> os;
        for (int64_t q = 0; q < nseg; q++)
            if (q % 64 < m && out[q] >= 0) os.push_back(out[q]);
        nstripes = (int64_t)os.size();
        out.swap(os);
    }
    const int64_t real = sbeg[nseg] - sbeg[0];
    const bool planar = slot_planar(h, kind, w);
    const int run = planar ? slot_runs(h, ents, sbeg0) : 1;  // sbeg0: the input order ents is in
    // runs with holes (build_transposed, hole_runs): absent rows are entries with voff < 0
    bool holes = false;
    for (const Entry &en : ents) holes = holes || en.voff < 0;
    if (holes && !(planar && run > 1 && kind == 0)) return fail(VBC_INVALID_ARG, "internal: runs with holes outside a planar B'x bin");
    // pair layout (vbc_planar.h run_pair): fp64 3-wide stripes with runs of 3, a lane pair per stripe
    // (for long segments: FE-3D's ~3 runs per stripe measured slower with 32-stripe chunks, 304 -> 315
    // us, ldoor's ~15 faster, 92 -> 81 us)
    bool pair = planar && run == 3 && esz == 8 && w == 3 && wsrc == 3 && h->planar_pair != 0 &&
                (h->planar_pair == 2 || real >= 3 * 8 * std::max<int64_t>(nseg, 1));
    int RPI = 0, split = 1;
    std::vector<int32_t> cr;
    int64_t nch = 0, rows = 0;
    const double target = planar ? (double)h->target_ranges_p : (double)h->target_ranges_s[kind];
    const double share = target * (double)real / (double)std::max<int64_t>(total_entries, 1);
    for (int attempt = 0; attempt < 2; attempt++) {
        RPI = pair ? 32 : slot_rpi(h, kind, w);
        cr = chunk_rows(sbeg, RPI);
        for (int32_t &c : cr) {
            c = (c + run - 1) / run * run;  // whole runs (an empty chunk: one padding run)
            if (pair) c /= 3;               // pair layout: rows are run-rows
        }
        nch = (int64_t)cr.size();
        rows = 0;
        for (int32_t c : cr) rows += c;
        // planar buckets with fewer chunks than wave slots: one chunk per workgroup of `split` waves
        split = 1;
        if (planar && kind == 0 && h->st.small_split > 1 && wsrc <= 8 && ((h->st.fuse_w >> wsrc) & 1)) {
            split = h->st.small_split;  // fused small-matrix split: one P for every bucket of the launch
        } else if (planar && h->planar_split != 0) {
            if (h->planar_split > 1) split = h->planar_split;
            else if ((double)nch / (pair ? 2 : 1) * 2 <= share) {  // in 64-stripe chunks
                // few chunks (at most half the wave slots): P waves per chunk while the grid stays within
                // twice the slots and every wave keeps >= 12 (fp64) / 6 (fp32) rows of its chunk.  Graph-
                // timed (profiles/r03_splitu_*.log, r03_split3_*.log): ct20stif stand-in fp64 (56 rows per
                // chunk) P = 2 6.5 us, 4 5.9, 8 6.2; fp32 5.1 / 4.3 / 4.2; ldoor's 1/8 shard fp64 11.5 /
                // 11.0 / 11.8, fp32 8.5 / 7.5 / 7.3; 1/4 shard fp64: lane pairs 22.3, P = 4 20.6; the 1/2
                // shard (2500 chunks) and the whole ldoor keep the lane pairs (37.6 vs P = 2 40.6; 67 vs 87)
                const double avg = (double)rows * (pair ? 3 : 1) / (double)std::max<int64_t>(nch, 1);  // x rows
                const double minrows = (double)h->split_rows * esz / 8.0;
                // (round 5: the doubled grid stays within ONE round of wave slots -- ldoor's 1/4 stripe shard,
                // 1249 chunks: P = 2 19.7 us, P = 4 20.5; the 1/8 shard keeps P = 4, 11.0 us against P = 2 11.8,
                // profiles/r05_shards_ab.log)
                while (split < 8 && (double)nch / (pair ? 2 : 1) * split * 2 <= share && avg / (split * 2) >= minrows)
                    split *= 2;
            }
        }
        // the split product runs the plain planar layout; so does a pair layout that would fill fewer than
        // half the wave slots, when the split product may be chosen instead (ldoor's 1/8 shard: 1250 pair
        // chunks 21.8 us, planar split 16.3 us)
        const bool drop = pair && (split > 1 || (!mask && h->planar_pair != 2 && h->planar_split != 0 && 2.0 * (double)nch < share));
        if (!drop) break;
        pair = false;
    }
    if (pair_only && !pair) return kBuildDeclined;  // (nothing reserved yet)
    int64_t nr = (int64_t)std::llround(share);
    // one wave per SIMD of the chip for this bucket (the target is CUs x occupancy x waves per workgroup)
    const double quantum = share / std::max(1, planar ? h->occ_p : h->occ_s[kind]);
    if (!planar && h->range_bytes > 0 && share >= 2 * quantum) {
        // small slotted buckets: half the waves per SIMD, each with a longer range (FE's stripe shards:
        // 1/2 89.7 -> 87.4 us, 1/4 49.0 -> 43.3 us, 1/8 28.1 -> 24.4 us; the full matrix keeps all)
        const double bytes = (double)rows * RPI * (w * esz + 4);
        if (bytes / share < (double)h->range_bytes) nr = (int64_t)std::llround(share / 2);
    }
    // plain planar bins: at most planar_wps waves per SIMD (fewer, longer ranges keep the resident
    // waves' x window in L2: ldoor fp64 lane pairs 3 -> 2 waves per SIMD 67.8 -> 65.4 us, fp32 4 -> 2
    // 36.5 -> 34.7 us, the C4 CSC product 36.7 -> 34.6 us; 1.5 or 2.5 per SIMD are slower,
    // profiles/r03_bxranges2_*.log, r03_wps_*.log)
    // (round 5: the fp64 lane-pair layout takes one wave per SIMD -- ldoor 64.4 -> 63.2 us, its 1/2 stripe
    // shard 36.5 -> 34.7 us; fp32 planar keeps two: ldoor fp32 34.9 vs 36.9, profiles/r05_shards_ab.log)
    const int wps = (pair && h->planar_wps_pair > 0) ? h->planar_wps_pair : h->planar_wps;
    if (planar && split == 1 && wps > 0) nr = std::min<int64_t>(nr, std::max<int64_t>(1, std::llround(quantum * wps)));
    nr = std::max<int64_t>(1, std::min<int64_t>(nr, nch));
    // fewer chunks than wave slots: whole waves per SIMD (ldoor's 1/4 shard: 2500 pair chunks as 2500
    // ranges 33.0 us, as 2048 ranges 27.7 us)
    const int64_t qi = (int64_t)quantum;
    if (split == 1 && qi >= 1 && nr < (int64_t)std::llround(share) && nr > qi) nr = nr / qi * qi;
    if (split > 1) nr = nch;
    bool affine = true;
    for (size_t q = 1; q < out.size() && affine; q++)
        affine = (int64_t)out[q] == (int64_t)out[0] + (int64_t)q * (out[1] - out[0]);
    std::vector<int32_t> rrow{0}, rchunk{0};
    int64_t acc = 0;
    for (int64_t c = 0; c < nch; c++) {
        acc += cr[c];
        // a table-mapped bin keeps <= kSlotOutEntries segments per range (their y offsets sit in LDS)
        const bool full = split > 1 || (!affine && (int64_t)(c + 2 - rchunk.back()) * RPI > kSlotOutEntries);
        if (c + 1 < nch && (full || ((int64_t)rrow.size() < nr && acc * nr >= (int64_t)rrow.size() * rows))) {
            rrow.push_back((int32_t)acc);
            rchunk.push_back((int32_t)(c + 1));
        }
    }
    rrow.push_back((int32_t)rows);
    nr = (int64_t)rchunk.size();
    if (h->verbose)
        fprintf(stderr, "[vbc] slot bin kind %d w %d planar %d pair %d run %d split %d chunks %lld rows %lld ranges %lld "
                "(target share %.0f)\n", kind, w, (int)planar, (int)pair, run, split, (long long)nch, (long long)rows,
                (long long)nr, share);
    ps = PendingSlot{};
    SlotBin &b = ps.b;
    b.kind = kind;
    b.wkey = w <= 8 ? w : 0;
    b.w = w;
    b.wst = wsrc;
    b.rpi = RPI;
    b.range0 = range0;
    b.nranges = (int32_t)nr;
    b.nseg = (int32_t)nstripes;
    b.ks = ks;
    b.fused = (planar && kind == 0 && split > 1 && h->st.small_split > 1 && wsrc <= 8 && ((h->st.fuse_w >> wsrc) & 1)) ? 1 : 0;
    b.u = h->slot_u;
    b.diag = h->diag;
    b.xcd = (planar && split == 1) ? h->xcd_p : 0;  // split grids are small (one chunk per workgroup)
    b.nowonly = h->slot_wonly ? 0 : 1;
    b.spl = slot_spl(h, kind, w);
    b.planar = planar ? 1 : 0;
    b.run = run;
    b.split = split;
    b.pair = pair ? 1 : 0;
    b.mask = (mask && planar && split == 1 && (!pair || h->planar_mask_pair)) ? 1 : 0;
    b.holes = holes ? 1 : 0;
    if (holes && (split == 1 || pair)) return fail(VBC_INVALID_ARG, "internal: runs with holes need the split product");
    if (planar && split > 1) {
        // split bins' slice loop (vbc_planar.h split_chunk): 0 one step at a time, 1 pipelined, 2 batched;
        // auto: the plain loop when a wave's slice is at most two steps of ~VBC_SPLIT_VALS values, else
        // batched (VBC_SPLIT_PIPE=0 / 1 / 2 forces one)
        const double rows_per_wave = (double)rows / (double)std::max<int64_t>(nch, 1) / split;
        const int u0 = (9 / w) / run * run;  // planar_split_step (vbc_planar.h, VBC_SPLIT_VALS = 9)
        const double step_rows = (double)std::min(8 * run, std::max(run, u0));
        // (fused bins only: a single-bucket split bin keeps the plain loop -- ldoor's 1/8 stripe shard 12.4 us
        // batched, 11.1 us plain, profiles/r04_ab22_*.log)
        b.deep = h->split_pipe >= 0 ? h->split_pipe : (b.fused && rows_per_wave > h->split_deep * step_rows ? 2 : 0);
        // VBC_SPLIT_NT_MB: above that many value bytes the batched loop reads keys and values non-temporally
        // (mode 3).  Off by default: slower on every table partition, the 300 MB ldoor 'min blocks' too
        // (68.3 -> 77.7 us; ct20stif strict 8.9 -> 12.3 us; profiles/r04_ab4_*.log)
        if (b.deep == 2 && h->split_nt_bytes > 0 && (double)h->nval * h->esz > (double)h->split_nt_bytes) b.deep = 3;
    }
    b.out_affine = 1;
    b.out_base = out.empty() ? 0 : out[0];
    b.out_stride = out.size() > 1 ? out[1] - out[0] : 0;
    for (size_t q = 1; q < out.size() && b.out_affine; q++)
        b.out_affine = (int64_t)out[q] == (int64_t)out[0] + (int64_t)q * b.out_stride;
    if (h->no_affine) b.out_affine = 0;  // (the VBC_ABLATION build only)
    {
        const int V = w <= 8 ? vec_elems(esz, w) : 1;
        const bool full = b.spl > 1 || planar || (RPI * (w / V) == 64 && V * esz <= 16);
        b.contig = b.out_affine && (kind == 0 ? (full && wsrc == w && (nseg <= 1 || b.out_stride == w))
                                              : (nseg <= 1 || b.out_stride == 1));
    }
    if (planar) b.range0 = 0;  // its own launch
    else range0 += (int)nr;
    const int64_t E = rows * RPI;
    ps.rows = rows;
    ps.real = real;
    ps.keys.resize(E);
    // VBC_CREATE_NARROW_VALUES: a slotted (non-planar) bin of an fp64 handle keeps its values as floats.  `val`
    // holds them widened (exactly), so narrowing gives the caller's bits back.  Only the stored size changes:
    // everything above was decided with esz.
    // VBC_CREATE_NARROW_PLANAR: so does a chunk-planar bin the plain kernel runs (spmv_planar: not pair, not split
    // -- which covers the fused small-matrix launch and runs with holes; lane streams are build_lanes'), its
    // chunk rows in the Float32 column-group arrangement (planar_off(4, ...), rows of 64 * w floats: 16-B aligned)
    // VBC_CREATE_NARROW_PAIRS: so does a lane-pair bin (spmv_planar_pair, B'x or the forward DOT form: never split,
    // fused or with holes), its run-rows the wide ones' 288 values as floats in put_pair_run's arrangement (1152 B: 16-B aligned)
    const bool narrow = esz == 8 && (pair ? h->narrow_pairs
                                          : planar ? h->narrow_planar && split == 1 && !b.fused && !holes
                                                   : h->narrow_values);
    const int vsz = narrow ? 4 : esz;
    b.vsz = narrow ? 4 : 0;
    ps.o_val = ar.reserve(E * w * vsz * (pair ? 3 : 1));
    if (narrow && h->rec) h->rec->narrow.emplace_back(ps.o_val, ps.o_val + (size_t)E * w * vsz * (pair ? 3 : 1));
    ps.o_out = ar.reserve(std::max<size_t>(out.size(), 1) * 4);
    ps.o_rrow = ar.reserve(rrow.size() * 4);
    ps.o_rchunk = ar.reserve(rchunk.size() * 4);
    if (b.mask) ps.o_nlive = ar.reserve((size_t)rows * 4);
    std::memcpy(ar.at<int32_t>(ps.o_out), out.data(), out.size() * 4);
    std::memcpy(ar.at<int32_t>(ps.o_rrow), rrow.data(), rrow.size() * 4);
    std::memcpy(ar.at<int32_t>(ps.o_rchunk), rchunk.data(), rchunk.size() * 4);
    uint32_t *key = ps.keys.data();
    char *vv = ar.at<char>(ps.o_val);
    int64_t row = 0;
    if (pair) {  // run-rows of 32 stripes: segments A (64 lanes x 16 B), B, C, D (vbc_planar.h run_pair)
        for (int64_t c = 0; c < nch; c++) {
            for (int32_t qr = 0; qr < cr[c]; qr++, row++) {
                const uint32_t last = qr + 1 == cr[c] ? kLast : 0u;
                char *blk = vv + row * 288 * vsz;
                if (b.mask) {  // live stripe slots of this run-row: a prefix in chunk-local length order
                    uint32_t nl = 0;
                    for (int sl = 0; sl < 32; sl++) {
                        const int64_t seg = c * 32 + sl;
                        if (seg < nseg && sbeg[seg] + 3 * qr < sbeg[seg + 1]) {
                            if (nl != (uint32_t)sl) return fail(VBC_INVALID_ARG, "masked pair chunk: live slots not a prefix");
                            nl++;
                        }
                    }
                    ar.at<uint32_t>(ps.o_nlive)[row] = nl;
                }
                for (int sl = 0; sl < 32; sl++) {
                    const int64_t seg = c * 32 + sl, e = row * 32 + sl;
                    const bool real_run = seg < nseg && sbeg[seg] + 3 * qr < sbeg[seg + 1];
                    double v[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
                    if (real_run) {
                        for (int d = 0; d < 3; d++)
                            std::memcpy(v[d], val + ents[pstart[seg] + 3 * qr + d].voff * esz, 3 * sizeof(double));
                        key[e] = ents[pstart[seg] + 3 * qr].key | last;
                    } else {
                        key[e] = kPad | last;
                    }
                    put_pair_run(h, narrow, blk, sl, v);
                }
            }
        }
    }
    for (int64_t c = 0; c < (pair ? 0 : nch); c++) {
        for (int32_t qr = 0; qr < cr[c]; qr++, row++) {
            const uint32_t last = qr + run == cr[c] ? kLast : 0u;  // on the last run's first row
            if (b.mask) {  // live lanes of this chunk row: a prefix in chunk-local length order
                uint32_t nl = 0;
                for (int sl = 0; sl < RPI; sl++) {
                    const int64_t seg = c * RPI + sl;
                    if (seg < nseg && sbeg[seg] + qr < sbeg[seg + 1]) {
                        if (nl != (uint32_t)sl) return fail(VBC_INVALID_ARG, "masked planar chunk: live lanes not a prefix");
                        nl++;
                    }
                }
                ar.at<uint32_t>(ps.o_nlive)[row] = nl;
            }
            for (int sl = 0; sl < RPI; sl++) {
                const int64_t seg = c * RPI + sl, e = row * RPI + sl;
                const bool real_row = seg < nseg && sbeg[seg] + qr < sbeg[seg + 1];
                const Entry *en = real_row ? &ents[pstart[seg] + qr] : nullptr;
                // padding rows gather x[0] (m >= 1: the bucket has entries), taken as 0
                key[e] = real_row ? (en->key | last) : (kPad | last);
                if (holes && real_row && qr % run == 0) {  // a run's first key: which of its rows are stored
                    uint32_t mk = 0;
                    for (int d = 0; d < run; d++) mk |= (en[d].voff >= 0 ? 1u : 0u) << (kHoleShift + d);
                    key[e] |= mk;
                }
                if (planar) {  // column-group-major chunk row (vbc_planar.h), in the arrangement of the stored size
                    char *rowp = vv + row * RPI * w * vsz;
                    for (int cc = 0; cc < w; cc++) {
                        char *dst = rowp + planar_off(vsz, w, sl, cc) * vsz;
                        const bool stored = real_row && cc < wsrc && en->voff >= 0;
                        if (stored && narrow) {
                            narrow_value(h, reinterpret_cast<const double *>(val) + en->voff + cc, dst);
                        } else if (stored) {
                            std::memcpy(dst, val + (en->voff + cc) * esz, (size_t)esz);
                        } else {
                            std::memset(dst, 0, (size_t)vsz);
                        }
                    }
                } else if (narrow) {  // (slotted, so never a run with holes: voff >= 0)
                    float *dst = reinterpret_cast<float *>(vv) + e * w;
                    const double *src = reinterpret_cast<const double *>(val) + (real_row ? en->voff : 0);
                    for (int cc = 0; cc < w; cc++) {
                        if (real_row && cc < wsrc) narrow_value(h, src + cc, dst + cc);
                        else dst[cc] = 0.0f;
                    }
                } else if (real_row) {
                    std::memcpy(vv + e * w * esz, val + en->voff * esz, (size_t)wsrc * esz);
                    if (wsrc < w) std::memset(vv + (e * w + wsrc) * esz, 0, (size_t)(w - wsrc) * esz);
                } else {
                    std::memset(vv + e * w * esz, 0, (size_t)w * esz);
                }
            }
        }
    }
    // compressed keys: measured faster on FE except the fp32 forward product (145 -> 158 us)
    const bool kc_wanted = h->slot_keys16 == 1 ? !(kind == 1 && esz == 4) : h->slot_keys16 == 2;
    // split bins (small matrices, latency-bound): 32-bit keys unless VBC_SPLIT_KC=1 -- a compressed key
    // costs a dependent scalar load (its row's pattern offset) before the key itself
    const bool split_kc = split == 1 || h->split_kc;
    ps.kc_ok = kc_wanted && split_kc && slot_keys_compressible(ps.keys, rows, RPI);
    return VBC_OK;
}

// Per-lane compacted streams (SlotBin::lanes, vbc_planar.h run_planar_lanes) for a planar B'x bucket in
// natural order with contiguous outputs (out[q] = out[0] + q * w, wsrc == w).  Tiles of S consecutive
// stripes (S a multiple of 4, at most one LDS tile buffer: 512 fp64 / 1024 fp32 3-wide stripes), k
// tiles per range, the ranges ~ the kernel's resident waves; inside a tile the stripes are cut into 64
// contiguous sub-blocks minimising the longest stream (binary search on the step count), and the
// sub-blocks go to the lanes by decreasing length, so the live lanes of every step are a prefix.
// An empty stripe is one zero run with PAD | LAST.  ents[sbeg[q] ..] are stripe q's rows (gather index
// keys), rows in runs of `run`.
// Whether a planar B'x bucket runs the lane-stream layout: VBC_PLANAR_LANES=1 forces it (where
// representable), 0 never; auto: a bucket the masked order would take (natural order pads beyond
// slots_pad) with natural contiguous outputs, few empty stripes, and >= 256 stripes per resident wave
// (sub-blocks of ~4 stripes per lane balance the streams).
bool want_lanes(const PlanCtx *h, int wps, int w, const std::vector<int64_t> &sbeg,
                const std::vector<int32_t> &out, int64_t total_entries, bool mask)
{
    if (h->planar_lanes == 0 || !slot_planar(h, 0, w) || wps != w) return false;
    const int64_t nseg = (int64_t)sbeg.size() - 1;
    if (nseg < 64 || nseg >= (int64_t(1) << 31)) return false;
    for (size_t q = 1; q < out.size(); q++)
        if ((int64_t)out[q] != (int64_t)out[0] + (int64_t)q * w) return false;
    int64_t empty = 0;
    for (int64_t q = 0; q < nseg; q++) empty += sbeg[q + 1] == sbeg[q];
    if (h->planar_lanes == 1) return true;
    if (!mask || empty * 100 > nseg) return false;
    const int64_t real = sbeg[nseg] - sbeg[0];
    const double share = (double)h->target_ranges_l * (double)real / (double)std::max<int64_t>(total_entries, 1);
    return (double)nseg >= 256.0 * std::max(1.0, share);
}

int build_lanes(PlanCtx *h, int w, const std::vector<Entry> &ents, const std::vector<int64_t> &sbeg,
                const std::vector<int32_t> &out, int run, int64_t total_entries, const char *val, Arena &ar,
                PendingSlot &ps)
{
    const int esz = h->esz;
    // lane pairs (spmv_pair_lanes): fp64 3-wide stripes in runs of 3 -- one 16-B x gather per lane per run
    const bool pair = h->lanes_pair && esz == 8 && w == 3 && run == 3;
    const int NS = pair ? 32 : 64;  // streams per tile
    const int64_t nseg = (int64_t)sbeg.size() - 1;
    const int64_t real = sbeg[nseg] - sbeg[0];
    std::vector<int32_t> len(nseg);  // runs per stripe (an empty stripe: one zero run)
    for (int64_t q = 0; q < nseg; q++) len[q] = (int32_t)std::max<int64_t>(1, (sbeg[q + 1] - sbeg[q]) / run);
    // (sized for half the resident waves -- round 5: fewer, longer tiles near the LDS cap; FE-3D 12,255 tiles of
    // 272 stripes 218.2 us, 10,163 of 328 213.8 us, profiles/r05zh_lanes_ab.log -- the selection rule above
    // keeps the full count)
    const double share = (double)h->target_ranges_l / std::max(1, h->lanes_rdiv) * (double)real /
                         (double)std::max<int64_t>(total_entries, 1);
    const int64_t nr_target = std::max<int64_t>(1, std::llround(share));
    // one tile per range (a wave) of at most one LDS tile buffer of outputs; S a multiple of 4 stripes,
    // the ranges a whole number of rounds of the target
    const int64_t smax = (kLaneTileBytes / (w * esz)) & ~3;
    const int64_t rounds = std::max<int64_t>(1, (nseg + nr_target * smax - 1) / (nr_target * smax));
    int64_t S = (nseg + rounds * nr_target - 1) / (rounds * nr_target);
    S = std::min<int64_t>(smax, std::max<int64_t>(4, (S + 3) / 4 * 4));
    const int64_t ntiles = (nseg + S - 1) / S, nr = ntiles;
    // per tile: NS contiguous streams (first stripe of each), their lengths in runs, the steps
    std::vector<int32_t> trow{0}, tseg;
    std::vector<int16_t> lseg((size_t)ntiles * 64);
    std::vector<std::vector<int32_t>> parts((size_t)ntiles);  // per tile: stream -> {first, end, runs}
    const int rows_per_step = pair ? 1 : run;  // a pair layout row is a run-row
    int64_t rows = 0;
    for (int64_t t = 0; t < ntiles; t++) {
        const int64_t a = t * S, e = std::min(nseg, a + S);
        tseg.push_back((int32_t)a);
        int64_t lo = 0, hi = 0;
        for (int64_t q = a; q < e; q++) {
            lo = std::max<int64_t>(lo, len[q]);
            hi += len[q];
        }
        auto nparts = [&](int64_t cap) {
            int64_t p = 1, cur = 0;
            for (int64_t q = a; q < e; q++) {
                if (cur + len[q] > cap) { p++; cur = len[q]; }
                else cur += len[q];
            }
            return p;
        };
        while (lo < hi) {
            const int64_t mid = (lo + hi) / 2;
            if (nparts(mid) <= NS) hi = mid;
            else lo = mid + 1;
        }
        const int64_t T = lo;
        std::vector<std::array<int64_t, 3>> pv;  // {length, first stripe, end}
        int64_t cur = 0, first = a;
        for (int64_t q = a; q < e; q++) {
            if (cur + len[q] > T) { pv.push_back({cur, first, q}); first = q; cur = 0; }
            cur += len[q];
        }
        pv.push_back({cur, first, e});
        std::stable_sort(pv.begin(), pv.end(), [](const std::array<int64_t, 3> &p, const std::array<int64_t, 3> &q) {
            return p[0] > q[0];
        });
        std::vector<int32_t> &pt = parts[t];
        for (int l = 0; l < 64; l++) {
            const bool has = l < NS && l < (int)pv.size();
            lseg[(size_t)t * 64 + l] = (int16_t)(has ? pv[l][1] - a : e - a);
            pt.push_back(has ? (int32_t)pv[l][1] : (int32_t)e);
            pt.push_back(has ? (int32_t)pv[l][2] : (int32_t)e);
            pt.push_back(has ? (int32_t)pv[l][0] : 0);  // the stream's length (runs)
        }
        rows += T * rows_per_step;
        trow.push_back((int32_t)rows);
    }
    tseg.push_back((int32_t)nseg);
    if (rows * 64 >= (int64_t(1) << 31)) return fail(VBC_INVALID_ARG, "lane-stream layout too large");
    const std::vector<int32_t> &rrow = trow;  // one tile per range
    std::vector<int32_t> rchunk(nr + 1);
    for (int64_t r = 0; r <= nr; r++) rchunk[r] = (int32_t)r;
    if (h->verbose)
        fprintf(stderr, "[vbc] lanes bin w %d run %d pair %d stripes %lld ranges %lld x %lld stripes (target %d), rows "
                "%lld (live %.3f)\n", w, run, (int)pair, (long long)nseg, (long long)nr, (long long)S, h->target_ranges_l,
                (long long)rows, (double)real / (double)std::max<int64_t>(1, rows * NS * (run / rows_per_step)));
    ps = PendingSlot{};
    SlotBin &b = ps.b;
    b.kind = 0;
    b.wkey = w;
    b.w = w;
    b.wst = w;
    b.rpi = NS;
    b.nranges = (int32_t)nr;
    b.nseg = (int32_t)nseg;
    b.u = h->slot_u;
    b.diag = h->diag;
    b.xcd = h->xcd_p;
    b.spl = 1;
    b.planar = 1;
    b.run = run;
    b.split = 1;
    b.pair = pair ? 1 : 0;
    b.mask = 1;
    b.lanes = 1;
    b.deep = h->lanes_deep;
    b.ntiles = (int32_t)ntiles;
    b.out_affine = 1;
    b.out_base = out.empty() ? 0 : out[0];
    b.out_stride = w;
    b.contig = 1;
    ps.rows = rows;
    ps.real = real;
    const int64_t vals_per_row = pair ? 288 : (int64_t)64 * w;
    const int64_t keys_per_row = NS;
    // VBC_CREATE_NARROW_PAIRS (build_slots): the lane-pair streams store floats, run-rows of 288 (put_pair_run);
    // everything above was decided with esz.  VBC_CREATE_NARROW_STREAMS: so do the plain lane streams (B'x and,
    // through build_fwd_lanes, forward), their rows in the Float32 column-group arrangement (planar_off(4, ...), rows
    // of 64 * w floats: 16-B aligned) -- S, smax, the tile count, nr_target and the stream cut above used esz.
    const bool narrow = esz == 8 && (pair ? h->narrow_pairs : h->narrow_streams);
    const int vsz = narrow ? 4 : esz;
    b.vsz = narrow ? 4 : 0;
    ps.o_val = ar.reserve((size_t)rows * vals_per_row * vsz);
    if (narrow && h->rec) h->rec->narrow.emplace_back(ps.o_val, ps.o_val + (size_t)rows * vals_per_row * vsz);
    ps.o_out = ar.reserve(4);
    ps.o_rrow = ar.reserve(rrow.size() * 4);
    ps.o_rchunk = ar.reserve(rchunk.size() * 4);
    ps.o_nlive = ar.reserve((size_t)rows * 4);
    ps.o_trow = ar.reserve(trow.size() * 4);
    ps.o_tseg = ar.reserve(tseg.size() * 4);
    ps.o_lseg = ar.reserve(lseg.size() * 2);
    ps.o_key = ar.reserve((size_t)rows * keys_per_row * 4);
    ps.key_bytes = (int64_t)(real / run) * 4;  // one key per run is read
    ps.lanes_done = true;
    std::memcpy(ar.at<int32_t>(ps.o_rrow), rrow.data(), rrow.size() * 4);
    std::memcpy(ar.at<int32_t>(ps.o_rchunk), rchunk.data(), rchunk.size() * 4);
    std::memcpy(ar.at<int32_t>(ps.o_trow), trow.data(), trow.size() * 4);
    std::memcpy(ar.at<int32_t>(ps.o_tseg), tseg.data(), tseg.size() * 4);
    std::memcpy(ar.at<int16_t>(ps.o_lseg), lseg.data(), lseg.size() * 2);
    *ar.at<int32_t>(ps.o_out) = b.out_base;
    uint32_t *key = ar.at<uint32_t>(ps.o_key);
    uint32_t *nlv = ar.at<uint32_t>(ps.o_nlive);
    char *vv = ar.at<char>(ps.o_val);
    std::memset(vv, 0, (size_t)rows * vals_per_row * vsz);
    std::memset(key, 0, (size_t)rows * keys_per_row * 4);
    for (int64_t t = 0; t < ntiles; t++) {
        const int64_t R0 = trow[t], T = (trow[t + 1] - R0) / rows_per_step;
        for (int64_t st = 0; st < T; st++) {
            uint32_t nl = 0;  // streams are in decreasing length: the live ones are a prefix
            while ((int)nl < NS && parts[t][3 * nl + 2] > st) nl++;
            for (int d = 0; d < rows_per_step; d++) nlv[R0 + st * rows_per_step + d] = nl;
        }
        for (int l = 0; l < NS; l++) {
            int64_t st = 0;
            for (int32_t q = parts[t][3 * l]; q < parts[t][3 * l + 1]; q++) {
                const int64_t nrun = (sbeg[q + 1] - sbeg[q]) / run;
                if (nrun == 0) {  // empty stripe: one zero run, PAD | LAST (writes its zeros)
                    key[(R0 + st * rows_per_step) * keys_per_row + l] = kPad | kLast;
                    st++;
                    continue;
                }
                for (int64_t u = 0; u < nrun; u++, st++) {
                    const int64_t row0 = R0 + st * rows_per_step;
                    key[row0 * keys_per_row + l] = ents[sbeg[q] + u * run].key | (u + 1 == nrun ? kLast : 0u);
                    if (pair) {  // the run's 3 x 3 values in the pair run-row form (run_pair)
                        double v[3][3];
                        for (int d = 0; d < 3; d++)
                            std::memcpy(v[d], val + ents[sbeg[q] + u * 3 + d].voff * esz, 3 * sizeof(double));
                        put_pair_run(h, narrow, vv + row0 * 288 * vsz, l, v);
                        continue;
                    }
                    for (int d = 0; d < run; d++) {
                        const Entry &en = ents[sbeg[q] + u * run + d];
                        char *rowp = vv + (row0 + d) * 64 * w * vsz;
                        for (int cc = 0; cc < w; cc++) {
                            char *dst = rowp + planar_off(vsz, w, l, cc) * vsz;
                            if (narrow) narrow_value(h, reinterpret_cast<const double *>(val) + en.voff + cc, dst);
                            else std::memcpy(dst, val + (en.voff + cc) * esz, (size_t)esz);
                        }
                    }
                }
            }
        }
    }
    return VBC_OK;
}

// One launch's slotted bins share one key form (the kernel is specialised on it).
void commit_launch_keys(const PlanCtx *h, std::vector<PendingSlot> &pss, Arena &ar)
{
    bool kc = false;
    for (const PendingSlot &ps : pss) {
        if (ps.lanes_done) continue;  // the lanes layout stores its own keys (its own launch)
        kc = true;
    }
    for (const PendingSlot &ps : pss) kc = kc && (ps.lanes_done || ps.kc_ok);
    for (PendingSlot &ps : pss)
        if (!ps.lanes_done) commit_slot_keys(ps, kc, ar, h->slot_dedup);
}

// ---- row-swept layout (vbc_sweep.hip) ------------------------------------------------------------

// Whether a bucket lacks x locality: the gathers of windows of 64 consecutive segments (the segments
// one slotted chunk folds together) span most of an x (length nx) too large for L2.  Mesh operators
// span a few bandwidths (FE: ~10^4 rows of 10^7); the costs.jl:63-83 generator spans all of x.
// Segment q's entries are ents[sbeg[q] .. sbeg[q+1]), keys = gather index.
bool sweep_possible(const PlanCtx *h, int w, int64_t nx)
{
    return h->sweep_mode != 0 && w <= 8 && nx < kSlotIdxLimit && (h->sweep_mode == 1 || (double)nx * h->esz >= 16e6);
}

bool want_sweep(const PlanCtx *h, int w, int64_t nx, const std::vector<int64_t> &sbeg,
                const std::vector<Entry> &ents)
{
    const int64_t nseg = (int64_t)sbeg.size() - 1;
    if (h->sweep_mode == 0 || w > 8 || nx >= kSlotIdxLimit || nseg <= 0 || nseg >= (int64_t(1) << 31)) return false;
    if (h->sweep_mode == 1) return true;
    const double xbytes = (double)nx * h->esz;
    if (xbytes < 16e6) return false;  // x stays in L2 / MALL anyway
    std::vector<double> span;
    for (int64_t a = 0; a < nseg; a += 64) {
        int64_t lo = INT64_MAX, hi = -1;
        for (int64_t e = sbeg[a]; e < sbeg[std::min(nseg, a + 64)]; e++) {
            lo = std::min<int64_t>(lo, ents[e].key);
            hi = std::max<int64_t>(hi, ents[e].key);
        }
        if (hi >= 0) span.push_back((double)(hi - lo + 1) * h->esz);
    }
    if (span.empty()) return false;
    std::nth_element(span.begin(), span.begin() + span.size() / 2, span.end());
    return span[span.size() / 2] >= 0.25 * xbytes;
}

// Segments per tile: as many as the wave's LDS tile holds (kind 0: w accumulators per stripe, kind 1:
// one per output row).  Capping narrow buckets so that every tile costs the same measured slower on
// the mixed-width NS workload (379 -> 395 us).
static int sweep_segments(const PlanCtx *h, int kind, int w)
{
    return (int)std::max(1, std::min(65535, h->sweep_tile / ((kind == 0 ? w : 1) * h->esz)));
}

// Lay out a swept bucket: tiles of S segments; each tile's entries in 64-lane steps, taken in
// ascending gather order by a min-heap over the segments' next entries (a segment enters a step at
// most once, and its entries keep their stored order).  out[q] = y offset of segment q.
int build_sweep(PlanCtx *h, int kind, int w, const std::vector<int64_t> &sbeg,
                const std::vector<Entry> &ents, const std::vector<int32_t> &out, const char *val, Arena &ar,
                int &tile0, PendingSweep &pw)
{
    const int esz = h->esz;
    const int64_t nseg = (int64_t)sbeg.size() - 1;
    const int S = sweep_segments(h, kind, w);
    const int64_t ntiles = (nseg + S - 1) / S;
    if (tile0 + ntiles >= (int64_t(1) << 31)) return fail(VBC_INVALID_ARG, "bucket too large");
    std::vector<int32_t> tstep{0};
    std::vector<uint32_t> keys;
    std::vector<uint16_t> locs;
    std::vector<int64_t> voffs;  // value offset of each lane slot, -1 = padding
    keys.reserve(ents.size() + 64 * ntiles);
    locs.reserve(ents.size() + 64 * ntiles);
    voffs.reserve(ents.size() + 64 * ntiles);
    typedef std::pair<uint32_t, int32_t> Head;  // (gather index, segment within tile)
    std::vector<Head> heap, picks;
    std::vector<int64_t> cur(S);
    for (int64_t t = 0; t < ntiles; t++) {
        const int64_t s0 = t * S;
        const int ns = (int)std::min<int64_t>(S, nseg - s0);
        heap.clear();
        for (int q = 0; q < ns; q++) {
            cur[q] = sbeg[s0 + q];
            if (cur[q] < sbeg[s0 + q + 1]) heap.push_back({ents[cur[q]].key, q});
        }
        std::make_heap(heap.begin(), heap.end(), std::greater<Head>());
        while (!heap.empty()) {
            picks.clear();
            while (!heap.empty() && picks.size() < 64) {
                std::pop_heap(heap.begin(), heap.end(), std::greater<Head>());
                picks.push_back(heap.back());
                heap.pop_back();
            }
            for (const Head &p : picks) {
                keys.push_back(p.first);
                locs.push_back((uint16_t)p.second);
                voffs.push_back(ents[cur[p.second]].voff);
            }
            for (size_t k = picks.size(); k < 64; k++) {
                keys.push_back(kPad);
                locs.push_back(0);
                voffs.push_back(-1);
            }
            for (const Head &p : picks)
                if (++cur[p.second] < sbeg[s0 + p.second + 1]) {
                    heap.push_back({ents[cur[p.second]].key, p.second});
                    std::push_heap(heap.begin(), heap.end(), std::greater<Head>());
                }
        }
        if ((int64_t)keys.size() / 64 >= (int64_t(1) << 31)) return fail(VBC_INVALID_ARG, "bucket too large");
        tstep.push_back((int32_t)(keys.size() / 64));
    }
    // Packed keys: a step's 64 entries are consecutive picks of the ascending heap, so their gather
    // indices lie within a narrow window above the first lane's: key = PAD | segment << lbits | delta,
    // one 32-bit load per lane instead of the 32-bit index plus the 16-bit segment (6 -> 4 B per entry
    // and one load instruction less per step), the base read once per step through the scalar cache.
    const int64_t nsteps = (int64_t)keys.size() / 64;
    int sbits = 1;
    while ((1 << sbits) < S) sbits++;
    const int lbits = 31 - sbits;
    bool packed = h->sweep_pack != 0 && lbits >= 8;
    std::vector<uint32_t> sbase;
    if (packed) {
        sbase.resize((size_t)nsteps);
        for (int64_t st = 0; st < nsteps && packed; st++) {
            const uint32_t b0 = keys[st * 64];  // the smallest pick: never padding
            sbase[st] = b0 & kSlotIdx;
            for (int l = 0; l < 64; l++) {
                const uint32_t k = keys[st * 64 + l];
                if (k & kPad) continue;
                if (k < b0 || ((k - b0) >> lbits) != 0) { packed = false; break; }
            }
        }
    }
    if (packed)
        for (int64_t e = 0; e < (int64_t)keys.size(); e++) {
            const uint32_t k = keys[e];
            keys[e] = (k & kPad) ? kPad : ((uint32_t)locs[e] << lbits) | (k - sbase[e / 64]);
        }
    pw = PendingSweep{};
    SweepBin &b = pw.b;
    b.kind = kind;
    b.packed = packed ? 1 : 0;
    b.lbits = packed ? lbits : 0;
    b.w = w;
    b.tile0 = tile0;
    b.ntiles = (int32_t)ntiles;
    b.S = S;
    b.nseg = (int32_t)nseg;
    b.out_affine = 1;
    b.out_base = out.empty() ? 0 : out[0];
    b.out_stride = out.size() > 1 ? out[1] - out[0] : 0;
    for (size_t q = 1; q < out.size() && b.out_affine; q++)
        b.out_affine = (int64_t)out[q] == (int64_t)out[0] + (int64_t)q * b.out_stride;
    tile0 += (int)ntiles;
    const int64_t E = (int64_t)keys.size();
    pw.o_tstep = ar.reserve(tstep.size() * 4);
    pw.o_key = ar.reserve(E * 4);
    pw.o_loc = ar.reserve(packed ? 4 : E * 2);
    pw.o_sbase = ar.reserve(packed ? (size_t)nsteps * 4 : 4);
    // VBC_CREATE_NARROW_SWEPT: the value rows store floats, row e at float offset e * w (an arena reservation, so
    // 16-B aligned); everything above -- S, the steps, the keys, packing -- was decided with esz.
    const bool narrow = esz == 8 && h->narrow_swept;
    const int vsz = narrow ? 4 : esz;
    b.vsz = narrow ? 4 : 0;
    pw.o_val = ar.reserve(E * w * vsz);
    if (narrow && h->rec) h->rec->narrow.emplace_back(pw.o_val, pw.o_val + (size_t)E * w * vsz);
    pw.o_out = ar.reserve(out.size() * 4);
    std::memcpy(ar.at<int32_t>(pw.o_tstep), tstep.data(), tstep.size() * 4);
    std::memcpy(ar.at<uint32_t>(pw.o_key), keys.data(), E * 4);
    if (packed) std::memcpy(ar.at<uint32_t>(pw.o_sbase), sbase.data(), (size_t)nsteps * 4);
    else std::memcpy(ar.at<uint16_t>(pw.o_loc), locs.data(), E * 2);
    std::memcpy(ar.at<int32_t>(pw.o_out), out.data(), out.size() * 4);
    char *vv = ar.at<char>(pw.o_val);
    for (int64_t e = 0; e < E; e++) {
        if (voffs[e] < 0) std::memset(vv + e * w * vsz, 0, (size_t)w * vsz);
        else if (narrow)
            for (int cc = 0; cc < w; cc++)
                narrow_value(h, reinterpret_cast<const double *>(val) + voffs[e] + cc, vv + (e * w + cc) * 4);
        else std::memcpy(vv + e * w * esz, val + voffs[e] * esz, (size_t)w * esz);
    }
    (kind == 0 ? h->st.bytes_t : h->st.bytes_f) +=
        E * ((packed ? 4 : 6) + (int64_t)w * vsz) + (packed ? nsteps * 4 : 0) + (int64_t)tstep.size() * 4 +
        (b.out_affine ? 0 : nseg * 4);
    return VBC_OK;
}

}  // namespace vbc
