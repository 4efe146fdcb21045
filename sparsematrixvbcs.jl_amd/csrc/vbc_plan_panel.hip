// The layout planner's multi-RHS layouts: the tile and panel layouts of the transposed product (build_tiles,
// build_panel), C = Bᵀ as stripes (transpose_stripes, which the forward-on-Bᵀ layout of vbc_plan.hip shares) and the
// forward panel layout built from it (build_forward_panel).  Pure host code (vbc_plan.h): no HIP call, no
// environment.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "vbc_plan_impl.h"

namespace vbc {

// Tile layout (vbc_tiles.h) of one width bucket (w <= 4, whole stripes) of the multi-RHS product: each
// stripe's stored rows grouped into tiles of consecutive rows of one row group -- Π's block rows (tgrp:
// their 0-based starts + m; a SparseMatrixVBC's u x w blocks, constructors_VBC.jl:95-105) or, for a 1DVBC,
// aligned runs of R rows (R in {4, 3, 2}: the node runs of a stiffness operator; the R adding the fewest
// tiles within kTilePad of padding).  A tile slot holds ub rows x w values (rows the tile does not store:
// zeros, masked in its key).  Stripes in natural order are cut into ranges (one wave each) of at most
// smax stripes (the LDS output stage) balanced by tiles, a whole number of rounds of resident waves; each
// range into 4 streams of consecutive stripes balanced by tiles (the wave's 16-lane rows), every stream
// padded to the longest with invalid tiles.  Returns false (nothing built) when the bucket does not fit:
// a tile taller than 4 rows, too much padding, too few rows per tile (auto), rows >= 2^26.
constexpr double kTilePad = 1.25;

// Launch order of the tile ranges (round 6): BFS balls of K ranges over the graph "two ranges store a tile of
// the same X row group", ball after ball.  Each XCD takes a contiguous run of the launch's ranges and keeps
// about K of them resident (K = one XCD's share of the wave slots), so at any moment it folds one ball: a
// compact region of the operator whose X rows -- its groups plus one layer -- fit the XCD's 4 MB L2, where
// the natural order's resident ranges form a slab of consecutive stripes whose X window (a 3D mesh's +-g^2
// rows) does not.  Only the order changes: every range keeps its stripes, streams and data.
// rg_off / rg_grp: the distinct row groups of each range (CSR, ranges in natural order).
static std::vector<int64_t> cluster_ranges(int64_t nrg, const std::vector<int64_t> &rg_off,
                                           const std::vector<int32_t> &rg_grp, int64_t ngroups, int64_t K)
{
    std::vector<int64_t> gcnt(ngroups + 1, 0);  // row group -> ranges (CSR)
    for (int32_t g : rg_grp) gcnt[g + 1]++;
    for (int64_t g = 0; g < ngroups; g++) gcnt[g + 1] += gcnt[g];
    std::vector<int32_t> grg(rg_grp.size());
    {
        std::vector<int64_t> pos(gcnt.begin(), gcnt.end() - 1);
        for (int64_t r = 0; r < nrg; r++)
            for (int64_t q = rg_off[r]; q < rg_off[r + 1]; q++) grg[pos[rg_grp[q]]++] = (int32_t)r;
    }
    std::vector<int64_t> order;
    order.reserve(nrg);
    std::vector<char> done(nrg, 0), gseen(ngroups, 0);
    std::vector<int64_t> touched;  // groups expanded by the current ball (reset after it)
    int64_t seed = 0;
    while ((int64_t)order.size() < nrg) {
        while (done[seed]) seed++;
        const size_t b0 = order.size();
        order.push_back(seed);
        done[seed] = 1;
        for (size_t h = b0; h < order.size() && (int64_t)(order.size() - b0) < K; h++) {
            const int64_t r = order[h];
            for (int64_t q = rg_off[r]; q < rg_off[r + 1] && (int64_t)(order.size() - b0) < K; q++) {
                const int32_t g = rg_grp[q];
                if (gseen[g]) continue;
                gseen[g] = 1;
                touched.push_back(g);
                for (int64_t t = gcnt[g]; t < gcnt[g + 1] && (int64_t)(order.size() - b0) < K; t++) {
                    const int32_t r2 = grg[t];
                    if (!done[r2]) {
                        done[r2] = 1;
                        order.push_back(r2);
                    }
                }
            }
        }
        for (int64_t g : touched) gseen[g] = 0;
        touched.clear();
    }
    return order;
}

static bool build_tiles(PlanCtx *h, const Stripes &s, const std::vector<int64_t> &stripes_in, int w,
                        const std::vector<int64_t> *tgrp, const char *val, Arena &ar, PendingPanel &pp)
{
    const std::vector<int64_t> &stripes = stripes_in;  // (natural order)
    if (h->panel_tiles == 0 || w < 1 || w > 4 || stripes.empty() || s.m >= (int64_t)kTileRow) return false;
    for (int64_t l : stripes)
        if (s.w[l] != w || s.vstride(l) != w) return false;
    const int esz = h->esz;
    int64_t rows = 0;
    for (int64_t l : stripes) rows += s.rbeg[l + 1] - s.rbeg[l];
    // group of a row: base row and height
    std::vector<int32_t> gk;  // tgrp: row -> block row
    if (tgrp) {
        gk.assign((size_t)s.m, 0);
        for (size_t k = 0; k + 1 < tgrp->size(); k++)
            for (int64_t i = (*tgrp)[k]; i < (*tgrp)[k + 1] && i < s.m; i++) gk[i] = (int32_t)k;
    }
    // tiles of a stripe under grouping R (R = 0: tgrp): consecutive stored rows of one group, a repeated
    // slot row (a hand-built stripe storing a row twice) starting a new tile
    auto group_of = [&](int64_t row, int R, int64_t &base, int &u) {
        if (R == 0) {
            const int32_t k = gk[row];
            base = (*tgrp)[k];
            u = (int)((*tgrp)[k + 1] - base);
        } else {
            base = row / R * R;
            u = R;
        }
    };
    auto count = [&](int R, int64_t &tiles, int &ub) {
        tiles = 0;
        ub = 1;
        for (int64_t l : stripes) {
            int64_t cb = -1;
            unsigned seen = 0;
            for (int64_t q = s.rbeg[l]; q < s.rbeg[l + 1]; q++) {
                int64_t base;
                int u;
                group_of(s.rows[q], R, base, u);
                if (u > 4) return false;
                const unsigned bit = 1u << (s.rows[q] - base);
                if (base != cb || (seen & bit)) {
                    tiles++;
                    cb = base;
                    seen = 0;
                }
                seen |= bit;
                ub = std::max(ub, u);
            }
        }
        return true;
    };
    int R = 0, ub = 1;
    int64_t tiles = 0;
    if (tgrp) {
        if (!count(0, tiles, ub)) return false;
        if ((double)tiles * ub > kTilePad * (double)std::max<int64_t>(rows, 1) && h->panel_tiles < 0) return false;
    } else {
        int64_t best = -1;
        for (int Rc = 4; Rc >= 1; Rc--) {
            int64_t t;
            int u;
            count(Rc, t, u);
            if (Rc > 1 && (double)t * Rc > kTilePad * (double)std::max<int64_t>(rows, 1)) continue;
            if (best < 0 || t < best) {
                best = t;
                R = Rc;
                ub = Rc;
                tiles = t;
            }
        }
    }
    // auto: only when tiles carry work (>= 1.5 rows each); VBC_PANEL_TILES=1 takes any
    if (h->panel_tiles < 0 && (double)rows < 1.5 * (double)std::max<int64_t>(tiles, 1)) return false;
    const int TV = ub * w;
    const int64_t n = (int64_t)stripes.size();
    std::vector<int64_t> tl(n);  // tiles per stripe (an empty stripe: one invalid LAST tile)
    {
        for (int64_t i = 0; i < n; i++) {
            const int64_t l = stripes[i];
            int64_t t = 0, cb = -1;
            unsigned seen = 0;
            for (int64_t q = s.rbeg[l]; q < s.rbeg[l + 1]; q++) {
                int64_t base;
                int u;
                group_of(s.rows[q], R, base, u);
                const unsigned bit = 1u << (s.rows[q] - base);
                if (base != cb || (seen & bit)) {
                    t++;
                    cb = base;
                    seen = 0;
                }
                seen |= bit;
            }
            tl[i] = std::max<int64_t>(t, 1);
        }
    }
    // ranges: <= smax stripes (the LDS stage), a whole number of rounds of resident waves, balanced by tiles
    const int64_t smax = std::max<int64_t>(1, kTileStageBytes / (w * 16 * esz));
    const int64_t slots = (int64_t)h->cus * std::max(1, h->occ_tiles);
    int64_t total = 0;
    for (int64_t t : tl) total += t;
    const int nbt = h->tile_nbt;  // the kernel's batch (streams padded to whole pairs of batches)
    // Ranges of ~tile_spr stripes: the hardware dispatches workgroups in order and each XCD takes a
    // contiguous run of ranges (xcd_block), so the stripes in flight on an XCD span its resident waves x
    // the range length -- and a 3D mesh's X rows are reused across +-g^2 nodes, so that front must stay
    // narrow for the X tiles to hit in the XCD's 4 MB L2 (c5-mesh: 28 stripes per range, L2 hit rate 57 %).
    int64_t nr = std::max<int64_t>((n + smax - 1) / smax, 1);
    nr = std::max<int64_t>(nr, (n + h->tile_spr - 1) / std::max(1, h->tile_spr));
    // few ranges: a whole number of rounds of resident waves, but no range so short that its streams'
    // padding to whole key pairs dominates (>= 4 batch pairs per stream on average)
    if (nr < 2 * slots) {
        const int64_t nr_cap = std::max<int64_t>(nr, total / (4 * 8 * nbt));
        nr = std::min<int64_t>(nr_cap, (nr + slots - 1) / slots * slots);
    }
    nr = std::min<int64_t>(n, nr);
    if (h->tile_ranges > 0) nr = std::min<int64_t>(n, h->tile_ranges);
    std::vector<int64_t> rb{0};  // range starts (stripe index)
    {
        int64_t cum = 0;
        for (int64_t i = 0; i < n; i++) {
            const int64_t cnt = i - rb.back();
            if (cnt > 0 && (cnt >= smax || (cum * nr >= (int64_t)rb.size() * total && (int64_t)rb.size() < nr))) rb.push_back(i);
            cum += tl[i];
        }
        rb.push_back(n);
    }
    const int64_t nrg = (int64_t)rb.size() - 1;
    // streams of each range: 4 runs of consecutive stripes balanced by tiles
    std::vector<int32_t> rinfo((size_t)nrg * 8, 0);
    std::vector<std::array<int64_t, 5>> sb(nrg);
    int64_t slot_total = 0;
    for (int64_t r = 0; r < nrg; r++) {
        const int64_t a = rb[r], e = rb[r + 1];
        int64_t rt = 0;
        for (int64_t i = a; i < e; i++) rt += tl[i];
        auto &b = sb[r];
        b[0] = a;
        int64_t cum = 0, i = a;
        for (int k = 1; k < 4; k++) {
            // first stripe of stream k: where the cumulative tiles pass k / 4 of the range's (closer side)
            while (i < e && (cum + tl[i]) * 4 <= k * rt) cum += tl[i++];
            if (i < e && (cum + tl[i]) * 4 - k * rt < k * rt - cum * 4) cum += tl[i++];
            b[k] = i;
        }
        b[4] = e;
        int64_t len = 0;
        for (int k = 0; k < 4; k++) {
            int64_t t = 0;
            for (int64_t q = b[k]; q < b[k + 1]; q++) t += tl[q];
            len = std::max(len, t);
        }
        len = (len + 2 * nbt - 1) / (2 * nbt) * (2 * nbt);  // whole key pairs (vbc_tiles.h)
        int32_t *ri = &rinfo[(size_t)r * 8];
        ri[0] = (int32_t)slot_total;
        ri[1] = (int32_t)len;
        ri[2] = (int32_t)a;
        ri[3] = (int32_t)(e - a);
        for (int k = 1; k < 4; k++) ri[3 + k] = (int32_t)(b[k] - a);
        slot_total += 4 * len;
        if (slot_total >= (int64_t(1) << 31) / std::max(1, TV)) return false;
    }
    // over-read padding past the last stream: keys 3 D batches ahead, values 2 D (vbc_tiles.h)
    const int dep = h->tile_depth;
    const int64_t kpad = 3 * dep * nbt + 16, vpad = (int64_t)(2 * dep * nbt + 2) * TV + 64;
    pp = PendingPanel{};
    pp.tile = true;
    TileBin &tb = pp.tb;
    tb.w = w;
    tb.ub = ub;
    tb.nbt = nbt;
    tb.depth = dep;
    tb.diag = h->tile_diag;
    {
        int64_t most = 1;
        for (size_t r = 0; r + 1 < rb.size(); r++) most = std::max<int64_t>(most, rb[r + 1] - rb[r]);
        tb.stage_bytes = (int32_t)((most * w * 16 * esz + 15) / 16 * 16);
    }
    tb.nranges = (int32_t)nrg;
    std::vector<int32_t> out(n);
    for (int64_t i = 0; i < n; i++) out[i] = (int32_t)s.col0[stripes[i]];
    tb.out_affine = 1;
    tb.out_base = out[0];
    tb.out_stride = n > 1 ? out[1] - out[0] : w;
    for (int64_t i = 1; i < n && tb.out_affine; i++) tb.out_affine = (int64_t)out[i] == (int64_t)out[0] + i * tb.out_stride;
    pp.o_key = ar.reserve((slot_total + kpad) * 4);
    pp.o_val = ar.reserve((slot_total * TV + vpad) * esz);
    pp.o_out = ar.reserve(n * 4);
    pp.o_rgrp = ar.reserve(rinfo.size() * 4);
    std::memcpy(ar.at<int32_t>(pp.o_out), out.data(), out.size() * 4);
    std::memcpy(ar.at<int32_t>(pp.o_rgrp), rinfo.data(), rinfo.size() * 4);
    uint32_t *key = ar.at<uint32_t>(pp.o_key);
    char *vv = ar.at<char>(pp.o_val);
    std::fill(key, key + slot_total + kpad, kTileRow);  // padding: invalid tiles (row field all ones)
    std::memset(vv, 0, (size_t)(slot_total * TV + vpad) * esz);
    bool masku = false;
    // the distinct X row groups of each range (cluster_ranges): group = block row (tgrp) or row / R
    // (VBC_TILE_CLUSTER=2: any range count, balls of an eighth of the ranges -- small-scale tests)
    const int64_t K = h->tile_cluster == 2 ? std::max<int64_t>(1, nrg / 8) : std::max<int64_t>(1, slots / 8);
    const bool cluster = h->tile_cluster == 2 ? nrg >= 2 : h->tile_cluster && nrg >= 4 * K;
    const int64_t ngroups = R == 0 ? (int64_t)tgrp->size() : s.m / R + 1;
    std::vector<int64_t> rg_off{0};
    std::vector<int32_t> rg_grp, last;
    if (cluster) last.assign((size_t)ngroups, -1);
    for (int64_t r = 0; r < nrg; r++) {
        const int32_t *ri = &rinfo[(size_t)r * 8];
        const int64_t len = ri[1];
        for (int k = 0; k < 4; k++) {
            int64_t slot = ri[0] + k * len;  // this stream's next tile slot
            for (int64_t i = sb[r][k]; i < sb[r][k + 1]; i++) {
                const int64_t l = stripes[i];
                if (s.rbeg[l + 1] == s.rbeg[l]) {  // empty stripe: one invalid LAST tile (its columns get beta * Y)
                    key[slot++] = kTileLast | kTileRow;
                    continue;
                }
                int64_t cb = -1, kbase = 0;
                unsigned seen = 0;
                for (int64_t q = s.rbeg[l]; q < s.rbeg[l + 1]; q++) {
                    int64_t base;
                    int u;
                    group_of(s.rows[q], R, base, u);
                    const int rr = (int)(s.rows[q] - base);
                    const unsigned bit = 1u << rr;
                    if (base != cb || (seen & bit)) {
                        if (cluster) {
                            const int64_t gi = R == 0 ? gk[base] : base / R;
                            if (last[gi] != r) {
                                last[gi] = (int32_t)r;
                                rg_grp.push_back((int32_t)gi);
                            }
                        }
                        if (cb >= 0) {
                            key[slot] = (uint32_t)kbase | kTileValid | (seen << kTileMaskShift);
                            masku = masku || seen != (1u << ub) - 1;
                            slot++;
                        }
                        cb = base;
                        kbase = base;
                        seen = 0;
                    }
                    seen |= bit;
                    std::memcpy(vv + (slot * TV + (int64_t)rr * w) * esz, val + (s.voff[l] + (q - s.rbeg[l]) * w) * esz,
                                (size_t)w * esz);
                }
                key[slot] = (uint32_t)kbase | kTileValid | (seen << kTileMaskShift) | kTileLast;
                masku = masku || seen != (1u << ub) - 1;
                slot++;
            }
        }
        if (cluster) rg_off.push_back((int64_t)rg_grp.size());
    }
    if (cluster) {  // launch the ranges ball by ball (the arena's rinfo rows permuted; the data stays put)
        const std::vector<int64_t> ord = cluster_ranges(nrg, rg_off, rg_grp, ngroups, K);
        int32_t *dst = ar.at<int32_t>(pp.o_rgrp);
        for (int64_t q = 0; q < nrg; q++) std::memcpy(dst + q * 8, &rinfo[(size_t)ord[q] * 8], 8 * sizeof(int32_t));
    }
    tb.masku = masku ? 1 : 0;
    h->st.bytes_m += slot_total * (4 + (int64_t)TV * esz) + nrg * 32;
    if (h->verbose)
        fprintf(stderr, "[vbc] tiles: w %d, %lld stripes, %lld rows -> %lld tiles of <= %d rows (%s), %lld ranges, %lld slots%s%s\n",
                w, (long long)n, (long long)rows, (long long)total, ub, R == 0 ? "block rows" : "row runs", (long long)nrg,
                (long long)slot_total, masku ? ", masked rows" : "", cluster ? ", clustered launch order" : "");
    return true;
}

// Panel layout (vbc_panel.h) of the transposed product: per width bucket (stripes wider than 16 are
// cut into 16-column pieces that share the stripe's rows), S = 16/w consecutive stripes per panel,
// each panel's rows padded to a multiple of 4, ranges of whole panels balanced by rows.
int build_panel(PlanCtx *h, const Stripes &s, const char *val, Arena &ar, PanelPlan &plan,
                std::vector<int32_t> &fill, const std::vector<int64_t> *tgrp)
{
    struct Piece {
        int64_t l;
        int c0;
    };
    std::map<int, std::vector<Piece>> buckets;  // piece width -> pieces
    // Stripes that store no row stay in the layout with one HEAD sentinel row (zero contribution), so
    // uniform-width matrices keep an affine stripe -> column map and no fill list is needed.
    (void)fill;
    for (int64_t l = 0; l < s.L; l++)
        for (int c0 = 0; c0 < s.w[l]; c0 += 16) buckets[std::min(16, s.w[l] - c0)].push_back({l, c0});
    // small tiles (u, w <= 4): the tile-granular layout (vbc_tiles.h) instead of panels
    if (!tgrp && !s.grp.empty()) tgrp = &s.grp;
    for (auto it = buckets.begin(); it != buckets.end();) {
        bool whole = it->first <= 4;
        std::vector<int64_t> st;
        for (const Piece &pc : it->second) {
            whole = whole && pc.c0 == 0;
            st.push_back(pc.l);
        }
        PendingPanel pp;
        if (whole && build_tiles(h, s, st, it->first, tgrp, val, ar, pp)) {
            plan.bins.push_back(pp);
            it = buckets.erase(it);
        } else {
            ++it;
        }
    }
    const int esz = h->esz;
    // groups of every bucket first: ranges are spread over the launch in proportion to them
    std::map<int, std::vector<int64_t>> pgroups;  // w -> groups per panel
    int64_t total_groups = 0;
    for (auto &kv : buckets) {
        const int S = 16 / kv.first;
        auto &pg = pgroups[kv.first];
        for (size_t p0 = 0; p0 < kv.second.size(); p0 += S) {
            int64_t rows = 0;
            for (size_t p = p0; p < std::min(kv.second.size(), p0 + S); p++)
                rows += std::max<int64_t>(1, s.rbeg[kv.second[p].l + 1] - s.rbeg[kv.second[p].l]);
            pg.push_back((rows + 3) / 4);
            total_groups += pg.back();
        }
    }
    if (total_groups >= (int64_t(1) << 31)) return fail(VBC_INVALID_ARG, "matrix too large for the panel layout");
    int range0 = 0;
    for (auto &kv : buckets) {
        const int w = kv.first, S = 16 / w;
        const std::vector<Piece> &pcs = kv.second;
        const std::vector<int64_t> &pg = pgroups[w];
        int64_t G = 0;
        for (int64_t g : pg) G += g;
        int64_t nr = (int64_t)std::llround((double)h->target_ranges_m * (double)G / (double)std::max<int64_t>(total_groups, 1));
        nr = std::max<int64_t>(1, std::min<int64_t>(nr, (int64_t)pg.size()));
        std::vector<int32_t> rgrp{0}, rseg{0};
        int64_t acc = 0;
        for (size_t p = 0; p < pg.size(); p++) {
            acc += pg[p];
            // close a range once it holds its share of the bucket's groups
            if (p + 1 < pg.size() && (int64_t)rgrp.size() < nr && acc * nr >= (int64_t)rgrp.size() * G) {
                rgrp.push_back((int32_t)acc);
                rseg.push_back((int32_t)((p + 1) * S));
            }
        }
        rgrp.push_back((int32_t)acc);
        nr = (int64_t)rseg.size();
        PendingPanel pp{};
        pp.b.w = w;
        pp.b.S = S;
        pp.b.range0 = range0;
        pp.b.nranges = (int32_t)nr;
        range0 += (int)nr;
        std::vector<int32_t> out(pcs.size());
        for (size_t p = 0; p < pcs.size(); p++) out[p] = (int32_t)(s.col0[pcs[p].l] + pcs[p].c0);
        pp.b.out_affine = 1;
        pp.b.out_base = out[0];
        pp.b.out_stride = out.size() > 1 ? out[1] - out[0] : 0;
        for (size_t q = 1; q < out.size() && pp.b.out_affine; q++)
            pp.b.out_affine = (int64_t)out[q] == (int64_t)out[0] + (int64_t)q * pp.b.out_stride;
        const int64_t Rp = acc * 4;
        const int64_t Ra = Rp + kPanelTail;  // over-read padding (vbc_panel.h)
        h->st.panel_val_bytes = std::max<int64_t>(h->st.panel_val_bytes, Ra * w * esz);
        pp.b.val_bytes = (int32_t)std::min<int64_t>(Ra * w * esz, 0x7FFFFFFF);
        pp.o_key = ar.reserve(Ra * 4);
        pp.o_val = ar.reserve(Ra * w * esz);
        pp.o_out = ar.reserve(out.size() * 4);
        pp.o_rgrp = ar.reserve(rgrp.size() * 4);
        pp.o_rseg = ar.reserve(rseg.size() * 4);
        std::memcpy(ar.at<int32_t>(pp.o_out), out.data(), out.size() * 4);
        std::memcpy(ar.at<int32_t>(pp.o_rgrp), rgrp.data(), rgrp.size() * 4);
        std::memcpy(ar.at<int32_t>(pp.o_rseg), rseg.data(), rseg.size() * 4);
        uint32_t *key = ar.at<uint32_t>(pp.o_key);
        char *vv = ar.at<char>(pp.o_val);
        int64_t row = 0;
        for (size_t p0 = 0; p0 < pcs.size(); p0 += S) {
            for (size_t p = p0; p < std::min(pcs.size(), p0 + S); p++) {
                const int64_t l = pcs[p].l;
                const int wl = s.w[l];
                for (int64_t q = s.rbeg[l]; q < s.rbeg[l + 1]; q++, row++) {
                    key[row] = (uint32_t)s.rows[q] | (q == s.rbeg[l] ? kHead : 0u);
                    std::memcpy(vv + row * w * esz, val + (s.voff[l] + (q - s.rbeg[l]) * wl + pcs[p].c0) * esz,
                                (size_t)w * esz);
                }
                if (s.rbeg[l + 1] == s.rbeg[l]) {  // empty stripe: one HEAD sentinel row
                    key[row] = kPanelSentinel | kHead;
                    std::memset(vv + row * w * esz, 0, (size_t)w * esz);
                    row++;
                }
            }
            for (; row % 4; row++) {
                key[row] = kPanelSentinel;
                std::memset(vv + row * w * esz, 0, (size_t)w * esz);
            }
        }
        for (; row < Ra; row++) {
            key[row] = kPanelSentinel;
            std::memset(vv + row * w * esz, 0, (size_t)w * esz);
        }
        h->st.bytes_m += Rp * (4 + (int64_t)w * esz) + (int64_t)out.size() * 4;
        plan.bins.push_back(pp);
    }
    plan.L.total_ranges = range0;
    return VBC_OK;
}

// C = Bᵀ as stripes (the layouts of B's forward product built as transposed products of C): C's stripes
// are B's output row groups g (rows [a_g, a_g + u_g), u_g <= maxu): Π's block rows for a SparseMatrixVBC,
// else runs of consecutive rows whose stripe lists are identical (a node's dof rows), else single rows.
// Every stripe l of B that stores rows of group g contributes w_l stored rows of C (its columns c,
// ascending), each holding the u_g values B[a_g .. a_g+u_g-1, col0_l + c] and gathering x row col0_l + c.
// Groups in row order, their stripes in stripe order (the reference's forward loop,
// multiply_VBC.jl:68-77).  Every row of a group is stored by the same stripes, so C holds exactly the
// values (fill zeros included) the reference multiplies.
int transpose_stripes(const PlanCtx *h, const Stripes &s, const char *val, int maxu, Stripes &c,
                      std::vector<char> &cv)
{
    const int esz = h->esz;
    const int64_t m = s.m;
    // row groups
    std::vector<int64_t> a;
    if (!s.grp.empty()) {
        for (size_t k = 0; k + 1 < s.grp.size(); k++)
            for (int64_t i = s.grp[k]; i < s.grp[k + 1]; i += maxu) a.push_back(i);  // taller blocks: pieces
    } else {
        // the stripes storing each row (rows ascend inside a stripe, so each list comes out sorted)
        std::vector<int64_t> cnt(m + 1, 0);
        for (int64_t q = 0; q < (int64_t)s.rows.size(); q++) cnt[s.rows[q] + 1]++;
        for (int64_t i = 0; i < m; i++) cnt[i + 1] += cnt[i];
        std::vector<int64_t> lst(s.rows.size()), fillp(cnt.begin(), cnt.end() - 1);
        for (int64_t l = 0; l < s.L; l++)
            for (int64_t q = s.rbeg[l]; q < s.rbeg[l + 1]; q++) lst[fillp[s.rows[q]]++] = l;
        auto same = [&](int64_t i, int64_t j) {
            return cnt[i + 1] - cnt[i] == cnt[j + 1] - cnt[j] &&
                   std::equal(lst.begin() + cnt[i], lst.begin() + cnt[i + 1], lst.begin() + cnt[j]);
        };
        for (int64_t i = 0; i < m;) {
            int64_t e = i + 1;
            while (e < m && e - i < maxu && cnt[i + 1] > cnt[i] && same(i, e)) e++;
            a.push_back(i);
            i = e;
        }
    }
    a.push_back(m);
    const int64_t ng = (int64_t)a.size() - 1;
    std::vector<int64_t> gof(m);
    for (int64_t g = 0; g < ng; g++)
        for (int64_t i = a[g]; i < a[g + 1]; i++) gof[i] = g;
    // (group, stripe) blocks: stored rows of B grouped
    struct Blk {
        int64_t g, l, q0;  // q0: first stored row of the stripe inside the group
    };
    std::vector<Blk> blks;
    for (int64_t l = 0; l < s.L; l++) {
        int64_t prev = -1;
        for (int64_t q = s.rbeg[l]; q < s.rbeg[l + 1]; q++) {
            const int64_t g = gof[s.rows[q]];
            if (g != prev) blks.push_back({g, l, q});
            prev = g;
        }
    }
    std::stable_sort(blks.begin(), blks.end(), [](const Blk &x, const Blk &y) { return x.g < y.g; });
    c = Stripes{};
    c.m = s.n;  // C = Bᵀ: its x is B's x (length n), its y is B's y (length m)
    c.n = m;
    c.L = ng;
    c.col0.resize(ng);
    c.w.resize(ng);
    c.rbeg.assign(ng + 1, 0);
    c.voff.resize(ng);
    for (int64_t g = 0; g < ng; g++) {
        c.col0[g] = a[g];
        c.w[g] = (int32_t)(a[g + 1] - a[g]);
    }
    for (const Blk &b : blks) c.rbeg[b.g + 1] += s.w[b.l];
    for (int64_t g = 0; g < ng; g++) c.rbeg[g + 1] += c.rbeg[g];
    const int64_t rows = c.rbeg[ng];
    if (rows >= (int64_t(1) << 31)) return fail(VBC_INVALID_ARG, "matrix too large for the forward panel layout");
    c.rows.resize(rows);
    int64_t nv = 0;
    for (int64_t g = 0; g < ng; g++) {
        c.voff[g] = nv;
        nv += (c.rbeg[g + 1] - c.rbeg[g]) * c.w[g];
    }
    cv.assign((size_t)std::max<int64_t>(nv, 1) * esz, 0);
    std::vector<int64_t> at(c.rbeg.begin(), c.rbeg.end() - 1);  // next stored row of each group
    for (const Blk &b : blks) {
        const int64_t l = b.l, wl = s.w[l], u = c.w[b.g];
        for (int64_t cc = 0; cc < wl; cc++) {
            const int64_t row = at[b.g]++;
            c.rows[row] = (int32_t)(s.col0[l] + cc);
            char *dst = cv.data() + (c.voff[b.g] + (row - c.rbeg[b.g]) * u) * esz;
            // a stripe that stores one row twice (hand-built input; the reference's constructors never do)
            // contributes both copies: they are added into the slot, not overwritten
            for (int64_t q = b.q0; q < s.rbeg[l + 1] && gof[s.rows[q]] == b.g; q++) {
                char *d = dst + (s.rows[q] - a[b.g]) * esz;
                const char *v = val + (s.voff[l] + (q - s.rbeg[l]) * wl + cc) * esz;
                if (h->rec) {  // a recording build: tags are copied, never summed, and a slot has one source
                    static const char zero8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (std::memcmp(d, zero8, (size_t)esz) != 0)
                        return fail(VBC_INVALID_ARG, "a stripe stores one row twice: such a matrix cannot be "
                                                     "VBC_CREATE_UPDATABLE in a layout of its transpose");
                    std::memcpy(d, v, (size_t)esz);
                } else if (esz == 8) {
                    double t, u2;
                    std::memcpy(&t, d, 8);
                    std::memcpy(&u2, v, 8);
                    t += u2;
                    std::memcpy(d, &t, 8);
                } else {
                    float t, u2;
                    std::memcpy(&t, d, 4);
                    std::memcpy(&u2, v, 4);
                    t += u2;
                    std::memcpy(d, &t, 4);
                }
            }
        }
    }
    return VBC_OK;
}

// Forward panel layout (VBC_CREATE_MULTI_FORWARD): Y = B·X is the transposed product of C = Bᵀ, so the
// transposed panel layout of C (transpose_stripes, groups up to 16 rows) serves it.
int build_forward_panel(PlanCtx *h, const Stripes &s, const char *val, Arena &ar, PanelPlan &plan)
{
    Stripes c;
    std::vector<char> cv;
    if (int st = transpose_stripes(h, s, val, 16, c, cv)) return st;
    const int64_t ng = c.L;
    int32_t widest = 0;
    for (int64_t g = 0; g < ng; g++) widest = std::max(widest, c.w[g]);
    h->st.mf_group = widest;
    const int64_t bytes0 = h->st.bytes_m;
    std::vector<int32_t> fill;
    // tile groups of C's rows (B's columns): B's stripes (Φ), so a u x w block of B is a w x u tile of C
    std::vector<int64_t> cg;
    for (int64_t l = 0; l < s.L; l++) cg.push_back(s.col0[l]);
    cg.push_back(s.n);
    const int st = build_panel(h, c, cv.data(), ar, plan, fill, &cg);
    h->st.bytes_mf = h->st.bytes_m - bytes0;
    h->st.bytes_m = bytes0;
    return st;
}

}  // namespace vbc
