// libvbc's create entry points (include/vbc.h, include/vbc_host.h) and their host-side checks.  A create is three
// steps: the device's facts (vbc_device.hip gather_facts), the layout planned on the host alone (vbc_plan.h
// plan_layout, from a LayoutConfig: no HIP call, no environment), and the device part (vbc_device.hip instantiate).
// The entries turn the reference's fields into Stripes (stripes_1d / stripes_2d / stripes_csc) first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "vbc_handle.h"
#include "vbc_plan.h"

using namespace vbc;

template <typename T>
static int64_t count_nonzeros(const char *val, int64_t n)
{
    const T *v = reinterpret_cast<const T *>(val);
    int64_t c = 0;
    for (int64_t i = 0; i < n; i++) c += (v[i] != T(0));
    return c;
}

// The two recording plans of an updatable create and the value map they give (vbc_update.hip value_map_host): pure
// host code.  `ft_narrow`, `arena_used`: the forward-on-Bᵀ guard's answer and the image size of the plan made with
// the caller's values, which the recording plans must reproduce.
template <typename F>
static int plan_value_map(const LayoutConfig &cfg, unsigned flags, StripesInput &in, F &&build, bool ft_narrow,
                          size_t arena_used, std::vector<uint32_t> &map, std::vector<UpdChunk> &chunks)
{
    const int64_t nval = in.nval;
    const size_t esz = (size_t)cfg.esz;
    if (nval > kUpdMaxSource)
        return fail(VBC_INVALID_ARG, "VBC_CREATE_UPDATABLE: val has more than 2^31 - 2 elements (the value map stores 32-bit source indices)");
    int st = VBC_OK;
    std::vector<char> arena[2];
    Recorder rec;
    std::vector<char> tv((size_t)std::max<int64_t>(nval, 1) * esz, 0);
    for (int pass = 0; pass < 2 && st == VBC_OK; pass++) {
        if (pass == 1)
            for (int64_t i = 0; i < nval; i++) {
                const uint64_t tag = (uint64_t)i + 1;
                std::memcpy(tv.data() + (size_t)i * esz, &tag, esz);  // little-endian: the low esz bytes
            }
        rec = Recorder{};
        rec.ft_narrow = ft_narrow;
        Plan P;
        const void *val = nullptr;
        if ((st = build(tv.data(), in, val)) == VBC_OK)
            st = plan_layout(cfg, in.s, static_cast<const char *>(val), in.nval, flags, P, &rec);
        arena[pass] = std::move(P.ar.host);
    }
    if (st != VBC_OK) return st;
    tv = std::vector<char>();
    if (arena[0].size() != arena_used)
        return fail(VBC_INVALID_ARG, "internal: a recording build of an updatable handle chose another layout");
    return value_map_host((int)esz, nval, arena[1], arena[0], rec.canon, rec.narrow, map, chunks);
}

// A create after its entry's own checks.  build(v, in, val): the entry's stripes and the values they address,
// from the caller's values (v = NULL) or from an array of the same shape (the recording plans of plan_value_map).
// Order: the checks, the device's facts, the plan with the caller's values, the device part; then, for
// VBC_CREATE_UPDATABLE, two recording plans of the same pattern on the host alone -- val all zero, val holding
// the tag i + 1 in element i, written before any blocking or transposition of the values -- whose arenas differ
// exactly in the value slots (vbc_update.hip build_value_map).
template <typename F>
static int create_handle(vbc_handle **out, int dtype, int device, unsigned flags, unsigned narrow, F &&build)
{
    // VBC_CREATE_NARROW_UPDATABLE arrives in `narrow` (check_narrow): the same map, with narrow chunks
    const bool narrow_updatable = (narrow & VBC_CREATE_NARROW_UPDATABLE) != 0;
    const bool updatable = (flags & VBC_CREATE_UPDATABLE) != 0 || narrow_updatable;
    flags &= ~VBC_CREATE_UPDATABLE;
    if (updatable && !out) return fail(VBC_INVALID_ARG, "out handle pointer is NULL");
    if (updatable) *out = nullptr;
    StripesInput in;
    const void *val = nullptr;
    if (int st = build(nullptr, in, val)) return st;
    if (!out) return fail(VBC_INVALID_ARG, "out handle pointer is NULL");
    *out = nullptr;
    if (int st = check_plan_input(dtype, in.s)) return st;
    int ndev = 0;
    VBC_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VBC_INVALID_ARG, "device ordinal out of range");
    const char *v = static_cast<const char *>(val);
    const int64_t nval = in.nval;
    DeviceFacts facts{};
    if (dtype != VBC_I64) {
        DeviceGuard g(device);
        if (!g.ok) return fail(VBC_HIP_ERROR, "hipSetDevice failed");
        if (int st = gather_facts(device, dtype == VBC_F64 ? 1u : 2u,
                                  (flags & (VBC_CREATE_MULTI | VBC_CREATE_MULTI_FORWARD)) != 0, facts))
            return st;
    }
    const LayoutConfig cfg = make_config(dtype, flags, narrow, facts);
    vbc_handle *h = nullptr;
    bool ft_narrow = false;
    {
        Plan P;
        if (int st = plan_layout(cfg, in.s, v, nval, flags, P, nullptr)) return st;
        ft_narrow = P.st.ft_narrow;
        if (int st = instantiate(P, cfg, device, &h)) return st;
    }
    h->m = in.s.m;
    h->n = in.s.n;
    h->L = in.s.L;
    h->K = in.K;
    h->nblocks = in.nblocks;
    h->nrows = (int64_t)in.s.rows.size();
    h->nval = nval;
    h->nnz = dtype == VBC_F64 ? count_nonzeros<double>(v, nval)
           : dtype == VBC_F32 ? count_nonzeros<float>(v, nval) : count_nonzeros<int64_t>(v, nval);
    if (!updatable) {
        *out = h;
        return VBC_OK;
    }
    std::vector<uint32_t> map;
    std::vector<UpdChunk> chunks;
    int st = plan_value_map(cfg, flags, in, build, ft_narrow, h->arena_used, map, chunks);
    if (st == VBC_OK) {
        DeviceGuard g(h->device);
        st = g.ok ? upload_value_map(h, map, chunks) : fail(VBC_HIP_ERROR, "hipSetDevice failed");
    }
    if (st != VBC_OK) { release(h); return st; }
    h->umap.mixed = narrow_updatable;
    h->updatable = true;
    *out = h;
    return VBC_OK;
}

extern "C" {

int vbcx_device_facts(int device, vbcx_facts *out)
{
    if (!out) return fail(VBC_INVALID_ARG, "NULL facts");
    int ndev = 0;
    VBC_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(VBC_INVALID_ARG, "device ordinal out of range");
    DeviceGuard g(device);
    if (!g.ok) return fail(VBC_HIP_ERROR, "hipSetDevice failed");
    return gather_facts(device, 3u, true, *out);
}

// VBC_CREATE_UPDATABLE_SHARDS belongs to the sharded creates (vbc_sharded.cpp), which pass VBC_CREATE_UPDATABLE on
// to their shards; the plain and *_ex creates end here.
static int refuse_narrow_flag(vbc_handle **out, const char *why)
{
    if (out) *out = nullptr;
    return fail(VBC_INVALID_ARG, why);
}
constexpr unsigned kNarrowBits = VBC_CREATE_NARROW_VALUES | VBC_CREATE_NARROW_PLANAR | VBC_CREATE_NARROW_PAIRS |
                                 VBC_CREATE_NARROW_STREAMS | VBC_CREATE_NARROW_SWEPT;
constexpr const char *kNarrowSweptAlone = "VBC_CREATE_NARROW_SWEPT is valid only together with VBC_CREATE_NARROW_VALUES";
constexpr const char *kNarrowSweptPlain = "VBC_CREATE_NARROW_SWEPT (with VBC_CREATE_NARROW_VALUES) needs Float32 values on a "
                                          "Float64 handle: pass it to vbc1d_create_ex / vbc2d_create_ex / "
                                          "vbc_csc_create_ex (the creates without vbc_types store the compute eltype)";
constexpr unsigned kNarrowBelowStreams = VBC_CREATE_NARROW_VALUES | VBC_CREATE_NARROW_PLANAR | VBC_CREATE_NARROW_PAIRS;
constexpr const char *kNarrowStreamsAlone = "VBC_CREATE_NARROW_STREAMS is valid only together with VBC_CREATE_NARROW_VALUES, "
                                            "VBC_CREATE_NARROW_PLANAR and VBC_CREATE_NARROW_PAIRS";
constexpr const char *kNarrowStreamsPlain = "VBC_CREATE_NARROW_STREAMS (with VBC_CREATE_NARROW_VALUES, VBC_CREATE_NARROW_PLANAR "
                                            "and VBC_CREATE_NARROW_PAIRS) needs Float32 values on a Float64 handle: pass it "
                                            "to vbc1d_create_ex / vbc2d_create_ex / vbc_csc_create_ex (the creates without "
                                            "vbc_types store the compute eltype)";
constexpr const char *kNarrowPairsAlone = "VBC_CREATE_NARROW_PAIRS is valid only together with VBC_CREATE_NARROW_VALUES and "
                                          "VBC_CREATE_NARROW_PLANAR";
constexpr const char *kNarrowPlain = "VBC_CREATE_NARROW_VALUES (and VBC_CREATE_NARROW_PLANAR / VBC_CREATE_NARROW_PAIRS with it) needs Float32 values "
                                     "on a Float64 handle: pass it to vbc1d_create_ex / vbc2d_create_ex / "
                                     "vbc_csc_create_ex (the creates without vbc_types store the compute eltype)";
constexpr const char *kNarrowUpdPlain = "VBC_CREATE_NARROW_UPDATABLE is valid only together with VBC_CREATE_NARROW_VALUES, "
                                        "which needs Float32 values on a Float64 handle: pass both to vbc1d_create_ex / "
                                        "vbc2d_create_ex / vbc_csc_create_ex";

// Why a set of narrow bits is refused on a handle that computes in `dtype`, or NULL: the bits each one builds on
// and the Float64 compute eltype, in the order the refusals take when several apply.  vbcx_plan_image and
// vbcx_value_map ask with their dtype; the *_ex creates (check_narrow) word the eltype refusals by vbc_types
// themselves and ask with VBC_F64.
static const char *narrow_bits_refusal(unsigned narrow, int dtype)
{
    if ((narrow & VBC_CREATE_NARROW_SWEPT) && !(narrow & VBC_CREATE_NARROW_VALUES)) return kNarrowSweptAlone;
    if ((narrow & VBC_CREATE_NARROW_SWEPT) && dtype != VBC_F64)
        return "VBC_CREATE_NARROW_SWEPT (with VBC_CREATE_NARROW_VALUES) needs a Float64 handle";
    if ((narrow & VBC_CREATE_NARROW_STREAMS) && (narrow & kNarrowBelowStreams) != kNarrowBelowStreams) return kNarrowStreamsAlone;
    if (narrow && !(narrow & VBC_CREATE_NARROW_VALUES))
        return "VBC_CREATE_NARROW_PLANAR is valid only together with VBC_CREATE_NARROW_VALUES";
    if ((narrow & VBC_CREATE_NARROW_PAIRS) && !(narrow & VBC_CREATE_NARROW_PLANAR)) return kNarrowPairsAlone;
    if (narrow && dtype != VBC_F64) return "VBC_CREATE_NARROW_VALUES needs a Float64 handle";
    return nullptr;
}

static int refuse_sharded_flag(vbc_handle **out)
{
    if (out) *out = nullptr;
    return fail(VBC_INVALID_ARG, "VBC_CREATE_UPDATABLE_SHARDS is a flag of the sharded creates (single handle: VBC_CREATE_UPDATABLE)");
}

static int stripes_1d(int64_t m, int64_t n, int64_t W, int64_t L, const int64_t *spl, const int64_t *pos,
               const int64_t *idx, const int64_t *ofs, const void *val, int64_t nval, StripesInput &in)
{
    // SparseMatrix1DVBC{W,Tv,Ti} inner constructor checks (SparseMatrixVBCs.jl:45-50)
    if (m < 0) return fail(VBC_INVALID_ARG, "number of rows (m) must be >= 0");
    if (n < 0) return fail(VBC_INVALID_ARG, "number of columns (n) must be >= 0");
    if (W <= 0) return fail(VBC_INVALID_ARG, "W must be > 0");
    if (L < 0 || !spl || !pos || !ofs) return fail(VBC_INVALID_ARG, "bad stripe arrays");
    if (spl[0] != 1 || spl[L] != n + 1) return fail(VBC_INVALID_ARG, "Φ.spl must run from 1 to n+1");
    if (pos[0] != 1 || ofs[0] != 1) return fail(VBC_INVALID_ARG, "pos[1] and ofs[1] must be 1");
    Stripes &s = in.s;
    s = Stripes{};
    s.m = m; s.n = n; s.L = L;
    s.col0.resize(L); s.w.resize(L); s.rbeg.resize(L + 1); s.voff.resize(L);
    const int64_t q = pos[L] - 1;
    if (q < 0 || (q > 0 && !idx)) return fail(VBC_INVALID_ARG, "bad pos");
    if (ofs[L] - 1 > nval) return fail(VBC_INVALID_ARG, "val shorter than ofs[L+1]-1");
    if (ofs[L] - 1 > 0 && !val) return fail(VBC_INVALID_ARG, "NULL val");
    for (int64_t l = 0; l < L; l++) {
        const int64_t w = spl[l + 1] - spl[l];
        if (w < 1) return fail(VBC_INVALID_ARG, "Φ.spl must be strictly increasing");
        if (w > W) return fail(VBC_ASSERTION, "AssertionError: w <= W");
        const int64_t R = pos[l + 1] - pos[l];
        if (R < 0) return fail(VBC_INVALID_ARG, "pos must be non-decreasing");
        if (ofs[l + 1] - ofs[l] != R * w) return fail(VBC_INVALID_ARG, "ofs[l+1]-ofs[l] != rows*w");
        s.col0[l] = spl[l] - 1;
        s.w[l] = (int32_t)w;
        s.rbeg[l] = pos[l] - 1;
        s.voff[l] = ofs[l] - 1;
    }
    s.rbeg[L] = q;
    s.rows.resize(q);
    for (int64_t r = 0; r < q; r++) {
        if (idx[r] < 1 || idx[r] > m) return fail(VBC_INVALID_ARG, "idx out of range 1:m");
        s.rows[r] = (int32_t)(idx[r] - 1);
    }
    in.nval = ofs[L] - 1;
    in.K = 0;
    in.nblocks = q;
    return VBC_OK;
}

// `narrow`: the narrow-storage bits as the *_ex creates checked them (they take them out of `flags`); the plain
// creates pass 0 and refuse both bits.
static int create_1d(vbc_handle **out, int64_t m, int64_t n, int64_t W, int64_t L, const int64_t *spl,
                     const int64_t *pos, const int64_t *idx, const int64_t *ofs, const void *val,
                     int64_t nval, int dtype, int device, unsigned flags, unsigned narrow)
{
    if (flags & VBC_CREATE_UPDATABLE_SHARDS) return refuse_sharded_flag(out);
    if (flags & VBC_CREATE_NARROW_SWEPT) return refuse_narrow_flag(out, kNarrowSweptPlain);
    if (flags & VBC_CREATE_NARROW_STREAMS) return refuse_narrow_flag(out, kNarrowStreamsPlain);
    if (flags & VBC_CREATE_NARROW_UPDATABLE) return refuse_narrow_flag(out, kNarrowUpdPlain);
    if (flags & kNarrowBits) return refuse_narrow_flag(out, kNarrowPlain);
    return create_handle(out, dtype, device, flags, narrow, [&](const void *v, StripesInput &in, const void *&sv) {
        sv = v ? v : val;
        return stripes_1d(m, n, W, L, spl, pos, idx, ofs, sv, nval, in);
    });
}

int vbc1d_create(vbc_handle **out, int64_t m, int64_t n, int64_t W, int64_t L, const int64_t *spl,
                 const int64_t *pos, const int64_t *idx, const int64_t *ofs, const void *val,
                 int64_t nval, int dtype, int device, unsigned flags)
{
    return create_1d(out, m, n, W, L, spl, pos, idx, ofs, val, nval, dtype, device, flags, 0);
}

static int stripes_2d(int64_t m, int64_t n, int64_t U, int64_t W, int64_t K, const int64_t *pspl, int64_t L,
               const int64_t *spl, const int64_t *pos, const int64_t *idx, const int64_t *ofs, const void *val,
               int64_t nval, StripesInput &in)
{
    // SparseMatrixVBC{U,W,Tv,Ti} inner constructor checks (SparseMatrixVBCs.jl:72-79)
    if (m < 0) return fail(VBC_INVALID_ARG, "number of rows (m) must be >= 0");
    if (n < 0) return fail(VBC_INVALID_ARG, "number of columns (n) must be >= 0");
    if (U <= 0) return fail(VBC_INVALID_ARG, "U must be > 0");
    if (W <= 0) return fail(VBC_INVALID_ARG, "W must be > 0");
    if (K < 0 || L < 0 || !pspl || !spl || !pos || !ofs) return fail(VBC_INVALID_ARG, "bad partition arrays");
    if (pspl[0] != 1 || pspl[K] != m + 1) return fail(VBC_INVALID_ARG, "Π.spl must run from 1 to m+1");
    if (spl[0] != 1 || spl[L] != n + 1) return fail(VBC_INVALID_ARG, "Φ.spl must run from 1 to n+1");
    if (pos[0] != 1 || ofs[0] != 1) return fail(VBC_INVALID_ARG, "pos[1] and ofs[1] must be 1");
    for (int64_t k = 0; k < K; k++) {
        const int64_t u = pspl[k + 1] - pspl[k];
        if (u < 1) return fail(VBC_INVALID_ARG, "Π.spl must be strictly increasing");
        if (u > U) return fail(VBC_ASSERTION, "AssertionError: u <= U");
    }
    if (ofs[L] - 1 > nval) return fail(VBC_INVALID_ARG, "val shorter than ofs[L+1]-1");
    const int64_t q = pos[L] - 1;
    if (q < 0 || (q > 0 && !idx)) return fail(VBC_INVALID_ARG, "bad pos");
    for (int64_t l = 0; l < L; l++)  // every stripe's blocks lie inside idx[0 .. q-1]
        if (pos[l + 1] < pos[l] || pos[l] < 1 || pos[l + 1] - 1 > q)
            return fail(VBC_INVALID_ARG, "pos must be non-decreasing within 1:pos[L+1]");
    for (int64_t l = 0; l < L; l++)
        if (ofs[l + 1] < ofs[l]) return fail(VBC_INVALID_ARG, "ofs must be non-decreasing");
    if (ofs[L] - 1 > 0 && !val) return fail(VBC_INVALID_ARG, "NULL val");
    Stripes &s = in.s;
    s = Stripes{};
    s.m = m; s.n = n; s.L = L;
    s.col0.resize(L); s.w.resize(L); s.rbeg.resize(L + 1); s.voff.resize(L);
    // Expand every u×w tile into u stored rows with explicit x-row indices: the tile is already
    // u row-major w-wide rows (constructors_VBC.jl:95-105), so val is used as is.
    int64_t rows = 0;
    for (int64_t l = 0; l < L; l++) {
        const int64_t w = spl[l + 1] - spl[l];
        if (w < 1) return fail(VBC_INVALID_ARG, "Φ.spl must be strictly increasing");
        if (w > W) return fail(VBC_ASSERTION, "AssertionError: w <= W");
        int64_t R = 0;
        for (int64_t Q = pos[l] - 1; Q < pos[l + 1] - 1; Q++) {
            const int64_t k = idx[Q];
            if (k < 1 || k > K) return fail(VBC_INVALID_ARG, "idx (block row) out of range 1:K");
            R += pspl[k] - pspl[k - 1];
        }
        if (ofs[l + 1] - ofs[l] != R * w) return fail(VBC_INVALID_ARG, "ofs[l+1]-ofs[l] != Σu*w");
        s.col0[l] = spl[l] - 1;
        s.w[l] = (int32_t)w;
        s.rbeg[l] = rows;
        s.voff[l] = ofs[l] - 1;
        rows += R;
    }
    s.rbeg[L] = rows;
    s.rows.resize(rows);
    int64_t r = 0;
    for (int64_t Q = 0; Q < q; Q++) {
        const int64_t k = idx[Q];
        for (int64_t i = pspl[k - 1] - 1; i < pspl[k] - 1; i++) s.rows[r++] = (int32_t)i;
    }
    s.grp.resize(K + 1);
    for (int64_t k = 0; k <= K; k++) s.grp[k] = pspl[k] - 1;
    in.nval = ofs[L] - 1;
    in.K = K;
    in.nblocks = q;
    return VBC_OK;
}

static int create_2d(vbc_handle **out, int64_t m, int64_t n, int64_t U, int64_t W, int64_t K,
                     const int64_t *pspl, int64_t L, const int64_t *spl, const int64_t *pos,
                     const int64_t *idx, const int64_t *ofs, const void *val, int64_t nval, int dtype,
                     int device, unsigned flags, unsigned narrow)
{
    if (flags & VBC_CREATE_UPDATABLE_SHARDS) return refuse_sharded_flag(out);
    if (flags & VBC_CREATE_NARROW_SWEPT) return refuse_narrow_flag(out, kNarrowSweptPlain);
    if (flags & VBC_CREATE_NARROW_STREAMS) return refuse_narrow_flag(out, kNarrowStreamsPlain);
    if (flags & VBC_CREATE_NARROW_UPDATABLE) return refuse_narrow_flag(out, kNarrowUpdPlain);
    if (flags & kNarrowBits) return refuse_narrow_flag(out, kNarrowPlain);
    return create_handle(out, dtype, device, flags, narrow, [&](const void *v, StripesInput &in, const void *&sv) {
        sv = v ? v : val;
        return stripes_2d(m, n, U, W, K, pspl, L, spl, pos, idx, ofs, sv, nval, in);
    });
}

int vbc2d_create(vbc_handle **out, int64_t m, int64_t n, int64_t U, int64_t W, int64_t K,
                 const int64_t *pspl, int64_t L, const int64_t *spl, const int64_t *pos,
                 const int64_t *idx, const int64_t *ofs, const void *val, int64_t nval, int dtype,
                 int device, unsigned flags)
{
    return create_2d(out, m, n, U, W, K, pspl, L, spl, pos, idx, ofs, val, nval, dtype, device, flags, 0);
}

// A SparseMatrixCSC as stripes.  bv: the values of the blocked stripes (sv then points into it).
static int stripes_csc(int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, const void *nzval,
                       int dtype, StripesInput &in, std::vector<char> &bv, const void *&sv)
{
    if (m < 0 || n < 0) return fail(VBC_INVALID_ARG, "number of rows/columns must be >= 0");
    if (!colptr || colptr[0] != 1) return fail(VBC_INVALID_ARG, "colptr[1] must be 1");
    Stripes &s = in.s;
    s = Stripes{};
    s.m = m; s.n = n; s.L = n;
    s.col0.resize(n); s.w.assign(n, 1); s.rbeg.resize(n + 1); s.voff.resize(n);
    for (int64_t j = 0; j < n; j++) {
        if (colptr[j + 1] < colptr[j]) return fail(VBC_INVALID_ARG, "colptr must be non-decreasing");
        s.col0[j] = j;
        s.rbeg[j] = colptr[j] - 1;
        s.voff[j] = colptr[j] - 1;
    }
    const int64_t nnz = colptr[n] - 1;
    if (nnz > 0 && (!rowval || !nzval)) return fail(VBC_INVALID_ARG, "NULL rowval or nzval");
    s.rbeg[n] = nnz;
    s.rows.resize(nnz);
    for (int64_t p = 0; p < nnz; p++) {
        if (rowval[p] < 1 || rowval[p] > m) return fail(VBC_INVALID_ARG, "rowval out of range 1:m");
        s.rows[p] = (int32_t)(rowval[p] - 1);
    }
    // Column blocking: runs of up to 8 consecutive columns with identical row patterns (the dof
    // columns of a node in a stiffness matrix) become one w-wide stripe, so TrSpMV! runs the blocked
    // kernels (planar with row runs for 3-dof operators).  Each output y[j] still sums its column in
    // stored row order (TrSpMV.jl:10-16), so the result is that of the unit-width layout, bit for bit.
    // VBC_CSC_BLOCK=0 keeps unit stripes.
    const char *eb = layout_knob("VBC_CSC_BLOCK");
    if (!(eb && atoi(eb) == 0) && n > 1 && (dtype == VBC_F64 || dtype == VBC_F32 || dtype == VBC_I64)) {
        std::vector<int64_t> g0;  // first column of each group
        for (int64_t j = 0; j < n;) {
            int64_t e = j + 1;
            const int64_t len = colptr[j + 1] - colptr[j];
            while (e < n && e - j < 8 && colptr[e + 1] - colptr[e] == len &&
                   std::equal(rowval + colptr[j] - 1, rowval + colptr[j + 1] - 1, rowval + colptr[e] - 1))
                e++;
            g0.push_back(j);
            j = e;
        }
        if ((int64_t)g0.size() < n) {
            const int64_t L = (int64_t)g0.size();
            const int esz = elem_size(dtype);
            Stripes b;
            b.m = m; b.n = n; b.L = L;
            b.col0.resize(L); b.w.resize(L); b.rbeg.resize(L + 1); b.voff.resize(L);
            bv.assign((size_t)std::max<int64_t>(nnz, 1) * esz, 0);
            const char *src = static_cast<const char *>(nzval);
            int64_t q = 0;
            for (int64_t l = 0; l < L; l++) {
                const int64_t j = g0[l], w = (l + 1 < L ? g0[l + 1] : n) - j, R = colptr[j + 1] - colptr[j];
                b.col0[l] = j;
                b.w[l] = (int32_t)w;
                b.rbeg[l] = q;
                q += R;
            }
            b.rbeg[L] = q;
            b.rows.resize(q);
            int64_t v = 0;
            for (int64_t l = 0; l < L; l++) {
                const int64_t j = g0[l], w = b.w[l], R = colptr[j + 1] - colptr[j];
                b.voff[l] = v;
                for (int64_t r = 0; r < R; r++) {
                    b.rows[b.rbeg[l] + r] = (int32_t)(rowval[colptr[j] - 1 + r] - 1);
                    for (int64_t c = 0; c < w; c++)
                        std::memcpy(bv.data() + (v + r * w + c) * esz, src + (colptr[j + c] - 1 + r) * esz, (size_t)esz);
                }
                v += R * w;
            }
            in.s = std::move(b);
            in.nval = nnz;
            in.K = 0;
            in.nblocks = q;
            sv = bv.data();
            return VBC_OK;
        }
    }
    in.nval = nnz;
    in.K = 0;
    in.nblocks = nnz;
    sv = nzval;
    return VBC_OK;
}

static int create_csc(vbc_handle **out, int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval,
                      const void *nzval, int dtype, int device, unsigned flags, unsigned narrow)
{
    if (flags & VBC_CREATE_UPDATABLE_SHARDS) return refuse_sharded_flag(out);
    if (flags & VBC_CREATE_NARROW_SWEPT) return refuse_narrow_flag(out, kNarrowSweptPlain);
    if (flags & VBC_CREATE_NARROW_STREAMS) return refuse_narrow_flag(out, kNarrowStreamsPlain);
    if (flags & VBC_CREATE_NARROW_UPDATABLE) return refuse_narrow_flag(out, kNarrowUpdPlain);
    if (flags & kNarrowBits) return refuse_narrow_flag(out, kNarrowPlain);
    std::vector<char> bv;
    // (the tags of an updatable create go into an nzval-shaped array, before the column blocking copies them)
    return create_handle(out, dtype, device, flags, narrow, [&](const void *v, StripesInput &in, const void *&sv) {
        return stripes_csc(m, n, colptr, rowval, v ? v : nzval, dtype, in, bv, sv);
    });
}

int vbc_csc_create(vbc_handle **out, int64_t m, int64_t n, const int64_t *colptr,
                   const int64_t *rowval, const void *nzval, int dtype, int device, unsigned flags)
{
    return create_csc(out, m, n, colptr, rowval, nzval, dtype, device, flags, 0);
}

int vbcx_plan_image(int64_t m, int64_t n, int64_t U, int64_t W, int64_t K, const int64_t *pspl, int64_t L,
                               const int64_t *spl, const int64_t *pos, const int64_t *idx, const int64_t *ofs,
                               const void *val, int64_t nval, int dtype, unsigned flags, const vbcx_facts *facts,
                               void *image, size_t capacity, size_t *bytes)
{
    if (!facts || !bytes) return fail(VBC_INVALID_ARG, "facts and bytes must not be NULL");
    StripesInput in;
    if (int st = pspl ? stripes_2d(m, n, U, W, K, pspl, L, spl, pos, idx, ofs, val, nval, in)
                      : stripes_1d(m, n, W, L, spl, pos, idx, ofs, val, nval, in))
        return st;
    if (flags & (VBC_CREATE_UPDATABLE | VBC_CREATE_UPDATABLE_SHARDS))
        return fail(VBC_INVALID_ARG, "vbcx_plan_image plans one layout: VBC_CREATE_UPDATABLE(_SHARDS) do not change it");
    if ((flags & VBC_CREATE_NARROW_UPDATABLE) && !(flags & VBC_CREATE_NARROW_VALUES))
        return fail(VBC_INVALID_ARG, "VBC_CREATE_NARROW_UPDATABLE is valid only together with VBC_CREATE_NARROW_VALUES");
    flags &= ~VBC_CREATE_NARROW_UPDATABLE;  // (it changes no layout)
    const unsigned narrow = flags & kNarrowBits;
    if (const char *why = narrow_bits_refusal(narrow, dtype)) return fail(VBC_INVALID_ARG, why);
    flags &= ~kNarrowBits;
    Plan P;
    if (int st = plan_layout(make_config(dtype, flags, narrow, *facts), in.s, static_cast<const char *>(val), in.nval,
                             flags, P, nullptr))
        return st;
    *bytes = P.ar.host.size();
    if (!image) return VBC_OK;
    if (capacity < *bytes) return fail(VBC_INVALID_ARG, "image buffer smaller than the arena image");
    std::memcpy(image, P.ar.host.data(), *bytes);
    return VBC_OK;
}

static_assert(sizeof(vbcx_map_chunk) == sizeof(UpdChunk) && offsetof(vbcx_map_chunk, vsz) == offsetof(UpdChunk, vsz) &&
                  offsetof(vbcx_map_chunk, map) == offsetof(UpdChunk, map) && offsetof(vbcx_map_chunk, n) == offsetof(UpdChunk, n),
              "vbc_host.h vbcx_map_chunk is vbc_handle.h UpdChunk");
static_assert(VBCX_MAP_ZERO == kUpdZero && VBCX_MAP_SKIP == kUpdSkip && VBCX_MAP_CANON == kUpdCanon, "vbc_host.h map entries");

int vbcx_value_map(int64_t m, int64_t n, int64_t U, int64_t W, int64_t K, const int64_t *pspl, int64_t L,
                   const int64_t *spl, const int64_t *pos, const int64_t *idx, const int64_t *ofs, const void *val,
                   int64_t nval, int dtype, unsigned flags, const vbcx_facts *facts, uint32_t *map, int64_t map_capacity,
                   int64_t *nentries, vbcx_map_chunk *chunks, int64_t chunk_capacity, int64_t *nchunks)
{
    if (!facts || !nentries || !nchunks) return fail(VBC_INVALID_ARG, "facts, nentries and nchunks must not be NULL");
    auto stripes = [&](const void *v, StripesInput &in, const void *&sv) {
        sv = v ? v : val;
        return pspl ? stripes_2d(m, n, U, W, K, pspl, L, spl, pos, idx, ofs, sv, nval, in)
                    : stripes_1d(m, n, W, L, spl, pos, idx, ofs, sv, nval, in);
    };
    StripesInput in;
    const void *sv = nullptr;
    if (int st = stripes(nullptr, in, sv)) return st;
    flags &= ~(VBC_CREATE_UPDATABLE | VBC_CREATE_UPDATABLE_SHARDS | VBC_CREATE_NARROW_UPDATABLE);
    const unsigned narrow = flags & kNarrowBits;
    if (const char *why = narrow_bits_refusal(narrow, dtype)) return fail(VBC_INVALID_ARG, why);
    flags &= ~kNarrowBits;
    const LayoutConfig cfg = make_config(dtype, flags, narrow, *facts);
    size_t arena_used = 0;
    bool ft_narrow = false;
    {
        Plan P;
        if (int st = plan_layout(cfg, in.s, static_cast<const char *>(val), in.nval, flags, P, nullptr)) return st;
        arena_used = P.ar.host.size();
        ft_narrow = P.st.ft_narrow;
    }
    std::vector<uint32_t> mp;
    std::vector<UpdChunk> ch;
    if (int st = plan_value_map(cfg, flags, in, stripes, ft_narrow, arena_used, mp, ch)) return st;
    *nentries = (int64_t)mp.size();
    *nchunks = (int64_t)ch.size();
    if (map && map_capacity >= *nentries && !mp.empty()) std::memcpy(map, mp.data(), mp.size() * 4);
    if (chunks && chunk_capacity >= *nchunks && !ch.empty()) std::memcpy(chunks, ch.data(), ch.size() * sizeof(UpdChunk));
    return VBC_OK;
}

// ---------------------------------------------------------------------------------------------
// Generic eltypes and index widths (vbc_types)
// ---------------------------------------------------------------------------------------------

extern "C++" {  // helpers of the typed entry points (templates need C++ linkage)

// Values converted to the compute eltype (empty when no conversion is needed: use `val` as is).
static int convert_values(const void *val, int64_t nval, const vbc_types *t, std::vector<char> &out)
{
    if (t->val_dtype == t->compute_dtype) return VBC_OK;
    if (nval > 0 && !val) return fail(VBC_INVALID_ARG, "NULL val");
    out.resize((size_t)std::max<int64_t>(nval, 1) * elem_size(t->compute_dtype));
    if (t->compute_dtype == VBC_F64) host_convert(val, t->val_dtype, nval, 1, reinterpret_cast<double *>(out.data()));
    else if (t->compute_dtype == VBC_F32) host_convert(val, t->val_dtype, nval, 1, reinterpret_cast<float *>(out.data()));
    else host_convert(val, t->val_dtype, nval, 1, reinterpret_cast<int64_t *>(out.data()));
    return VBC_OK;
}

// VBC_CREATE_NARROW_VALUES on an *_ex create: checked before any device work; the flag is then taken out of
// `flags` and handed on as the creates' `narrow` argument.
static int check_narrow(vbc_handle **out, const vbc_types *t, unsigned &flags, unsigned &narrow)
{
    narrow = 0;
    const bool upd = (flags & VBC_CREATE_NARROW_UPDATABLE) != 0;  // (its refusals name it)
    if (!(flags & (kNarrowBits | VBC_CREATE_NARROW_UPDATABLE))) return VBC_OK;
    const unsigned bits = flags & kNarrowBits;
    const bool types_ok = t->val_dtype == VBC_F32 && t->compute_dtype == VBC_F64;
    // SWEPT, then STREAMS, beside the bits it builds on: its eltype and VBC_CREATE_UPDATABLE refusals name it,
    // whatever else is set (without those bits the shared ladder refuses it, in the same place)
    if ((bits & VBC_CREATE_NARROW_SWEPT) && (bits & VBC_CREATE_NARROW_VALUES)) {
        if (!types_ok)
            return refuse_narrow_flag(out, "VBC_CREATE_NARROW_SWEPT (with VBC_CREATE_NARROW_VALUES) needs val_dtype VBC_F32 "
                                           "and compute_dtype VBC_F64");
        if (flags & VBC_CREATE_UPDATABLE)
            return refuse_narrow_flag(out, "VBC_CREATE_NARROW_SWEPT (with VBC_CREATE_NARROW_VALUES) cannot be combined with "
                                           "VBC_CREATE_UPDATABLE: a narrow handle is made updatable by "
                                           "VBC_CREATE_NARROW_UPDATABLE instead");
    }
    if ((bits & VBC_CREATE_NARROW_STREAMS) && (bits & kNarrowBelowStreams) == kNarrowBelowStreams) {
        if (!types_ok)
            return refuse_narrow_flag(out, "VBC_CREATE_NARROW_STREAMS (with VBC_CREATE_NARROW_VALUES) needs val_dtype VBC_F32 "
                                           "and compute_dtype VBC_F64");
        if (flags & VBC_CREATE_UPDATABLE)
            return refuse_narrow_flag(out, "VBC_CREATE_NARROW_STREAMS (with VBC_CREATE_NARROW_VALUES) cannot be combined with "
                                           "VBC_CREATE_UPDATABLE: a narrow handle is made updatable by "
                                           "VBC_CREATE_NARROW_UPDATABLE instead");
    }
    // Without VALUES, and with no SWEPT or STREAMS to name the refusal first, this entry differs from the shared
    // ladder: NARROW_UPDATABLE names itself, and PAIRS goes before PLANAR.
    if (!(bits & (VBC_CREATE_NARROW_VALUES | VBC_CREATE_NARROW_SWEPT | VBC_CREATE_NARROW_STREAMS))) {
        if (upd)
            return refuse_narrow_flag(out, "VBC_CREATE_NARROW_UPDATABLE is valid only together with VBC_CREATE_NARROW_VALUES");
        if (bits & VBC_CREATE_NARROW_PAIRS) return refuse_narrow_flag(out, kNarrowPairsAlone);
    }
    if (const char *why = narrow_bits_refusal(bits, VBC_F64)) return refuse_narrow_flag(out, why);
    if (!types_ok)
        return refuse_narrow_flag(out, upd ? "VBC_CREATE_NARROW_UPDATABLE with VBC_CREATE_NARROW_VALUES needs val_dtype "
                                             "VBC_F32 and compute_dtype VBC_F64"
                                           : "VBC_CREATE_NARROW_VALUES needs val_dtype VBC_F32 and compute_dtype VBC_F64");
    if (flags & VBC_CREATE_UPDATABLE)
        return refuse_narrow_flag(out, upd ? "VBC_CREATE_NARROW_UPDATABLE cannot be combined with VBC_CREATE_UPDATABLE: "
                                             "pass VBC_CREATE_NARROW_VALUES | VBC_CREATE_NARROW_UPDATABLE alone"
                                           : "VBC_CREATE_NARROW_VALUES cannot be combined with VBC_CREATE_UPDATABLE (the update "
                                             "kernel writes values of the compute eltype; a narrow handle is made "
                                             "updatable by VBC_CREATE_NARROW_UPDATABLE instead)");
    narrow = flags & (kNarrowBits | VBC_CREATE_NARROW_UPDATABLE);
    flags &= ~(kNarrowBits | VBC_CREATE_NARROW_UPDATABLE);
    return VBC_OK;
}

static int check_types(const vbc_types *t)
{
    if (!t) return fail(VBC_INVALID_ARG, "NULL vbc_types");
    if (t->reserved != 0) return fail(VBC_INVALID_ARG, "vbc_types.reserved must be 0");
    if (t->index_bits != 32 && t->index_bits != 64) return fail(VBC_INVALID_ARG, "index_bits must be 32 or 64");
    if (!known_dtype(t->val_dtype)) return fail(VBC_UNSUPPORTED_DTYPE, "unknown val_dtype");
    if (t->compute_dtype != VBC_F64 && t->compute_dtype != VBC_F32 && t->compute_dtype != VBC_I64)
        return fail(VBC_UNSUPPORTED_DTYPE, "compute_dtype must be VBC_F64, VBC_F32 or VBC_I64");
    if (t->compute_dtype == VBC_I64 && is_float(t->val_dtype))
        return fail(VBC_UNSUPPORTED_DTYPE, "floating-point values on an integer handle (InexactError)");
    return VBC_OK;
}

// Index array as Int64 (a copy only for Ti = Int32).
struct Idx64 {
    std::vector<int64_t> buf;
    const int64_t *p = nullptr;
    void set(const void *src, int bits, int64_t n)
    {
        if (!src || bits == 64) {
            p = static_cast<const int64_t *>(src);
            return;
        }
        const int32_t *s32 = static_cast<const int32_t *>(src);
        buf.assign(s32, s32 + std::max<int64_t>(n, 0));
        p = buf.data();
    }
};

}  // extern "C++"

int vbc1d_create_ex(vbc_handle **out, int64_t m, int64_t n, int64_t W, int64_t L, const void *spl, const void *pos,
                    const void *idx, const void *ofs, const void *val, int64_t nval, const vbc_types *t, int device,
                    unsigned flags)
{
    if (int st = check_types(t)) return st;
    unsigned narrow;
    if (int st = check_narrow(out, t, flags, narrow)) return st;
    if (L < 0 || !spl || !pos || !ofs) return fail(VBC_INVALID_ARG, "bad stripe arrays");
    Idx64 S, P, I, O;
    S.set(spl, t->index_bits, L + 1);
    P.set(pos, t->index_bits, L + 1);
    O.set(ofs, t->index_bits, L + 1);
    const int64_t q = P.p[L] - 1;
    if (q < 0 || (q > 0 && !idx)) return fail(VBC_INVALID_ARG, "bad pos");
    I.set(idx, t->index_bits, q);
    std::vector<char> cv;
    if (int st = convert_values(val, nval, t, cv)) return st;
    return create_1d(out, m, n, W, L, S.p, P.p, I.p, O.p, cv.empty() ? val : cv.data(), nval, t->compute_dtype,
                     device, flags, narrow);
}

int vbc2d_create_ex(vbc_handle **out, int64_t m, int64_t n, int64_t U, int64_t W, int64_t K, const void *pspl,
                    int64_t L, const void *spl, const void *pos, const void *idx, const void *ofs, const void *val,
                    int64_t nval, const vbc_types *t, int device, unsigned flags)
{
    if (int st = check_types(t)) return st;
    unsigned narrow;
    if (int st = check_narrow(out, t, flags, narrow)) return st;
    if (K < 0 || L < 0 || !pspl || !spl || !pos || !ofs) return fail(VBC_INVALID_ARG, "bad partition arrays");
    Idx64 PS, S, P, I, O;
    PS.set(pspl, t->index_bits, K + 1);
    S.set(spl, t->index_bits, L + 1);
    P.set(pos, t->index_bits, L + 1);
    O.set(ofs, t->index_bits, L + 1);
    const int64_t q = P.p[L] - 1;
    if (q < 0 || (q > 0 && !idx)) return fail(VBC_INVALID_ARG, "bad pos");
    I.set(idx, t->index_bits, q);
    std::vector<char> cv;
    if (int st = convert_values(val, nval, t, cv)) return st;
    return create_2d(out, m, n, U, W, K, PS.p, L, S.p, P.p, I.p, O.p, cv.empty() ? val : cv.data(), nval,
                     t->compute_dtype, device, flags, narrow);
}

int vbc_csc_create_ex(vbc_handle **out, int64_t m, int64_t n, const void *colptr, const void *rowval,
                      const void *nzval, const vbc_types *t, int device, unsigned flags)
{
    if (int st = check_types(t)) return st;
    unsigned narrow;
    if (int st = check_narrow(out, t, flags, narrow)) return st;
    if (n < 0 || !colptr) return fail(VBC_INVALID_ARG, "colptr[1] must be 1");
    Idx64 CP, RV;
    CP.set(colptr, t->index_bits, n + 1);
    const int64_t nnz = CP.p[n] - 1;
    if (nnz < 0) return fail(VBC_INVALID_ARG, "bad colptr");
    RV.set(rowval, t->index_bits, nnz);
    std::vector<char> cv;
    if (int st = convert_values(nzval, nnz, t, cv)) return st;
    return create_csc(out, m, n, CP.p, RV.p, cv.empty() ? nzval : cv.data(), t->compute_dtype, device, flags, narrow);
}

}  // extern "C"
