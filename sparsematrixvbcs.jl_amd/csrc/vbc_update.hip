// vbc_update_values (vbc.h VBC_CREATE_UPDATABLE): the value map of a handle and the streaming kernel that
// rewrites every stored value slot of its arena from a new val array.
//
// The map is found at create time from two extra host builds of the same pattern (vbc_create.hip
// plan_value_map): one whose val holds the tag i + 1 in element i, one whose val is all zero.  The builders
// only ever copy values, so the arena words that differ between the two are exactly the value
// slots and the tag names the source element.  Runs of slots, joined over short all-zero gaps (padding
// slots), become regions; each region is widened to whole 16-byte quads and cut into chunks (vbc_handle.h
// UpdChunk), so one grid-stride launch covers any number of buckets.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>

#include "vbc_handle.h"

namespace vbc {

namespace {

// Source element converted to the compute eltype: C casts, as host_convert does at create (Bool: its byte).
template <typename S, typename D>
__device__ __forceinline__ D update_value(gptr<const S> src, uint32_t e)
{
    if (e >= kUpdSkip) return D(0);
    const D v = (D)src[e & ~kUpdCanon];
    if constexpr (std::is_floating_point<D>::value) {
        if (e & kUpdCanon) return D(0) + v;  // the create path adds the value into a zeroed slot (-0 -> +0)
    }
    return v;
}

// One chunk of the mixed kernel below: update_values_kernel's loop body (kept apart from it so that the kernels
// every other handle launches compile exactly as before) with D the chunk's stored eltype -- double, or float for
// a narrow chunk: four floats and four entries per quad, one 16-byte map load, four gathers, one 16-byte store;
// kUpdCanon stores 0.0f + v, which is the create path's (float)(0.0 + (double)v).
template <typename S, typename D>
__device__ __forceinline__ void update_chunk(const UpdChunk ch, const uint32_t *map, gptr<const S> src, D *arena)
{
    constexpr int V = 16 / (int)sizeof(D);
    constexpr int U = kUpdChunkQuads / 256;
    typedef uint32_t mv __attribute__((ext_vector_type(V)));
    typedef D dv __attribute__((ext_vector_type(V)));
    const gptr<const mv> mp = (gptr<const mv>)G(map + ch.map);
    const gptr<dv> dp = (gptr<dv>)G(arena + ch.dst);
    mv m[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t q = threadIdx.x + u * 256;
        if (q < ch.n) m[u] = __builtin_nontemporal_load(mp + q);
    }
    dv v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t q = threadIdx.x + u * 256;
        if (q < ch.n) {
#pragma unroll
            for (int i = 0; i < V; i++) v[u][i] = update_value<S, D>(src, m[u][i]);
        }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t q = threadIdx.x + u * 256;
        if (q < ch.n) {
            bool skip = false;
#pragma unroll
            for (int i = 0; i < V; i++) skip = skip || m[u][i] == kUpdSkip;
            if (!skip) {
                __builtin_nontemporal_store(v[u], dp + q);
            } else {
                const gptr<D> d1 = (gptr<D>)(dp + q);
#pragma unroll
                for (int i = 0; i < V; i++)
                    if (m[u][i] != kUpdSkip) d1[i] = v[u][i];
            }
        }
    }
}

// One 16-byte quad per lane: the map as one vector load, a gather of the source elements, one non-temporal
// vector store (the next product streams the arena from HBM anyway).  A quad with a kUpdSkip entry (the
// ends of a region that does not start or stop on a quad) stores its slots one by one and leaves the rest.
template <typename S, typename D>
__global__ __launch_bounds__(256) void update_values_kernel(const UpdChunk *chunks, int64_t nchunks,
                                                            const uint32_t *map, const S *src_, D *arena)
{
    constexpr int V = 16 / (int)sizeof(D);
    constexpr int U = kUpdChunkQuads / 256;
    typedef uint32_t mv __attribute__((ext_vector_type(V)));
    typedef D dv __attribute__((ext_vector_type(V)));
    const gptr<const S> src = G(src_);
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const UpdChunk ch = chunks[c];
        const gptr<const mv> mp = (gptr<const mv>)G(map + ch.map);
        const gptr<dv> dp = (gptr<dv>)G(arena + ch.dst);
        mv m[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t q = threadIdx.x + u * 256;
            if (q < ch.n) m[u] = __builtin_nontemporal_load(mp + q);
        }
        dv v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t q = threadIdx.x + u * 256;
            if (q < ch.n) {
#pragma unroll
                for (int i = 0; i < V; i++) v[u][i] = update_value<S, D>(src, m[u][i]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t q = threadIdx.x + u * 256;
            if (q < ch.n) {
                bool skip = false;
#pragma unroll
                for (int i = 0; i < V; i++) skip = skip || m[u][i] == kUpdSkip;
                if (!skip) {
                    __builtin_nontemporal_store(v[u], dp + q);
                } else {
                    const gptr<D> d1 = (gptr<D>)(dp + q);
#pragma unroll
                    for (int i = 0; i < V; i++)
                        if (m[u][i] != kUpdSkip) d1[i] = v[u][i];
                }
            }
        }
    }
}

// VBC_CREATE_NARROW_UPDATABLE: Float32 sources into a Float64 handle whose chunks say their stored size (uniform
// for the workgroup: one branch per chunk).  A narrow chunk is rewritten as floats, a wide chunk of the same
// handle by the body every other handle runs (the float source widened).  Launched for such handles only.
__global__ __launch_bounds__(256) void update_values_mixed_kernel(const UpdChunk *chunks, int64_t nchunks,
                                                                  const uint32_t *map, const float *src_, double *arena)
{
    const gptr<const float> src = G(src_);
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const UpdChunk ch = chunks[c];
        if (ch.vsz == 4) update_chunk<float, float>(ch, map, src, reinterpret_cast<float *>(arena));
        else update_chunk<float, double>(ch, map, src, arena);
    }
}

inline int64_t update_grid(const vbc_handle *h)
{
    return std::min<int64_t>(h->umap.nchunks, (int64_t)std::max(h->cus, 1) * 8);
}

template <typename S, typename D>
int launch(const vbc_handle *h, const void *d_val, hipStream_t s)
{
    const ValueMap &um = h->umap;
    if (um.nchunks == 0) return VBC_OK;
    hipLaunchKernelGGL((update_values_kernel<S, D>), dim3((unsigned)update_grid(h)), dim3(256), 0, s, um.d_chunks,
                       um.nchunks, um.d_map, static_cast<const S *>(d_val), static_cast<D *>(h->d_arena));
    VBC_HIP(hipGetLastError());
    return VBC_OK;
}

template <typename D>
int launch_from(const vbc_handle *h, const void *d_val, int val_dtype, hipStream_t s)
{
    switch (val_dtype) {
    case VBC_F64:
        if constexpr (std::is_floating_point<D>::value) return launch<double, D>(h, d_val, s);
        break;
    case VBC_F32:
        if constexpr (std::is_floating_point<D>::value) return launch<float, D>(h, d_val, s);
        break;
    case VBC_I64: return launch<int64_t, D>(h, d_val, s);
    case VBC_I32: return launch<int32_t, D>(h, d_val, s);
    case VBC_BOOL: return launch<uint8_t, D>(h, d_val, s);
    default: break;
    }
    return fail(VBC_UNSUPPORTED_DTYPE, "floating-point values on an integer handle (InexactError)");
}

inline uint64_t arena_word(const std::vector<char> &a, size_t i, int esz)
{
    uint64_t w = 0;
    std::memcpy(&w, a.data() + i * esz, (size_t)esz);
    return w;
}

}  // namespace

int update_launch(const vbc_handle *h, const void *d_val, int val_dtype, hipStream_t s)
{
    if (h->umap.mixed) {  // VBC_CREATE_NARROW_UPDATABLE (vbc_update_values has refused every other val_dtype)
        if (h->dtype != VBC_F64 || val_dtype != VBC_F32)
            return fail(VBC_UNSUPPORTED_DTYPE, "a VBC_CREATE_NARROW_UPDATABLE handle takes Float32 values only");
        const ValueMap &um = h->umap;
        if (um.nchunks == 0) return VBC_OK;
        hipLaunchKernelGGL(update_values_mixed_kernel, dim3((unsigned)update_grid(h)), dim3(256), 0, s, um.d_chunks,
                           um.nchunks, um.d_map, static_cast<const float *>(d_val), static_cast<double *>(h->d_arena));
        VBC_HIP(hipGetLastError());
        return VBC_OK;
    }
    if (h->dtype == VBC_F64) return launch_from<double>(h, d_val, val_dtype, s);
    if (h->dtype == VBC_F32) return launch_from<float>(h, d_val, val_dtype, s);
    return launch_from<int64_t>(h, d_val, val_dtype, s);
}

// The map of a handle, on the host alone.  `tagged` / `zeroed`: the arena images of the two recording plans;
// `canon`: the byte ranges whose values went through transpose_stripes; `narrow`: the byte ranges of the value
// regions stored as Float32 on a Float64 handle (VBC_CREATE_NARROW_UPDATABLE; both lists ascend).  The images are
// compared word by word, 4 bytes wide inside a narrow range and esz wide elsewhere; a region never crosses the end
// of a range, so every chunk has one stored size.  `dst` counts words of that size from the arena's start (a
// narrow range starts on an arena reservation, 256-byte aligned).
int value_map_host(int esz, int64_t nval, const std::vector<char> &tagged, const std::vector<char> &zeroed,
                   const ByteRanges &canon, const ByteRanges &narrow, std::vector<uint32_t> &map,
                   std::vector<UpdChunk> &chunks)
{
    map.clear();
    chunks.clear();
    if (tagged.size() != zeroed.size())
        return fail(VBC_INVALID_ARG, "internal: the recording builds of an updatable handle disagree on the arena size");
    const size_t bytes = tagged.size();
    const size_t kGap = 64;  // most padding slots between two runs of one region
    size_t ci = 0;           // canon ranges ascend
    // the words of `sz` bytes that lie wholly inside the bytes [sb, se)
    auto stretch = [&](size_t sb, size_t se, int sz) -> int {
        const size_t V = 16 / (size_t)sz;
        const size_t i0 = (sb + sz - 1) / sz, i1 = se / sz;
        auto close = [&](size_t rb, size_t re) {
            const size_t b = rb / V * V, e = (re + V - 1) / V * V;
            while (map.size() % V) map.push_back(kUpdSkip);  // a quad's entries are one aligned vector load
            const size_t m0 = map.size();
            for (size_t i = b; i < e; i++) {
                uint32_t ent = kUpdSkip;
                if (i >= rb && i < re) {
                    const uint64_t t = arena_word(tagged, i, sz);
                    if (t == arena_word(zeroed, i, sz)) {
                        ent = kUpdZero;
                    } else {
                        ent = (uint32_t)(t - 1);
                        while (ci < canon.size() && canon[ci].second <= i * sz) ci++;
                        if (ci < canon.size() && canon[ci].first <= i * sz) ent |= kUpdCanon;
                    }
                }
                map.push_back(ent);
            }
            for (size_t q = 0; q < (e - b) / V; q += kUpdChunkQuads)
                chunks.push_back({(uint64_t)(b + q * V), (uint64_t)(m0 + q * V),
                                  (uint32_t)std::min<size_t>(kUpdChunkQuads, (e - b) / V - q),
                                  sz == esz ? 0u : (uint32_t)sz});
        };
        bool open = false, gap_zero = true;
        size_t rb = 0, re = 0;
        for (size_t i = i0; i < i1; i++) {
            const uint64_t t = arena_word(tagged, i, sz), z = arena_word(zeroed, i, sz);
            if (t == z) {
                gap_zero = gap_zero && t == 0;
                continue;
            }
            if (z != 0 || t < 1 || t > (uint64_t)nval)
                return fail(VBC_INVALID_ARG, "internal: an arena word of an updatable handle is neither layout nor a copied value");
            if (open && !(gap_zero && i - re <= kGap)) {
                close(rb, re);
                open = false;
            }
            if (!open) rb = i;
            open = true;
            re = i + 1;
            gap_zero = true;
        }
        if (open) close(rb, re);
        return VBC_OK;
    };
    // a quad that reaches past its stretch (or the arena's end) must not be stored whole: its outside entries are
    // kUpdSkip already (they lie outside every region), which sends the quad down the slot-by-slot path
    size_t at = 0;
    for (const auto &r : narrow) {
        if (esz != 8 || r.first < at || r.second < r.first || r.second > bytes || r.first % 16)
            return fail(VBC_INVALID_ARG, "internal: bad narrow value range of an updatable handle");
        if (int st = stretch(at, r.first, esz)) return st;
        if (int st = stretch(r.first, r.second, 4)) return st;
        at = r.second;
    }
    return stretch(at, bytes, esz);
}

// The device copy of the map.  The caller has set the device.
int upload_value_map(vbc_handle *h, const std::vector<uint32_t> &map, const std::vector<UpdChunk> &chunks)
{
    ValueMap &um = h->umap;
    um.entries = (int64_t)map.size();
    um.nchunks = (int64_t)chunks.size();
    const size_t map_bytes = (map.size() * 4 + 255) & ~size_t(255);
    um.bytes = map_bytes + std::max<size_t>(chunks.size() * sizeof(UpdChunk), 256);
    VBC_HIP(hipMalloc(&um.d_buf, um.bytes));
    char *b = static_cast<char *>(um.d_buf);
    if (!map.empty()) VBC_HIP(hipMemcpy(b, map.data(), map.size() * 4, hipMemcpyHostToDevice));
    if (!chunks.empty())
        VBC_HIP(hipMemcpy(b + map_bytes, chunks.data(), chunks.size() * sizeof(UpdChunk), hipMemcpyHostToDevice));
    um.d_map = reinterpret_cast<const uint32_t *>(b);
    um.d_chunks = reinterpret_cast<const UpdChunk *>(b + map_bytes);
    return VBC_OK;
}

}  // namespace vbc

