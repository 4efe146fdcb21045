// vbc_sharded_update_values, row split (vbc.h VBC_CREATE_UPDATABLE_SHARDS): the kernel that permutes the whole
// matrix's val into packed order -- shard 0's values, then shard 1's, ... -- so that every shard's new values
// are one contiguous slice (vbc_internal.h ValuePlan).  Raw elements of the caller's val_dtype are moved; the
// conversion to the compute eltype happens later, in each shard's update kernel (vbc_update.hip).
//
// The grid runs over destination tiles of kPackTile elements.  A tile's runs are tile_first[t] .. tile_first[t+1]
// (built at create), so a lane finds the run of its first element by a binary search over that short range of
// the ascending dst offsets and then walks forward.  One 16-byte quad of destination per lane and step:
// consecutive lanes write consecutive quads, and read consecutive source elements wherever a run continues
// (the ldoor row shards: runs of about 18 elements).  The source is in general not 16-byte aligned against the
// destination (a run may start anywhere), so it is gathered element by element.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vbc_internal.h"

namespace vbc {

namespace {

template <typename T>
__global__ __launch_bounds__(256) void pack_values_kernel(const int64_t *__restrict__ rdst,
                                                          const int64_t *__restrict__ rsrc,
                                                          const int64_t *__restrict__ tile_first, int64_t ntiles,
                                                          int64_t nval, const T *__restrict__ val,
                                                          T *__restrict__ packed)
{
    constexpr int V = 16 / (int)sizeof(T);           // elements per quad
    constexpr int Q = (int)(kPackTile / V);          // quads per tile
    typedef T tv __attribute__((ext_vector_type(V)));
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t base = t * kPackTile;
        const int64_t r_lo = tile_first[t], r_hi = tile_first[t + 1];
        for (int q = threadIdx.x; q < Q; q += 256) {
            const int64_t d = base + (int64_t)q * V;
            if (d >= nval) break;
            int64_t lo = r_lo, hi = r_hi;  // the last run with rdst <= d lies in [lo, hi]
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (rdst[mid] <= d) lo = mid;
                else hi = mid - 1;
            }
            int64_t r0 = rdst[lo], r1 = rdst[lo + 1], s0 = rsrc[lo];
            tv v;
#pragma unroll
            for (int i = 0; i < V; i++) {
                const int64_t e = d + i;
                T x = T(0);
                if (e < nval) {
                    while (e >= r1) {  // rdst[nruns] == nval > e: the walk ends inside the table
                        lo++;
                        r0 = r1;
                        r1 = rdst[lo + 1];
                        s0 = rsrc[lo];
                    }
                    x = __builtin_nontemporal_load(val + (s0 + (e - r0)));
                }
                v[i] = x;
            }
            if (d + V <= nval) {
                *reinterpret_cast<tv *>(packed + d) = v;  // d is a multiple of V: 16-byte aligned
            } else {
#pragma unroll
                for (int i = 0; i < V; i++)
                    if (d + i < nval) packed[d + i] = v[i];
            }
        }
    }
}

template <typename T>
int launch(const int64_t *rdst, const int64_t *rsrc, const int64_t *tile_first, int64_t ntiles, int64_t nval,
           const void *val, void *packed, int cus, hipStream_t s)
{
    const int64_t grid = std::min<int64_t>(ntiles, (int64_t)std::max(cus, 1) * 8);
    hipLaunchKernelGGL((pack_values_kernel<T>), dim3((unsigned)grid), dim3(256), 0, s, rdst, rsrc, tile_first, ntiles,
                       nval, static_cast<const T *>(val), static_cast<T *>(packed));
    if (hipGetLastError() != hipSuccess) return fail(VBC_HIP_ERROR, "launch of the value pack kernel failed");
    return VBC_OK;
}

}  // namespace

int pack_launch(const int64_t *rdst, const int64_t *rsrc, const int64_t *tile_first, int64_t ntiles, int64_t nval,
                const void *val, void *packed, int vsz, int cus, void *stream)
{
    if (ntiles <= 0 || nval <= 0) return VBC_OK;
    hipStream_t s = (hipStream_t)stream;
    switch (vsz) {
    case 8: return launch<uint64_t>(rdst, rsrc, tile_first, ntiles, nval, val, packed, cus, s);
    case 4: return launch<uint32_t>(rdst, rsrc, tile_first, ntiles, nval, val, packed, cus, s);
    case 1: return launch<uint8_t>(rdst, rsrc, tile_first, ntiles, nval, val, packed, cus, s);
    default: return fail(VBC_UNSUPPORTED_DTYPE, "unknown val_dtype");
    }
}

}  // namespace vbc
