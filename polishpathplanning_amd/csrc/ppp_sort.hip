/* ppp_sort.hip -- rocPRIM behind plain functions: the device radix sort (voxel_down orders points by voxel id with it) and the
   device-wide exclusive scan (the mesh sampler offsets its rows and samples with it) */
#include <cstring>
#include "ppp_sort.h"
#include <rocprim/rocprim.hpp>

hipError_t ppp_sort_pairs_u32(void *tmp, size_t *tmp_bytes, const unsigned *key_in, unsigned *key_out, const int *val_in, int *val_out,
                              size_t n, int end_bit, hipStream_t stream)
{
    return rocprim::radix_sort_pairs(tmp, *tmp_bytes, key_in, key_out, val_in, val_out, n, 0u, (unsigned)end_bit, stream);
}

namespace {
struct SaturatingAdd {
    __host__ __device__ unsigned operator()(unsigned a, unsigned b) const
    {
        const unsigned long long s = (unsigned long long)a + b;
        return s > 0xffffffffull ? 0xffffffffu : (unsigned)s;
    }
};
} // namespace

hipError_t ppp_scan_exclusive_u32(void *tmp, size_t *tmp_bytes, const unsigned *in, unsigned *out, size_t n, hipStream_t stream)
{
    return rocprim::exclusive_scan(tmp, *tmp_bytes, in, out, 0u, n, SaturatingAdd(), stream);
}
