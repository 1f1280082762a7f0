// live_search.hpp -- the binary search the destination-stationary builders share (regions.hip, sample.hip): which live
// record of an ascending offsets table holds a byte of the joined text.
#pragma once

#include <hip/hip_runtime.h>

namespace lm {

// largest s in [lo, hi) with dst[s] <= x (dst[lo] <= x)
template <class Off>
__device__ __forceinline__ unsigned long long find_live(const Off &dst, unsigned long long lo, unsigned long long hi, unsigned long long x)
{
    while (hi - lo > 1) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        if (dst(mid) <= x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

}  // namespace lm
