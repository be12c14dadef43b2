// segments.cuh -- the segment tables of the segmented forms of K1's digit pass (msm_seg.cuh) and of K2's fold (bpoly_seg.cuh): many independent sums over ranges
// of ONE input array in one launch set.  The tables are device memory the caller may rewrite while a call is queued: every kernel clamps what it reads from them
// to the array (begin <= end <= n_total, length <= the launch's longest segment), so a stale or hostile table gives a wrong sum, never a read past the arrays.
#pragma once
#include <stdint.h>

namespace mb {

struct MsmSegments { const uint32_t *begin, *end; uint32_t n_total; };      // device pointers, one word per segment each

__device__ __forceinline__ void msm_segment_range(const MsmSegments &sg, uint32_t m, uint32_t n_max, uint32_t &first, uint32_t &len) {
    const uint32_t b = sg.begin[m], e = sg.end[m];
    first = b < sg.n_total ? b : sg.n_total;
    const uint32_t last = e < first ? first : (e < sg.n_total ? e : sg.n_total);
    len = last - first < n_max ? last - first : n_max;
}

}  // namespace mb
